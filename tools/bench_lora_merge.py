"""Time of a full LoRA re-merge (MMDiTEngine.apply_lora after a scale change) at FLUX.1-dev's block shapes, against a
device-to-device copy of the same base bytes.

    python tools/bench_lora_merge.py                     # 2 double + 4 single blocks of FLUX.1-dev, ranks 16 and 128
    python tools/bench_lora_merge.py --double 4 --single 8 --ranks 16 64 128

One adapter sits on every attention and MLP Linear of every block (q, k, v, out and the two MLP Linears of both streams of a
double block; q, k, v, proj_mlp and proj_out of a single block).  A re-merge reads every touched part's base rows and writes
its live rows -- twice the base bytes, plus the small operands -- in one launch per part; the copy moves the same base bytes
once in and once out in one call, which is the floor for that traffic.  The two are timed in alternating windows of the same
process (device events around `--reps` repetitions after a warm-up, the median of `--rounds` windows and their spread).  The
engine's weights are left unset: the merge does not read them by value.

Prints one JSON line: per rank the merge and copy time of the benchmarked depth, their ratio, the traffic rate of the merge
(2 x base bytes + operand bytes over its time), and the merge time scaled by the Linear count to FLUX.1-dev's 19 + 38 blocks."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from magcache_amd import _lib  # noqa: E402
from magcache_amd import mmdit as MM  # noqa: E402
from magcache_amd.lora import lora_target_names  # noqa: E402

DEV = "cuda:0"
DIM, HEADS, TXT_DIM, VEC_DIM = 3072, 24, 4096, 768
FULL_DOUBLE, FULL_SINGLE = 19, 38


def block_targets(n_double, n_single):
    """attention and MLP Linears of the blocks, with their [out, in] shapes"""
    d = DIM
    shapes = {"attn.to_q": (d, d), "attn.to_k": (d, d), "attn.to_v": (d, d), "attn.to_out.0": (d, d), "attn.add_q_proj": (d, d),
              "attn.add_k_proj": (d, d), "attn.add_v_proj": (d, d), "attn.to_add_out": (d, d), "ff.net.0.proj": (4 * d, d),
              "ff.net.2": (d, 4 * d), "ff_context.net.0.proj": (4 * d, d), "ff_context.net.2": (d, 4 * d), "proj_mlp": (4 * d, d),
              "proj_out": (d, 5 * d)}
    out = {}
    for name in lora_target_names("flux", n_double, n_single):
        if "blocks." not in name or "norm" in name:
            continue
        leaf = name.split(".", 2)[2][:-len(".weight")]
        out[name] = shapes[leaf]
    return out


def window(fn, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(reps):
        fn(i)
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / reps      # ms


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--double", type=int, default=2)
    ap.add_argument("--single", type=int, default=4)
    ap.add_argument("--ranks", type=int, nargs="+", default=[16, 128])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lora_merge needs the GPU: there is nothing to time without one")
    e = MM.MMDiTEngine(_lib.MC_FAMILY_FLUX, DIM, HEADS, a.double, a.single, 64, 64, TXT_DIM, 64, VEC_DIM, 256, device=DEV)
    targets = block_targets(a.double, a.single)
    base_bytes = sum(o * i * 2 for o, i in targets.values())
    full_bytes = base_bytes // (a.double * 24 + a.single * 12) * (FULL_DOUBLE * 24 + FULL_SINGLE * 12)   # in units of d^2 elements
    src = torch.empty(base_bytes, dtype=torch.uint8, device=DEV)
    dst = torch.empty(base_bytes, dtype=torch.uint8, device=DEV)
    stream = MM._stream()
    result = dict(dim=DIM, double=a.double, single=a.single, parts=len(targets), base_bytes=base_bytes, reps=a.reps, rounds=a.rounds,
                  ranks={})
    g = torch.Generator().manual_seed(0)
    for rank in a.ranks:
        sd = {}
        for name, (o, i) in targets.items():
            mod = name[:-len(".weight")]
            sd[mod + ".lora_A.weight"] = (torch.randn(rank, i, generator=g) * 0.02).bfloat16()
            sd[mod + ".lora_B.weight"] = (torch.randn(o, rank, generator=g) * 0.02).bfloat16()
        e.load_lora(sd, adapter="bench")
        info = e.lora_info()
        rank_pad = (rank + 15) // 16 * 16      # the kernel's rank step
        operand_bytes = sum((o + i) * rank_pad * 2 for o, i in targets.values())

        def merge(i):
            _lib.check(e.lib.mc_mmdit_lora_scale(e.h, b"bench", 1.0 + (i & 1)))      # every part is dirty again
            _lib.check(e.lib.mc_mmdit_lora_apply(e.h, stream))

        def copy(i):
            dst.copy_(src)
        for fn in (merge, copy):
            window(fn, 3)
        t_merge, t_copy = [], []
        for _ in range(a.rounds):
            t_merge.append(window(merge, a.reps))
            t_copy.append(window(copy, a.reps))
        m, c = statistics.median(t_merge), statistics.median(t_copy)
        result["ranks"][str(rank)] = dict(
            merge_ms=round(m, 4), merge_ms_min_max=[round(min(t_merge), 4), round(max(t_merge), 4)],
            copy_ms=round(c, 4), copy_ms_min_max=[round(min(t_copy), 4), round(max(t_copy), 4)],
            merge_over_copy=round(m / c, 3), operand_bytes=operand_bytes, base_copy_bytes=info["base_bytes"],
            merge_traffic_TBps=round((2 * base_bytes + operand_bytes) / (m * 1e-3) / 1e12, 3),
            copy_traffic_TBps=round(2 * base_bytes / (c * 1e-3) / 1e12, 3),
            flux_dev_full_merge_ms=round(m * full_bytes / base_bytes, 3), flux_dev_full_base_bytes=full_bytes)
        e.unload_lora()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
