"""Time of a full LoRA re-merge on the Wan engine (Engine.apply_lora after a scale change) at Wan2.1's 1.3B and 14B widths,
against a device-to-device copy of the same base bytes.

    python tools/bench_wan_lora.py                       # both widths, 2 layers each, ranks 16 and 128
    python tools/bench_wan_lora.py --layers 4 --ranks 16 64 128 --widths 14B

One adapter sits on every block Linear (self-attention q, k, v, o; cross-attention q, k, v, o; ffn.0 and ffn.2): ten merge
launches per layer.  A re-merge reads every touched part's base rows and writes its live rows, the copy moves the same bytes
once in and once out in one call -- the floor for that traffic.  The two are timed in alternating windows of one process
(device events around `--reps` repetitions after a warm-up, the median of `--rounds` windows and their spread), as
tools/bench_lora_merge.py does for the MM-DiT engine: the kernel is the same bf16 merge.  The engine's weights are left
unset: the merge does not read them by value.

Prints one JSON line: per width and rank the merge and copy time at the benchmarked depth, their ratio, the traffic rate of the
merge, and the merge time scaled by the layer count to the full model (30 / 40 layers)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from magcache_amd import _lib  # noqa: E402
from magcache_amd import engine as E  # noqa: E402

DEV = "cuda:0"
WIDTHS = {"1.3B": E.WAN_T2V_1_3B, "14B": E.WAN_T2V_14B}
GRID = (1, 16, 16)        # the merge does not depend on the latent grid: the smallest workspace


def block_targets(cfg, layers):
    d, ffn = cfg["dim"], cfg["ffn_dim"]
    out = {}
    for i in range(layers):
        for a in ("self_attn", "cross_attn"):
            for w in ("q", "k", "v", "o"):
                out[f"blocks.{i}.{a}.{w}"] = (d, d)
        out[f"blocks.{i}.ffn.0"], out[f"blocks.{i}.ffn.2"] = (ffn, d), (d, ffn)
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
    ap.add_argument("--widths", nargs="+", default=["1.3B", "14B"], choices=list(WIDTHS))
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--ranks", type=int, nargs="+", default=[16, 128])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_wan_lora needs the GPU: there is nothing to time without one")
    result = dict(layers=a.layers, reps=a.reps, rounds=a.rounds, widths={})
    g = torch.Generator().manual_seed(0)
    for width in a.widths:
        full = WIDTHS[width]
        cfg = dict(full, num_layers=a.layers)
        e = E.Engine(cfg, GRID, device=DEV, n_branches=1)
        targets = block_targets(cfg, a.layers)
        base_bytes = sum(o * i * 2 for o, i in targets.values())
        src = torch.empty(base_bytes, dtype=torch.uint8, device=DEV)
        dst = torch.empty(base_bytes, dtype=torch.uint8, device=DEV)
        stream = E._stream()
        per_rank = {}
        for rank in a.ranks:
            sd = {}
            for mod, (o, i) in targets.items():
                sd[mod + ".lora_A.weight"] = (torch.randn(rank, i, generator=g) * 0.02).bfloat16()
                sd[mod + ".lora_B.weight"] = (torch.randn(o, rank, generator=g) * 0.02).bfloat16()
            e.load_lora(sd, adapter="bench")
            info = e.lora_info()
            rank_pad = (rank + 15) // 16 * 16
            operand_bytes = sum((o + i) * rank_pad * 2 for o, i in targets.values())

            def merge(i):
                _lib.check(e.lib.mc_lora_scale(e.h, b"bench", 1.0 + (i & 1)))      # every part is dirty again
                _lib.check(e.lib.mc_lora_apply(e.h, stream))

            def copy(i):
                dst.copy_(src)
            for fn in (merge, copy):
                window(fn, 3)
            t_merge, t_copy = [], []
            for _ in range(a.rounds):
                t_merge.append(window(merge, a.reps))
                t_copy.append(window(copy, a.reps))
            m, c = statistics.median(t_merge), statistics.median(t_copy)
            per_rank[str(rank)] = dict(
                merge_ms=round(m, 4), merge_ms_min_max=[round(min(t_merge), 4), round(max(t_merge), 4)],
                copy_ms=round(c, 4), copy_ms_min_max=[round(min(t_copy), 4), round(max(t_copy), 4)],
                merge_over_copy=round(m / c, 3), operand_bytes=operand_bytes, base_copy_bytes=info["base_bytes"],
                merge_traffic_TBps=round((2 * base_bytes + operand_bytes) / (m * 1e-3) / 1e12, 3),
                copy_traffic_TBps=round(2 * base_bytes / (c * 1e-3) / 1e12, 3),
                full_model_merge_ms=round(m * full["num_layers"] / a.layers, 3))
            e.unload_lora()
        result["widths"][width] = dict(dim=cfg["dim"], ffn_dim=cfg["ffn_dim"], parts=len(targets), base_bytes=base_bytes,
                                       full_layers=full["num_layers"], full_base_bytes=base_bytes // a.layers * full["num_layers"],
                                       ranks=per_rank)
        del e, src, dst
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
