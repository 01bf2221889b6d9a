"""Time of one adapter apply over FLUX.1-dev's attention and MLP Linears for a DoRA and for a LoKr adapter.

Each distinct part shape is merged through mc_op_adapter_merge with caller-owned scratch (the asynchronous form; the store's
apply adds one hipMalloc / hipFree pair per part, which is not in these figures) and through mc_op_lora_merge for comparison;
the per-shape medians are summed with the number of such parts in the 19 double and 38 single blocks.  Prints one JSON line.

    python tools/bench_adapter_merge.py [--rank 16] [--reps 10]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from magcache_amd import _lib  # noqa: E402

DEV = "cuda:0"
D = 3072
# (rows, K): parts per double block, parts per single block -- q, k, v, add_q/k/v, to_out, to_add_out; ff / ff_context in and out;
# single: q, k, v, proj_mlp; proj_out
PARTS = {(D, D): (8, 3), (4 * D, D): (2, 1), (D, 4 * D): (2, 0), (D, 5 * D): (0, 1)}
N_DOUBLE, N_SINGLE = 19, 38


def ptr(t):
    return C.c_void_p(t.data_ptr())


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rank", type=int, default=16)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    lib = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    per_shape, total = {}, {"lora": 0.0, "dora": 0.0, "lokr": 0.0, "copy": 0.0}
    for (rows, K), (nd, ns) in PARTS.items():
        count = nd * N_DOUBLE + ns * N_SINGLE
        W = (torch.randn(rows, K, device=DEV) * 0.02).bfloat16()
        out = torch.empty_like(W)
        down = (torch.randn(args.rank, K, device=DEV) * 0.05).bfloat16()
        up = (torch.randn(rows, args.rank, device=DEV) * 0.05).bfloat16()
        w1, w2 = torch.randn(8, 8, device=DEV) * 0.1, torch.randn(rows // 8, K // 8, device=DEV) * 0.1
        mag = W.float().norm(dim=1)
        pair = (_lib.McAdapterTerm * 1)(_lib.McAdapterTerm(_lib.MC_ADAPTER_PAIR, 1.0, down.data_ptr(), up.data_ptr(), 0, 0, args.rank, 0, 0, 0, 0))
        kron = (_lib.McAdapterTerm * 1)(_lib.McAdapterTerm(_lib.MC_ADAPTER_KRON, 1.0, w1.data_ptr(), w2.data_ptr(), 0, 0, 0, 8, 8, rows // 8, K // 8))
        old = (_lib.McLoraTerm * 1)(_lib.McLoraTerm(down.data_ptr(), up.data_ptr(), args.rank, 1.0))
        need = max(lib.mc_op_adapter_merge_scratch(rows, K, pair, 1), lib.mc_op_adapter_merge_scratch(rows, K, kron, 1))
        raw = torch.empty(need + 256, dtype=torch.uint8, device=DEV)
        sp = C.c_void_p(raw.data_ptr() + (-raw.data_ptr()) % 256)

        def lora():
            _lib.check(lib.mc_op_lora_merge(ptr(W), K, ptr(out), K, rows, K, old, 1, sp, need, stream))

        def dora():
            _lib.check(lib.mc_op_adapter_merge(ptr(W), K, ptr(out), K, rows, K, pair, 1, ptr(mag), sp, need, stream))

        def lokr():
            _lib.check(lib.mc_op_adapter_merge(ptr(W), K, ptr(out), K, rows, K, kron, 1, None, sp, need, stream))

        def copy():
            out.copy_(W)
        ms = {name: timed(fn, args.reps) for name, fn in (("lora", lora), ("dora", dora), ("lokr", lokr), ("copy", copy))}
        per_shape[f"{rows}x{K}"] = dict(parts=count, **{k: round(v, 4) for k, v in ms.items()})
        for k, v in ms.items():
            total[k] += v * count
    print(json.dumps(dict(rank=args.rank, reps=args.reps, per_shape_ms=per_shape, flux1_dev_apply_ms={k: round(v, 2) for k, v in total.items()})))


if __name__ == "__main__":
    main()
