#!/usr/bin/env python3
"""Per-shape rate of the four Linear paths -- bf16 (gemm_bf16_v2), MX fp8 (gemm_mxfp8.hip), MXFP6 (gemm_mxfp6.hip, W6A6) and
MXFP4 (gemm_mxfp4.hip, W4A4) -- at the Wan2.1 1.3B (M = 32 768) and 14B (M = 75 776 = 75 600 tokens padded to 256) Linear
shapes and at the block shapes of FLUX.1-dev 1024^2 (4096 image + 512 text tokens, dim 3072), each with its epilogue.  The
four are timed back to back after a 1 s pre-heat each and interleaved over rounds (the median round counts): the method of
tools/mxfp4_shapes.py, which this tool extends by one format and five shapes.

    python tools/mxfp6_shapes.py [rounds=3] [launches=20] [substring of the shape names to run]

One JSON line per shape and a summary line.  The quantise passes are NOT in these times (both engines run them as separate
kernels in the MXFP6 mode; the forward-level figures are tools/bench_wan14b.py's and tools/bench_mmdit.py's)."""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import hip_ops as H  # noqa: E402
import mxfp4_ref as R4  # noqa: E402
import mxfp6_ref as R6  # noqa: E402

DEV = "cuda:0"
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
launches = int(sys.argv[2]) if len(sys.argv) > 2 else 20
only = sys.argv[3] if len(sys.argv) > 3 else ""
PEAK = {"bf16": 2500.0, "mxfp8": 5000.0, "mxfp6": 10000.0, "mxfp4": 10000.0}      # dense TFLOP/s (MI355X)

SHAPES = [("14B qkv", 75776, 15360, 5120, 0), ("14B ffn1+gelu", 75776, 13824, 5120, 1), ("14B ffn2+resid", 75776, 5120, 13824, 2),
          ("14B o+resid", 75776, 5120, 5120, 2),
          ("1.3B qkv", 32768, 4608, 1536, 0), ("1.3B ffn1+gelu", 32768, 8960, 1536, 1), ("1.3B ffn2+resid", 32768, 1536, 8960, 2),
          ("FLUX double qkv", 4096, 9216, 3072, 0), ("FLUX double mlp-in+gelu", 4096, 12288, 3072, 1),
          ("FLUX double mlp-out+resid", 4096, 3072, 12288, 2), ("FLUX single mlp-in+gelu", 4608, 12288, 3072, 1),
          ("FLUX single linear2+resid", 4608, 3072, 15360, 2)]


def time_it(fn, n):
    t0 = time.time()
    while time.time() - t0 < 1.0:            # sustained-power regime
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


out = []
g = torch.Generator(device=DEV).manual_seed(0)
for name, M, N, K, epi in SHAPES:
    if only not in name:
        continue
    A = torch.randn(M, K, generator=g, device=DEV).bfloat16()
    W = (torch.randn(N, K, generator=g, device=DEV) * 0.03).bfloat16()
    bias = torch.randn(N, generator=g, device=DEV)
    a8, sa8 = H.quantize_rows_mx(A)
    w8, sw8 = H.quantize_rows_mx(W)
    a6, sa6 = R6.op_quantize(A)
    w6, sw6 = R6.op_quantize(W, rows_pad=N)
    a4, sa4 = R4.op_quantize(A)
    w4, sw4 = R4.op_quantize(W, rows_pad=N)
    gate = torch.randn(N, generator=g, device=DEV) if epi == 2 else None
    cb = torch.empty(M, N, dtype=torch.bfloat16, device=DEV) if epi < 2 else None
    x = torch.randn(M, N, generator=g, device=DEV) if epi == 2 else None
    fns = {"bf16": lambda: H.gemm(A, W, bias, epi, Cb=cb, X=x, gate=gate),
           "mxfp8": lambda: H.gemm_mxfp8(a8, sa8, w8, sw8, bias, epi, Cb=cb, X=x, gate=gate),
           "mxfp6": lambda: R6.op_gemm(a6, sa6, w6, sw6, bias, epi, Cb=cb, X=x, gate=gate),
           "mxfp4": lambda: R4.op_gemm(a4, sa4, w4, sw4, bias, epi, Cb=cb, X=x, gate=gate)}
    res = {k: [] for k in fns}
    for r in range(rounds):
        for k, fn in fns.items():
            res[k].append(time_it(fn, launches))
    fl = 2.0 * M * N * K
    ent = {"shape": name, "M": M, "N": N, "K": K, "epilogue": ["bf16", "gelu", "gated residual (fp32 RMW)"][epi]}
    for k, ts in res.items():
        t = sorted(ts)[len(ts) // 2]
        ent[k + "_us"] = round(t * 1e3, 1)
        ent[k + "_tflops"] = round(fl / t / 1e9, 1)
        ent[k + "_frac_of_its_peak"] = round(fl / t / 1e9 / PEAK[k], 3)
    ent["mxfp6_over_mxfp8"] = round(ent["mxfp8_us"] / ent["mxfp6_us"], 3)
    ent["mxfp6_over_mxfp4"] = round(ent["mxfp4_us"] / ent["mxfp6_us"], 3)
    ent["mxfp6_over_bf16"] = round(ent["bf16_us"] / ent["mxfp6_us"], 3)
    out.append(ent)
    print(json.dumps(ent), flush=True)
    del A, W, a8, w8, a6, w6, a4, w4, cb, x, fns
    torch.cuda.empty_cache()
print(json.dumps({"summary": {e["shape"]: [e["bf16_us"], e["mxfp8_us"], e["mxfp6_us"], e["mxfp4_us"], e["mxfp6_over_mxfp8"]] for e in out},
                  "columns": "microseconds bf16, MX fp8, MXFP6, MXFP4; MXFP6 speed-up over MX fp8"}))
