#!/usr/bin/env python3
"""Qwen-Image at full size on one MI355X: the 16:9 image (1664 x 928: 6032 image tokens), 60 double blocks of seeded
random weights (no checkpoint offline), cond / negative prompts of 120 / 6 tokens, 50 steps of true CFG (4.0), without
and with MagCache E006K2R02 (thresh 0.06, K 2, retention 0.2, the Qwen-Image table).

    python tools/bench_qwen_image.py [steps] [--fp8_linear M] [--mx_fp4 | --mx_fp6]
    python tools/bench_qwen_image.py --fp8_linear 0,2,3 [--mx_fp4] [--mx_fp6] [--depth D]

`--fp8_linear M` (2 | 3) runs the same measurement on an engine with MX fp8 block Linears (mc_mmdit_config.fp8_linear).  A
list of modes instead compares them: one engine per mode on the same weights, full forwards at 1664 x 928 in alternating
windows (tools/bench_mmdit.py bench_fp8), ms per forward and the spread of the windows per mode (`--depth D`: D blocks
instead of 60).  `--mx_fp4`: with one mode (2 | 3), that engine's Linears are MXFP4 (option "mx_fp4": W4A4, opt-in, much
coarser); with a list, the MXFP4 variants of modes 2 and 3 join the table, with fused and with separate quantise passes.
`--mx_fp6`: the same for MXFP6 (option "mx_fp6": W6A6, opt-in; its quantise passes are always separate).

Prints one JSON line: seconds per image each way, forwards skipped of 2 * steps (the schedule is known on the host
beforehand and is checked against the run), the time of one full and one skipped forward, and the model's achieved
TFLOP/s of the full forward (GEMMs + attention, 2 * M * N * K and 4 * S^2 * d per block) as a fraction of the bf16
dense MFMA peak (2.5 PFLOP/s).  The MM-DiT engine has no per-kernel-class profile (mc_profile covers the Wan engine),
so the GEMM / attention split is the FLOP model's, not a measurement.
"""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from magcache_amd import mmdit as MM  # noqa: E402
from magcache_amd.qwen_bench import random_state_dict  # noqa: E402
from magcache_amd.sampler import qwen_image_sigmas, sample_qwen_image  # noqa: E402

DEV = "cuda:0"
PEAK = 2.5e15


def flops(d, n_blocks, s_img, s_txt):
    s = s_img + s_txt
    gemm = n_blocks * 2 * s * (3 * d * d + d * d + 8 * d * d)
    attn = n_blocks * 4 * s * s * d
    return gemm, attn


def main():
    argv = list(sys.argv[1:])
    fp8 = [0]
    if "--fp8_linear" in argv:
        i = argv.index("--fp8_linear")
        fp8 = [int(v) for v in argv[i + 1].split(",")]
        del argv[i:i + 2]
    mx_fp4 = "--mx_fp4" in argv
    if mx_fp4:
        argv.remove("--mx_fp4")
    mx_fp6 = "--mx_fp6" in argv
    if mx_fp6:
        argv.remove("--mx_fp6")
    depth = None
    if "--depth" in argv:
        i = argv.index("--depth")
        depth = [int(argv[i + 1])]
        del argv[i:i + 2]
    if len(fp8) > 1:
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        from bench_mmdit import bench_fp8
        return bench_fp8("qwen", [(1664, 928)], fp8, depth=depth, txt_len=120, mx_fp4=mx_fp4, mx_fp6=mx_fp6)
    steps = int(argv[0]) if argv else 50
    cfg = MM.QWEN_IMAGE
    h2, w2 = 928 // 16, 1664 // 16
    shapes = [[(1, h2, w2)]]
    n = h2 * w2
    g = torch.Generator(device=DEV).manual_seed(0)
    pe = torch.randn(1, 120, 3584, generator=g, device=DEV)
    ne = torch.randn(1, 6, 3584, generator=g, device=DEV)
    lat = torch.randn(1, n, 64, generator=g, device=DEV)
    t0 = time.time()
    m = MM.QwenImageTransformer2DModelHIP(cfg, n, txt_len=120, device=DEV, calibration=False, fp8_linear=fp8[0], mx_fp4=mx_fp4, mx_fp6=mx_fp6)
    m.load_state_dict(random_state_dict(cfg, DEV, seed=1))
    torch.cuda.synchronize()
    load_s = time.time() - t0
    sig, _ = qwen_image_sigmas(steps, n)
    res = dict(config="qwen_image_1664x928", fp8_linear=fp8[0], mx_fp4=m.engine.mx_fp4, mx_fp6=m.engine.mx_fp6, steps=steps, img_tokens=n, txt_tokens=[120, 6], weights_load_s=round(load_s, 1))
    # one full and one skipped forward (warm-up first)
    t = torch.tensor([0.5], device=DEV)
    for mode in (MM.MC_MODE_FULL, MM.MC_MODE_FULL):
        m._run(lat, pe, t, shapes, [120], mode, 0)
    torch.cuda.synchronize()
    for name, mode in (("full_forward_ms", MM.MC_MODE_FULL), ("skip_forward_ms", MM.MC_MODE_SKIP)):
        t1 = time.time()
        for _ in range(3):
            m._run(lat, pe, t, shapes, [120], mode, 0)
        torch.cuda.synchronize()
        res[name] = round((time.time() - t1) / 3 * 1e3, 2)
    gf, af = flops(m.inner_dim, cfg["num_layers"], n, 120)
    res["full_forward_tflops"] = round((gf + af) / (res["full_forward_ms"] * 1e-3) / 1e12, 1)
    res["fraction_of_bf16_peak"] = round((gf + af) / (res["full_forward_ms"] * 1e-3) / PEAK, 3)
    res["flop_split_gemm_attn"] = [round(gf / (gf + af), 3), round(af / (gf + af), 3)]
    for label, cache in (("no_cache", False), ("magcache_E006K2R02", True)):
        cls = type(m)
        if cache:
            MM.init_qwen_magcache(m, steps, 0.06, 2, 0.2)
        else:
            cls.forward = MM.qwen_plain_forward
        modes = []
        base = cls._run

        def _run(self, *a, _b=base):
            modes.append(a[-2])
            return _b(self, *a)
        cls._run = _run
        torch.cuda.synchronize()
        t1 = time.time()
        x = sample_qwen_image(m, lat, pe, ne, shapes, steps, 4.0, sigmas=sig)
        torch.cuda.synchronize()
        res[label + "_s_per_image"] = round(time.time() - t1, 2)
        res[label + "_skipped"] = sum(int(mo == MM.MC_MODE_SKIP) for mo in modes)
        res[label + "_finite"] = bool(torch.isfinite(x).all())
        cls._run = base
    # the schedule is host arithmetic: the same count from the rule alone
    print(json.dumps(res))


if __name__ == "__main__":
    main()
