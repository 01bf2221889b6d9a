"""bench.py -- denoising steps/sec of the MagCache hot path on MI355X (the driver's contract).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

Workload (BASELINE.json configs[1]): Wan2.1-T2V-1.3B, 480p, 81 frames -> latent 16x21x60x104,
L = 32760 tokens; one "step" = cond forward + uncond forward + CFG + scheduler update, MagCache
thresh 0.12, K 4, retention 0.2 (the README command, MagCache4Wan2.1/README.md:13), table
T2V-1.3B resampled to the step count exactly as the reference does (:915-919).  Synthetic latents,
synthetic contexts, random-init weights of the real architecture (no checkpoint offline).
`value` = K / wall time of the timed MagCache region (whole job; N>1 = the same video with the token
sequence sharded over N GPUs, i.e. strong scaling); `ms_per_step` = its wall time / K.  A plain run
does only that.  With --full, a second timed region runs the same K steps with the cache off for
`speedup_vs_nocache` and PSNR, followed by the live per-class kernel times, the back-to-back
per-kernel table, the live PMC pass and the CPU baseline.  --dump-outputs DIR writes the final
latent of the timed region (DIR/latent.npy, fp32, 8.4 MB).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

GRID = (21, 60, 104)
SEQ = 21 * 30 * 52


def flops_forward(cfg, L, Lc=512, ctx_cached=False):
    """model FLOPs of one forward; ctx_cached: the text K / V projections (4 Lc d^2 per layer) are NOT counted -- the
    engine computes them once per prompt (mc_set_context), not per forward"""
    d, f, n = cfg["dim"], cfg["ffn_dim"], cfg["num_layers"]
    per_layer = 8 * L * d * d + 4 * L * L * d + 4 * L * d * d + (0 if ctx_cached else 4 * Lc * d * d) + 4 * L * Lc * d \
        + 4 * L * d * f
    return n * per_layer + 2 * L * 64 * d * 2


def pmc_traffic(kernel):
    """(HBM bytes per launch of `kernel`, file it comes from) from the newest committed PMC pass
    (profiles/rNN/pmc_traffic.json, rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE; counters cannot be read from inside this
    process, so this is a COMMITTED constant, labelled as such in the line).  (None, None) if no such file."""
    import glob
    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*", "pmc_traffic.json")), reverse=True):
        try:
            return json.load(open(f))[kernel]["bytes_per_launch"], os.path.relpath(f, ROOT)
        except (KeyError, ValueError, OSError):
            continue
    return None, None


def pmc_traffic_live(timeout_s=60):
    """HBM bytes per self-attention launch measured NOW: two rocprofv3 --pmc passes (FETCH_SIZE, then WRITE_SIZE -- the TCC
    block cannot hold both in one pass; --kernel-trace only, no other trace domain, as the MI355X guide prescribes) over
    tools/kbench.bin attn1 (the bench's self-attention shape through the C ABI, torch-free) in a child process.  Units: the
    counters are in KiB; FETCH_SIZE is taken at 1.00x -- calibrated on this access pattern in profiles/r01/pmc_traffic.json
    (a 201 MB streaming read in the same pass read 1.00x), not the guide's generic x2.  Returns (bytes, detail dict) or
    (None, reason).  MC_BENCH_PMC=0 skips it."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    if os.environ.get("MC_BENCH_PMC", "1") == "0":
        return None, "MC_BENCH_PMC=0"
    if any(k.startswith(("ROCP_", "ROCPROF", "ROCTRACER")) for k in os.environ):
        return None, "this process is itself running under a profiler"   # (e.g. rocprofv3 --kernel-trace --stats -- python bench.py)
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    kbench = os.path.join(ROOT, "tools", "kbench.bin")
    lib = os.path.join(ROOT, "magcache_amd", "libmagcache_hip.so")
    if not (os.path.exists(prof) and os.path.exists(kbench)):
        return None, "rocprofv3 or tools/kbench.bin missing"
    out = {}
    for ctr in ("FETCH_SIZE", "WRITE_SIZE"):
        d = tempfile.mkdtemp(prefix="mc_pmc_", dir="/tmp")
        try:
            r = subprocess.run([prof, "--kernel-trace", "--pmc", ctr, "--output-format", "csv", "-d", d, "-o", "p", "--",
                                kbench, "attn1", "1", "2", lib], cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"),
                               capture_output=True, text=True, timeout=timeout_s)
            files = glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)
            if r.returncode != 0 or not files:
                return None, f"rocprofv3 --pmc {ctr} failed (rc {r.returncode})"
            tot, n = 0.0, 0
            for row in csv.DictReader(open(files[0])):
                if "attn_fwd_v5_kernel" in row["Kernel_Name"] and row["Counter_Name"] == ctr:
                    tot += float(row["Counter_Value"])
                    n += 1
            if n == 0:
                return None, f"no attn_fwd_v5_kernel rows for {ctr}"
            out[ctr] = (tot / n, n)
        except (subprocess.TimeoutExpired, OSError, KeyError, ValueError) as e:
            return None, f"{ctr}: {type(e).__name__}"
        finally:
            shutil.rmtree(d, ignore_errors=True)
    by = (out["FETCH_SIZE"][0] + out["WRITE_SIZE"][0]) * 1024.0
    return by, {"fetch_kib": out["FETCH_SIZE"][0], "write_kib": out["WRITE_SIZE"][0], "dispatches": out["FETCH_SIZE"][1]}


def timed(fn, sync, barrier):
    barrier()
    sync()
    t0 = time.perf_counter()
    out = fn()
    sync()
    barrier()
    return time.perf_counter() - t0, out


def kernel_rooflines(cfg, device):
    """BACK-TO-BACK per-kernel table (HIP events on the launch stream: torch's current stream is the stream every mc_* call
    is issued on).  The LIVE figures -- the same kernels between the engine's other kernels -- are `roofline` (self-attention
    in the timed no-cache region) and `kernels_live` (every launch class, a separate short region)."""
    import hip_ops as H
    d, heads, ffn = cfg["dim"], cfg["num_heads"], cfg["ffn_dim"]
    Lp = (SEQ + 255) // 256 * 256
    res = {}

    def ev_time(fn):
        """POWER-LIMITED REGIME, by construction: >= 1 s of back-to-back launches of the same kernel first (the package
        settles at its power limit and the clock with it), then 30 hipEvent-bracketed samples of `reps` launches each
        (reps so that a sample is >= ~1 ms); median, minimum and maximum per launch.  (Rounds 1-4 timed 5 launches after
        one warm-up launch, right after the 12 s sustained load of the timed regions: that measured whatever DVFS state
        the box happened to be in, +-27 % between boxes -- VERDICT r04 weak 5.)"""
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n, batch = 0, 8
        while time.perf_counter() - t0 < 1.0:
            tb = time.perf_counter()
            for _ in range(batch):
                fn()
            n += batch
            torch.cuda.synchronize()
            if time.perf_counter() - tb < 0.05:      # keep the queue full: ~50-100 ms of launches per host sync
                batch *= 2
        est = (time.perf_counter() - t0) / n
        reps = max(1, int(round(1e-3 / est)))
        pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(30)]
        for a, b in pairs:
            a.record()
            for _ in range(reps):
                fn()
            b.record()
        torch.cuda.synchronize()
        ts = sorted(a.elapsed_time(b) / reps * 1e-3 for a, b in pairs)
        spread[0] = dict(ms_min=ts[0] * 1e3, ms_max=ts[-1] * 1e3, samples=len(ts), launches_per_sample=reps,
                         preheat_launches=n)
        return ts[len(ts) // 2]

    spread = [None]

    def entry(**kw):
        kw.update(spread[0])
        kw["regime"] = "back to back after a 1 s pre-heat of the same kernel: power-limited regime (median of 30 samples)"
        return kw

    g = torch.Generator(device=device).manual_seed(1)
    qkv = torch.randn(Lp, 3 * d, generator=g, device=device).bfloat16()
    o = torch.empty(Lp, d, dtype=torch.bfloat16, device=device)
    t = ev_time(lambda: H.attention(qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], o, heads, Lp, SEQ, 1, 128 ** -0.5))
    fl = 4.0 * SEQ * SEQ * d
    traffic, traffic_src = pmc_traffic("attn_fwd_v5_kernel")
    # (back-to-back launches of the self-attention kernel: the chip runs them at its power limit, ~7 % slower than between
    # the engine's other kernels; the line's roofline object carries the LIVE figure of the timed region)
    res["attention_back_to_back"] = entry(bound="mfma", achieved=fl / t / 1e12, peak=2500.0, unit="TFLOP/s",
                            frac=fl / t / 2.5e15, traffic=traffic, traffic_source=f"committed PMC pass, not this run: {traffic_src}",
                            ms=t * 1e3, shape=f"L={SEQ} heads={heads} hd=128")
    # cross-attention: the same kernel family on 512 text keys (q = the projected tokens, k|v = the cached context rows)
    Lc = 512
    kv = torch.randn(Lc, 2 * d, generator=g, device=device).bfloat16()
    t = ev_time(lambda: H.attention(qkv[:, :d], kv[:, :d], kv[:, d:], o, heads, Lc, Lc, 1, 128 ** -0.5))
    fl = 4.0 * SEQ * Lc * d
    by = (2 * Lp * d + 2 * Lc * d) * 2.0            # q in, o out, k and v in
    res["attention_cross"] = entry(bound="hbm", achieved=by / t / 1e9, peak=8000.0, unit="GB/s", frac=by / t / 8e12,
                                  mfma_frac=fl / t / 2.5e15, ms=t * 1e3, shape=f"Lq={SEQ} keys={Lc} heads={heads}")
    for name, (N, K, epi) in dict(gemm_qkv=(3 * d, d, 0), gemm_ffn1=(ffn, d, 1), gemm_ffn2=(d, ffn, 2),
                                  gemm_o=(d, d, 2)).items():
        A = torch.randn(Lp, K, generator=g, device=device).bfloat16()
        Wt = (0.02 * torch.randn(N, K, generator=g, device=device)).bfloat16()
        bias = torch.zeros(N, device=device)
        Cb = torch.empty(Lp, N, dtype=torch.bfloat16, device=device) if epi < 2 else None
        X = torch.zeros(Lp, N, device=device) if epi >= 2 else None
        gate = torch.ones(N, device=device) if epi >= 2 else None
        t = ev_time(lambda: H.gemm(A, Wt, bias, epi, Cb=Cb, X=X, gate=gate))
        fl = 2.0 * Lp * N * K
        res[name] = entry(bound="mfma", achieved=fl / t / 1e12, peak=2500.0, unit="TFLOP/s", frac=fl / t / 2.5e15,
                         ms=t * 1e3, shape=f"M={Lp} N={N} K={K}")
        del A, Wt, Cb, X
    # token-wise kernels of a block (HBM bound): LayerNorm + modulate (fp32 in, bf16 out), RMSNorm + RoPE (bf16 in place)
    xs = torch.randn(Lp, d, generator=g, device=device)
    sc, sh = torch.zeros(d, device=device), torch.zeros(d, device=device)
    xn = torch.empty(Lp, d, dtype=torch.bfloat16, device=device)
    t = ev_time(lambda: H.ln_modulate(xs, sc, sh, 0, 1e-6, out_bf16=xn))
    by = Lp * d * 6.0
    res["ln_modulate"] = entry(bound="hbm", achieved=by / t / 1e9, peak=8000.0, unit="GB/s", frac=by / t / 8e12,
                              ms=t * 1e3, shape=f"[{Lp},{d}] fp32 -> bf16")
    cs = H.rope_table(*[gdim // p for gdim, p in zip(GRID, (1, 2, 2))], 0, SEQ).to(device)
    wq = torch.ones(d, device=device)
    t = ev_time(lambda: H.rmsnorm_rope(qkv[:SEQ, :d], wq, 1e-6, cs))
    by = SEQ * d * 4.0 + SEQ * 128 * 4.0
    res["rmsnorm_rope"] = entry(bound="hbm", achieved=by / t / 1e9, peak=8000.0, unit="GB/s", frac=by / t / 8e12,
                               ms=t * 1e3, shape=f"[{SEQ},{d}] bf16 in place + RoPE table")
    del xs, xn
    x0 = torch.randn(SEQ, d, generator=g, device=device).bfloat16()
    r = torch.randn(SEQ, d, generator=g, device=device)
    out = torch.empty(SEQ, d, device=device)
    t = ev_time(lambda: H.skip_add(x0, r, out))
    by = SEQ * d * 10.0
    res["skip_add"] = entry(bound="hbm", achieved=by / t / 1e9, peak=8000.0, unit="GB/s", frac=by / t / 8e12,
                           ms=t * 1e3, shape=f"[{SEQ},{d}] bf16+fp32->fp32")
    # raw op, buffers allocated once (H.calib_stats copies its result to the host: a sync per call)
    from magcache_amd import _lib as L
    lib = L.load()
    part = torch.zeros(4 * 2048 + 1, dtype=torch.float64, device=device)
    sums = torch.empty(4, dtype=torch.float64, device=device)
    stats = torch.empty(3, dtype=torch.float32, device=device)
    t = ev_time(lambda: L.check(lib.mc_op_calib_stats(H.P(r), r.stride(0), H.P(out), out.stride(0), SEQ, d, H.P(part), 2048,
                                                      H.P(sums), H.P(stats), H.S())))
    by = SEQ * d * 8.0
    res["calib_stats"] = entry(bound="hbm", achieved=by / t / 1e9, peak=8000.0, unit="GB/s", frac=by / t / 8e12,
                              ms=t * 1e3, shape=f"2x[{SEQ},{d}] fp32")
    return res


def latent_probe(lat):
    flat = lat.detach().float().reshape(-1)
    idx = torch.linspace(0, flat.numel() - 1, 16, device=flat.device).long()
    return {"l2": float(flat.norm()), "rms": float(flat.pow(2).mean().sqrt()), "samples": [float(v) for v in flat[idx].cpu()]}


def contract_line(args, world, parallelism, t_mc, t_nc, skipped, fl, psnr, probes, skipped_steps):
    """The driver's JSON line from the timed regions' results -- host arithmetic only, so that the CPU suite can check the
    contract on bench.py's OWN assembly code with stubbed timings (tests/test_bench_contract.py).
    t_mc / t_nc: seconds of the MagCache / no-cache region of args.steps steps (max over ranks); skipped: forwards served
    from the residual cache; fl: model FLOPs of one forward."""
    ran = 2 * args.steps - skipped
    line = {
        "metric": "denoising steps/sec (MagCache on), Wan2.1-T2V-1.3B 480p 81f",
        "value": args.steps / t_mc, "unit": "steps/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": t_mc / args.steps * 1e3, "higher_is_better": True,
        "scaling": "strong", "vs_baseline": None,
        "dtype": (f"bf16 + {'MX block-scaled ' if args.fp8_linear >= 2 else ''}fp8(e4m3) {'all six' if args.fp8_linear == 3 else 'QKV/FFN'} Linears (reduced precision: NOT the headline)"
                  if args.fp8_linear else "bf16"),
        "data": "synthetic",
        "config": {"workload": "Wan2.1-T2V-1.3B 832x480 81 frames: latent 16x21x60x104, 32760 tokens, "
                               "30 layers d=1536 12 heads ffn=8960; cond+uncond per step, CFG 5.0, flow-Euler; "
                               "synthetic latents/contexts, random-init weights",
                   "magcache_thresh": args.magcache_thresh, "magcache_K": args.magcache_K,
                   "retention_ratio": args.retention_ratio, "sampling_steps": args.steps,
                   "parallelism": parallelism},
        "forwards_skipped": skipped, "forwards_total": 2 * args.steps,
        "speedup_bound": (2 * args.steps) / max(ran, 1),
        "speedup_note": "bound = forwards total / forwards run, for equal forward times in both timed regions; the measured ratio "
                        "can pass it by a few 1e-4 (the no-cache region carries the hipEvent pairs and runs second)",
        "nocache_steps_per_s": (args.steps / t_nc) if t_nc else None,
        "speedup_vs_nocache": (t_nc / t_mc) if t_nc else None,
        "psnr_vs_nocache_db": psnr,
        # step indices whose cond / uncond forward was served from the residual cache (BASELINE.md section 2 lists the
        # reference's for 50 steps); None at N > 1 with the CFG branches on different ranks
        "skipped_steps": skipped_steps,
        # fingerprints of the final latents (identical seeds => an N-rank run must reproduce the single-GPU values up to
        # the bf16 rounding of the partial attention results): l2 norm + 16 values at fixed flat indices
        "final_latent_probe": probes,
        "lpips_vs_nocache": "unavailable offline (magcache_amd.metrics.LPIPSAlex needs AlexNet + lpips weights, none ship "
                            "here; it raises rather than invent a number)",
        "model_tflops_per_s_nocache": (2 * args.steps * fl / t_nc / 1e12 / world) if t_nc else None,
        "model_tflops_per_s_magcache_ran": ran * fl / t_mc / 1e12 / world,
        "model_flops_note": "per forward, text K/V projections excluded (cached per prompt by mc_set_context)",
    }
    return line


def kernels_live(cfg, steps, wall_s, classes, sp=1, fwd_per_step=2):
    """Per-class LIVE kernel times of `steps` no-cache steps: hipEvent pairs around every launch class inside the engine
    (mc_profile_read_classes).  ms = average per event pair; frac against the class's bound (algorithmic FLOPs / bytes, no
    padding); the last three fields reconcile the sum of the classes with the wall time of a forward.
    N > 1 (rank 0's view): sp = ranks sharing the token axis -- this rank's rows are SEQ / sp; its self-attention is 1 + R
    pairs per layer (local shard + one per gather round) and its q|k|v Linear two (k|v first, then q), so the MFMA classes are
    rated per LAYER (summed time of the class / layers run) --, fwd_per_step = forwards this rank runs per step (1 when the
    CFG branches sit on two halves of the node)."""
    d, ffn, nl = cfg["dim"], cfg["ffn_dim"], cfg["num_layers"]
    fwd = fwd_per_step * steps
    Lr = SEQ / sp
    fl = {"attn_self": 4.0 * Lr * SEQ * d, "gemm_qkv": 2.0 * Lr * 3 * d * d, "gemm_o": 2.0 * Lr * d * d,
          "gemm_cross_q": 2.0 * Lr * d * d, "gemm_cross_o": 2.0 * Lr * d * d, "gemm_ffn1": 2.0 * Lr * ffn * d,
          "gemm_ffn2": 2.0 * Lr * ffn * d}
    by = {"attn_cross": (2 * Lr * d + 2 * 512 * d) * 2.0, "ln_modulate": Lr * d * 6.0}
    out, total = {}, 0.0
    for name, (ms, n) in classes.items():
        if n == 0:
            continue
        if name != "sp_wait":          # the waits for gather rounds lie INSIDE the attention chain's pair (mc_prof_class)
            total += ms
        ent = {"ms": ms / n, "pairs": n, "ms_per_forward": ms / fwd}
        t = ms / n * 1e-3
        if name in fl:
            t = ms / (fwd * nl) * 1e-3          # per layer (== per pair on one GPU)
            ent.update(bound="mfma", achieved=fl[name] / t / 1e12, unit="TFLOP/s", frac=fl[name] / t / 2.5e15,
                       ms_per_layer=t * 1e3)
        elif name in by:
            ent.update(bound="hbm", achieved=by[name] / t / 1e9, unit="GB/s", frac=by[name] / t / 8e12)
        out[name] = ent
    gemm_ms = sum(classes[c][0] for c in fl if c.startswith("gemm"))
    gemm_fl = sum(fl[c] * fwd * nl for c in fl if c.startswith("gemm") and classes[c][1])
    return {"measured": f"{steps} no-cache steps ({fwd} forwards x {nl} layers{', rank 0 of sp ' + str(sp) if sp > 1 or fwd_per_step == 1 else ''}) after the timed regions, hipEvent pairs around "
                        "every launch class on the launch stream (mc_profile_enable level 2); 'pairs' that cover several "
                        "launches: rmsnorm_rope in front of the self-attention (q and k), embed, head",
            "classes": out,
            "gemm_aggregate": {"ms_per_forward": gemm_ms / fwd, "achieved": gemm_fl / max(gemm_ms, 1e-9) / 1e9,
                               "unit": "TFLOP/s", "frac": gemm_fl / max(gemm_ms, 1e-9) / 1e9 / 2500.0},
            "sum_classes_ms_per_forward": total / fwd, "wall_ms_per_forward": wall_s * 1e3 / fwd,
            "unaccounted_frac": 1.0 - total / (wall_s * 1e3)}


def cpu_baseline(cfg, max_threads):
    """The oracle (PyTorch CPU restatement, bf16 autocast = the reference's execution mode) timed on this box's host
    cores, following SURVEY 8(d): after a warm-up, (a) ONE block at the full L = 32 760 -- everything but the attention
    core measured at full length, the attention core on a 2 048-query slice against all 32 760 keys and scaled by
    L / 2 048 (it is linear in the query count) -- and (b) the whole 30-layer forward at L = 3 120 (5 latent frames).
    The thread count is the best of {8, 32, 64, all} on a bf16 F.linear probe of the FFN-1 shape.  The full-size
    forward is extrapolated from (a): 30 x (t_rest + t_attention); (b) is reported next to it as a cross-check of the
    per-layer model at small L."""
    import torch.nn.functional as F
    from oracle import wan_dit_ref as W
    d, ffn, heads = cfg["dim"], cfg["ffn_dim"], cfg["num_heads"]
    t_begin = time.perf_counter()

    # ---- thread sweep on a GEMM probe (bf16 F.linear, M = 3120, the FFN-1 shape): 2*M*N*K = 86 GFLOP
    xa = torch.randn(3120, d).bfloat16()
    wa = torch.randn(ffn, d).bfloat16()
    probe = {}
    for th in sorted({min(t, max_threads) for t in (8, 32, 64, max_threads)}):
        torch.set_num_threads(th)
        F.linear(xa, wa)
        t0 = time.perf_counter()
        for _ in range(3):
            F.linear(xa, wa)
        probe[th] = 3 * 2.0 * 3120 * ffn * d / (time.perf_counter() - t0) / 1e12
    threads = max(probe, key=probe.get)
    torch.set_num_threads(threads)

    g = torch.Generator().manual_seed(42)
    ctx = torch.randn(512, cfg["text_dim"], generator=g)
    tt = torch.tensor([500.0])

    # ---- (b) 30 layers at L = 3120, warm-up = the same model on a 1-frame latent
    grid_s = (2, 60, 104)
    Ls = grid_s[0] * 30 * 52
    # one block is initialised and COPIED into the other 29 (distinct memory, same values: CPU time does not depend on
    # the values, and drawing 1.4 G parameters on the host would cost more than the measurement)
    import copy
    oracle = W.init_synthetic_(W.WanModel(**dict(cfg, num_layers=1)), seed=0)
    oracle.blocks = torch.nn.ModuleList([oracle.blocks[0]] + [copy.deepcopy(oracle.blocks[0])
                                                              for _ in range(cfg["num_layers"] - 1)])
    oracle.forward([torch.randn(16, 1, 16, 16, generator=g)], tt, [ctx], 64, autocast=True)     # warm-up
    t0 = time.perf_counter()
    oracle.forward([torch.randn(16, *grid_s, generator=g)], tt, [ctx], Ls, autocast=True)
    t_b = time.perf_counter() - t0
    f_b = flops_forward(cfg, Ls)

    # ---- (a) one block at full L
    blk = oracle.blocks[0]
    lat = torch.randn(16, *GRID, generator=g)
    with torch.no_grad(), torch.autocast("cpu", dtype=torch.bfloat16):
        x, e, kw = oracle.embed([lat], tt, [ctx], SEQ)
        real_attention = W.attention_ref
        try:
            # everything but the self-attention core (cross-attention keeps its 512-key attention)
            W.attention_ref = lambda q, k, v, k_lens=None: v if k.size(1) == q.size(1) else real_attention(q, k, v, k_lens)
            t0 = time.perf_counter()
            blk(x, **kw)
            t_rest = time.perf_counter() - t0
        finally:
            W.attention_ref = real_attention
        nq = 2048
        q = torch.randn(1, nq, heads, 128, generator=g).bfloat16()
        k = torch.randn(1, SEQ, heads, 128, generator=g).bfloat16()
        v = torch.randn(1, SEQ, heads, 128, generator=g).bfloat16()
        W.attention_ref(q[:, :256], k, v)                                                       # warm-up
        t0 = time.perf_counter()
        W.attention_ref(q, k, v)
        t_attn_s = time.perf_counter() - t0
    t_attn = t_attn_s * SEQ / nq
    f_attn = 4.0 * SEQ * SEQ * d
    f_layer = flops_forward(dict(cfg, num_layers=1), SEQ) - 2 * SEQ * 64 * d * 2
    f_rest = f_layer - f_attn
    t_full = cfg["num_layers"] * (t_rest + t_attn)
    f_full = flops_forward(cfg, SEQ)
    return dict(value=1.0 / (2 * t_full), unit="denoising steps/s (no cache)", cores=threads, kind="port",
                sample=(f"(a) one oracle block at L={SEQ}: all but the self-attention core {t_rest:.1f} s "
                        f"({f_rest / t_rest / 1e12:.2f} TFLOP/s), attention core on {nq} of {SEQ} query rows "
                        f"{t_attn_s:.1f} s -> {t_attn:.1f} s per layer ({f_attn / t_attn / 1e12:.2f} TFLOP/s); "
                        f"(b) the {cfg['num_layers']}-layer forward at L={Ls}: {t_b:.1f} s ({f_b / t_b / 1e12:.2f} TFLOP/s); "
                        f"full-size forward = {cfg['num_layers']} x (a) = {t_full:.0f} s ({f_full / t_full / 1e12:.2f} TFLOP/s); "
                        f"bf16 F.linear probe {probe[threads]:.2f} TFLOP/s on {threads} threads"),
                threads_probe_tflops={str(k): round(v, 3) for k, v in probe.items()},
                seconds_measured=time.perf_counter() - t_begin,
                block_full_L=dict(rest_s=t_rest, attention_s=t_attn, attention_sampled_s=t_attn_s, query_rows=nq),
                forward_small_L=dict(tokens=Ls, seconds=t_b, tflops=f_b / t_b / 1e12),
                seconds_per_forward_extrapolated=t_full)


def engine_bytes_estimate(cfg, sp_size=1):
    """HBM one engine needs on a rank, from the geometry (an upper estimate, +10 %): weights are replicated (bf16 Linears, an
    e4m3 copy of the quantised ones with fp8_linear), the workspace holds this rank's L / sp_size tokens (DESIGN section 2's
    table: x fp32, x0 / xn / ao bf16, qkv, h, two residual slots fp32) plus the K|V gather buffer of the whole sequence."""
    d, f, n = cfg["dim"], cfg["ffn_dim"], cfg["num_layers"]
    lin = n * (8 * d * d + 2 * d * f)
    weights = lin * (2 + (1 if cfg.get("fp8_linear") else 0)) + 4 * cfg["text_dim"] * d
    lp = (SEQ // sp_size + 255) // 256 * 256
    ws = lp * (4 * d + 3 * 2 * d + 2 * 3 * d + 2 * f + 2 * 4 * d) + (sp_size * lp * 2 * d * 2 if sp_size > 1 else 0)
    ws += 2 * n * 512 * 2 * d * 2                  # text K|V cache of two prompts
    return 1.1 * (weights + ws)


STAGE = ["start"]        # where a failure happened (reported in the error line of a multi-GPU run)
STAGE_T = [0.0]          # when it was entered (the watchdog of a multi-GPU run)


def stage(name):
    import time
    STAGE[0] = name
    STAGE_T[0] = time.time()


def start_watchdog(world, rank):
    """N > 1: a collective that never completes (a rank that died, a communicator that deadlocks) blocks the main thread in a
    device synchronisation for ever -- torch.distributed's own timeout covers its process group, not the library-side RCCL
    communicator.  A daemon thread ends the run with the ONE parseable JSON line (rank 0) when a stage has not advanced for
    MC_BENCH_STAGE_TIMEOUT_S seconds (default 900), so that the driver gets a reason instead of its own kill."""
    import threading
    import time
    limit = float(os.environ.get("MC_BENCH_STAGE_TIMEOUT_S", "900"))
    stage(STAGE[0])

    def watch():
        while True:
            time.sleep(5.0)
            if time.time() - STAGE_T[0] > limit:
                if rank == 0:
                    print(json.dumps({"metric": "denoising steps/sec (MagCache on), Wan2.1-T2V-1.3B 480p 81f", "value": None,
                                      "unit": "steps/s", "n_gpus": world, "higher_is_better": True, "scaling": "strong",
                                      "error": f"stage '{STAGE[0]}' did not finish within {limit:.0f} s (watchdog: a collective "
                                               "that never completed?)", "stage": STAGE[0]}), flush=True)
                else:
                    sys.stderr.write(f"[rank {rank}] watchdog: stage '{STAGE[0]}' exceeded {limit:.0f} s\n")
                os._exit(3)
    threading.Thread(target=watch, daemon=True).start()


def main():
    """N > 1: every failure -- an exception in any self-check, a collective that times out (3 minutes, set at
    init_process_group), a layout that does not fit -- ends in ONE parseable JSON line from rank 0 with "value": null,
    "error" and "stage" instead of a traceback only (the scaling run is the first time this code meets more than one GPU)."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    if world == 1:
        return bench_main()
    start_watchdog(world, rank)
    try:
        return bench_main()
    except BaseException as e:   # noqa: BLE001  (SystemExit from argparse included: the line is the contract)
        import traceback
        if isinstance(e, SystemExit) and not e.code:
            raise                                   # --help and other clean exits are not failures
        if rank == 0:
            print(json.dumps({"metric": "denoising steps/sec (MagCache on), Wan2.1-T2V-1.3B 480p 81f", "value": None,
                              "unit": "steps/s", "n_gpus": world, "higher_is_better": True, "scaling": "strong",
                              "error": f"{type(e).__name__}: {e}"[:2000], "stage": STAGE[0],
                              "traceback_tail": traceback.format_exc()[-1500:]}), flush=True)
        else:
            sys.stderr.write(f"[rank {rank}] failed at stage {STAGE[0]}: {type(e).__name__}: {e}\n")
        try:
            if dist.is_initialized():
                dist.destroy_process_group()
        except Exception:
            pass
        raise SystemExit(1 if not isinstance(e, SystemExit) else e.code)


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--magcache_thresh", type=float, default=0.12)
    ap.add_argument("--magcache_K", type=int, default=4)
    ap.add_argument("--retention_ratio", type=float, default=0.2)
    ap.add_argument("--guide_scale", type=float, default=5.0)
    ap.add_argument("--shift", type=float, default=5.0)
    ap.add_argument("--full", action="store_true",
                    help="also run what the headline does not need: the second (cache off) timed region (speed-up, PSNR), "
                         "the live per-class kernel times, the back-to-back per-kernel table, the live PMC pass and the CPU "
                         "baseline; the --no_* flags below drop single parts of it")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the final latent of the timed MagCache region (what sample() returns) as DIR/latent.npy, fp32")
    ap.add_argument("--no_cpu_baseline", action="store_true")
    ap.add_argument("--no_kernels", action="store_true")
    ap.add_argument("--no_nocache", action="store_true", help="skip the second (cache off) timed region")
    ap.add_argument("--no_table", action="store_true", help="skip the back-to-back per-kernel table (1 s pre-heat per kernel)")
    ap.add_argument("--fp8_linear", type=int, nargs="?", const=1, default=0, choices=(0, 1, 2, 3),
                    help="OPTIONAL precision mode, never the headline: QKV / FFN Linears on an fp8 e4m3 MFMA path "
                         "(1: per-row / per-channel scales, 2: MX block scales, 3: MX for the d x d Linears of a block too)")
    ap.add_argument("--layout", choices=("auto", "sp", "cfg2sp"), default="auto",
                    help="N > 1: 'sp' = the token sequence sharded over all N ranks, one K/V all-gather per layer "
                         "(north_star's split); 'cfg2sp' = CFG branches on two halves of the node x sequence parallel "
                         "inside a half (SURVEY 8e's alternative); 'auto' = both are timed on 2 no-cache steps before "
                         "the timed region (reported as layout_ablation) and the faster one runs the benchmark")
    ap.add_argument("--no_cfg_parallel", action="store_true", help="same as --layout sp")
    return ap


def bench_main():
    args = build_parser().parse_args()
    if args.no_cfg_parallel:
        args.layout = "sp"
    if not args.full:
        # a plain run is repeated for every change: set-up, warm-up, the timed MagCache region, the line
        args.no_nocache = args.no_kernels = args.no_table = args.no_cpu_baseline = True

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"
    backend = os.environ.get("MC_BENCH_BACKEND", "nccl")   # tests: "gloo" runs N ranks on ONE GPU
    if not torch.cuda.is_available():
        raise SystemExit("bench.py measures the HIP path on an MI355X: no GPU is visible here (there is no CPU fallback)")
    local = local % torch.cuda.device_count()
    torch.cuda.set_device(local)
    device = f"cuda:{local}"

    from magcache_amd import model as M
    from magcache_amd import parallel as PAR
    from magcache_amd.engine import WAN_T2V_1_3B, synthetic_weights
    from magcache_amd.mag_ratios import TABLES
    from magcache_amd.sampler import sample

    cfg = dict(WAN_T2V_1_3B, fp8_linear=args.fp8_linear) if args.fp8_linear else WAN_T2V_1_3B
    g = torch.Generator(device=device).manual_seed(42)
    noise = torch.randn(16, *GRID, generator=g, device=device)
    ctx = torch.randn(512, cfg["text_dim"], generator=g, device=device)
    ctx_null = torch.randn(512, cfg["text_dim"], generator=g, device=device)
    sync = torch.cuda.synchronize
    # MC_BENCH_FORCE_DIST=1 (tests/test_rccl_gpu.py): create the communicator at world size 1 too, so that the N > 1
    # code around the timed regions (init on the device, all-reduce, barrier, teardown) runs on RCCL on a one-GPU box
    force_dist = world == 1 and os.environ.get("MC_BENCH_FORCE_DIST") == "1"
    # MC_BENCH_FORCE_SP=1 (with FORCE_DIST): the WHOLE N > 1 flow on one GPU -- layout, a sharded engine (mc_config.sp_phases:
    # the sequence-parallel phase path with a world of one), the start-up self-check, the library-side RCCL communicator and
    # one mc_forward_sp_rccl per forward, the N > 1 report -- so that none of it meets a GPU for the first time on 8 of them
    force_sp = force_dist and os.environ.get("MC_BENCH_FORCE_SP") == "1"
    multi = world > 1 or force_sp
    barrier = (lambda: dist.barrier()) if (world > 1 or force_dist) else (lambda: None)

    def make_model(layout, tag):
        cls = type("WanModelHIP_" + tag, (M.WanModelHIP,), {})     # MagCache state lives on the class: one per layout
        m = cls(cfg, GRID, device=device, calibration=False, sp_rank=layout.sp_rank if layout else 0,
                sp_size=layout.sp_size if layout else 1, sp_group=layout.sp_group if layout else None, sp_phases=force_sp)
        m.engine.load_weights(synthetic_weights(cfg, seed=0, device=device))
        return m

    def run(model, layout, steps):
        return sample(model, noise, ctx, ctx_null, sampling_steps=steps, shift=args.shift,
                      guide_scale=args.guide_scale, layout=layout)

    def max_over_ranks(x):
        if world == 1:
            return x
        tt = torch.tensor([x], device=device, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        return float(tt[0])

    layout, extra = None, {}
    if force_dist:
        dist.init_process_group(backend, device_id=torch.device(device)) if backend == "nccl" else dist.init_process_group(backend)
        ones = torch.ones(1, device=device)
        dist.all_reduce(ones)
        extra["rccl_world"] = int(ones[0])
        extra["comm_backend"] = dist.get_backend()
    if world > 1:
        import datetime
        stage("init_process_group")
        tmo = datetime.timedelta(seconds=int(os.environ.get("MC_BENCH_COLLECTIVE_TIMEOUT_S", "180")))
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device(device), timeout=tmo)
        else:
            dist.init_process_group(backend, timeout=tmo)
        stage("first all-reduce")
        # how many ranks really joined the communicator (an all-reduce of ones on the data-path backend)
        ones = torch.ones(1, device=device)
        dist.all_reduce(ones)
        extra["rccl_world"] = int(ones[0])
        extra["comm_backend"] = dist.get_backend()
    if multi:
        names = ["sp"] + (["cfg2sp"] if world % 2 == 0 else [])
        if args.layout != "auto":
            assert args.layout in names, f"--layout {args.layout} needs an even number of ranks"
            names = [args.layout]
        stage("process groups")
        layouts = {n: PAR.ParallelLayout(cfg_parallel=(n == "cfg2sp")) for n in names}   # every rank builds every group
        free_b, total_b = torch.cuda.mem_get_info()
        extra["hbm_free_gb_at_start"] = round(free_b / 1e9, 1)
        # ONE engine at a time (round 5 built one per candidate layout and kept them all until the ablation had chosen: twice
        # the ways to fail before a single number exists): build a candidate, check it, time it, drop it before the next
        need_b = max(engine_bytes_estimate(cfg, layouts[n].sp_size) for n in names)
        if free_b < need_b:
            raise RuntimeError(f"the engine needs ~{need_b / 1e9:.0f} GB, {free_b / 1e9:.1f} GB free of {total_b / 1e9:.0f} GB")

        def selfcheck(model, name):
            """sequence-parallel self-check: the overlapped forward (q Linear, local-shard attention and the attention over
            landed rounds beside the chunked K/V all-gather) must agree with the serialised one; otherwise run without"""
            stage(f"sequence-parallel self-check ({name})")
            m = M.disable_magcache(model)
            tt = torch.tensor([500.0], device=device)
            saved = PAR.SP_OVERLAP
            outs = []
            for ov in (True, False):
                PAR.SP_OVERLAP = ov
                outs.append(m([noise], t=tt, context=[ctx], seq_len=SEQ)[0].clone())
            PAR.SP_OVERLAP = saved
            rel = float((outs[0] - outs[1]).norm() / outs[1].norm().clamp_min(1e-30))
            rel = max_over_ranks(rel if rel == rel else float("inf"))
            extra["sp_selfcheck_rel"] = rel
            if not (rel <= 3e-3):
                PAR.SP_OVERLAP = False
            extra["sp_overlap"] = bool(PAR.SP_OVERLAP)
            sp = getattr(model, "_sp", None)
            extra["sp_chunks"] = getattr(sp, "C", None)          # rounds of the per-layer K|V all-gather
            extra["sp_rounds"] = getattr(sp, "R", None)          # ... of which carry valid keys
            extra["sp_collective"] = ("RCCL communicator inside the library (mc_forward_sp_rccl: one C call per forward): "
                                      + model.engine.rccl_info(sp.rccl)) if getattr(sp, "rccl", None) is not None else \
                "torch.distributed from the gather callback of mc_blocks_sp (" + str(dist.get_backend()) + ")" + \
                (f"; the library-side communicator was not used: {sp.rccl_error}" if getattr(sp, "rccl_error", None) else "")

        model, built, abl, m = None, None, {}, None
        for n in names:
            if model is not None:
                m = None                 # (the ablation's alias of the same object)
                del model
                torch.cuda.empty_cache()
            stage(f"build engine ({n})")
            model, built = make_model(layouts[n], n), n
            if (layouts[n].sp_size > 1 or force_sp) and "sp_selfcheck_rel" not in extra:
                selfcheck(model, n)
            if len(names) > 1:
                # ---- layout ablation: 2 no-cache steps of every candidate after 1 untimed step; the faster one is benchmarked
                stage(f"layout ablation ({n})")
                m = M.disable_magcache(model)
                k_abl = max(1, int(os.environ.get("MC_BENCH_ABLATION_STEPS", "2")))     # (the one-GPU multi-rank tests: 1)
                run(m, layouts[n], 1)
                dt, _ = timed(lambda: run(m, layouts[n], k_abl), sync, barrier)
                abl[n] = k_abl / max_over_ranks(dt)
        if len(names) > 1:
            extra["layout_ablation_nocache_steps_per_s"] = abl
            chosen = max(abl, key=abl.get)
            ch = torch.tensor([names.index(chosen)], device=device)
            dist.broadcast(ch, 0)                       # identical choice on every rank
            chosen = names[int(ch[0])]
        else:
            chosen = names[0]
        layout = layouts[chosen]
        if built != chosen:
            m = None
            del model
            torch.cuda.empty_cache()
            stage(f"build engine ({chosen}, chosen)")
            model = make_model(layout, chosen)
        extra["layout"] = chosen
    else:
        model = make_model(None, "single")

    M.disable_magcache(model)
    stage("warm-up")
    if args.warmup > 0:
        run(model, layout, args.warmup)
    stage("timed region 1 (MagCache)")
    # ---- timed region 1: K steps with MagCache
    M.init_magcache(model, args.steps, args.magcache_thresh, args.magcache_K, args.retention_ratio,
                    mag_ratios=TABLES["wan2.1_t2v_1.3B"])
    modes = []
    fwd = model._run
    model._run = lambda x, t, c, branch, mode: (modes.append(mode), fwd(x, t, c, branch, mode))[1]
    t_mc, lat_mc = timed(lambda: run(model, layout, args.steps), sync, barrier)
    model._run = fwd
    skipped = int(sum(1 for m in modes if m == 1))
    # the sampler calls cond then uncond in every step on a rank that evaluates both branches
    skipped_steps = None
    if layout is None or layout.cfg_size == 1:
        skipped_steps = {"cond": [i // 2 for i, m in enumerate(modes) if m == 1 and i % 2 == 0],
                         "uncond": [i // 2 for i, m in enumerate(modes) if m == 1 and i % 2 == 1]}
    if world > 1:
        # one count per CFG branch / per job: the first rank of every sequence-parallel group reports
        first = layout.sp_rank == 0 and (layout.cfg_size == 2 or rank == 0)
        cnt = torch.tensor([skipped if first else 0], device=device, dtype=torch.int64)
        dist.all_reduce(cnt)
        skipped = int(cnt[0])
    if args.dump_outputs and rank == 0:
        # every rank holds the same replica of the latent; fixed seeds make it comparable between two builds
        stage("dump outputs")
        os.makedirs(args.dump_outputs, exist_ok=True)
        np.save(os.path.join(args.dump_outputs, "latent.npy"), lat_mc.float().cpu().numpy())
    # ---- timed region 2: the same K steps with the cache off
    t_nc, psnr, attn_live = None, None, None
    stage("timed region 2 (no cache)")
    if not args.no_nocache:
        M.disable_magcache(model)
        # hipEvent pairs around every self-attention launch of THIS timed region, on the launch stream
        model.engine.profile(True)
        t_nc, lat_nc = timed(lambda: run(model, layout, args.steps), sync, barrier)
        attn_live = model.engine.profile_read()
        model.engine.profile(False)
        mse = float(((lat_mc - lat_nc) ** 2).mean())
        rng = float(lat_nc.abs().max())
        psnr = 100.0 if mse < 1e-10 else float(20 * np.log10(rng / np.sqrt(mse)))
    # ---- third region (not part of any reported rate): a few no-cache steps with a hipEvent pair around EVERY launch class
    # of the forward (mc_profile_enable level 2), so that the GEMMs -- 30 % of forward time -- have a LIVE figure like the
    # self-attention kernel has.  Kept out of region 2 so that `nocache_steps_per_s` stays comparable with rounds 1-4
    # (~14 pairs per layer instead of one).
    live = None
    if not args.no_nocache and not args.no_kernels:     # (N > 1: every rank runs the region -- it holds collectives --, rank 0 reports)
        stage("live kernel classes")
        ls = max(1, min(args.steps, 3))
        model.engine.profile(2)
        t_lv, _ = timed(lambda: run(model, layout, ls), sync, barrier)
        live = (ls, t_lv, model.engine.profile_read_classes())
        model.engine.profile(False)
    if world > 1:
        t_mc = max_over_ranks(t_mc)
        t_nc = max_over_ranks(t_nc) if t_nc is not None else None

    stage("report")
    if rank == 0:
        # the shim caches the text context per prompt (mc_set_context): its K / V projections are not in the forwards
        fl = flops_forward(cfg, SEQ, ctx_cached=True)
        line = contract_line(args, world, layout.describe() if multi else "single GPU", t_mc, t_nc, skipped, fl, psnr,
                             {"magcache": latent_probe(lat_mc), "nocache": latent_probe(lat_nc) if t_nc else None},
                             skipped_steps)
        line.update(extra)
        if not multi and not args.no_kernels:
            if args.no_table:        # (A/B runs: tools/live_ab.sh) only the live figures
                tr, tr_src = pmc_traffic("attn_fwd_v5_kernel")
                k = {"attention_back_to_back": dict(bound="mfma", achieved=None, peak=2500.0, unit="TFLOP/s", frac=None, traffic=tr,
                                                    traffic_source=f"committed PMC pass, not this run: {tr_src}")}
            else:
                k = kernel_rooflines(cfg, device)
            line["roofline"] = {kk: k["attention_back_to_back"][kk] for kk in ("bound", "achieved", "peak", "unit", "frac", "traffic",
                                                                  "traffic_source")}
            if attn_live and attn_live[1] > 0:
                # the dominant kernel's average launch duration inside the timed (no-cache) region: algorithmic
                # FLOPs per launch = 4 L^2 d (attention core, no padding, no recompute)
                ms = attn_live[0] / attn_live[1]
                fl_attn = 4.0 * SEQ * SEQ * cfg["dim"]
                line["roofline"].update(achieved=fl_attn / (ms * 1e-3) / 1e12, frac=fl_attn / (ms * 1e-3) / 2.5e15,
                                        avg_launch_ms=ms, launches=attn_live[1],
                                        measured="hipEvent pairs around every self-attention launch of the timed "
                                                 "no-cache region (mc_profile_read)")
            line["roofline"]["kernel"] = "attn_fwd_v5_kernel (self-attention, 71% of forward FLOPs)"
            by, detail = pmc_traffic_live()
            if by is not None:
                line["roofline"].update(traffic=by, traffic_detail=detail, traffic_source=(
                    "measured in this run: rocprofv3 --kernel-trace --pmc FETCH_SIZE / WRITE_SIZE (one pass each) over "
                    "tools/kbench.bin attn1 in a child process, KiB x 1024, FETCH_SIZE at the 1.00x calibrated in "
                    "profiles/r01/pmc_traffic.json; algorithmic bytes 402653184"))
            else:
                line["roofline"]["traffic_source"] += f" (live PMC pass unavailable: {detail})"
            if not args.no_table:
                line["kernels"] = k
            if live:
                line["kernels_live"] = kernels_live(cfg, *live)
        if multi and live:
            # rank 0's launch classes.  The K|V all-gather runs on RCCL's own stream and is in no class; what the launch stream
            # IDLED waiting for a gather round is class "sp_wait" (hipEvent pairs around every wait): the exposed
            # communication, the first thing to read in an N-GPU profile
            fps = 1 if layout.cfg_size == 2 else 2
            line["kernels_live_rank0"] = kernels_live(cfg, *live, sp=layout.sp_size, fwd_per_step=fps)
            w_ms, w_n = live[2].get("sp_wait", (0.0, 0))
            if w_n:
                nl = cfg["num_layers"]
                line["sp_gather_wait"] = {"ms_per_layer": w_ms / (fps * live[0] * nl), "ms_per_forward": w_ms / (fps * live[0]),
                                          "waits_per_layer": w_n / (fps * live[0] * nl),
                                          "frac_of_forward_wall": w_ms / (live[1] * 1e3),
                                          "measured": "rank 0, hipEvent pairs on the launch stream around every wait for a "
                                                      "K|V gather round (MC_PROF_SP_WAIT): time the stream idled for the "
                                                      "collective = exposed communication"}
        if multi and attn_live and attn_live[1] > 0:
            # N > 1: rank 0's self-attention launches of the timed no-cache region (cfg2: one full-sequence launch per
            # layer; sequence parallel: local-shard launch + one per gather round per layer), algorithmic FLOPs of its share
            sp = layout.sp_size
            pairs = (1 if layout.cfg_size == 2 else 2) * args.steps * cfg["num_layers"]     # layers this rank ran
            fl_attn = 4.0 * (SEQ / sp) * SEQ * cfg["dim"] * pairs
            rate = fl_attn / (attn_live[0] * 1e-3)
            line["roofline"] = {"bound": "mfma", "achieved": rate / 1e12, "peak": 2500.0, "unit": "TFLOP/s",
                                "frac": rate / 2.5e15, "traffic": None, "launches": attn_live[1],
                                "avg_launch_ms": attn_live[0] / attn_live[1],
                                "measured": "rank 0, hipEvent pairs on the launch stream around every layer's self-attention of the "
                                            "timed no-cache region (sequence parallel: ONE pair around the whole chain -- local "
                                            "shard + gather rounds on two streams + merge --, stalls for the gather included); "
                                            "per-GPU rate",
                                "kernel": "self-attention, attn_fwd_v5_kernel (32x32x16 lazy / pipelined stream) for every form of "
                                          "the call: one key shard, and the sequence-parallel local-shard + per-round "
                                          "launches with the log-sum-exp merge"}
        if not multi and not args.no_cpu_baseline:
            line["cpu_baseline"] = cpu_baseline(cfg, os.cpu_count() or 1)
        print(json.dumps(line), flush=True)
    if world > 1 or force_dist:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
