#!/usr/bin/env python3
"""A/B measurements of the table forms an engine with token_timestep_sets runs (profiles/r15/TOKEN_SETS.md), one process, the
arms interleaved round by round:

  gemm    gemm_bf16_v2's gated-residual epilogue with a two-valued selector, two-set form (gate / gate2 / sel: the baseline,
          measured twice per round -- arms A1, A2 -- so that the A/A spread of the run is known) against the table form (arm B,
          n_sets = 2 .. 64 over the same two rows), at the TI2V-5B 704 x 1280 x 121f shapes: O (K = 3072) and FFN-2 with the
          residual capture (K = 14336)
  embed   the embed class (MC_PROF_EMBED: patch embedding, distinct-value pass, time chain, text embedding) of mc_embed on a
          default engine (two sets, per-set chain) and on one with token_timestep_sets = 64, same geometry, per-token t
  pass    launch_token_t_sets alone (reference library's mc_test_token_t_sets) at 27 280 and 75 600 tokens with 2, 21, 64 values,
          next to launch_token_t_prepare at 2 values

usage: token_sets_ab.py [gemm] [embed] [pass] [--rounds N] [--json FILE]      (no argument: all three)
Times are device-event times around `reps` back-to-back launches, per launch; medians over the rounds."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

DEV = "cuda:0"
GRID_5B = (31, 44, 80)          # 121 frames of 704 x 1280 through the Wan2.2 VAE (4 x 16 x 16): 27 280 tokens


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def med(v):
    return statistics.median(v)


def gemm_ab(rounds, reps=10):
    import hip_ops as H
    import token_sets_ops as TS
    from magcache_amd import _lib
    lib = _lib.load()
    L = GRID_5B[0] * (GRID_5B[1] // 2) * (GRID_5B[2] // 2)
    M, N = (L + 255) // 256 * 256, 3072
    out = {}
    g = torch.Generator(device=DEV).manual_seed(1)
    for name, K, capture in (("O", 3072, False), ("FFN-2+capture", 14336, True)):
        assert lib.mc_op_gemm_bf16_kernel(M, N, K, 3 if capture else 2) == 4, "the by-shape dispatch should run gemm_bf16_v2 here"
        A = torch.randn(M, K, generator=g, device=DEV).to(torch.bfloat16)
        W = (0.02 * torch.randn(N, K, generator=g, device=DEV)).to(torch.bfloat16)
        bias = torch.randn(N, generator=g, device=DEV)
        X = torch.randn(M, N, generator=g, device=DEV)
        X0 = X.to(torch.bfloat16) if capture else None
        R = torch.empty(M, N, device=DEV) if capture else None
        stride = 30 * 6 * N                                   # the engine's set stride at 30 layers
        table = 0.01 * torch.randn(64 * stride, generator=g, device=DEV)
        sel = torch.zeros(M, dtype=torch.uint8, device=DEV)
        sel[:L // GRID_5B[0]] = 1                             # TI2V: the conditioning frame's tokens take the second set
        g0, g1 = table[:N], table[stride:stride + N]

        def two_set():
            H.check_on(lib, lib.mc_op_gemm_bf16_resid_sel(H.P(A), K, H.P(W), K, H.P(bias), M, N, K, int(capture), H.P(X), N, H.P(g0),
                                                          H.P(g1), H.P(sel), H.P(X0), N, H.P(R), N, H.S()))

        def table_form(n_sets):
            return lambda: H.check_on(lib, TS.gemm_resid_sets(lib, A, W, bias, X, table, stride, n_sets, sel, X0=X0, R=R))
        # same result first (x is updated in place: from equal copies)
        keep = X.clone()
        two_set()
        want = X.clone()
        X.copy_(keep)
        table_form(64)()
        assert torch.equal(X, want), "table form differs from the two-set form"
        arms = {"A1 two-set": two_set, "A2 two-set": two_set, "B table n_sets=2": table_form(2), "B table n_sets=64": table_form(64)}
        for fn in arms.values():
            timed(fn, 3)
        t = {k: [] for k in arms}
        for _ in range(rounds):
            for k, fn in arms.items():
                t[k].append(timed(fn, reps))
        res = {k: med(v) for k, v in t.items()}
        base = 0.5 * (res["A1 two-set"] + res["A2 two-set"])
        res["A/A spread %"] = 100.0 * abs(res["A1 two-set"] - res["A2 two-set"]) / base
        res["round-to-round spread of A1 %"] = 100.0 * (max(t["A1 two-set"]) - min(t["A1 two-set"])) / base
        for k in ("B table n_sets=2", "B table n_sets=64"):
            res[k + " vs A %"] = 100.0 * (res[k] - base) / base
        res["TFLOP/s A"] = 2.0 * M * N * K / (base * 1e-3) / 1e12
        out[f"{name} M={M} N={N} K={K}"] = res
        print(name, json.dumps(res, indent=1), flush=True)
        del A, W, X, X0, R, table
    return out


def embed_ab(rounds, reps=5):
    from magcache_amd import wan22
    from magcache_amd.engine import Engine, synthetic_weights
    cfg = dict(wan22.WAN22_TI2V_5B)
    L = GRID_5B[0] * (GRID_5B[1] // 2) * (GRID_5B[2] // 2)
    engines = {}
    for name, extra in (("default (2 sets)", {}), ("token_timestep_sets=64", {"token_timestep_sets": 64})):
        e = Engine(dict(cfg, no_context_cache=1, **extra), GRID_5B, device=DEV, n_branches=1)
        e.load_weights(synthetic_weights(cfg, seed=0, device=DEV))
        engines[name] = e
    g = torch.Generator(device=DEV).manual_seed(2)
    lat = torch.randn(cfg["in_dim"], *GRID_5B, generator=g, device=DEV)
    ctx = torch.randn(64, cfg["text_dim"], generator=g, device=DEV)
    per_frame = L // GRID_5B[0]
    t2 = torch.full((L,), 937.0, device=DEV)
    t2[:per_frame] = 0.0
    t31 = (torch.linspace(999.0, 0.0, GRID_5B[0], device=DEV)).repeat_interleave(per_frame)
    t1 = torch.tensor([937.0], device=DEV)
    cases = [("default (2 sets)", "two values", t2), ("token_timestep_sets=64", "two values", t2),
             ("token_timestep_sets=64", "31 values", t31), ("default (2 sets)", "scalar t", None),
             ("token_timestep_sets=64", "scalar t", None)]
    res = {f"{en} / {cn}": [] for en, cn, _ in cases}
    launches = {}
    for r in range(rounds + 1):                       # round 0 warms up
        for en, cn, tok in cases:
            e = engines[en]
            e.set_token_timesteps(tok)
            e.profile(2)
            for _ in range(reps):
                e.embed(lat, t1, ctx)
            ms, n = e.profile_read_classes()["embed"]
            e.profile(0)
            if r:
                res[f"{en} / {cn}"].append(ms / reps)
                launches[f"{en} / {cn}"] = n // reps
    out = {k: {"embed class ms (median)": med(v), "min": min(v), "max": max(v), "event pairs per call": launches[k]} for k, v in res.items()}
    out["workspace bytes"] = {k: int(e.lib.mc_workspace_bytes(e.h)) for k, e in engines.items()}
    print(json.dumps(out, indent=1), flush=True)
    return out


def pass_ab(rounds, reps=20):
    import hip_ops as H
    import token_sets_ops as TS
    out = {}
    for n_all in (27280, 75600):
        pad = (n_all + 255) // 256 * 256
        t2, vals = torch.zeros(4, device=DEV), torch.zeros(64, device=DEV)
        sel = torch.zeros(pad, dtype=torch.uint8, device=DEV)
        arms = {}
        for k in (2, 21, 64):
            g = torch.Generator().manual_seed(k)
            t = torch.linspace(999.0, 0.0, k)[torch.randint(0, k, (n_all,), generator=g)].to(DEV)
            arms[f"token_t_sets cap=64, {k} values"] = (
                lambda t=t: TS.TS("token_t_sets", H.P(t), n_all, 0, n_all, pad, 64, H.P(t2), H.P(vals), H.P(sel), H.S()))
            if k == 2:
                arms["token_t_prepare, 2 values"] = lambda t=t: H.token_t_prepare(t, n_all, 0, n_all, pad, t2, sel)
        for fn in arms.values():
            timed(fn, 3)
        ts = {k: [] for k in arms}
        for _ in range(rounds):
            for k, fn in arms.items():
                ts[k].append(1e3 * timed(fn, reps))
        out[f"{n_all} tokens"] = {k: {"us (median)": med(v), "min": min(v), "max": max(v)} for k, v in ts.items()}
    print(json.dumps(out, indent=1), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["gemm", "embed", "pass"])
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("token_sets_ab.py measures on the GPU: no device found")
    out = {}
    for w in a.what:
        out[w] = {"gemm": gemm_ab, "embed": embed_ab, "pass": pass_ab}[w](a.rounds)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
