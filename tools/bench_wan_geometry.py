"""One Wan engine over several latent grids (Engine.set_geometry) against one engine per grid.

    python tools/bench_wan_geometry.py 21x60x104 21x90x160                 # Wan2.1-T2V-1.3B, 81 frames at 480p and 720p
    python tools/bench_wan_geometry.py 21x60x104 21x90x160 --cfg 14b --layers 4

GRID = FxHxW of the VAE latent.  Prints one JSON line:
  create_load_s            mc_create + the weight load of an engine: what a second engine costs without set_geometry
  switch_without_reserve   per grid the set_geometry wall time on an engine created at the smallest grid (a larger plan
                           allocates a larger workspace first)
  per_grid                 with the workspace reserved for every grid: the set_geometry wall time; the full-forward time of
                           the switched engine against a fresh engine of that grid in alternating windows (the fresh
                           engine's window-to-window spread is the yardstick for "the same"); whether the two outputs are
                           the same bits; the workspace bytes
  weight_bytes_held_once   HBM the weights, the RoPE table and the engine's other allocations take, held once
Synthetic weights and inputs; host clock around a device synchronise."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from magcache_amd.engine import WAN_T2V_1_3B, WAN_T2V_14B, Engine, synthetic_weights  # noqa: E402

DEV = "cuda:0"


def timed(fn, n=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n, out


def tokens(grid):
    return grid[0] * (grid[1] // 2) * (grid[2] // 2)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("grids", nargs="+", metavar="GRID", help="latent grid FxHxW, e.g. 21x60x104")
    ap.add_argument("--cfg", choices=["1.3b", "14b"], default="1.3b")
    ap.add_argument("--layers", type=int, default=None, help="number of blocks (default: the model's)")
    ap.add_argument("--rounds", type=int, default=5, help="windows per engine and grid")
    ap.add_argument("--per-round", type=int, default=2, help="full forwards per window")
    a = ap.parse_args()
    grids = [tuple(int(v) for v in g.split("x")) for g in a.grids]
    cfg = dict(WAN_T2V_1_3B if a.cfg == "1.3b" else WAN_T2V_14B)
    if a.layers:
        cfg["num_layers"] = a.layers
    name = lambda g: "x".join(map(str, g))   # noqa: E731

    def make(grid):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        free0 = torch.cuda.mem_get_info()[0]
        t0 = time.perf_counter()
        e = Engine(cfg, grid, device=DEV, n_branches=2, calibration=False)
        e.load_weights(synthetic_weights(cfg, seed=0, device=DEV))
        torch.cuda.synchronize()
        secs = time.perf_counter() - t0
        torch.cuda.empty_cache()
        return e, secs, free0 - torch.cuda.mem_get_info()[0] - e.workspace.numel()

    def inputs(grid):
        g = torch.Generator(device=DEV).manual_seed(tokens(grid))
        return (torch.randn(cfg["in_dim"], *grid, generator=g, device=DEV),
                torch.randn(cfg["text_len"], cfg["text_dim"], generator=g, device=DEV))

    def forward(e, inp):
        return lambda: e.forward(inp[0], 500.0, inp[1], branch=0)

    def switch(e, grid):
        base = e.workspace.data_ptr()
        t, _ = timed(lambda: e.set_geometry(grid))
        return {"set_geometry_ms": t * 1e3, "reallocated": e.workspace.data_ptr() != base}

    order = sorted(range(len(grids)), key=lambda i: tokens(grids[i]))
    one, create_s, weight_bytes = make(grids[order[0]])        # created at the smallest grid: every first switch grows
    data = [inputs(g) for g in grids]
    no_reserve = {name(grids[i]): switch(one, grids[i]) for i in order[1:]}
    one.reserve(grids)
    res = []
    for i, grid in enumerate(grids):
        fresh, fresh_s, _ = make(grid)
        sw = switch(one, grid)
        f_fresh, f_one = forward(fresh, data[i]), forward(one, data[i])
        same = bool(torch.equal(f_fresh(), f_one()))
        for f in (f_fresh, f_one):
            timed(f, 1)
        ms = {"fresh": [], "switched": []}
        for _ in range(a.rounds):
            ms["fresh"].append(timed(f_fresh, a.per_round)[0] * 1e3)
            ms["switched"].append(timed(f_one, a.per_round)[0] * 1e3)
        res.append({"grid": name(grid), "tokens": tokens(grid),
                    "forward_ms_fresh": float(np.median(ms["fresh"])), "forward_ms_switched": float(np.median(ms["switched"])),
                    "windows_fresh_ms": [round(v, 3) for v in ms["fresh"]],
                    "windows_switched_ms": [round(v, 3) for v in ms["switched"]],
                    "fresh_window_spread_ms": float(max(ms["fresh"]) - min(ms["fresh"])), "bitwise_equal_to_fresh": same,
                    "switch_with_reserve": sw, "workspace_bytes": one.geometry_bytes(grid),
                    "workspace_bytes_fresh_engine": fresh.ws.numel(), "create_load_s_fresh_engine": fresh_s})
        del fresh, f_fresh
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    print(json.dumps({"config": f"Wan2.1-T2V-{a.cfg.upper()} widths, {cfg['num_layers']} blocks, one engine over "
                                f"{', '.join(name(g) for g in grids)}, {cfg['text_len']} text tokens, synthetic weights/inputs",
                      "forwards_per_window": a.per_round, "create_load_s": create_s, "weight_bytes_held_once": weight_bytes,
                      "weight_bytes_one_engine_per_grid": weight_bytes * len(grids),
                      "reserved_workspace_bytes": one.ws.numel(), "switch_without_reserve": no_reserve, "per_grid": res}))


if __name__ == "__main__":
    main()
