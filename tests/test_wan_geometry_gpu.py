"""GPU: the latent grid as a property of the call on the Wan engine (mc_set_geometry / mc_geometry_bytes) and the RoPE table
it builds on the device (mc_op_rope_axes -> mc_op_rope_expand).

The bar is provenance independence, bit for bit: an engine that was created at one grid, ran there and was switched to
another computes what an engine created at that grid computes -- outputs, residual slots, calibration statistics, a skipped
forward, a declared CFG pair -- in both directions, also after every byte of the workspace was overwritten with NaNs."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from magcache_amd import _lib  # noqa: E402
from magcache_amd import model as M  # noqa: E402
from magcache_amd import wan22  # noqa: E402
from magcache_amd.engine import (MC_MODE_CALIB, MC_MODE_FULL, MC_MODE_SKIP, WAN_T2V_1_3B, Engine,  # noqa: E402
                                 synthetic_weights)
from magcache_amd.mag_ratios import TABLES  # noqa: E402
from magcache_amd.sampler import cfg_euler_, sample  # noqa: E402
from oracle import wan_dit_ref as W  # noqa: E402

DEV = "cuda:0"
# 32 tokens; 105 (odd sizes); 256 = exactly one tile, no pad row; 495 = two query tiles, the last key tile 47 wide
G32, G105, G256, G495 = (2, 8, 8), (3, 10, 14), (4, 16, 16), (5, 18, 22)
EINVAL, ESTATE = _lib.MC_EINVAL, _lib.MC_ESTATE


def ptr(t):
    return C.c_void_p(t.data_ptr())


def bits(t):
    return t.detach().clone().contiguous().view(torch.int32).cpu()


def tokens(grid):
    return grid[0] * (grid[1] // 2) * (grid[2] // 2)


# ------------------------------------------------------------------------------------------------ (a) the RoPE table
def host_table(F, Hp, Wp, tok0, n_tok):
    cs = np.full((n_tok, 64, 2), np.nan, dtype=np.float32)
    _lib.check(_lib.load().mc_op_rope_table(F, Hp, Wp, tok0, n_tok, cs.ctypes.data_as(C.c_void_p)))
    return torch.from_numpy(cs)


def device_axes(F, Hp, Wp):
    lib = _lib.load()
    n = C.c_size_t()
    _lib.check(lib.mc_op_rope_axes(F, Hp, Wp, None, C.byref(n)))
    axes = np.empty(n.value, dtype=np.float32)
    _lib.check(lib.mc_op_rope_axes(F, Hp, Wp, axes.ctypes.data_as(C.c_void_p), None))
    return torch.from_numpy(axes).to(DEV)


@pytest.mark.parametrize("F,Hp,Wp,tok0,n_tok,n_rows", [
    (1, 1, 1, 0, 1, 1), (3, 5, 7, 0, 105, 256), (3, 5, 7, 37, 50, 64), (3, 5, 7, 90, 40, 41), (5, 30, 52, 0, 7800, 7936)])
def test_rope_expand_equals_the_host_table_bitwise(F, Hp, Wp, tok0, n_tok, n_rows):
    lib = _lib.load()
    axes = device_axes(F, Hp, Wp)
    cs = torch.full((n_rows + 2, 64, 2), float("nan"), device=DEV)       # two rows of sentinel behind the table
    _lib.check(lib.mc_op_rope_expand(ptr(axes), F, Hp, Wp, tok0, n_tok, n_rows, ptr(cs),
                                     C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    got = cs.cpu()
    assert torch.equal(bits(got[:n_tok]), bits(host_table(F, Hp, Wp, tok0, n_tok)))
    assert bool((got[n_tok:n_rows, :, 0] == 1).all()) and bool((got[n_tok:n_rows, :, 1] == 0).all())
    assert bool(torch.isnan(got[n_rows:]).all()), "rope_expand wrote past n_rows"


def test_rope_expand_refuses_bad_arguments():
    lib = _lib.load()
    axes = device_axes(3, 5, 7)
    cs = torch.zeros(65, 64, 2, device=DEV)
    good = dict(axes=ptr(axes), F=3, Hp=5, Wp=7, tok0=0, n_tok=50, n_rows=64, cs=ptr(cs))
    bad = [dict(axes=None), dict(cs=None), dict(F=0), dict(Hp=0), dict(Wp=-1), dict(n_tok=0), dict(n_rows=0),
           dict(n_tok=65), dict(tok0=-1), dict(cs=C.c_void_p(cs.data_ptr() + 4)), dict(cs=C.c_void_p(cs.data_ptr() + 8))]
    for change in bad:
        a = dict(good, **change)
        st = lib.mc_op_rope_expand(a["axes"], a["F"], a["Hp"], a["Wp"], a["tok0"], a["n_tok"], a["n_rows"], a["cs"], None)
        assert st == EINVAL, change
    torch.cuda.synchronize()
    assert not bool(cs.any()), "a refused call wrote"


# ------------------------------------------------------------------------------------------------ toys
def toy(kind):
    if kind == "t2v":
        return W.tiny_config()
    if kind == "i2v":
        return W.tiny_config(i2v=True)
    if kind == "vace":            # three layers, control blocks on 0 and 2: the last layer carries a hint (unfused capture)
        return dict(W.tiny_config(num_layers=3), model_type="vace", vace_layers=[0, 2], vace_in_dim=16)
    assert kind == "mxfp8"
    return dict(W.tiny_config(num_heads=4, ffn_dim=512), fp8_linear=2)


def make_engine(cfg, grid, calibration=True, **kw):
    e = Engine(cfg, grid, device=DEV, n_branches=2, calibration=calibration, **kw)
    e.load_weights(synthetic_weights(cfg, seed=0, std=0.05, device=DEV))
    return e


@functools.lru_cache(maxsize=None)
def inputs(kind, grid):
    cfg = toy(kind) if isinstance(kind, str) else dict(kind)
    g = torch.Generator(device=DEV).manual_seed(7 + tokens(grid))
    lat = torch.randn(cfg["in_dim"], *grid, generator=g, device=DEV)
    ctx = [torch.randn(n, cfg["text_dim"], generator=g, device=DEV) for n in (cfg["text_len"], 37)]
    clip = torch.randn(257, cfg.get("clip_dim", 0) or 1, generator=g, device=DEV)
    vace = torch.randn(cfg.get("vace_in_dim", 0) or 1, *grid, generator=g, device=DEV)
    return lat, ctx, clip, vace


def condition(e, kind, grid):
    """the per-video conditioning an I2V / VACE engine needs before its first forward (again after a switch)"""
    _, _, clip, vace = inputs(kind, grid)
    if kind == "i2v":
        e.set_clip_fea(clip)
    if kind == "vace":
        e.set_vace_context(vace, 0.75)


def trace(e, kind, grid, everything):
    """what a caller can read after: FULL forwards of both branches and their residual slots; (everything) two CALIB forwards
    per branch and the three statistics; SKIP forwards; (everything) a declared CFG pair"""
    lat, ctx, _, _ = inputs(kind, grid)
    lat2 = lat * 0.9 + 0.05
    t = [torch.tensor([v], device=DEV) for v in (700.0, 550.0, 400.0)]
    seen = [bits(e.forward(lat, t[0], ctx[b], branch=b)) for b in (0, 1)]
    seen += [bits(e.residual(b)) for b in (0, 1)]
    if everything:
        for x, tt in ((lat, t[0]), (lat2, t[1])):
            for b in (0, 1):
                seen.append(bits(e.forward(x, tt, ctx[b], branch=b, mode=MC_MODE_CALIB)))
        assert e.calib_has_stats(0) and e.calib_has_stats(1)
        seen.append(bits(e.buffer("calib_stats", torch.float32)[:6]))
        seen += [bits(e.residual(b)) for b in (0, 1)]
    seen += [bits(e.forward(lat2, t[2], ctx[b], branch=b, mode=MC_MODE_SKIP)) for b in (0, 1)]
    if everything:
        e.pair_begin()
        seen += [bits(e.forward(lat2, t[1], ctx[b], branch=b)) for b in (0, 1)]
        e.pair_end()
        seen += [bits(e.residual(b)) for b in (0, 1)]
    return seen


@functools.lru_cache(maxsize=None)
def fresh_trace(kind, grid):
    e = make_engine(toy(kind), grid)
    condition(e, kind, grid)
    return trace(e, kind, grid, kind == "t2v")


def switched_trace(kind, g_from, g_to, nan):
    """created at g_from, one FULL forward there (with a cached text context, so that there is one to forget), switched"""
    e = make_engine(toy(kind), g_from)
    if nan:
        e.reserve([g_from, g_to])                    # the switch keeps this memory ...
    condition(e, kind, g_from)
    lat, ctx, _, _ = inputs(kind, g_from)
    e.set_context(0, ctx[0])
    e.forward(lat, 700.0, None, branch=0)
    if nan:
        torch.cuda.synchronize()
        e.ws.fill_(0xFF)                             # ... every byte of it a NaN, as fp32 and as bf16
        base = e.workspace.data_ptr()
    e.set_geometry(g_to)
    if nan:
        assert e.workspace.data_ptr() == base
    assert e.grid == g_to and e.seq_len == e.tokens_per_rank == tokens(g_to)
    condition(e, kind, g_to)
    return trace(e, kind, g_to, kind == "t2v")


def assert_same(got, want, what):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        ref = b.view(torch.float32)               # equal bits prove nothing about NaNs or a buffer nobody wrote
        assert bool(torch.isfinite(ref).all()) and bool(ref.any()), f"{what}: item {i} of the fresh engine's trace is degenerate"
        assert a.shape == b.shape and torch.equal(a, b), f"{what}: item {i} of the trace differs from the fresh engine's"


# ------------------------------------------------------------------------------------------------ (b) provenance
@pytest.mark.parametrize("nan", [False, True], ids=["kept", "nan_workspace"])
@pytest.mark.parametrize("g_from,g_to", [(G32, G105), (G105, G32), (G256, G495), (G495, G256), (G105, G256), (G495, G32)],
                         ids=lambda g: "x".join(map(str, g)))
def test_switched_engine_equals_fresh_engine_bitwise(g_from, g_to, nan):
    assert_same(switched_trace("t2v", g_from, g_to, nan), fresh_trace("t2v", g_to), f"t2v {g_from} -> {g_to}")


@pytest.mark.parametrize("kind", ["i2v", "vace", "mxfp8"])
@pytest.mark.parametrize("g_from,g_to", [(G105, G495), (G495, G105)], ids=lambda g: "x".join(map(str, g)))
def test_switched_i2v_vace_fp8_engines_equal_fresh_ones(kind, g_from, g_to):
    assert_same(switched_trace(kind, g_from, g_to, True), fresh_trace(kind, g_to), f"{kind} {g_from} -> {g_to}")


def test_switching_back_and_forth_keeps_both_grids_right():
    e = make_engine(toy("t2v"), G105)
    for g in (G495, G105, G256, G105):
        e.set_geometry(g)
        assert_same(trace(e, "t2v", g, True), fresh_trace("t2v", g), f"... -> {g}")


# ------------------------------------------------------------------------------------------------ (c) 1.3B widths
CFG_13 = dict(WAN_T2V_1_3B, num_layers=1, text_len=64)
G13_SMALL, G13_BIG = (2, 16, 16), (8, 58, 50)       # 128 tokens; 5800 tokens, Lp 5888, last key tile 40 wide


def trace_13(e, grid):
    lat, ctx, _, _ = inputs(tuple(sorted(CFG_13.items())), grid)
    t = torch.tensor([700.0], device=DEV)
    seen = [bits(e.forward(lat, t, ctx[b], branch=b)) for b in (0, 1)]
    seen += [bits(e.residual(b)) for b in (0, 1)]
    seen += [bits(e.forward(lat * 0.9, t, ctx[b], branch=b, mode=MC_MODE_SKIP)) for b in (0, 1)]
    return seen


def test_generated_gemm_is_in_the_switched_path():
    lib = _lib.load()
    d, ffn = CFG_13["dim"], CFG_13["ffn_dim"]
    shapes = [(3 * d, d, 0), (ffn, d, 1), (d, ffn, 2), (d, d, 2)]          # q|k|v, FFN-1, FFN-2, O: (N, K, epilogue)
    assert tokens(G13_BIG) == 5800 and tokens(G13_SMALL) == 128
    assert [lib.mc_op_gemm_bf16_kernel(5888, n, k, epi) for n, k, epi in shapes] == [4, 4, 4, 4]
    assert [lib.mc_op_gemm_bf16_kernel(256, n, k, epi) for n, k, epi in shapes] == [1, 1, 1, 1]
    want = {}
    for g in (G13_SMALL, G13_BIG):
        want[g] = trace_13(make_engine(CFG_13, g, calibration=False), g)
    for g_from, g_to in ((G13_SMALL, G13_BIG), (G13_BIG, G13_SMALL)):
        e = make_engine(CFG_13, g_from, calibration=False)
        trace_13(e, g_from)
        e.set_geometry(g_to)
        assert_same(trace_13(e, g_to), want[g_to], f"1.3B widths {g_from} -> {g_to}")


# ------------------------------------------------------------------------------------------------ (d) state and refusals
def status_of(fn):
    with pytest.raises(_lib.MagCacheHipError) as ei:
        fn()
    return ei.value.status


def test_plan_larger_than_the_bound_workspace_is_refused_and_nothing_changes():
    e = make_engine(toy("t2v"), G105)
    lat, ctx, _, _ = inputs("t2v", G105)
    assert e.ws.numel() == e.lib.mc_workspace_bytes(e.h) == e.geometry_bytes(G105)
    assert e.geometry_bytes(G495) > e.ws.numel()
    want = bits(e.forward(lat, 700.0, ctx[0], branch=0))
    want_skip = bits(e.forward(lat * 0.5, 600.0, ctx[0], branch=0, mode=MC_MODE_SKIP))
    assert e.lib.mc_set_geometry(e.h, *G495) == EINVAL
    msg = e.lib.mc_last_error().decode()
    assert str(e.geometry_bytes(G495)) in msg and str(e.ws.numel()) in msg, msg
    # untouched: same plan, the residual of the forward before is still there, the old grid's output comes out again
    assert e.lib.mc_workspace_bytes(e.h) == e.ws.numel()
    assert torch.equal(bits(e.forward(lat * 0.5, 600.0, ctx[0], branch=0, mode=MC_MODE_SKIP)), want_skip)
    assert torch.equal(bits(e.forward(lat, 700.0, ctx[0], branch=0)), want)


def test_state_is_forgotten_by_a_switch_like_on_a_fresh_engine():
    fresh = make_engine(toy("t2v"), G32)
    lat32, ctx32, _, _ = inputs("t2v", G32)
    e = make_engine(toy("t2v"), G105)
    lat, ctx, _, _ = inputs("t2v", G105)
    e.set_context(0, ctx[0])
    e.forward(lat, 700.0, None, branch=0)
    e.set_token_timesteps(torch.full((tokens(G105),), 700.0, device=DEV))
    e.set_geometry(G32)
    assert e._tok_t is None
    skip = lambda eng: eng.forward(lat32, 700.0, ctx32[0], branch=0, mode=MC_MODE_SKIP)   # noqa: E731
    assert status_of(lambda: skip(e)) == status_of(lambda: skip(fresh)) == ESTATE
    assert "residual_cache[0] is empty" in e.lib.mc_last_error().decode()
    assert status_of(lambda: e.use_context(0)) == ESTATE
    assert status_of(lambda: e.forward(lat32, 700.0, None, branch=0)) == ESTATE
    assert not e.calib_has_stats(0) and not e.calib_has_stats(1)
    # I2V: the CLIP context went with the plan
    ei = make_engine(toy("i2v"), G105, calibration=False)
    condition(ei, "i2v", G105)
    ei.forward(inputs("i2v", G105)[0], 700.0, inputs("i2v", G105)[1][0])
    ei.set_geometry(G32)
    li, ci, _, _ = inputs("i2v", G32)
    fresh_i = make_engine(toy("i2v"), G32, calibration=False)
    assert status_of(lambda: ei.forward(li, 700.0, ci[0])) == status_of(lambda: fresh_i.forward(li, 700.0, ci[0])) == ESTATE
    assert "mc_set_clip_fea" in ei.lib.mc_last_error().decode()
    # VACE: so did the control context
    ev = make_engine(toy("vace"), G105, calibration=False)
    condition(ev, "vace", G105)
    ev.set_geometry(G32)
    lv, cv, _, _ = inputs("vace", G32)
    assert status_of(lambda: ev.forward(lv, 700.0, cv[0])) == ESTATE
    assert "mc_set_vace_context" in ev.lib.mc_last_error().decode()


def test_refusals():
    cfg = toy("t2v")
    for kw in (dict(sp_phases=True), dict(sp_rank=0, sp_size=2)):
        sharded = Engine(cfg, G256, device=DEV, **kw)
        assert sharded.lib.mc_set_geometry(sharded.h, *G32) == EINVAL, kw
        with pytest.raises(ValueError):
            sharded.set_geometry(G32)
        n = C.c_size_t()
        assert sharded.lib.mc_geometry_bytes(sharded.h, *G256, C.byref(n)) == 0 and n.value == sharded.ws.numel()
    e = make_engine(cfg, G105)
    lat, ctx, _, _ = inputs("t2v", G105)
    want = bits(e.forward(lat, 700.0, ctx[0]))
    # an odd H or W, an empty grid: refused as mc_create refuses them, by both calls
    n = C.c_size_t()
    for bad in ((2, 9, 8), (2, 8, 7), (0, 8, 8), (2, 0, 8), (-1, 8, 8)):
        assert e.lib.mc_set_geometry(e.h, *bad) == EINVAL, bad
        assert e.lib.mc_geometry_bytes(e.h, *bad, C.byref(n)) == EINVAL, bad
        with pytest.raises(_lib.MagCacheHipError):
            Engine(cfg, bad, device=DEV)
    assert e.lib.mc_set_geometry(None, *G32) == EINVAL and e.lib.mc_geometry_bytes(e.h, *G32, None) == EINVAL
    # between mc_embed and mc_head of a phase forward
    e.embed(lat, 700.0, ctx[0])
    assert e.lib.mc_set_geometry(e.h, *G32) == ESTATE
    e.block_pre_attn(0)
    assert e.lib.mc_set_geometry(e.h, *G32) == ESTATE
    e.block_post_attn(0, 0, MC_MODE_FULL)
    e.block_pre_attn(1)
    e.block_post_attn(1, 0, MC_MODE_FULL)
    e.head(0, MC_MODE_FULL)
    # none of the refused calls changed anything
    assert e.grid == G105 and torch.equal(bits(e.forward(lat, 700.0, ctx[0])), want)
    e.set_geometry(G32)
    assert_same(trace(e, "t2v", G32, True), fresh_trace("t2v", G32), "after the refusals")


def test_reserve_binds_once():
    e = make_engine(toy("t2v"), G105)
    need = e.reserve([G32, G495, G256])
    assert need == max(e.geometry_bytes(g) for g in (G32, G105, G256, G495)) == e.ws.numel()
    base = e.workspace.data_ptr()
    assert e.reserve([G32]) == need and e.workspace.data_ptr() == base
    for g in (G495, G32, G256, G105):
        e.set_geometry(g)
        assert e.workspace.data_ptr() == base and e.lib.mc_workspace_bytes(e.h) == e.geometry_bytes(g)
        assert_same(trace(e, "t2v", g, True), fresh_trace("t2v", g), f"reserved, -> {g}")
    # without reserve a larger grid gets a larger workspace
    small = make_engine(toy("t2v"), G32)
    before = small.ws.numel()
    small.set_geometry(G495)
    assert small.ws.numel() == small.geometry_bytes(G495) > before


# ------------------------------------------------------------------------------------------------ (e) the shims
STEPS = 6


def shim(name, grid, **kw):
    cfg = toy("t2v")
    m = type(name, (M.WanModelHIP,), {})(cfg, grid, device=DEV, calibration=False, **kw)
    m.engine.load_weights(synthetic_weights(cfg, seed=0, std=0.05, device=DEV))
    M.init_magcache(m, STEPS, 0.12, 4, 0.2, mag_ratios=TABLES["wan2.1_t2v_1.3B"])
    modes, fwd = [], m._run
    m._run = lambda x, t, c, branch, mode: (modes.append(mode), fwd(x, t, c, branch, mode))[1]
    return m, modes


def test_shim_follows_the_grid_of_the_call_and_restarts_the_schedule():
    lat, ctx, _, _ = inputs("t2v", G495)
    fresh, modes_fresh = shim("WanModelHIPGeoFresh", G495)
    want = bits(sample(fresh, lat, ctx[0], ctx[1], sampling_steps=STEPS, seq_len=tokens(G495)))
    skips = [i for i, mode in enumerate(modes_fresh) if mode == MC_MODE_SKIP]
    assert skips and len(modes_fresh) == 2 * STEPS

    m, modes = shim("WanModelHIPGeoDynamic", G105, dynamic_geometry=True)
    lat1, ctx1, _, _ = inputs("t2v", G105)
    x = lat1.clone()
    for i in range(4):                                  # part of a sample at the first grid: the schedule is under way
        t = torch.tensor([900.0 - 100.0 * i], device=DEV)
        outs = [m([x], t=t, context=[c], seq_len=tokens(G105))[0] for c in ctx]       # the contexts of the G495 run: cached
        cfg_euler_(x, outs[0].contiguous(), outs[1].contiguous(), 5.0, -0.1)
    assert m.cnt == 8 and len(modes) == 8
    del modes[:]
    got = bits(sample(m, lat, ctx[0], ctx[1], sampling_steps=STEPS, seq_len=tokens(G495)))
    assert bool(torch.isfinite(want.view(torch.float32)).all()) and not torch.equal(want, bits(lat))
    assert m.latent_grid == G495 == m.engine.grid and m.cnt == 0
    assert [i for i, mode in enumerate(modes) if mode == MC_MODE_SKIP] == skips
    assert torch.equal(got, want)
    # and back, on the same weights
    fresh1, _ = shim("WanModelHIPGeoFresh105", G105)
    want1 = bits(sample(fresh1, lat1, ctx[0], ctx[1], sampling_steps=STEPS, seq_len=tokens(G105)))
    assert torch.equal(bits(sample(m, lat1, ctx[0], ctx[1], sampling_steps=STEPS, seq_len=tokens(G105))), want1)


def test_default_shim_keeps_its_grid():
    m, _ = shim("WanModelHIPGeoFixed", G105)
    lat, ctx, _, _ = inputs("t2v", G32)
    with pytest.raises(AssertionError):
        m([lat], t=torch.tensor([700.0], device=DEV), context=[ctx[0]], seq_len=tokens(G32))
    assert m.latent_grid == G105 == m.engine.grid
    sharded = type("WanModelHIPGeoSharded", (M.WanModelHIP,), {})(toy("t2v"), G256, device=DEV, calibration=False, sp_phases=True,
                                                                 dynamic_geometry=True)
    with pytest.raises(ValueError):
        sharded([lat], t=torch.tensor([700.0], device=DEV), context=[ctx[0]], seq_len=tokens(G32))


def run_experts(hi, lo, grid, steps, upto):
    """the two-expert CFG loop of Wan2.2 I2V (y concatenated to the latent) for the first `upto` steps"""
    cfg = dict(toy("t2v"), in_dim=36)
    g = torch.Generator(device=DEV).manual_seed(3 + tokens(grid))
    x, y = torch.randn(16, *grid, generator=g, device=DEV), torch.randn(20, *grid, generator=g, device=DEV)
    ctx = [torch.randn(n, cfg["text_dim"], generator=g, device=DEV) for n in (21, 9)]
    ts, sig = wan22.get_timesteps(5.0, steps)
    for i in range(upto):
        m = hi if ts[i] >= 900 else lo
        t = torch.tensor([float(ts[i])], device=DEV)
        outs = [m([x], t=t, context=[c], seq_len=tokens(grid), y=[y])[0] for c in ctx]
        cfg_euler_(x, outs[0].contiguous(), outs[1].contiguous(), 3.5, float(sig[i + 1] - sig[i]))
    return bits(x)


def experts(name, grid, steps, **kw):
    cfg = dict(toy("t2v"), in_dim=36)
    hi, lo = wan22.make_experts(cfg, grid, device=DEV, name=name, **kw)
    for m, seed in ((hi, 11), (lo, 12)):
        m.engine.load_weights(synthetic_weights(cfg, seed=seed, std=0.05, device=DEV))
    split = wan22.high_noise_steps(5.0, steps, 0.9)
    assert 0 < split < steps
    wan22.init_magcache(hi, wan22.table_without_pad("wan2.2_i2v_A14B"), steps, 0.12, 2, 0.2, split_steps=split, mode="i2v")
    modes = []
    for m in (hi, lo):
        m.engine.forward = (lambda orig: lambda *a, **k: (modes.append(k["mode"]), orig(*a, **k))[1])(m.engine.forward)
    return hi, lo, modes, split


def test_wan22_experts_switch_together():
    steps = 12
    hi, lo, modes_fresh, split = experts("WanModelHIP22GeoFresh", G256, steps)
    want = run_experts(hi, lo, G256, steps, steps)
    assert MC_MODE_SKIP in modes_fresh and type(hi).cnt == 0
    hi, lo, modes, _ = experts("WanModelHIP22GeoDynamic", G105, steps, dynamic_geometry=True)
    assert hi.dynamic_geometry and lo.dynamic_geometry
    run_experts(hi, lo, G105, steps, split + 2)        # both experts have run at the first grid; the sample is abandoned
    assert type(hi).cnt == 2 * (split + 2)
    del modes[:]
    got = run_experts(hi, lo, G256, steps, steps)
    assert hi.latent_grid == lo.latent_grid == G256 == hi.engine.grid == lo.engine.grid and type(hi).cnt == 0
    assert modes == modes_fresh
    assert bool(torch.isfinite(want.view(torch.float32)).all()) and torch.equal(got, want)
