"""One timestep per latent frame on the Wan engine (token_timestep_sets): the whole forward against the per-token oracle
oracle/wan22_dit_ref.WanModel22, which takes arbitrary t [1, seq_len] and runs live on the CPU.  Synthetic weights, the tiny
TI2V geometry of tests/golden/wan22_ti2v_forward_golden.npz with five latent frames (120 tokens: one padded row tile)."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from magcache_amd import _lib, model as M, wan22  # noqa: E402
from magcache_amd._lib import MC_MODE_SKIP  # noqa: E402
from magcache_amd.engine import Engine  # noqa: E402
from oracle import magcache_ref as MR  # noqa: E402
from oracle import wan22_dit_ref as W22  # noqa: E402

DEV = "cuda:0"
CFG = dict(dim=256, ffn_dim=512, freq_dim=64, num_heads=2, num_layers=2, text_len=64, in_dim=48, out_dim=48, text_dim=128, eps=1e-6)
GRID = (5, 8, 12)
L = GRID[0] * (GRID[1] // 2) * (GRID[2] // 2)
T_FRAMES = [0.0, 999.0, 612.5, 875.0, 250.0]           # one distinct value per latent frame, in no order
SEED, STD = 13, 0.05


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def inputs(grid=GRID, cfg=CFG, seed=5):
    g = torch.Generator().manual_seed(seed)
    lat = torch.randn(cfg["in_dim"], *grid, generator=g)
    ctx = torch.randn(23, cfg["text_dim"], generator=g)
    ctxn = torch.randn(11, cfg["text_dim"], generator=g)
    return lat, ctx, ctxn


@pytest.fixture(scope="module")
def oracle():
    return W22.init_synthetic_(W22.WanModel22(**CFG), seed=SEED, std=STD).eval()


def shim(name, oracle, cfg=CFG, grid=GRID, **kw):
    m = type(name, (M.WanModelHIP,), {})(cfg, grid, device=DEV, calibration=False, **kw)
    m.load_state_dict(oracle.state_dict())
    return m


def oracle_errors(oracle, got, lat, tt, ctx, seq_len):
    with torch.no_grad():
        ref32 = oracle.forward([lat], tt, [ctx], seq_len, autocast=False)[0]
        refbf = oracle.forward([lat], tt, [ctx], seq_len, autocast=True)[0]
    return rel_l2(got.cpu(), ref32), rel_l2(refbf, ref32)


def test_per_frame_timesteps_vs_oracle(oracle):
    """Five latent frames, five distinct timesteps, capacity 8: the engine's error against the fp32 oracle stays below twice the
    oracle's own bf16-autocast error (+ 1e-3) and below 2e-2 -- the criterion of
    test_wan22_ti2v_per_token_timesteps_vs_reference_golden.  The oracle's e_bf for these inputs, measured on the CPU, is
    2.9e-3 (< 1e-2: the 2e-2 cap does not bind for the reference).  The engine reports the frame values in descending order
    and no token without a set."""
    lat, ctx, _ = inputs()
    m = shim("WanModelHIP_FrameT", oracle, token_timestep_sets=8)
    assert m.engine.token_timestep_capacity == 8
    tt = wan22.frame_timesteps(T_FRAMES, GRID)
    got = m([lat.to(DEV)], t=tt.to(DEV), context=[ctx.to(DEV)], seq_len=L)[0]
    e_hip, e_bf = oracle_errors(oracle, got, lat, tt, ctx, L)
    print(f"e_hip {e_hip:.3e} e_bf {e_bf:.3e}")
    assert e_bf < 1e-2, e_bf
    assert e_hip < 2 * e_bf + 1e-3 and e_hip < 2e-2, (e_hip, e_bf)
    assert m.engine.token_timestep_values() == sorted(T_FRAMES, reverse=True)
    assert m.engine.token_timestep_record() == (999.0, 0.0, 0)
    # an untagged tensor with as many values passes the up-front check as well, and gives the same bits
    again = m([lat.to(DEV)], t=tt.clone().to(DEV), context=[ctx.to(DEV)], seq_len=L)[0]
    assert torch.equal(again, got)


def test_cfg_pair_keeps_the_front_of_a_per_frame_forward(oracle):
    """mc_pair_begin / _end on a capacity engine: the distinct-value pass and the batched chain are part of the kept front, the
    second forward of the pair reuses the sets -- the same bits as two full forwards"""
    lat, ctx, ctxn = (v.to(DEV) for v in inputs())
    m = shim("WanModelHIP_FrameT_Pair", oracle, token_timestep_sets=8)
    tt = wan22.frame_timesteps(T_FRAMES, GRID).to(DEV)
    want = [m([lat], t=tt, context=[c], seq_len=L)[0].clone() for c in (ctx, ctxn)]
    m.pair_begin()
    got = [m([lat], t=tt, context=[c], seq_len=L)[0].clone() for c in (ctx, ctxn)]
    m.pair_end()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and not torch.equal(got[0], got[1])


@pytest.mark.parametrize("fp8_linear", [0, 2], ids=["bf16", "mxfp8"])
def test_capacity_engine_equals_default_engine_bit_for_bit(fp8_linear):
    """A two-valued `mask * t` and a scalar t on the default engine (two sets, per-set chain, SEL epilogues) and on a
    capacity-8 engine (batched chain, table epilogues, strided LayerNorm): the same bits.  Once with MX fp8 Linears, whose
    fused LayerNorm quantiser and GEMM epilogue take the table too."""
    cfg = dict(CFG, dim=512, num_heads=4, fp8_linear=fp8_linear) if fp8_linear else CFG
    orc = W22.init_synthetic_(W22.WanModel22(**{k: v for k, v in cfg.items() if k != "fp8_linear"}), seed=SEED, std=STD).eval()
    lat, ctx, _ = inputs(cfg=cfg)
    a = shim("WanModelHIP_FrameT_Default%d" % fp8_linear, orc, cfg=cfg)
    b = shim("WanModelHIP_FrameT_Cap%d" % fp8_linear, orc, cfg=cfg, token_timestep_sets=8)
    assert a.engine.token_timestep_capacity == 2 and b.engine.token_timestep_capacity == 8
    per_frame = GRID[1] // 2 * (GRID[2] // 2)
    mask = torch.ones(1, L)
    mask[0, :per_frame] = 0.0                             # the conditioning frame's tokens carry t = 0
    for t in ((mask * 937.5).to(DEV), torch.tensor([612.5], device=DEV)):
        xa = a([lat.to(DEV)], t=t, context=[ctx.to(DEV)], seq_len=L)[0].clone()
        xb = b([lat.to(DEV)], t=t.clone(), context=[ctx.to(DEV)], seq_len=L)[0]
        assert bool(torch.isfinite(xa).all()) and torch.equal(xa, xb), tuple(t.shape)
    assert b.engine.token_timestep_values() == [937.5, 0.0]          # (the last per-token forward)


def test_magcache_with_per_frame_timesteps(oracle, golden_dir):
    """wan22.init_magcache over 8 steps of a staggered per-frame schedule (frame f lags f steps behind frame 1, frame 0 is a
    conditioning frame at t = 0): the FULL / SKIP sequence is oracle.magcache_ref.RuleState's, with a SKIP after a FULL, and
    every call is within 3e-2 relative L2 of the oracle loop run on the CPU with the same schedule -- the bar of the TI2V loop
    test."""
    meta = json.loads(str(np.load(os.path.join(golden_dir, "wan22_ti2v_forward_golden.npz"))["meta"]))
    steps, guide = 8, 5.0
    table = wan22.table_without_pad(meta["table"])
    sig, ts = MR.flow_timesteps(steps, 5.0)
    sig, ts = np.asarray(sig, dtype=np.float64), np.asarray(ts, dtype=np.float64)
    idx = np.array([[steps if f == 0 else max(i - (f - 1), 0) for f in range(GRID[0])] for i in range(steps + 1)])
    sig_f = np.concatenate([sig[:steps], [0.0]])[np.minimum(idx, steps)]          # [steps + 1, F]; index `steps`: sigma 0
    lat, ctx, ctxn = inputs(seed=7)
    m = shim("WanModelHIP_FrameT_MagCache", oracle, token_timestep_sets=8)
    cls = type(m)
    wan22.init_magcache(m, table, steps, meta["thresh"], meta["K"], meta["R"], split_steps=None, mode="t2v")
    rule = MR.RuleState("wan22_ti2v", 2 * steps, meta["thresh"], meta["K"], meta["R"], cls.mag_ratios)
    modes, errs, want_skips = [], [], []
    run = m._run
    m._run = lambda x, t, c, branch, mode, **kw: (modes.append(mode), run(x, t, c, branch, mode, **kw))[1]
    x, xo = lat.clone().to(DEV), lat.clone()
    cache = [None, None]

    def oracle_call(xo, tt, c):
        skip, p = rule.step()
        want_skips.append(int(skip))
        with torch.no_grad(), torch.autocast("cpu", enabled=False):
            h, e, kw = oracle.embed([xo], tt, [c], L)
            ori = h
            if skip:
                h = h + cache[p]
            else:
                for blk in oracle.blocks:
                    h = blk(h, **kw)
            cache[p] = h - ori
            return oracle.unpatchify(oracle.head(h, e), kw["grid_sizes"])[0].float()
    try:
        for i in range(steps):
            tt = wan22.frame_timesteps(1000.0 * sig_f[i], GRID)
            dt = torch.tensor(sig_f[i + 1] - sig_f[i], dtype=torch.float32).reshape(1, -1, 1, 1)
            outs = []
            for c in (ctx, ctxn):
                td = tt.to(DEV)
                td._mc_distinct_at_most = GRID[0]
                got = m([x], t=td, context=[c.to(DEV)], seq_len=L)[0]
                ref = oracle_call(xo, tt, c)
                errs.append(rel_l2(got.cpu(), ref))
                outs.append((got, ref))
            (ec, rc), (eu, ru) = outs
            x = x + dt.to(DEV) * (eu + guide * (ec - eu))
            xo = xo + dt * (ru + guide * (rc - ru))
        m.check_token_timesteps()
    finally:
        m._run = run
        cls.forward = M.plain_forward
    got_skips = [int(mo == MC_MODE_SKIP) for mo in modes]
    print("skips", got_skips, "errs", ["%.2e" % e for e in errs])
    assert got_skips == want_skips
    assert any(a == 0 and b == 1 for a, b in zip(want_skips[:-2], want_skips[2:])), want_skips      # a SKIP after a FULL, same branch
    assert max(errs) < 3e-2, errs


def test_capacity_is_enforced(oracle):
    """capacity 4, five frame values: untagged -> refused before anything runs; tagged as at most 4 (a lie) -> the engine's
    record surfaces at check_token_timesteps(); an honest tag passes"""
    lat, ctx, _ = inputs()
    m = shim("WanModelHIP_FrameT_Cap4", oracle, token_timestep_sets=4)
    five = wan22.frame_timesteps(T_FRAMES, GRID)
    with pytest.raises(ValueError, match="distinct values"):
        m([lat.to(DEV)], t=five.clone().to(DEV), context=[ctx.to(DEV)], seq_len=L)
    lie = five.clone().to(DEV)
    lie._mc_distinct_at_most = 4
    m([lat.to(DEV)], t=lie, context=[ctx.to(DEV)], seq_len=L)
    with pytest.raises(ValueError, match="no modulation set") as ex:
        m.check_token_timesteps()
    assert "neither" not in str(ex.value)
    assert m.engine.token_timestep_record()[2] == L // GRID[0]            # the smallest value's frame overflowed
    four = wan22.frame_timesteps([0.0, 999.0, 612.5, 999.0, 250.0], GRID).to(DEV)
    four._mc_distinct_at_most = 4
    m([lat.to(DEV)], t=four, context=[ctx.to(DEV)], seq_len=L)
    m.check_token_timesteps()
    assert m.engine.token_timestep_values() == [999.0, 612.5, 250.0, 0.0]


def test_set_geometry_on_a_capacity_engine(oracle):
    """change the grid, then a per-frame forward on the new grid against the oracle (the bar of the first test); with both
    grids reserved the switch allocates nothing"""
    grid2 = (6, 8, 8)
    L2 = grid2[0] * (grid2[1] // 2) * (grid2[2] // 2)
    m = shim("WanModelHIP_FrameT_Geo", oracle, token_timestep_sets=8, dynamic_geometry=True)
    e = m.engine
    e.reserve([GRID, grid2])
    base = e.workspace.data_ptr()
    lat, ctx, _ = inputs()
    m([lat.to(DEV)], t=wan22.frame_timesteps(T_FRAMES, GRID).to(DEV), context=[ctx.to(DEV)], seq_len=L)
    lat2, _, _ = inputs(grid=grid2, seed=9)
    tf2 = [500.0, 0.0, 999.0, 750.0, 125.0, 875.0]
    tt2 = wan22.frame_timesteps(tf2, grid2)
    got = m([lat2.to(DEV)], t=tt2.to(DEV), context=[ctx.to(DEV)], seq_len=L2)[0]
    assert e.workspace.data_ptr() == base and m.latent_grid == grid2
    e_hip, e_bf = oracle_errors(oracle, got, lat2, tt2, ctx, L2)
    assert e_hip < 2 * e_bf + 1e-3 and e_hip < 2e-2, (e_hip, e_bf)
    assert e.token_timestep_values() == sorted(tf2, reverse=True)
    m([lat.to(DEV)], t=wan22.frame_timesteps(T_FRAMES, GRID).to(DEV), context=[ctx.to(DEV)], seq_len=L)
    assert e.workspace.data_ptr() == base and e.token_timestep_record()[2] == 0


def test_create_errors():
    """token_timestep_sets 1, 2, 65, and 8 together with no_token_timesteps: MC_EINVAL; a VACE engine still refuses per-token t"""
    for bad in (dict(token_timestep_sets=1), dict(token_timestep_sets=2), dict(token_timestep_sets=65),
                dict(token_timestep_sets=8, no_token_timesteps=1)):
        with pytest.raises(_lib.MagCacheHipError) as ex:
            Engine(dict(CFG, **bad), GRID, device=DEV)
        assert ex.value.status == _lib.MC_EINVAL, bad
    e = Engine(dict(CFG, in_dim=16, out_dim=16, vace_layers=[0], vace_in_dim=16, token_timestep_sets=8), GRID, device=DEV)
    with pytest.raises(_lib.MagCacheHipError) as ex:
        e.set_token_timesteps(torch.zeros(L, device=DEV))
    assert ex.value.status == _lib.MC_EINVAL
