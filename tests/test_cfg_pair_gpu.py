"""The declared CFG pair (mc_pair_begin / mc_pair_end): the second forward of a pair continues from the context-free front
the first one computed -- the embeds of the latent and of t, and layer 0 up to its normalised cross-attention q.  Everything
here is a BITWISE comparison against the same calls on a fresh engine that never hears the declaration: outputs, residual
slots and calibration statistics after every forward, for every pair case of the MagCache schedule, for every rule that must
drop a kept front, and for a whole sampler loop; plus the launch counts that show that the front really ran once.

Shapes: d = 256 (2 heads), ffn 512, text_len 64; 48 tokens (grid 2 x 8 x 12: Lp = 256, mostly padding) and 288 tokens
(grid 3 x 16 x 24: Lp = 512, a ragged last tile); 1 layer (layer 0 is also the capture layer) and 2 layers."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from magcache_amd import model as M  # noqa: E402
from magcache_amd.engine import MC_MODE_CALIB, MC_MODE_FULL, MC_MODE_SKIP, Engine, synthetic_weights  # noqa: E402
from magcache_amd.mag_ratios import TABLES  # noqa: E402
from magcache_amd.sampler import sample  # noqa: E402

DEV = "cuda:0"
GRID_48, GRID_288 = (2, 8, 12), (3, 16, 24)
F, S, C = MC_MODE_FULL, MC_MODE_SKIP, MC_MODE_CALIB
# one pair per sampler step, in an order that gives every later pair the residuals it needs: both run, uncond skipped, cond
# skipped, both run again (after a pair that kept nothing), calibration without and with statistics
STEPS = [(F, F), (F, S), (S, F), (F, F), (C, C), (C, C)]


def small_cfg(num_layers, dim=256, ffn_dim=512, **kw):
    return dict(dim=dim, ffn_dim=ffn_dim, num_heads=dim // 128, num_layers=num_layers, in_dim=16, out_dim=16, freq_dim=64,
                text_dim=64, text_len=64, eps=1e-6, **kw)


def make_engine(cfg, grid, calibration=True):
    e = Engine(cfg, grid, device=DEV, n_branches=2, calibration=calibration)
    e.load_weights(synthetic_weights(cfg, seed=0, std=0.05, device=DEV))
    return e


def inputs(grid):
    g = torch.Generator(device=DEV).manual_seed(7)
    lat = torch.randn(16, *grid, generator=g, device=DEV)
    ctx = [torch.randn(n, 64, generator=g, device=DEV) for n in (64, 37)]     # cond, uncond (shorter: zero padded inside)
    return lat, ctx


def bits(t):
    return t.detach().clone().view(torch.int32).cpu()


def state(e, out):
    """everything a forward leaves behind that a caller can read: the output, both residual slots, the calibration statistics"""
    return [bits(out), bits(e.buffer("residual_branch0", torch.float32)), bits(e.buffer("residual_branch1", torch.float32)),
            bits(e.buffer("calib_stats", torch.float32))] + [e.calib_has_stats(b) for b in (0, 1)]


def run_steps(cfg, grid, declare, cached_ctx, counts=None):
    """STEPS on a fresh engine; the latent is updated IN PLACE between steps (same address, new values: what a sampler does)
    and t changes with it.  Returns the state after every forward."""
    e = make_engine(cfg, grid)
    lat, ctx = inputs(grid)
    if cached_ctx:
        for slot in (0, 1):
            e.set_context(slot, ctx[slot])
    if counts is not None:
        e.profile(1)
    seen = []
    for i, modes in enumerate(STEPS):
        t = torch.tensor([900.0 - 150.0 * i], device=DEV)
        if declare:
            e.pair_begin()
        for b, mode in enumerate(modes):
            if cached_ctx:
                e.use_context(b)
            seen.append(state(e, e.forward(lat, t, None if cached_ctx else ctx[b], branch=b, mode=mode)))
        if declare:
            e.pair_end()
        if counts is not None:
            counts.append(e.profile_read()[1])
        lat.mul_(0.9).add_(0.05)
    return seen


@functools.lru_cache(maxsize=None)
def undeclared_steps(num_layers, grid, cached_ctx):
    return run_steps(small_cfg(num_layers), grid, False, cached_ctx)


@pytest.mark.parametrize("grid", [GRID_48, GRID_288], ids=["48tok", "288tok"])
@pytest.mark.parametrize("num_layers,cached_ctx", [(1, False), (2, True)], ids=["1layer-ctx_by_pointer", "2layers-ctx_cached"])
def test_every_pair_case_is_bit_identical(num_layers, cached_ctx, grid):
    want = undeclared_steps(num_layers, grid, cached_ctx)
    counts = []
    got = run_steps(small_cfg(num_layers), grid, True, cached_ctx, counts)
    for i, (g, w) in enumerate(zip(got, want)):
        for k, (a, b) in enumerate(zip(g, w)):
            same = torch.equal(a, b) if torch.is_tensor(a) else a == b
            assert same, f"step {i // 2} {STEPS[i // 2]}, forward {i % 2}: item {k} (out, residual 0, residual 1, stats, has 0, has 1) differs"
    # self-attention launches per step: a pair whose two forwards ran shares layer 0's, every other pair shares nothing
    nl = num_layers
    assert counts == [2 * nl - 1, nl, nl, 2 * nl - 1, 2 * nl - 1, 2 * nl - 1], counts


def pair(e, lat, t, ctx, declare, between=None, t2=None):
    if declare:
        e.pair_begin()
    a = bits(e.forward(lat, t, ctx[0], branch=0))
    if between is not None:
        between(e)
    b = bits(e.forward(lat, t if t2 is None else t2, ctx[1], branch=1))
    if declare:
        e.pair_end()
    return a, b


def invalidation_case(name, declare):
    cfg = small_cfg(2, dim=512, fp8_linear=1) if name == "fp8_engine" else small_cfg(2)
    e = make_engine(cfg, GRID_288, calibration=False)
    lat, ctx = inputs(GRID_288)
    t = torch.tensor([700.0], device=DEV)
    e.profile(1)
    if name == "other_t":
        outs = pair(e, lat, t, ctx, declare, t2=torch.tensor([650.0], device=DEV))
    elif name == "other_t_host":          # t by value (t_host), not through a device pointer
        outs = pair(e, lat, 700.0, ctx, declare, t2=650.0)
    elif name == "set_weight":
        w = dict(synthetic_weights(cfg, seed=1, std=0.05, device=DEV))["blocks.0.self_attn.q.weight"]
        outs = pair(e, lat, t, ctx, declare, between=lambda eng: eng.set_weight("blocks.0.self_attn.q.weight", w))
    elif name == "third_forward":
        outs = pair(e, lat, t, ctx, declare)
        lat.mul_(0.5)                      # same address, other values: nothing of the finished pair may be used
        outs = outs + (bits(e.forward(lat, t, ctx[1], branch=1)),)
    elif name == "third_forward_inside":   # the declaration covers TWO forwards, also when mc_pair_end has not come yet
        if declare:
            e.pair_begin()
        outs = pair(e, lat, t, ctx, False)
        lat.mul_(0.5)
        outs = outs + (bits(e.forward(lat, t, ctx[1], branch=1)),)
        if declare:
            e.pair_end()
    else:
        assert name == "fp8_engine"
        outs = pair(e, lat, t, ctx, declare)
    return outs, e.profile_read()[1]


@pytest.mark.parametrize("name", ["other_t", "other_t_host", "set_weight", "third_forward", "third_forward_inside", "fp8_engine"])
def test_rules_that_drop_a_kept_front(name):
    want, n_want = invalidation_case(name, False)
    got, n_got = invalidation_case(name, True)
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), f"{name}: forward {i} differs from the undeclared run"
    # nothing was shared where a rule forbids it (2 layers per forward); only the regular pair ahead of a third forward was
    shared = 1 if name.startswith("third_forward") else 0
    assert n_want == 2 * len(want) and n_got == n_want - shared, (n_got, n_want)


def test_declared_pair_records_one_front():
    """profile level 2: the forward that continues from a kept front logs no pairs for it -- fewer pairs, not cheaper ones"""
    nl = 2
    per = {}
    for declare in (False, True):
        e = make_engine(small_cfg(nl), GRID_288, calibration=False)
        lat, ctx = inputs(GRID_288)
        for slot in (0, 1):
            e.set_context(slot, ctx[slot])
        e.profile(2)
        t = torch.tensor([500.0], device=DEV)
        if declare:
            e.pair_begin()
        for b in (0, 1):
            e.use_context(b)
            e.forward(lat, t, None, branch=b)
        if declare:
            e.pair_end()
        per[declare] = {k: n for k, (_, n) in e.profile_read_classes().items()}
    off, on = per[False], per[True]
    assert off["attn_self"] == 2 * nl and on["attn_self"] == 2 * nl - 1
    for k in ("gemm_qkv", "gemm_o", "gemm_cross_q"):
        assert off[k] == 2 * nl and on[k] == 2 * nl - 1, (k, off[k], on[k])
    assert (off["ln_modulate"], on["ln_modulate"]) == (6 * nl, 6 * nl - 2)         # layer 0's first LayerNorm and its norm3
    assert (off["rmsnorm_rope"], on["rmsnorm_rope"]) == (4 * nl, 4 * nl - 2)       # the q / k pair and the cross-attention q
    assert (off["embed"], on["embed"]) == (2, 1)                                   # cached contexts: nothing left to embed
    for k in ("attn_cross", "gemm_cross_o", "gemm_ffn1", "gemm_ffn2", "head"):     # everything behind the context: unchanged
        assert off[k] == on[k], (k, off[k], on[k])
    assert (off["other"], on["other"]) == (0, 1)                                   # the first forward's copy of the stream


def test_sampler_loop_with_magcache_is_bit_identical():
    cfg = small_cfg(2)
    lat, ctx = inputs(GRID_288)
    finals, skips = [], []
    for declare in (True, False):
        cls = type("WanModelHIPPair" + str(declare), (M.WanModelHIP,), {})
        m = cls(cfg, GRID_288, device=DEV, calibration=False)
        m.engine.load_weights(synthetic_weights(cfg, seed=0, std=0.05, device=DEV))
        M.init_magcache(m, 6, 0.12, 4, 0.2, mag_ratios=TABLES["wan2.1_t2v_1.3B"])
        modes, fwd = [], m._run
        m._run = lambda x, t, c, branch, mode: (modes.append(mode), fwd(x, t, c, branch, mode))[1]
        m.engine.profile(1)
        finals.append(bits(sample(m, lat, ctx[0], ctx[1], sampling_steps=6, cfg_pair=declare)))
        skips.append([i for i, mode in enumerate(modes) if mode == MC_MODE_SKIP])
        # the shim path really shares: one self-attention launch fewer for every step whose two forwards ran, and only there
        ran = [sum(mode != MC_MODE_SKIP for mode in modes[2 * i:2 * i + 2]) for i in range(6)]
        both = sum(r == 2 for r in ran)
        assert both > 0 and len(modes) == 12
        assert m.engine.profile_read()[1] == 2 * sum(ran) - (both if declare else 0), (ran, declare)
    assert skips[0] == skips[1] and len(skips[0]) > 0, skips
    assert torch.equal(finals[0], finals[1])
