"""GPU: per-call token geometry of the MM-DiT engine (mc_mmdit_set_geometry / mc_mmdit_geometry_bytes, MMDiTEngine.set_geometry
/ reserve, the shims' dynamic_geometry).

The central property is provenance independence: an engine that was created at geometry G1, ran forwards there and was
switched to G2 gives BITWISE what an engine freshly created at G2 gives on the same weights and inputs -- output and cached
residual of a FULL forward, the three statistics after two CALIB forwards, the output of a SKIP forward.  Bitwise is the
bar, not a tolerance: every launch dispatches by shape and the shapes are equal, split-K sums in index order, and rows
[S, S_pad) are masked as keys and ignored as queries; a difference is a stale buffer or a stale derived integer.

Toy widths throughout (dim 256, 2 heads, 1-2 double + 1-2 single blocks, oracle weights), every fresh-engine result is
computed once per (family, geometry) and shared."""
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

from magcache_amd import _lib  # noqa: E402
from magcache_amd import mmdit as MM  # noqa: E402
from magcache_amd._lib import MC_EINVAL, MC_ESTATE, MC_OK  # noqa: E402
from oracle import flux_ref as FR  # noqa: E402
from oracle import hunyuan_ref as HR  # noqa: E402

import qwen_image_ref as QR  # noqa: E402

DEV = "cuda:0"
FULL, SKIP, CALIB = MM.MC_MODE_FULL, MM.MC_MODE_SKIP, MM.MC_MODE_CALIB
ZERO = (0, 0, 0)
BUFFERS = ("x", "x0", "xn", "qkv", "attn_lse", "am", "tokens", "txt_in", "txt_e", "emod", "vecs", "head_tokens", "residual0",
           "residual1", "residual2", "residual3", "splitk0", "splitk1", "calib_partial", "calib_sums", "calib_stats")


# ------------------------------------------------------------------------------------------------ families at toy width
class Flux:
    """geometry = (img_tokens, txt_len)"""
    cfg = FR.tiny_config(num_layers=2, num_single_layers=2)
    branches = (None,)
    _sd = None

    @classmethod
    def sd(cls):
        if cls._sd is None:
            cls._sd = FR.init_synthetic_(FR.FluxTransformer2DModel(**cls.cfg), seed=3, std=0.05).state_dict()
        return cls._sd

    @classmethod
    def engine(cls, geo, weights=True, **kw):
        c = cls.cfg
        e = MM.MMDiTEngine(MM.MC_FAMILY_FLUX, 256, 2, c["num_layers"], c["num_single_layers"], 64, 64, c["joint_attention_dim"],
                           geo[1], c["pooled_projection_dim"], geo[0], calibration=True, device=DEV, **kw)
        if weights:
            e.load_weights(cls.sd())
        return e

    @staticmethod
    def args(geo):
        return geo[0], ZERO, geo[1]

    @staticmethod
    def inputs(geo):
        li, lt = geo
        g = torch.Generator().manual_seed(1000 * li + lt)
        ids = torch.zeros(lt + li, 3)
        ids[lt:, 1] = torch.arange(li) // 8
        ids[lt:, 2] = torch.arange(li) % 8
        return SimpleNamespace(img=torch.randn(li, 64, generator=g).to(DEV), txt=[torch.randn(lt, 256, generator=g).to(DEV)],
                               valid=[lt], vec=torch.randn(128, generator=g).to(DEV), rope=MM.flux_rope(ids), guidance=4000.0)


class Hunyuan:
    """geometry = ((F, H, W), txt_len); the text comes with a prefix mask (23 valid rows)"""
    cfg = HR.tiny_config(double=1, single=2)
    branches = (None,)
    _sd = None

    @classmethod
    def sd(cls):
        if cls._sd is None:
            cls._sd = HR.init_synthetic_(HR.HYVideoDiffusionTransformer(**cls.cfg), seed=4, std=0.05).state_dict()
        return cls._sd

    @staticmethod
    def tokens(grid):
        return grid[0] * (grid[1] // 2) * (grid[2] // 2)

    @classmethod
    def engine(cls, geo, weights=True, **kw):
        c = cls.cfg
        e = MM.MMDiTEngine(MM.MC_FAMILY_HUNYUAN, 256, 2, c["mm_double_blocks_depth"], c["mm_single_blocks_depth"], 16, 16,
                           c["text_states_dim"], geo[1], c["text_states_dim_2"], cls.tokens(geo[0]), latent_grid=geo[0],
                           refiner_depth=2, calibration=True, device=DEV, **kw)
        if weights:
            e.load_weights(cls.sd())
        return e

    @classmethod
    def args(cls, geo):
        return cls.tokens(geo[0]), geo[0], geo[1]

    @staticmethod
    def inputs(geo):
        (f, h, w), lt = geo
        g = torch.Generator().manual_seed(100 * f + 10 * h + w + lt)
        return SimpleNamespace(img=torch.randn(16, f, h, w, generator=g).to(DEV), txt=[torch.randn(lt, 256, generator=g).to(DEV)],
                               valid=[23], vec=torch.randn(128, generator=g).to(DEV),
                               rope=HR.get_rotary_pos_embed((f, h // 2, w // 2)), guidance=6000.0)


class Qwen:
    """geometry = (img_shapes, txt_len): txt_len is the maximum, the cond prompt has 37 rows and the uncond one 5"""
    cfg = QR.tiny_config(num_layers=2)
    branches = (0, 1)
    _sd = None

    @classmethod
    def sd(cls):
        if cls._sd is None:
            cls._sd = QR.init_synthetic_(QR.QwenImageTransformer2DModel(**cls.cfg), seed=5, std=0.05).state_dict()
        return cls._sd

    @staticmethod
    def tokens(shapes):
        return sum(f * h * w for f, h, w in shapes)

    @classmethod
    def engine(cls, geo, weights=True, **kw):
        c = cls.cfg
        e = MM.MMDiTEngine(MM.MC_FAMILY_QWEN, 256, 2, c["num_layers"], 0, 64, 64, c["joint_attention_dim"], geo[1], 0,
                           cls.tokens(geo[0]), calibration=True, device=DEV, **kw)
        if weights:
            e.load_weights(cls.sd())
        return e

    @classmethod
    def args(cls, geo):
        return cls.tokens(geo[0]), ZERO, geo[1]

    @classmethod
    def inputs(cls, geo):
        shapes, lt = geo
        li = cls.tokens(shapes)
        g = torch.Generator().manual_seed(7 * li + lt)
        return SimpleNamespace(img=torch.randn(li, 64, generator=g).to(DEV),
                               txt=[torch.randn(n, 256, generator=g).to(DEV) for n in (37, 5)], valid=[37, 5], vec=None,
                               rope=MM.qwen_rope(list(shapes), lt), guidance=0.0)


def fwd(e, inp, mode, t=500.0, b=None):
    k = b or 0
    return e.forward(inp.img, t, inp.guidance, inp.txt[k], inp.valid[k], inp.vec, mode=mode, branch=b)


def probe(e, inp, branches=(None,)):
    """FULL (output, cached residual), CALIB x 2 (the three statistics), SKIP (output), on every CFG branch"""
    r = {}
    for b in branches:
        r[f"full{b}"] = fwd(e, inp, FULL, 500.0, b)
        r[f"residual{b}"] = e.residual(b).clone()
    for t in (500.0, 400.0):
        for b in branches:
            r[f"calib{t}{b}"] = fwd(e, inp, CALIB, t, b)
            if t == 400.0:
                r[f"stats{b}"] = torch.tensor(e.calib_stats())
    for b in branches:
        r[f"skip{b}"] = fwd(e, inp, SKIP, 300.0, b)
    return {k: v.cpu() for k, v in r.items()}


def plan(e):
    """workspace bytes and (offset, bytes) of every buffer the plan has"""
    out = {"bytes": e.lib.mc_mmdit_workspace_bytes(e.h)}
    for name in BUFFERS:
        off, nb = _lib.C.c_size_t(), _lib.C.c_size_t()
        if e.lib.mc_mmdit_buffer_info(e.h, name.encode(), _lib.C.byref(off), _lib.C.byref(nb)) == MC_OK:
            out[name] = (off.value, nb.value)
    return out


def assert_same(got, want):
    assert got.keys() == want.keys()
    for k in want:
        assert bool(torch.isfinite(want[k]).all()), k
        assert torch.equal(got[k], want[k]), f"{k}: max |diff| {float((got[k] - want[k]).abs().max())}"


_fresh = {}


def fresh(fam, geo, rope=True):
    """probe and plan of an engine created at `geo` (once per family and geometry; nobody changes the result)"""
    key = (fam.__name__, geo, rope)
    if key not in _fresh:
        e = fam.engine(geo)
        inp = fam.inputs(geo)
        if rope:
            e.set_rope(*inp.rope)
        _fresh[key] = (probe(e, inp, fam.branches), plan(e))
    return _fresh[key]


def switch(fam, e, geo, rope=True):
    e.set_geometry(*fam.args(geo))
    inp = fam.inputs(geo)
    if rope:
        e.set_rope(*inp.rope)
    return inp


def used(fam, geo):
    """an engine created at `geo` that has run forwards there"""
    e = fam.engine(geo)
    inp = fam.inputs(geo)
    e.set_rope(*inp.rope)
    probe(e, inp, fam.branches)
    return e


def check_switched(fam, e, geo):
    inp = switch(fam, e, geo)
    want, want_plan = fresh(fam, geo)
    assert plan(e) == want_plan
    assert_same(probe(e, inp, fam.branches), want)


# ------------------------------------------------------------------------------------------------ provenance independence
F1A, F1B = (512, 256), (200, 256)     # text boundary on the 256-row grid: row-split single launches; S_pad 768 -> 512, S = 456
F2A, F2B = (216, 40), (256, 256)      # boundary off the grid (two launches per Linear) -> on it (one row-split launch)


def test_flux_text_boundary_on_the_tile_grid_shrink_and_grow():
    e = used(Flux, F1A)
    check_switched(Flux, e, F1B)
    check_switched(Flux, e, F1A)


def test_flux_text_boundary_moves_onto_the_tile_grid():
    e = used(Flux, F2A)
    check_switched(Flux, e, F2B)


def test_no_stale_reads_after_the_workspace_was_filled_with_nan():
    """every byte of the bound workspace 0xFF (NaN in every float format) before the switch: set_geometry must re-establish
    all that set_workspace + zeroed memory establish (pad rows, the calibration ticket)"""
    e = used(Flux, F1A)
    torch.cuda.synchronize()
    e.ws.fill_(0xFF)
    check_switched(Flux, e, F1B)


def test_split_k_scratch_appears_and_the_plan_is_not_monotone():
    """At dim 256 no K is long enough for the by-shape split (K / slices >= 2048), so the scratch is made to appear with the
    gemm_splitk force option, as at real widths it appears below 128 output tiles: the engine created at 216 + 40 tokens
    under the default policy has no "splitk0"; switched to FEWER tokens (200 + 40) under forced slices it has one, and that
    smaller geometry needs the larger workspace -- why set_geometry asks whether the plan fits, not whether it shrank."""
    lib = _lib.load()
    g1, g2 = (216, 40), (200, 40)
    e = used(Flux, g1)
    with pytest.raises(_lib.MagCacheHipError, match="unknown buffer"):
        e.buffer("splitk0")
    b1 = e.geometry_bytes(*Flux.args(g1))
    assert b1 == lib.mc_mmdit_workspace_bytes(e.h)
    try:
        _lib.check(lib.mc_set_option(b"gemm_splitk", 2))
        b2 = e.geometry_bytes(*Flux.args(g2))
        assert b2 > b1 and sum(g2) < sum(g1)
        inp = switch(Flux, e, g2)
        assert e.buffer("splitk0").numel() > 0 and e.buffer("splitk1").numel() > 0
        b = Flux.engine(g2)
        b.set_rope(*inp.rope)
        assert plan(e) == plan(b) and plan(e)["bytes"] == b2
        assert_same(probe(e, inp), probe(b, inp))
    finally:
        _lib.check(lib.mc_set_option(b"gemm_splitk", 1))


H_A, H_B = ((2, 8, 12), 40), ((3, 6, 8), 56)


def test_hunyuan_grid_change_and_refused_odd_height():
    lib = _lib.load()
    e = used(Hunyuan, H_A)
    check_switched(Hunyuan, e, H_B)        # F, H, W and the text length change; 36 + 56 rows, prefix mask, unpatchify
    inp = Hunyuan.inputs(H_B)
    before = fwd(e, inp, FULL).cpu()
    assert lib.mc_mmdit_set_geometry(e.h, 36, 3, 7, 8, 56) == MC_EINVAL      # 3 * (7 // 2) * (8 // 2) == 36, H odd
    assert "latent grid" in lib.mc_last_error().decode()
    assert plan(e) == fresh(Hunyuan, H_B)[1]
    assert torch.equal(fwd(e, inp, FULL).cpu(), before)
    assert torch.equal(before, fresh(Hunyuan, H_B)[0]["fullNone"])


Q_PLAIN, Q_EDIT = (((1, 6, 8),), 48), (((1, 6, 8), (1, 4, 6)), 48)


def test_qwen_image_to_edit_and_back_both_cfg_branches():
    e = used(Qwen, Q_PLAIN)
    check_switched(Qwen, e, Q_EDIT)        # noisy + reference tokens; txt_valid 37 / 5 < txt_len 48
    inp = switch(Qwen, e, Q_PLAIN)
    fwd(e, inp, FULL, b=0)
    with pytest.raises(_lib.MagCacheHipError, match="residual cache is empty"):
        fwd(e, inp, SKIP, b=1)             # branch 1 has cached nothing since the switch
    e.reset()
    assert_same(probe(e, inp, Qwen.branches), fresh(Qwen, Q_PLAIN)[0])


# ------------------------------------------------------------------------------------------------ refusals and state
def test_plan_larger_than_the_bound_workspace_is_refused_and_nothing_changes():
    lib = _lib.load()
    e = Flux.engine(F2A)
    inp = Flux.inputs(F2A)
    e.set_rope(*inp.rope)
    before, plan0, bound = fwd(e, inp, FULL).cpu(), plan(e), e.ws.numel()
    need = e.geometry_bytes(*Flux.args(F1A))
    assert need > bound
    assert lib.mc_mmdit_set_geometry(e.h, F1A[0], 0, 0, 0, F1A[1]) == MC_EINVAL
    msg = lib.mc_last_error().decode()
    assert str(need) in msg and str(bound) in msg, msg
    assert plan(e) == plan0
    assert torch.equal(fwd(e, inp, FULL).cpu(), before)
    assert torch.equal(before, fresh(Flux, F2A)[0]["fullNone"])
    for bad in ((0, 40), (216, 0), (-5, 40)):
        assert lib.mc_mmdit_set_geometry(e.h, bad[0], 0, 0, 0, bad[1]) == MC_EINVAL
    assert torch.equal(fwd(e, inp, FULL).cpu(), before)


def test_set_geometry_inside_a_phase_forward_is_a_state_error():
    lib = _lib.load()
    e = Flux.engine(F2A)
    inp = Flux.inputs(F2A)
    e.set_rope(*inp.rope)
    e.begin(inp.img, 500.0, inp.guidance, inp.txt[0], inp.valid[0], inp.vec, FULL)
    assert lib.mc_mmdit_set_geometry(e.h, 200, 0, 0, 0, 40) == MC_ESTATE
    for blk in range(e.n_blocks):
        e.block_pre(blk)
        e.block_post(blk)
    out = torch.empty(F2A[0], 64, device=DEV)
    e.end(out)
    assert torch.equal(out.cpu(), fresh(Flux, F2A)[0]["fullNone"])
    e.set_geometry(200, ZERO, 40)          # legal again after mc_mmdit_end


def test_sequence_parallel_engine_keeps_its_geometry():
    lib = _lib.load()
    e = Flux.engine(F2B, weights=False, sp_rank=0, sp_size=2)
    assert lib.mc_mmdit_set_geometry(e.h, 512, 0, 0, 0, 256) == MC_EINVAL
    assert "sequence-parallel" in lib.mc_last_error().decode()
    assert e.geometry_bytes(512, ZERO, 256) > 0        # asking is allowed


def test_controlnet_samples_do_not_survive_the_switch():
    e = Flux.engine(F2A)
    inp = Flux.inputs(F2A)
    e.set_rope(*inp.rope)
    g = torch.Generator().manual_seed(9)
    e.set_controlnet([torch.randn(F2A[0], 256, generator=g).to(DEV)], [torch.randn(F2A[0], 256, generator=g).to(DEV)])
    assert not torch.equal(fwd(e, inp, FULL).cpu(), fresh(Flux, F2A)[0]["fullNone"])
    inp = switch(Flux, e, F1B)
    assert e._controlnet is None
    assert torch.equal(fwd(e, inp, FULL).cpu(), fresh(Flux, F1B)[0]["fullNone"])


def test_rope_table_is_the_identity_after_the_switch():
    e = used(Flux, F1A)                    # 768 table rows with real angles ...
    inp = switch(Flux, e, F1B, rope=False) # ... must not show through at 512
    want = fresh(Flux, F1B, rope=False)[0]
    assert_same(probe(e, inp), want)
    assert not torch.equal(want["fullNone"], fresh(Flux, F1B)[0]["fullNone"])
    e2 = used(Flux, F1B)                   # and a table that has to grow (512 -> 768 rows)
    inp = switch(Flux, e2, F1A, rope=False)
    assert_same(probe(e2, inp), fresh(Flux, F1A, rope=False)[0])


def test_reserve_keeps_the_workspace_and_the_results():
    a = used(Flux, F2A)
    need = a.reserve([Flux.args(F2A), Flux.args(F1A), dict(img_tokens=F1B[0], txt_len=F1B[1])])
    assert need == a.ws.numel() == max(a.geometry_bytes(*Flux.args(g)) for g in (F2A, F1A, F1B))
    ptr = a.workspace.data_ptr()
    for geo in (F1A, F1B, F2A):
        check_switched(Flux, a, geo)
        assert a.workspace.data_ptr() == ptr
    b = used(Flux, F2A)
    ptr = b.workspace.data_ptr()
    check_switched(Flux, b, F1A)           # grows: a new workspace tensor, the same results
    assert b.workspace.data_ptr() != ptr
    ptr = b.workspace.data_ptr()
    check_switched(Flux, b, F2A)           # fits: kept
    assert b.workspace.data_ptr() == ptr


# ------------------------------------------------------------------------------------------------ shims
def record(cls, pos):
    modes, base = [], cls.__mro__[1]._run

    def _run(self, *a):
        modes.append(a[pos])
        return base(self, *a)
    cls._run = _run
    return modes


def flux_calls(geo):
    inp = Flux.inputs(geo)
    li, lt = geo
    ids = torch.zeros(li, 3)
    ids[:, 1], ids[:, 2] = torch.arange(li) // 8, torch.arange(li) % 8
    kw = dict(hidden_states=inp.img[None], encoder_hidden_states=inp.txt[0][None], pooled_projections=inp.vec[None],
              img_ids=ids.to(DEV), txt_ids=torch.zeros(lt, 3, device=DEV), guidance=torch.tensor([4.0], device=DEV), return_dict=False)
    return [dict(kw, timestep=torch.tensor([t], device=DEV)) for t in (0.75, 0.5, 0.25)]


def flux_model(geo, **kw):
    m = type("FluxGeometry", (MM.FluxTransformer2DModelHIP,), {})(Flux.cfg, geo[0], txt_len=geo[1], device=DEV, **kw)
    m.load_state_dict(Flux.sd())
    return MM.init_flux_magcache(m, 3, 0.05, 5, 0.34, mag_ratios=[1.0, 0.99, 0.9])


def hunyuan_calls(geo):
    inp = Hunyuan.inputs(geo)
    mask = torch.zeros(1, geo[1], dtype=torch.long, device=DEV)
    mask[0, :23] = 1
    kw = dict(text_states=inp.txt[0][None], text_mask=mask, text_states_2=inp.vec[None], freqs_cos=inp.rope[0], freqs_sin=inp.rope[1],
              guidance=torch.tensor([6000.0], device=DEV), return_dict=False)
    return [dict(kw, x=inp.img[None], t=torch.tensor([t], device=DEV)) for t in (900.0, 600.0, 300.0)]


def hunyuan_model(geo, **kw):
    m = type("HunyuanGeometry", (MM.HYVideoDiffusionTransformerHIP,), {})(Hunyuan.cfg, geo[0], txt_len=geo[1], device=DEV, **kw)
    m.load_state_dict(Hunyuan.sd())
    return MM.init_hunyuan_magcache(m, 3, 0.05, 5, 0.34, mag_ratios=[1.0, 0.99, 0.9])


def qwen_calls(geo):
    inp = Qwen.inputs(geo)
    kw = dict(hidden_states=inp.img[None], img_shapes=[list(geo[0])], return_dict=False)
    return [dict(kw, encoder_hidden_states=inp.txt[i % 2][None], txt_seq_lens=[inp.valid[i % 2]],
                 timestep=torch.tensor([t], device=DEV)) for i, t in enumerate((0.75, 0.75, 0.5, 0.5, 0.25, 0.25))]


def qwen_model(geo, **kw):
    m = type("QwenGeometry", (MM.QwenImageTransformer2DModelHIP,), {})(Qwen.cfg, Qwen.tokens(geo[0]), txt_len=geo[1], device=DEV, **kw)
    m.load_state_dict(Qwen.sd())
    return MM.init_qwen_magcache(m, 3, 0.05, 5, 0.34, mag_ratios=[0.99, 0.99, 0.9, 0.9])


def sample(m, calls, modes):
    del modes[:]
    outs = [m(**c)[0].cpu() for c in calls]
    return outs, list(modes)


@pytest.mark.parametrize("model,calls,mode_pos,g1,g2,want_modes", [
    (flux_model, flux_calls, -1, F2A, F2B, [FULL, SKIP, FULL]),
    (hunyuan_model, hunyuan_calls, -1, H_A, H_B, [FULL, SKIP, FULL]),
    (qwen_model, qwen_calls, -2, Q_PLAIN, Q_EDIT, [FULL, FULL, SKIP, SKIP, FULL, FULL]),
], ids=["flux", "hunyuan", "qwen"])
def test_shims_follow_the_call_geometry(model, calls, mode_pos, g1, g2, want_modes):
    """two 3-step samples at two geometries back to back on ONE dynamic_geometry model: outputs and skip decisions of each
    equal those of a fresh model built at that geometry; a change in the middle of a sample is a ValueError"""
    dyn = model(g1, dynamic_geometry=True)
    modes = record(type(dyn), mode_pos)
    got = [sample(dyn, calls(g), modes) for g in (g1, g2)]
    assert dyn.cnt == 0
    for g, (outs, mo) in zip((g1, g2), got):
        ref = model(g)
        want, want_mo = sample(ref, calls(g), record(type(ref), mode_pos))
        assert mo == want_mo == want_modes
        for a, b in zip(outs, want):
            assert bool(torch.isfinite(b).all()) and torch.equal(a, b)
    dyn(**calls(g2)[0])
    assert dyn.cnt == 1
    with pytest.raises(ValueError, match="middle of a sample"):
        dyn(**calls(g1)[1])


def test_default_shims_still_assert_on_another_shape():
    m = flux_model(F2A)
    assert m.dynamic_geometry is False
    c = flux_calls(F2A)[0]
    with pytest.raises(AssertionError):
        m(**dict(c, hidden_states=c["hidden_states"][:, :50]))
    q = qwen_model(Q_PLAIN)
    with pytest.raises(AssertionError):
        q(**qwen_calls(Q_EDIT)[0])
    h = hunyuan_model(H_A)
    with pytest.raises(AssertionError):
        h(**hunyuan_calls(H_B)[0])
