"""GPU: mc_mmdit_config.fp8_linear (2 | 3) -- MX fp8 block Linears on the MM-DiT engine, FLUX, HunyuanVideo and Qwen-Image at toy
width 512 (4 heads: the MX GEMM needs K >= 512), synthetic weights of std 0.05.

The geometries make every guard work: ranges of 72 / 200 / 272 rows (FLUX, the image range starts at row 72), 144 + 64
(HunyuanVideo, the text range starts at row 144), 64 + 192 and 64 + 256 (Qwen-Image and -Edit, prompts of 37 and 5 rows) are
partial tiles off the 64-row grid of the scale images; FLUX at 512 + 256 has only exact multiples of 256.

References (tests/mmdit_fp8_ref.py): the plain fp32 oracle, and the fake-quant oracle whose chosen nn.Linears MX-quantise the
bf16-rounded input and weight.  On the CPU the fake-quant oracle is 4.5e-2 .. 6.2e-2 from the plain one on these inputs, so
the project's fp8 bar of 8e-2 (test_fp8_linear_option_forward_vs_oracle) leaves room for the engine's bf16 rounding and no more.

Distance of the engine from the fake-quant oracle (check 2): it cannot be derived, rounding differences flip quantisation bins
downstream.  Measured on the first green run (profiles/r10/MMDIT_FP8.md): 2.9e-2 .. 5.4e-2 over the cases and modes, the
largest at FLUX 512 + 256 in mode 3 (FQ_MEASURED); the bound is FQ_BAR = 1.5 x that = 8.1e-2.  The engine must also be closer
to the fake-quant oracle than to the plain one: it was, by a factor of 0.64 .. 0.81 in every case."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from magcache_amd import _lib  # noqa: E402
from magcache_amd import mmdit as MM  # noqa: E402

import mmdit_fp8_ref as R  # noqa: E402
from mmdit_fp8_ref import Flux, Hunyuan, Qwen, rel_l2  # noqa: E402

DEV = "cuda:0"
FULL, SKIP, CALIB = MM.MC_MODE_FULL, MM.MC_MODE_SKIP, MM.MC_MODE_CALIB
FP8_BAR = 8e-2
FQ_MEASURED = 5.4e-2
FQ_BAR = 1.5 * FQ_MEASURED

CASES = {"flux_odd": (Flux, R.FLUX_ODD), "flux_exact": (Flux, R.FLUX_EXACT), "hunyuan": (Hunyuan, R.HUNYUAN_GEO),
         "qwen": (Qwen, R.QWEN_GEO), "qwen_edit": (Qwen, R.QWEN_EDIT_GEO)}


def make_engine(fam, geo, mode, weights=True, **kw):
    args, extra = fam.engine_args(geo)
    e = MM.MMDiTEngine(*args, calibration=True, device=DEV, fp8_linear=mode, **extra, **kw)
    if weights:
        e.load_weights(fam.oracle().state_dict())
    return e


def dev_inputs(fam, geo):
    inp = fam.inputs(geo)
    inp.img, inp.txt = inp.img.to(DEV), [t.to(DEV) for t in inp.txt]
    inp.vec = inp.vec.to(DEV) if inp.vec is not None else None
    return inp


def fwd(e, inp, mode, t=500.0, b=None):
    k = b or 0
    return e.forward(inp.img, t, inp.guidance, inp.txt[k], inp.valid[k], inp.vec, mode=mode, branch=b)


_engines, _outs = {}, {}


def engine(case, mode):
    """the engine of (case, fp8_linear mode), created once with the RoPE of its geometry"""
    if (case, mode) not in _engines:
        fam, geo = CASES[case]
        e = make_engine(fam, geo, mode)
        e.set_rope(*fam.inputs(geo).rope)
        _engines[(case, mode)] = e
    return _engines[(case, mode)]


def full_out(case, mode, b):
    """FULL forward of that engine on the case's inputs (once; nobody changes the result)"""
    if (case, mode, b) not in _outs:
        fam, geo = CASES[case]
        _outs[(case, mode, b)] = fwd(engine(case, mode), dev_inputs(fam, geo), FULL, b=b).cpu()
    return _outs[(case, mode, b)]


def rows(e, name, dtype, width):
    return e.buffer(name, dtype).view(-1, width)


# ------------------------------------------------------------------------------------------------ 1, 2, 3, 6
@pytest.mark.parametrize("mode", [2, 3])
@pytest.mark.parametrize("case", list(CASES))
def test_forward_vs_plain_and_fake_quant_oracle(case, mode):
    fam, geo = CASES[case]
    for b in fam.branches:
        plain, fq = R.references(fam, geo, mode, b)
        got = full_out(case, mode, b)
        assert bool(torch.isfinite(got).all())
        e_plain, e_fq = rel_l2(got, plain), rel_l2(got, fq)
        print(f"{case} branch {b} mode {mode}: vs plain fp32 oracle {e_plain:.3e}, vs fake-quant oracle {e_fq:.3e}, "
              f"fake-quant vs plain {rel_l2(fq, plain):.3e}")
        assert e_plain < FP8_BAR                                           # check 1
        assert e_fq < FQ_BAR and e_fq < e_plain                            # check 2
        bf16 = full_out(case, 0, b)                                        # check 3: the mode is really on
        assert rel_l2(full_out(case, 2, b), bf16) > 1e-3
        if mode == 3:
            assert rel_l2(got, full_out(case, 2, b)) > 1e-4
    # check 6: the pad rows [S, S_pad) of "x" and "qkv" are still zero, bit for bit
    e = engine(case, mode)
    li, _, lt = fam.geometry(geo)
    s = li + lt
    x, qkv = rows(e, "x", torch.float32, R.DIM), rows(e, "qkv", torch.bfloat16, 3 * R.DIM)
    assert x.shape[0] % 256 == 0 and x.shape[0] >= s
    assert not bool(x[s:].view(torch.int32).any()) and not bool(qkv[s:].view(torch.int16).any())
    if fam is Qwen:   # text rows come first; those beyond the prompt are padding that must stay finite
        assert bool(torch.isfinite(x[:lt]).all()) and bool(torch.isfinite(qkv[:lt].float()).all())


# ------------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("mode", [2, 3])
@pytest.mark.parametrize("case", ["flux_odd", "hunyuan", "qwen"])
def test_fused_and_separate_quantisers_give_the_same_bits(case, mode):
    fam, geo = CASES[case]
    lib = _lib.load()
    e, inp = engine(case, mode), dev_inputs(fam, geo)
    b = fam.branches[0]
    fused = full_out(case, mode, b)
    try:
        _lib.check(lib.mc_set_option(b"fp8_fused_quant", 0))
        separate = fwd(e, inp, FULL, b=b).cpu()
    finally:
        _lib.check(lib.mc_set_option(b"fp8_fused_quant", 1))
    assert torch.equal(separate, fused)


# ------------------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize("mode", [2, 3])
@pytest.mark.parametrize("case", ["flux_odd", "hunyuan", "qwen"])
def test_skip_after_full_and_calibration(case, mode):
    fam, geo = CASES[case]
    e, inp = engine(case, mode), dev_inputs(fam, geo)
    e.reset()
    for b in fam.branches:
        full = fwd(e, inp, FULL, b=b).clone()
        skip = fwd(e, inp, SKIP, b=b)
        assert float((skip - full).abs().max()) < 1e-4 * float(full.abs().max())
    e.reset()
    for t in (500.0, 400.0):
        for b in fam.branches:
            fwd(e, inp, CALIB, t, b)
    stats = torch.tensor(e.calib_stats())
    assert bool(torch.isfinite(stats).all()) and float(stats[0]) > 0


# ------------------------------------------------------------------------------------------------ 7
def test_flux_controlnet_sample_on_the_last_single_block_mode_3():
    """the capture moves from the MX output GEMM's epilogue to the add launch: residual = x_final - x0 taken after the add"""
    fam, geo = CASES["flux_odd"]
    e, inp = engine("flux_odd", 3), dev_inputs(fam, geo)
    li, lt = geo
    g = torch.Generator().manual_seed(9)
    samples = [torch.randn(li, R.DIM, generator=g).to(DEV) for _ in range(2)]
    try:
        e.reset()
        e.set_controlnet(None, samples)
        out = fwd(e, inp, FULL).cpu()
        x = rows(e, "x", torch.float32, R.DIM)[lt:lt + li]
        x0 = rows(e, "x0", torch.bfloat16, R.DIM)[lt:lt + li]
        assert torch.equal(e.residual(), x - x0.float())
        assert rel_l2(out, full_out("flux_odd", 3, None)) > 1e-2
        skip = fwd(e, inp, SKIP).cpu()
        assert float((skip - out).abs().max()) < 1e-4 * float(out.abs().max())
    finally:
        e.set_controlnet()
        e.reset()
    assert torch.equal(fwd(e, inp, FULL).cpu(), full_out("flux_odd", 3, None))


# ------------------------------------------------------------------------------------------------ 8
def qwen_loop(mode):
    fam, geo = CASES["qwen"]
    cls = type("QwenFp8Loop%d" % mode, (MM.QwenImageTransformer2DModelHIP,), {})
    m = cls(Qwen.cfg, Qwen.tokens(geo[0]), txt_len=geo[1], device=DEV, fp8_linear=mode)
    m.load_state_dict(fam.oracle().state_dict())
    MM.init_qwen_magcache(m, sample_steps=6, magcache_thresh=0.06, K=2)
    modes, base = [], MM.QwenImageTransformer2DModelHIP._run

    def _run(self, *a):
        modes.append(a[-2])
        return base(self, *a)
    cls._run = _run
    inp = dev_inputs(fam, geo)
    outs = []
    for i in range(12):
        t = torch.tensor([1.0 - (i // 2) / 6.0], device=DEV)
        outs.append(m(hidden_states=inp.img[None], encoder_hidden_states=inp.txt[i % 2][None], txt_seq_lens=[inp.valid[i % 2]],
                      timestep=t, img_shapes=[list(geo[0])], return_dict=False)[0].cpu())
    return outs, modes


def test_qwen_magcache_loop_mode_2_keeps_the_skip_schedule():
    """six steps, two branches: the decision is host arithmetic on the table, so the skip list is the bf16 engine's"""
    ref, ref_modes = qwen_loop(0)
    got, got_modes = qwen_loop(2)
    assert got_modes == ref_modes and SKIP in ref_modes and FULL in ref_modes
    errs = [rel_l2(a, b) for a, b in zip(got, ref)]
    print("per-call relative L2, mode 2 vs the bf16 engine:", ["%.2e" % v for v in errs])
    assert max(errs) < FP8_BAR and max(errs) > 1e-3


# ------------------------------------------------------------------------------------------------ 9
@pytest.mark.parametrize("mode", [2, 3])
def test_switched_geometry_equals_a_fresh_engine(mode):
    fam = Flux
    e = make_engine(fam, R.FLUX_ODD, mode)
    inp = dev_inputs(fam, R.FLUX_ODD)
    e.set_rope(*inp.rope)
    fwd(e, inp, FULL)
    e.set_geometry(*fam.geometry(R.FLUX_EXACT))
    inp = dev_inputs(fam, R.FLUX_EXACT)
    e.set_rope(*inp.rope)
    out = fwd(e, inp, FULL).cpu()
    fresh = engine("flux_exact", mode)
    assert e.lib.mc_mmdit_workspace_bytes(e.h) == fresh.lib.mc_mmdit_workspace_bytes(fresh.h)
    assert e.geometry_bytes(*fam.geometry(R.FLUX_EXACT)) == fresh.lib.mc_mmdit_workspace_bytes(fresh.h)
    assert torch.equal(out, full_out("flux_exact", mode, None))
    res = e.residual().cpu()
    fwd(fresh, inp, FULL)
    assert torch.equal(res, fresh.residual().cpu())
    for name in ("aq", "a_mx"):
        assert e.buffer(name).numel() == fresh.buffer(name).numel() > 0


# ------------------------------------------------------------------------------------------------ 10
def test_refusals_and_the_first_struct_layout():
    lib = _lib.load()
    for bad in (1, 4, -1):
        with pytest.raises(_lib.MagCacheHipError) as ex:
            make_engine(Flux, R.FLUX_ODD, bad, weights=False)
        assert ex.value.status == _lib.MC_EINVAL and "fp8_linear" in str(ex.value)
    with pytest.raises(_lib.MagCacheHipError) as ex:   # width 256: the MX GEMM needs K >= 512
        MM.MMDiTEngine(MM.MC_FAMILY_FLUX, 256, 2, 1, 1, 64, 64, 256, 72, 128, 200, device=DEV, fp8_linear=2)
    assert ex.value.status == _lib.MC_EINVAL and "512" in str(ex.value)
    with pytest.raises(_lib.MagCacheHipError) as ex:
        make_engine(Flux, R.FLUX_EXACT, 2, weights=False, sp_rank=0, sp_size=2)
    assert ex.value.status == _lib.MC_EINVAL and "sp_size" in str(ex.value)
    # bf16 engines plan no fp8 buffers; mc_mmdit_create reads the first layout only, whatever stands behind sp_size
    bf16 = make_engine(Flux, R.FLUX_ODD, 0, weights=False)
    with pytest.raises(_lib.MagCacheHipError, match="unknown buffer"):
        bf16.buffer("aq")
    fp8 = make_engine(Flux, R.FLUX_ODD, 2, weights=False)
    assert lib.mc_mmdit_workspace_bytes(fp8.h) > lib.mc_mmdit_workspace_bytes(bf16.h)
    args, _ = Flux.engine_args(R.FLUX_ODD)
    names = [n for n, _ in _lib.McMmditConfig._fields_]
    c = _lib.McMmditConfig(**dict(zip(names, args)), calibration=1, sp_size=1, fp8_linear=2)
    h = C.c_void_p()
    _lib.check(lib.mc_mmdit_create(C.byref(c), C.byref(h)))
    try:
        assert lib.mc_mmdit_workspace_bytes(h) == lib.mc_mmdit_workspace_bytes(bf16.h)
        assert lib.mc_mmdit_buffer_info(h, b"aq", None, None) == _lib.MC_EINVAL
    finally:
        lib.mc_mmdit_destroy(h)
    old = C.sizeof(c) - 4
    for nbytes in (old - 4, C.sizeof(c) + 4, old + 2):
        assert lib.mc_mmdit_create_sized(C.byref(c), nbytes, C.byref(h)) == _lib.MC_EINVAL
