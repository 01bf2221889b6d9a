"""GPU: the option "mx_fp4" on the MM-DiT engine -- with mc_mmdit_config.fp8_linear 2 | 3 the MX Linears are MXFP4 (W4A4) on
launch_gemm_mxfp4, their operands written by the FP4 tail of the LayerNorm kernel and the EPI_GELU_MXFP4 epilogue.  FLUX,
HunyuanVideo and Qwen-Image at toy width 512, the cases, engines and oracles of tests/test_mmdit_fp8_gpu.py.

References: the plain fp32 oracle and the FP4 fake-quant oracle (tests/mmdit_mxfp4_ref.py), which is Q = 2.07e-1 .. 3.23e-1
from the plain one on these inputs (tests/test_mmdit_mxfp4_cpu.py).  MXFP4 is coarse: these are synthetic weights of std 0.05,
nothing here judges real weights, and the mode is opt-in.

Distance of the engine from the fake-quant oracle (check 2): it cannot be derived, rounding differences flip quantisation bins
downstream.  Measured on the first green run (profiles/r13/MMDIT_MXFP4.md, profiles/r13/tolerance_probe.json key
mmdit_mxfp4_vs_fake_quant): 1.25e-1 .. 2.58e-1 over the cases, modes and branches, 0.59 .. 0.81 of the engine's distance from
the plain oracle; FQ_MEASURED is the largest value and the bound is FQ_BAR = 1.5 x that = 3.87e-1, the margin
test_mmdit_fp8_gpu.py gives the same check.  The engine is deterministic: the margin covers compiler and box
differences only."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from magcache_amd import _lib  # noqa: E402
from magcache_amd import mmdit as MM  # noqa: E402

import hip_ops as H  # noqa: E402
import mmdit_fp8_ref as R  # noqa: E402
import mmdit_mxfp4_ref as R4  # noqa: E402
import mxfp4_ref as F4  # noqa: E402
import test_mmdit_fp8_gpu as G8  # noqa: E402  (its cases and its cache of bf16 / MX fp8 engines and outputs)
from conftest import tolerance_probe  # noqa: E402
from mmdit_fp8_ref import Flux, Hunyuan, Qwen, rel_l2  # noqa: E402
from test_mmdit_lora_gpu import lora_sd, merged_state_dict  # noqa: E402

DEV = G8.DEV
CASES = G8.CASES
FULL, SKIP, CALIB = MM.MC_MODE_FULL, MM.MC_MODE_SKIP, MM.MC_MODE_CALIB
D = R.DIM
FQ_MEASURED = 2.58e-1   # FLUX 512 + 256 in mode 3; the smallest was 1.25e-1 (Qwen-Image-Edit, mode 2)
FQ_BAR = 1.5 * FQ_MEASURED


def option(v=None):
    lib = _lib.load()
    if v is not None:
        _lib.check(lib.mc_set_option(b"mx_fp4", v))
    got = C.c_int(-1)
    _lib.check(lib.mc_get_option(b"mx_fp4", C.byref(got)))
    return got.value


def bits(t):
    return t.detach().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16 if t.element_size() == 2 else torch.uint8).cpu()


_engines, _outs, _measured = {}, {}, {}


def engine(case, mode):
    """the MXFP4 engine of (case, fp8_linear mode), created once with the RoPE of its geometry"""
    if (case, mode) not in _engines:
        fam, geo = CASES[case]
        e = G8.make_engine(fam, geo, mode, mx_fp4=True)
        assert e.mx_fp4 is True
        e.set_rope(*fam.inputs(geo).rope)
        _engines[(case, mode)] = e
    return _engines[(case, mode)]


def full_out(case, mode, b):
    if (case, mode, b) not in _outs:
        fam, geo = CASES[case]
        _outs[(case, mode, b)] = G8.fwd(engine(case, mode), G8.dev_inputs(fam, geo), FULL, b=b).cpu()
    return _outs[(case, mode, b)]


def row_ranges(fam, geo):
    """(first image row, image rows, first text row, text rows) of the joint buffers"""
    li, _, lt = fam.geometry(geo)
    return (0, li, li, lt) if fam is Hunyuan else (lt, li, 0, lt)


# ------------------------------------------------------------------------------------------------ 1
def test_option_is_latched_by_create():
    lib = _lib.load()
    fam, geo = CASES["flux_odd"]
    inp = G8.dev_inputs(fam, geo)
    rope = fam.inputs(geo).rope

    def make(mode, **kw):
        e = G8.make_engine(fam, geo, mode, **kw)
        e.set_rope(*rope)
        return e

    def run(e):
        return bits(G8.fwd(e, inp, FULL))
    want8, want16 = bits(G8.full_out("flux_odd", 2, None)), bits(G8.full_out("flux_odd", 0, None))
    assert option() == 0
    try:
        option(1)
        under, bf16_under = make(2), make(0)
    finally:
        option(0)
    after = make(2)
    assert lib.mc_mmdit_mx_fp4(under.h) == 1 and under.mx_fp4 is True
    assert lib.mc_mmdit_mx_fp4(bf16_under.h) == 0 and bf16_under.mx_fp4 is False
    assert lib.mc_mmdit_mx_fp4(after.h) == 0 and after.mx_fp4 is False
    got4 = run(under)                                   # after the reset: the engine kept what it read
    assert lib.mc_mmdit_mx_fp4(under.h) == 1
    assert not torch.equal(got4, want8) and not torch.equal(got4, want16)
    assert torch.equal(run(after), want8), "an engine created after the reset must be the MX fp8 engine"
    assert torch.equal(run(bf16_under), want16), "the option must do nothing to a bf16 engine"
    # the Python keyword: set around the create call only, the previous value (0 or 1) put back
    kw = make(2, mx_fp4=True)
    assert option() == 0 and kw.mx_fp4 is True and torch.equal(run(kw), got4)
    assert torch.equal(got4, bits(full_out("flux_odd", 2, None)))
    assert make(0, mx_fp4=True).mx_fp4 is False and option() == 0
    try:
        option(1)
        stands = make(2, mx_fp4=False)                  # no explicit request: the process-wide value stands
        assert option() == 1 and stands.mx_fp4 is True
    finally:
        option(0)
    shim = MM.FluxTransformer2DModelHIP(Flux.cfg, geo[0], txt_len=geo[1], device=DEV, calibration=False, fp8_linear=3, mx_fp4=True)
    assert shim.engine.mx_fp4 is True and shim.engine.fp8_linear == 3 and option() == 0


# ------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("mode", [2, 3])
@pytest.mark.parametrize("case", list(CASES))
def test_forward_vs_plain_and_fake_quant_oracle(case, mode):
    fam, geo = CASES[case]
    for b in fam.branches:
        plain, fq = R4.references(fam, geo, mode, b)
        got = full_out(case, mode, b)
        assert bool(torch.isfinite(got).all())
        q = rel_l2(fq, plain)
        e_plain, e_fq = rel_l2(got, plain), rel_l2(got, fq)
        e16, e8 = rel_l2(G8.full_out(case, 0, b), plain), rel_l2(G8.full_out(case, mode, b), plain)
        print(f"{case} branch {b} mode {mode}: vs plain fp32 oracle {e_plain:.3e}, vs FP4 fake-quant oracle {e_fq:.3e}, "
              f"fake-quant vs plain (Q) {q:.3e}; bf16 engine {e16:.3e}, MX fp8 engine {e8:.3e} vs plain")
        _measured[f"{case}/mode{mode}/branch{b}"] = dict(e_fq=e_fq, e_plain=e_plain, q=q, e_bf16=e16, e_mxfp8=e8)
        tolerance_probe("mmdit_mxfp4_vs_fake_quant", _measured)
        assert R4.Q_BAND[0] <= q <= R4.Q_BAND[1]
        assert e_fq < e_plain                       # the engine is the quantised model, not the plain one
        assert e_plain < 2 * q                      # a wrong scale or nibble order gives O(1)
        assert e16 < e8 < e_plain
        assert e_fq < FQ_BAR
    # the pad rows [S, S_pad) of "x" and "qkv" are still zero, bit for bit
    e = engine(case, mode)
    li, _, lt = fam.geometry(geo)
    s = li + lt
    x, qkv = G8.rows(e, "x", torch.float32, D), G8.rows(e, "qkv", torch.bfloat16, 3 * D)
    assert x.shape[0] % 256 == 0 and x.shape[0] >= s
    assert not bool(x[s:].view(torch.int32).any()) and not bool(qkv[s:].view(torch.int16).any())
    # what is really planned: packed rows of 5 dim / 2 bytes, the scale image of the MX fp8 engine
    e8 = G8.engine(case, mode)
    assert e.buffer("aq").numel() == x.shape[0] * 5 * D // 2 and e8.buffer("aq").numel() == x.shape[0] * 5 * D
    assert e.buffer("a_mx").numel() == e8.buffer("a_mx").numel()
    assert e.geometry_bytes(*fam.geometry(geo)) == e.lib.mc_mmdit_workspace_bytes(e.h) < e8.lib.mc_mmdit_workspace_bytes(e8.h)


# ------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("mode", [2, 3])
@pytest.mark.parametrize("case", ["flux_odd", "hunyuan", "qwen"])
def test_fused_and_separate_quantisers_give_the_same_bits(case, mode):
    fam, geo = CASES[case]
    lib = _lib.load()
    e, inp = engine(case, mode), G8.dev_inputs(fam, geo)
    b = fam.branches[0]
    img0, li, txt0, lt = row_ranges(fam, geo)

    def operands():
        """the valid rows of "aq" (packed) and every scale byte of "a_mx" that belongs to a valid row"""
        aq = e.buffer("aq").view(-1, 5 * D // 2)
        amx = e.buffer("a_mx")
        ltp, lip, sp = F4.ceil256(lt), F4.ceil256(li), aq.shape[0]
        blocks = 5 * D // 32 + (D // 32 if mode == 3 else 0)
        regions = [(0, blocks, ltp, lt), (blocks * ltp, blocks, lip, li), (blocks * (ltp + lip), 5 * D // 32, sp, li + lt)]
        scales = [amx[o:o + n * pad].view(n, pad)[:, F4.mx_perm(torch.arange(rows, device=DEV))].cpu() for o, n, pad, rows in regions]
        return aq[:li + lt].cpu(), scales
    e.buffer("aq").fill_(0xA5)
    e.buffer("a_mx").fill_(0xA5)
    fused = bits(G8.fwd(e, inp, FULL, b=b))
    aq_f, mx_f = operands()
    assert torch.equal(fused, bits(full_out(case, mode, b)))
    try:
        _lib.check(lib.mc_set_option(b"fp8_fused_quant", 0))
        e.buffer("aq").fill_(0xA5)
        e.buffer("a_mx").fill_(0xA5)
        separate = bits(G8.fwd(e, inp, FULL, b=b))
        aq_s, mx_s = operands()
    finally:
        _lib.check(lib.mc_set_option(b"fp8_fused_quant", 1))
    assert torch.equal(separate, fused)
    assert torch.equal(aq_s, aq_f) and bool((aq_f != 0xA5).any())
    for s_sep, s_fus in zip(mx_s, mx_f):
        assert torch.equal(s_sep, s_fus)


# ------------------------------------------------------------------------------------------------ 4
def test_first_linear_equals_the_single_ops_by_hand():
    """FLUX 200 + 72: the image range starts at joint row 72, off the 64-row grid of the scale images"""
    fam, geo = CASES["flux_odd"]
    lib = _lib.load()
    e, inp = engine("flux_odd", 2), G8.dev_inputs(fam, geo)
    img0, li, _, _ = row_ranges(fam, geo)
    sd = fam.oracle().state_dict()
    try:
        _lib.check(lib.mc_set_option(b"fp8_fused_quant", 0))
        e.begin(inp.img, 500.0, inp.guidance, inp.txt[0], inp.valid[0], inp.vec, FULL)
        e.block_pre(0)
        torch.cuda.synchronize()
        xn = G8.rows(e, "xn", torch.bfloat16, D)[img0:img0 + li].clone()
        got = G8.rows(e, "qkv", torch.bfloat16, 3 * D)[img0:img0 + li].clone()
        aq_engine = e.buffer("aq").view(-1, 5 * D // 2)[img0:img0 + li, :D // 2].clone()
        for blk in range(e.n_blocks):                    # finish the forward: the engine is shared
            if blk:
                e.block_pre(blk)
            e.block_post(blk)
        e.end(torch.empty(li, 64, device=DEV))
        torch.cuda.synchronize()
    finally:
        _lib.check(lib.mc_set_option(b"fp8_fused_quant", 1))
    p = "transformer_blocks.0.attn."
    w = torch.cat([sd[p + n + ".weight"] for n in ("to_q", "to_k", "to_v")]).to(torch.bfloat16).to(DEV).contiguous()
    bias = torch.cat([sd[p + n + ".bias"] for n in ("to_q", "to_k", "to_v")]).float().to(DEV).contiguous()
    aq, sa = F4.op_quantize(xn)
    wq, sw = F4.op_quantize(w, rows_pad=3 * D)
    want = torch.zeros(li, 3 * D, dtype=torch.bfloat16, device=DEV)
    F4.op_gemm(aq, sa, wq, sw, bias, 0, Cb=want)
    assert torch.equal(aq_engine, aq), "the engine's operand rows are the op's bits"
    assert torch.equal(bits(got[:, 2 * D:]), bits(want[:, 2 * D:])), "v rows (no head norm, no RoPE)"
    # block_pre applies the per-head norm and RoPE to q | k: the shipped op on the hand result, with the image rows' table
    cos, sin = (t.float().to(DEV).contiguous() for t in fam.inputs(geo).rope)
    cs = torch.zeros(li, 128, dtype=torch.float32, device=DEV)
    H.rope_table_from_cos_sin(cos[img0:], sin[img0:], li, cs)
    H.headnorm_rope(want, D, sd[p + "norm_q.weight"].float().to(DEV).contiguous(), sd[p + "norm_k.weight"].float().to(DEV).contiguous(),
                    1e-6, cs, 0, R.HEADS)
    torch.cuda.synchronize()
    assert torch.equal(bits(got), bits(want)), "q | k | v rows"
    assert float(got.float().abs().max()) > 0


# ------------------------------------------------------------------------------------------------ 5
def head_by_hand(fam, geo, e, x):
    """the final layer on fp32 rows x [Li, d] in float64: LayerNorm without affine, modulated by the engine's own "emod" rows,
    times the head weights (HunyuanVideo: in the engine's (ph, pw, c) column order, as "head_tokens" holds them)"""
    args, _ = fam.engine_args(geo)
    n_double, n_single = args[3], args[4]
    off = n_double * 12 * D + n_single * 3 * D
    mf = e.buffer("emod", torch.float32)[off:off + 2 * D].double().cpu()
    hy = fam is Hunyuan
    scale, shift = (mf[D:], mf[:D]) if hy else (mf[:D], mf[D:])
    sd = fam.oracle().state_dict()
    name = "final_layer.linear." if hy else "proj_out."
    w, b = sd[name + "weight"].double(), sd[name + "bias"].double()
    if hy:
        c = w.shape[0] // 4
        w, b = w.view(c, 4, D).permute(1, 0, 2).reshape(4 * c, D), b.view(c, 4).t().reshape(4 * c)
    x = x.double().cpu()
    n = torch.nn.functional.layer_norm(x, (D,), eps=1e-6)
    return (n * (1 + scale) + shift) @ w.t() + b


@pytest.mark.parametrize("case", ["flux_odd", "hunyuan", "qwen"])
def test_full_skip_and_calibration(case):
    fam, geo = CASES[case]
    e, inp = engine(case, 3), G8.dev_inputs(fam, geo)
    b = fam.branches[0]
    img0, li, _, _ = row_ranges(fam, geo)
    e.reset()
    full = G8.fwd(e, inp, FULL, b=b).clone()
    x = G8.rows(e, "x", torch.float32, D)[img0:img0 + li].clone()
    x0 = G8.rows(e, "x0", torch.bfloat16, D)[img0:img0 + li].clone()
    res = e.residual(b).clone()
    assert torch.equal(bits(res), bits(x - x0.float())), "residual = x_final - x0 of the FP4 forward"
    assert torch.equal(bits(full), bits(full_out(case, 3, b)))
    # SKIP: the head applied to x0 + residual (fp32 kernels against float64: 2e-5 of the largest output covers the fp32
    # LayerNorm and a 512-term fp32 dot product, and is 1e-4 of what separates SKIP from a forward with other weights)
    skip = G8.fwd(e, inp, SKIP, b=b).clone()
    assert torch.equal(bits(e.residual(b)), bits(res))
    want = head_by_hand(fam, geo, e, x0.float() + res)
    got = e.buffer("head_tokens", torch.float32).view(li, 64)[:, :want.shape[1]] if fam is Hunyuan else skip
    err = float((got.double().cpu() - want).abs().max())
    print(f"{case}: SKIP head vs float64 by hand: max abs {err:.3e} of {float(want.abs().max()):.3e}")
    assert err < 2e-5 * float(want.abs().max())
    assert float((skip - full).abs().max()) < 1e-4 * float(full.abs().max())
    # CALIB at another timestep: the three statistics from the two residual buffers, in float64
    G8.fwd(e, inp, CALIB, 400.0, b)
    stats = e.calib_stats()
    new = e.residual(b)
    slots = [G8.rows(e, n, torch.float32, D)[img0:img0 + li] for n in ("residual0", "residual1")]
    prev = [s for s in slots if s.data_ptr() != new.data_ptr()]
    assert len(prev) == 1 and torch.equal(bits(prev[0]), bits(res))
    r, rp = new.double().cpu(), prev[0].double().cpu()
    rho = r.norm(dim=1) / rp.norm(dim=1)
    cos = (r * rp).sum(dim=1) / (r.norm(dim=1) * rp.norm(dim=1))
    want_stats = (float(rho.mean()), float(rho.std()), float((1 - cos).mean()))
    print(f"{case}: calibration statistics {stats} vs torch {want_stats}")
    for got_v, want_v, atol in zip(stats, want_stats, (1e-3, 5e-4, 4e-4)):     # the bars of test_mmdit_gpu.py's calibration tests
        assert abs(got_v - want_v) <= atol
    assert stats[0] > 0
    e.reset()


# ------------------------------------------------------------------------------------------------ 6
def test_lora_adapters_equal_host_merged_weights_bitwise_mode_3():
    """FLUX toy, fp8_linear 3: every target below runs on its MXFP4 copy, so the identity holds only if the packed rows and the
    block scales of exactly the touched rows were requantised from the merged rows"""
    fam, geo = Flux, R.FLUX_ODD
    sd = {k: v.detach() for k, v in fam.oracle().state_dict().items()}
    inp = G8.dev_inputs(fam, geo)
    rope = fam.inputs(geo).rope

    def make(weights):
        e = G8.make_engine(fam, geo, 3, weights=False, mx_fp4=True)
        e.load_weights(weights)
        e.set_rope(*rope)
        return e

    def run(e):
        return bits(G8.fwd(e, inp, FULL))
    targets = ["transformer_blocks.0.attn.to_k", "transformer_blocks.1.attn.add_q_proj", "transformer_blocks.0.ff.net.0.proj",
               "transformer_blocks.1.ff_context.net.2", "single_transformer_blocks.0.proj_mlp", "single_transformer_blocks.1.attn.to_v",
               "transformer_blocks.1.attn.to_out.0", "single_transformer_blocks.1.proj_out"]
    la = lora_sd(sd, targets, 4, seed=8, alpha=8)
    lb = lora_sd(sd, targets[:2], 24, seed=9, alpha=12)
    e = make(sd)
    base_out = run(e)
    assert torch.equal(base_out, bits(full_out("flux_odd", 3, None)))
    assert e.load_lora(la, adapter="a") == [] and e.load_lora(lb, adapter="b", scale=-2.0) == []
    got = run(e)
    assert torch.equal(got, run(make(merged_state_dict(sd, [(la, 1.0), (lb, -2.0)]))))
    assert not torch.equal(got, base_out)
    e.unload_lora()                                        # ... and requantised back
    assert torch.equal(run(e), base_out)
    # set_weight after create: the MXFP4 copy follows the bf16 weight
    name = "transformer_blocks.0.ff.net.2.weight"
    e.set_weight(name, sd[name] * 1.5)
    changed = run(e)
    assert not torch.equal(changed, base_out)
    e.set_weight(name, sd[name])
    assert torch.equal(run(e), base_out)


def test_flux_controlnet_sample_on_the_last_single_block_mode_3():
    """as on the MX fp8 engine: the capture moves from the MXFP4 output GEMM's epilogue to the add launch"""
    fam, geo = CASES["flux_odd"]
    e, inp = engine("flux_odd", 3), G8.dev_inputs(fam, geo)
    li, lt = geo
    g = torch.Generator().manual_seed(9)
    samples = [torch.randn(li, D, generator=g).to(DEV) for _ in range(2)]
    try:
        e.reset()
        e.set_controlnet(None, samples)
        out = G8.fwd(e, inp, FULL).cpu()
        x = G8.rows(e, "x", torch.float32, D)[lt:lt + li]
        x0 = G8.rows(e, "x0", torch.bfloat16, D)[lt:lt + li]
        assert torch.equal(bits(e.residual()), bits(x - x0.float()))
        assert rel_l2(out, full_out("flux_odd", 3, None)) > 1e-2
    finally:
        e.set_controlnet()
        e.reset()
    assert torch.equal(bits(G8.fwd(e, inp, FULL)), bits(full_out("flux_odd", 3, None)))


@pytest.mark.parametrize("mode", [2, 3])
def test_switched_geometry_equals_fresh_engines(mode):
    fam = Flux
    e = G8.make_engine(fam, R.FLUX_ODD, mode, mx_fp4=True)
    e.reserve([fam.geometry(R.FLUX_ODD), fam.geometry(R.FLUX_EXACT)])
    for geo, case in ((R.FLUX_EXACT, "flux_exact"), (R.FLUX_ODD, "flux_odd")):
        e.ws.fill_(0xFF)                                   # NaN in every float format: nothing of the old plan may be read
        e.set_geometry(*fam.geometry(geo))
        inp = G8.dev_inputs(fam, geo)
        e.set_rope(*inp.rope)
        out = bits(G8.fwd(e, inp, FULL))
        fresh = engine(case, mode)
        assert e.geometry_bytes(*fam.geometry(geo)) == fresh.lib.mc_mmdit_workspace_bytes(fresh.h) == e.lib.mc_mmdit_workspace_bytes(e.h)
        assert torch.equal(out, bits(full_out(case, mode, None))), case
        for name in ("aq", "a_mx"):
            assert e.buffer(name).numel() == fresh.buffer(name).numel() > 0
        assert e.mx_fp4 is True


# ------------------------------------------------------------------------------------------------ 7
def test_refusals():
    lib = _lib.load()
    with pytest.raises(_lib.MagCacheHipError) as ex:       # 5 heads: dim 640 is no multiple of the MXFP4 GEMM's K tile
        MM.MMDiTEngine(MM.MC_FAMILY_FLUX, 640, 5, 1, 1, 64, 64, 256, 72, 128, 200, device=DEV, fp8_linear=2, mx_fp4=True)
    msg = str(ex.value)
    assert ex.value.status == _lib.MC_EINVAL and "640" in msg and "mx_fp4" in msg and "q|k|v" in msg and "in_features" in msg
    assert "640" in lib.mc_last_error().decode()
    with pytest.raises(_lib.MagCacheHipError) as ex:
        G8.make_engine(Flux, R.FLUX_EXACT, 2, weights=False, sp_rank=0, sp_size=2, mx_fp4=True)
    assert ex.value.status == _lib.MC_EINVAL and "sp_size" in str(ex.value)
    assert option() == 0                                   # a create that failed put the option back too
