"""GPU: the option "mx_fp6" on the MM-DiT engine -- with mc_mmdit_config.fp8_linear 2 | 3 the MX Linears are MXFP6 (W6A6, OCP
e2m3) on launch_gemm_mxfp6, their operands always written by separate quantise passes.  The smallest FLUX-family and
Qwen-family toys of tests/test_mmdit_mxfp4_gpu.py (FLUX 200 + 72 tokens, Qwen-Image 192 + 64; width 512).

  1. latch and refusals: the create call latches the option (other bits than the MX fp8 engine; an engine created after the
     reset is the MX fp8 engine again); a width that is no multiple of 256 names the Linear; sp_size 2; both formats at once;
  2. one double block's q|k|v Linear by hand from the single ops, bit for bit;
  3. a single block's linear2 by hand (mode 3): it reads the whole packed "aq" row of 5 dim * 3 / 4 bytes -- [attention |
     GELU(MLP-in)] -- with the joint range's scale image;
  4. the forward is identical under fp8_fused_quant 0 and 1 (there is no fused FP6 producer);
  5. against the fp32 oracle the errors are ordered bf16 < {MX fp8, MXFP6} < MXFP4, MXFP6 <= 1.5 x MX fp8 and <= 0.5 x MXFP4 of
     the same run, and MXFP6 stays below 1.5 x its measured distance (profiles/r14/tolerance_probe.json:
     mmdit_mxfp6_vs_fp32_oracle; the oracles' synthetic weights of std 0.05 and the inputs of the cases, seeds in
     tests/mmdit_fp8_ref.py)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from magcache_amd import _lib  # noqa: E402
from magcache_amd import mmdit as MM  # noqa: E402

import hip_ops as H  # noqa: E402
import mmdit_fp8_ref as R  # noqa: E402
import mxfp6_ref as F6  # noqa: E402
import test_mmdit_fp8_gpu as G8  # noqa: E402  (its cases and its cache of bf16 / MX fp8 engines and outputs)
from conftest import tolerance_probe  # noqa: E402
from mmdit_fp8_ref import Flux, rel_l2  # noqa: E402

DEV = G8.DEV
CASES = {k: G8.CASES[k] for k in ("flux_odd", "qwen")}
FULL = MM.MC_MODE_FULL
D = R.DIM
EPI_RESID = 2
# measured on MI355X (profiles/r14/tolerance_probe.json: mmdit_mxfp6_vs_fp32_oracle), the largest over the cases and modes; the
# bar is 1.5 x this
MXFP6_REL_L2_MEASURED = 7.10e-2   # FLUX 200 + 72 in mode 3; the smallest was 4.94e-2 (Qwen-Image, mode 2)


def option(v=None, key=b"mx_fp6"):
    lib = _lib.load()
    if v is not None:
        _lib.check(lib.mc_set_option(key, v))
    got = C.c_int(-1)
    _lib.check(lib.mc_get_option(key, C.byref(got)))
    return got.value


def bits(t):
    return t.detach().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16 if t.element_size() == 2 else torch.uint8).cpu()


_engines, _outs, _plain, _measured = {}, {}, {}, {}


def engine(case, mode):
    """the MXFP6 engine of (case, fp8_linear mode), created once with the RoPE of its geometry"""
    if (case, mode) not in _engines:
        fam, geo = CASES[case]
        e = G8.make_engine(fam, geo, mode, mx_fp6=True)
        assert e.mx_fp6 is True and e.mx_fp4 is False
        e.set_rope(*fam.inputs(geo).rope)
        _engines[(case, mode)] = e
    return _engines[(case, mode)]


def full_out(case, mode, b):
    if (case, mode, b) not in _outs:
        fam, geo = CASES[case]
        _outs[(case, mode, b)] = G8.fwd(engine(case, mode), G8.dev_inputs(fam, geo), FULL, b=b).cpu()
    return _outs[(case, mode, b)]


def plain_oracle(case, b):
    if (case, b) not in _plain:
        fam, geo = CASES[case]
        _plain[(case, b)] = fam.reference(fam.oracle(), geo, fam.inputs(geo), b or 0)
    return _plain[(case, b)]


# ------------------------------------------------------------------------------------------------ 1
def test_option_is_latched_by_create_and_refusals():
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
    assert option() == 0 and option(key=b"mx_fp4") == 0
    try:
        option(1)
        under, bf16_under = make(2), make(0)
        option(1, key=b"mx_fp4")                        # both element formats: refused, and the message names both options
        with pytest.raises(_lib.MagCacheHipError) as ex:
            make(2)
        assert ex.value.status == _lib.MC_EINVAL and "mx_fp4" in str(ex.value) and "mx_fp6" in str(ex.value)
    finally:
        option(0)
        option(0, key=b"mx_fp4")
    after = make(2)
    assert lib.mc_mmdit_mx_fp6(under.h) == 1 and under.mx_fp6 is True and lib.mc_mmdit_mx_fp4(under.h) == 0
    assert lib.mc_mmdit_mx_fp6(bf16_under.h) == 0 and bf16_under.mx_fp6 is False
    assert lib.mc_mmdit_mx_fp6(after.h) == 0 and after.mx_fp6 is False
    got6 = run(under)                                   # after the reset: the engine kept what it read
    assert not torch.equal(got6, want8) and not torch.equal(got6, want16)
    assert torch.equal(run(after), want8), "an engine created after the reset must be the MX fp8 engine"
    assert torch.equal(run(bf16_under), want16), "the option must do nothing to a bf16 engine"
    # the Python keyword: set around the create call only, the previous value put back
    kw = make(2, mx_fp6=True)
    assert option() == 0 and kw.mx_fp6 is True and torch.equal(run(kw), got6)
    assert torch.equal(got6, bits(full_out("flux_odd", 2, None)))
    assert make(0, mx_fp6=True).mx_fp6 is False and option() == 0
    shim = MM.FluxTransformer2DModelHIP(Flux.cfg, geo[0], txt_len=geo[1], device=DEV, calibration=False, fp8_linear=3, mx_fp6=True)
    assert shim.engine.mx_fp6 is True and shim.engine.fp8_linear == 3 and option() == 0
    # what is really planned: packed rows of 5 dim * 3 / 4 bytes, the scale image of the MX fp8 engine
    e8 = G8.engine("flux_odd", 2)
    n_rows = G8.rows(under, "x", torch.float32, D).shape[0]
    assert under.buffer("aq").numel() == n_rows * 5 * D * 3 // 4 and e8.buffer("aq").numel() == n_rows * 5 * D
    assert under.buffer("a_mx").numel() == e8.buffer("a_mx").numel()
    # ---- refusals
    with pytest.raises(_lib.MagCacheHipError) as ex:       # 5 heads: dim 640 is no multiple of 256
        MM.MMDiTEngine(MM.MC_FAMILY_FLUX, 640, 5, 1, 1, 64, 64, 256, 72, 128, 200, device=DEV, fp8_linear=2, mx_fp6=True)
    msg = str(ex.value)
    assert ex.value.status == _lib.MC_EINVAL and "640" in msg and "mx_fp6" in msg and "q|k|v" in msg and "in_features" in msg
    assert "640" in lib.mc_last_error().decode()
    with pytest.raises(_lib.MagCacheHipError) as ex:
        G8.make_engine(Flux, R.FLUX_EXACT, 2, weights=False, sp_rank=0, sp_size=2, mx_fp6=True)
    assert ex.value.status == _lib.MC_EINVAL and "sp_size" in str(ex.value)
    with pytest.raises(_lib.MagCacheHipError) as ex:
        make(2, mx_fp4=True, mx_fp6=True)
    assert ex.value.status == _lib.MC_EINVAL
    assert option() == 0 and option(key=b"mx_fp4") == 0    # a create that failed put the options back too


# ------------------------------------------------------------------------------------------------ 2
def test_double_block_qkv_equals_the_single_ops_by_hand():
    """FLUX 200 + 72: the image range starts at joint row 72, off the 64-row grid of the scale images"""
    fam, geo = CASES["flux_odd"]
    e, inp = engine("flux_odd", 2), G8.dev_inputs(fam, geo)
    li, lt = geo
    img0 = lt
    sd = fam.oracle().state_dict()
    kb = D * 3 // 4
    e.begin(inp.img, 500.0, inp.guidance, inp.txt[0], inp.valid[0], inp.vec, FULL)
    e.block_pre(0)
    torch.cuda.synchronize()
    xn = G8.rows(e, "xn", torch.bfloat16, D)[img0:img0 + li].clone()
    got = G8.rows(e, "qkv", torch.bfloat16, 3 * D)[img0:img0 + li].clone()
    aq_engine = e.buffer("aq").view(-1, 5 * kb)[img0:img0 + li, :kb].clone()
    for blk in range(e.n_blocks):                    # finish the forward: the engine is shared
        if blk:
            e.block_pre(blk)
        e.block_post(blk)
    e.end(torch.empty(li, 64, device=DEV))
    torch.cuda.synchronize()
    p = "transformer_blocks.0.attn."
    w = torch.cat([sd[p + n + ".weight"] for n in ("to_q", "to_k", "to_v")]).to(torch.bfloat16).to(DEV).contiguous()
    bias = torch.cat([sd[p + n + ".bias"] for n in ("to_q", "to_k", "to_v")]).float().to(DEV).contiguous()
    aq, sa = F6.op_quantize(xn)
    wq, sw = F6.op_quantize(w, rows_pad=3 * D)
    want = torch.zeros(li, 3 * D, dtype=torch.bfloat16, device=DEV)
    F6.op_gemm(aq, sa, wq, sw, bias, 0, Cb=want)
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


# ------------------------------------------------------------------------------------------------ 3
def test_single_block_linear2_equals_the_single_ops_by_hand():
    """mode 3, the first single block (not the last block: no residual capture): x += gate * bf16(proj_out([attention | GELU]))"""
    fam, geo = CASES["flux_odd"]
    e, inp = engine("flux_odd", 3), G8.dev_inputs(fam, geo)
    li, lt = geo
    S = li + lt
    args, _ = fam.engine_args(geo)
    n_double, n_single = args[3], args[4]
    assert n_single >= 2
    blk = n_double
    sd = fam.oracle().state_dict()
    kb = 5 * D * 3 // 4
    e.begin(inp.img, 500.0, inp.guidance, inp.txt[0], inp.valid[0], inp.vec, FULL)
    for b in range(blk):
        e.block_pre(b)
        e.block_post(b)
    e.block_pre(blk)
    torch.cuda.synchronize()
    x_before = G8.rows(e, "x", torch.float32, D)[:S].clone()
    e.buffer("aq").fill_(0xA5)
    e.block_post(blk)
    torch.cuda.synchronize()
    x_after = G8.rows(e, "x", torch.float32, D)[:S].clone()
    am = G8.rows(e, "am", torch.bfloat16, 5 * D)[:S].clone()
    aq_rows = e.buffer("aq").view(-1, kb)
    Sp = aq_rows.shape[0]
    aq_engine = aq_rows[:S].clone()
    # the joint range's scale image: behind the text and image regions of "a_mx" (mode 3: 5 d / 32 + d / 32 blocks each)
    ltp, lip = F6.ceil256(lt), F6.ceil256(li)
    off = (5 * D // 32 + D // 32) * (ltp + lip)
    mx_engine = e.buffer("a_mx")[off:off + 5 * D // 32 * Sp].view(5 * D // 32, Sp).clone()
    gate = e.buffer("emod", torch.float32)[n_double * 12 * D + 2 * D:n_double * 12 * D + 3 * D].clone()
    for b in range(blk + 1, e.n_blocks):             # finish the forward: the engine is shared
        e.block_pre(b)
        e.block_post(b)
    e.end(torch.empty(li, 64, device=DEV))
    torch.cuda.synchronize()
    aq, sa = F6.op_quantize(am, rows_pad=Sp)
    assert aq.shape == (S, kb)
    assert torch.equal(aq_engine, aq), "the packed 5 dim rows of \"aq\" are the op's bits of \"am\""
    assert torch.equal(F6.scale_rows(mx_engine, S), F6.scale_rows(sa, S)), "the joint range's scale image"
    p = f"single_transformer_blocks.{blk - n_double}.proj_out."
    w = sd[p + "weight"].to(torch.bfloat16).to(DEV).contiguous()
    assert w.shape == (D, 5 * D)
    wq, sw = F6.op_quantize(w, rows_pad=D)
    want = x_before.clone()
    F6.op_gemm(aq, sa, wq, sw, sd[p + "bias"].float().to(DEV).contiguous(), EPI_RESID, X=want, gate=gate)
    assert torch.equal(bits(x_after), bits(want)), "x after the single block"
    assert not torch.equal(bits(x_after), bits(x_before)) and bool(torch.isfinite(x_after).all())
    assert torch.equal(bits(G8.fwd(e, inp, FULL)), bits(full_out("flux_odd", 3, None)))


# ------------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("mode", [2, 3])
@pytest.mark.parametrize("case", list(CASES))
def test_forward_is_identical_under_fp8_fused_quant_0_and_1(case, mode):
    fam, geo = CASES[case]
    lib = _lib.load()
    e, inp = engine(case, mode), G8.dev_inputs(fam, geo)
    b = fam.branches[0]
    e.buffer("aq").fill_(0xA5)
    one = bits(G8.fwd(e, inp, FULL, b=b))
    aq_one = e.buffer("aq").cpu()
    assert torch.equal(one, bits(full_out(case, mode, b)))
    try:
        _lib.check(lib.mc_set_option(b"fp8_fused_quant", 0))
        e.buffer("aq").fill_(0xA5)
        zero = bits(G8.fwd(e, inp, FULL, b=b))
        aq_zero = e.buffer("aq").cpu()
    finally:
        _lib.check(lib.mc_set_option(b"fp8_fused_quant", 1))
    assert torch.equal(zero, one) and torch.equal(aq_zero, aq_one) and bool((aq_one != 0xA5).any())


# ------------------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize("mode", [2, 3])
@pytest.mark.parametrize("case", list(CASES))
def test_errors_against_the_fp32_oracle_are_ordered_and_bounded(case, mode):
    fam, geo = CASES[case]
    e4 = G8.make_engine(fam, geo, mode, mx_fp4=True)
    e4.set_rope(*fam.inputs(geo).rope)
    inp = G8.dev_inputs(fam, geo)
    for b in fam.branches:
        plain = plain_oracle(case, b)
        got = full_out(case, mode, b)
        assert bool(torch.isfinite(got).all())
        err = dict(bf16=rel_l2(G8.full_out(case, 0, b), plain), mxfp8=rel_l2(G8.full_out(case, mode, b), plain),
                   mxfp6=rel_l2(got, plain), mxfp4=rel_l2(G8.fwd(e4, inp, FULL, b=b).cpu(), plain))
        print(f"{case} branch {b} mode {mode}: relative L2 against the fp32 oracle: " + ", ".join(f"{k} {v:.3e}" for k, v in err.items()))
        _measured[f"{case}/mode{mode}/branch{b}"] = err
        tolerance_probe("mmdit_mxfp6_vs_fp32_oracle", _measured)
        assert err["bf16"] < err["mxfp8"] < err["mxfp4"] and err["bf16"] < err["mxfp6"] < err["mxfp4"], err
        assert err["mxfp6"] <= 1.5 * err["mxfp8"], err
        assert err["mxfp6"] <= 0.5 * err["mxfp4"], err
        assert err["mxfp6"] < 1.5 * MXFP6_REL_L2_MEASURED, err
