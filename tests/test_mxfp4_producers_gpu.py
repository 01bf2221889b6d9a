"""GPU: the two fused MXFP4 producers, each against the separate pass it replaces, bit for bit (no tolerance).

  * launch_ln_modulate_mxfp4 (the FP4 tail of ln_modulate_kernel) == launch_ln_modulate into bf16 followed by
    launch_quantize_rows_mxfp4;
  * EPI_GELU_MXFP4 of launch_gemm_mxfp4 == EPI_GELU_BF16 followed by launch_quantize_rows_mxfp4.

Both write into a destination wider than the row, at a column offset, the way the MM-DiT engine writes into "aq"; the buffers
are filled with 0xA5 first, and every byte outside the written rows x columns and every scale byte of a row >= M must still be
0xA5 afterwards.  The launchers are reached through the test-only wrappers of the reference library (csrc/test_ops.cpp), which
links the shipped kernel objects."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import hip_ops as H  # noqa: E402
import mxfp4_ref as F4  # noqa: E402
from magcache_amd import _lib  # noqa: E402

DEV = "cuda:0"
FILL = 0xA5
EPI_GELU_BF16, EPI_GELU_MXFP4 = 1, 13
_vp, _i, _l, _f = C.c_void_p, C.c_int, C.c_long, C.c_float
_SIG = {
    "mc_test_ln_modulate_mxfp4": [_vp, _l, _vp, _vp, _i, _f, _vp, _l, _vp, _l, _i, _i, _vp, _vp, _vp, _vp],
    "mc_test_gemm_mxfp4_gelu_quant": [_vp, _l, _vp, _l, _vp, _l, _vp, _l, _vp, _i, _i, _i, _vp, _l, _vp, _l, _vp],
}


def call(name, *args):
    """mc_test_<name> of the reference library -> the launcher's hipError_t"""
    fn = getattr(H.ref_lib(), name)
    fn.restype, fn.argtypes = C.c_int, _SIG[name]
    return fn(*args)


def ceil(m, a):
    return (m + a - 1) // a * a


def filled(*shape):
    return torch.full(shape, FILL, dtype=torch.uint8, device=DEV)


def untouched_outside(buf, rows, col0, cols):
    """every byte of buf outside [0, rows) x [col0, col0 + cols) is still FILL"""
    mask = torch.ones_like(buf, dtype=torch.bool)
    mask[:rows, col0:col0 + cols] = False
    return bool((buf[mask] == FILL).all())


def scale_rows_untouched(s, M):
    """every scale byte of a row >= M is still FILL"""
    keep = torch.ones(s.shape[1], dtype=torch.bool, device=s.device)
    keep[F4.mx_perm(torch.arange(M, device=s.device))] = False
    return bool((s[:, keep] == FILL).all())


# ------------------------------------------------------------------------------------------------ LayerNorm tail
def ln_both(x, sc, sh, sc2=None, sh2=None, sel=None, mode=0, col0=32, extra=48):
    """-> (fused buffer, fused scale image, reference bytes [M, D / 2], reference scale image)"""
    M, D = x.shape
    rows_pad = ceil(M, 64) + 64
    xn = torch.empty(M, D, dtype=torch.bfloat16, device=DEV)
    H.ln_modulate_sel(x, sc, sh, mode, 1e-6, out_bf16=xn, sc2=sc2, sh2=sh2, sel=sel)
    q_ref, s_ref = F4.op_quantize(xn, s=filled(D // 32, rows_pad), rows_pad=rows_pad)
    buf, s = filled(M + 3, col0 + D // 2 + extra), filled(D // 32, rows_pad)
    st = call("mc_test_ln_modulate_mxfp4", H.P(x), x.stride(0), H.P(sc), H.P(sh), mode, 1e-6, C.c_void_p(buf.data_ptr() + col0),
              buf.stride(0), H.P(s), rows_pad, M, D, H.P(sc2), H.P(sh2), H.P(sel), H.S())
    assert st == 0, f"launch_ln_modulate_mxfp4: hipError_t {st}"
    torch.cuda.synchronize()
    return buf, s, q_ref, s_ref


@pytest.mark.parametrize("M", [1, 5, 65, 200])
@pytest.mark.parametrize("D", [256, 512, 1280, 3072])
def test_ln_tail_equals_ln_then_quantise(D, M):
    g = torch.Generator().manual_seed(D + M)
    x = (torch.randn(M, D, generator=g) * 2 + 0.3).to(DEV)
    sc, sh = (torch.randn(D, generator=g) * 0.5).to(DEV), torch.randn(D, generator=g).to(DEV)
    col0 = 32
    buf, s, q_ref, s_ref = ln_both(x, sc, sh, col0=col0)
    assert torch.equal(buf[:M, col0:col0 + D // 2], q_ref)
    assert torch.equal(s, s_ref)
    assert untouched_outside(buf, M, col0, D // 2) and scale_rows_untouched(s, M)
    assert bool(q_ref.any())   # not a comparison of two empty results


def test_ln_tail_per_token_modulation():
    M, D = 70, 512
    g = torch.Generator().manual_seed(7)
    x = torch.randn(M, D, generator=g).to(DEV)
    sc, sh, sc2, sh2 = ((torch.randn(D, generator=g) * w).to(DEV) for w in (0.5, 1.0, 0.5, 1.0))
    sel = (torch.rand(M, generator=g) < 0.5).to(torch.uint8).to(DEV)
    assert 0 < int(sel.sum()) < M
    buf, s, q_ref, s_ref = ln_both(x, sc, sh, sc2, sh2, sel)
    assert torch.equal(buf[:M, 32:32 + D // 2], q_ref) and torch.equal(s, s_ref)
    assert untouched_outside(buf, M, 32, D // 2) and scale_rows_untouched(s, M)
    plain = ln_both(x, sc, sh)[2]
    assert not torch.equal(plain[sel.bool()], q_ref[sel.bool()]) and torch.equal(plain[~sel.bool()], q_ref[~sel.bool()])


def test_ln_tail_all_zero_row():
    """a zero row with shift 0 is a zero row after LayerNorm: scale byte 0 (e = -127) and codes 0 in every block"""
    M, D = 6, 512
    g = torch.Generator().manual_seed(11)
    x = torch.randn(M, D, generator=g).to(DEV)
    x[2] = 0
    sc, sh = (torch.randn(D, generator=g) * 0.5).to(DEV), torch.zeros(D, device=DEV)
    buf, s, q_ref, s_ref = ln_both(x, sc, sh)
    assert torch.equal(buf[:M, 32:32 + D // 2], q_ref) and torch.equal(s, s_ref)
    assert not bool(buf[2, 32:32 + D // 2].any())
    assert not bool(s[:, int(F4.mx_perm(torch.tensor(2)))].any())
    assert bool(buf[1, 32:32 + D // 2].any())


def test_ln_tail_refusals():
    M, D = 5, 512
    x, sc, sh = torch.randn(M, D, device=DEV), torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
    buf, s = filled(M, 512), filled(D // 32, 128)

    def st(ldq=512, mx_rows=64, q=buf, mx=s):
        return call("mc_test_ln_modulate_mxfp4", H.P(x), D, H.P(sc), H.P(sh), 0, 1e-6, H.P(q), ldq, H.P(mx), mx_rows, M, D, None, None,
                    None, H.S())
    assert st() == 0
    for bad in (dict(ldq=264), dict(ldq=D // 2 - 16), dict(mx_rows=32), dict(mx_rows=0), dict(q=None), dict(mx=None)):
        assert st(**bad) == H.HIP_INVALID_VALUE, bad
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ GELU epilogue
_operands = {}


def operands(M, N, K):
    """quantised A [M, K] and W [N, K] with their scale images, and a bias; made once per shape"""
    if (M, N, K) not in _operands:
        g = torch.Generator().manual_seed(M + 3 * N + 7 * K)
        A = (torch.randn(M, K, generator=g) * 1.5).to(torch.bfloat16).to(DEV)
        W = (torch.randn(N, K, generator=g) * 0.05).to(torch.bfloat16).to(DEV)
        aq, sa = F4.op_quantize(A)
        wq, sw = F4.op_quantize(W)
        _operands[(M, N, K)] = (aq, sa, wq, sw, (torch.randn(N, generator=g) * 0.5).to(DEV))
    return _operands[(M, N, K)]


def gelu_quant(aq, sa, wq, sw, bias, M, N, K, cq, ldcq, c_mx, rows_pad_c):
    return call("mc_test_gemm_mxfp4_gelu_quant", H.P(aq), aq.stride(0), H.P(sa), sa.shape[1], H.P(wq), wq.stride(0), H.P(sw),
                sw.shape[1], H.P(bias), M, N, K, cq, ldcq, H.P(c_mx), rows_pad_c, H.S())


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("K", [512, 768])
@pytest.mark.parametrize("N", [256, 768])
@pytest.mark.parametrize("M", [72, 256, 272])
def test_gelu_epilogue_equals_gelu_then_quantise(M, N, K, with_bias):
    aq, sa, wq, sw, bias = operands(M, N, K)
    bias = bias if with_bias else None
    rows_pad = F4.ceil256(M)
    cb = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    F4.op_gemm(aq, sa, wq, sw, bias, EPI_GELU_BF16, Cb=cb)
    q_ref, s_ref = F4.op_quantize(cb, s=filled(N // 32, rows_pad), rows_pad=rows_pad)
    col0 = 48
    buf, s = filled(M + 3, col0 + N // 2 + 32), filled(N // 32, rows_pad)
    st = gelu_quant(aq, sa, wq, sw, bias, M, N, K, C.c_void_p(buf.data_ptr() + col0), buf.stride(0), s, rows_pad)
    assert st == 0, f"launch_gemm_mxfp4(EPI_GELU_MXFP4): hipError_t {st}"
    torch.cuda.synchronize()
    assert torch.equal(buf[:M, col0:col0 + N // 2], q_ref)
    assert torch.equal(s, s_ref)
    assert untouched_outside(buf, M, col0, N // 2) and scale_rows_untouched(s, M)
    assert bool(q_ref.any()) and bool((cb.float().abs() > 0.1).any())   # not a comparison of two empty results


def test_gelu_epilogue_refusals():
    M, N, K = 72, 256, 512
    aq, sa, wq, sw, bias = operands(M, N, K)
    buf, s = filled(M, 256), filled(N // 32, 256)

    def st(ldcq=256, rows_pad_c=256, cq=buf, c_mx=s):
        return gelu_quant(aq, sa, wq, sw, bias, M, N, K, H.P(cq), ldcq, c_mx, rows_pad_c)
    assert st() == 0
    for bad in (dict(ldcq=136), dict(ldcq=N // 2 - 16), dict(rows_pad_c=64), dict(rows_pad_c=0), dict(cq=None), dict(c_mx=None)):
        assert st(**bad) == H.HIP_INVALID_VALUE, bad
    torch.cuda.synchronize()
    # the MX fp8 GEMM refuses the FP4 epilogue (its operands are valid: the plain epilogue runs), and the shipped single op
    # of the MXFP4 GEMM, which has no Cq / c_mx arguments, cannot launch it
    A8 = torch.randn(M, K, device=DEV).to(torch.bfloat16)
    W8 = (torch.randn(N, K, device=DEV) * 0.05).to(torch.bfloat16)
    (a8, sa8), (w8, sw8) = H.quantize_rows_mx(A8), H.quantize_rows_mx(W8)
    cb = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    H.gemm_mxfp8(a8, sa8, w8, sw8, None, EPI_GELU_BF16, Cb=cb)
    for gemm, ops in ((H.gemm_mxfp8, (a8, sa8, w8, sw8)), (F4.op_gemm, (aq, sa, wq, sw))):
        with pytest.raises(_lib.MagCacheHipError) as ex:
            gemm(*ops, None, EPI_GELU_MXFP4, Cb=cb)
        assert ex.value.status == _lib.MC_EINVAL
    torch.cuda.synchronize()
