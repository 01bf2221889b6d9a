"""GPU: the MX fp8 GEMM (gemm_mxfp8.hip) over any row count M > 0.

The kernel works in tiles of 256 rows.  With M % 256 != 0 the last tile is partial: its LDS-DMA reads clamp to row M - 1, and
every epilogue skips the rows m >= M.  Checked here through the shipped mc_op_gemm_mxfp8 (A has exactly M rows, its scale image
is padded to 256 as the contract asks):

  * rows [0, M) are BITWISE the rows of a launch over ceil256(M) rows of the zero-padded operand -- the path the kernel always
    had.  An output row depends on its own A row only, so equality is the bar, not a tolerance;
  * 64 sentinel rows behind row M - 1 of every output keep their bits (epilogues 0, 1, 2, 3 and 5; for 3 both X and R);
  * the fp32 output is the fp64 product of the dequantised operands within the bar of test_gemm_mxfp8_vs_dequantised_reference;
  * EPI_GELU_MXFP8: the e4m3 rows and scale bytes of rows < M are those of quantising the bf16 GELU output, the bytes of rows
    >= M keep their sentinel.

Epilogue 3 (X0 / R) and EPI_GELU_MXFP8 (Cq / c_mx) have no shipped single-op call: they go through the reference library's
mc_test_* wrappers, which link the shipped gemm_mxfp8 object."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import hip_ops as H  # noqa: E402
from hip_ops import P, S  # noqa: E402

DEV = "cuda:0"
GUARD = 64
SHAPES = [(1, 256, 512), (255, 256, 512), (257, 512, 1024), (300, 256, 2560), (272, 1536, 512)]
EPI_BF16, EPI_GELU, EPI_RESID, EPI_CAPTURE, EPI_F32 = 0, 1, 2, 3, 5


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def rnd(*shape, seed, scale=1.0, dtype=torch.float32):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(*shape, generator=g, device=DEV) * scale).to(dtype)


def ceil256(m):
    return (m + 255) // 256 * 256


def guarded(rows, cols, dtype, fill, body=None):
    """[rows + GUARD, cols] filled with `fill`; rows [0, rows) = body where given.  Returns (whole, the first `rows` rows)"""
    whole = torch.full((rows + GUARD, cols), fill, dtype=dtype, device=DEV)
    if body is not None:
        whole[:rows] = body
    return whole, whole[:rows]


def capture(aq, sa, wq, sw, bias, X, gate, X0, R):
    """EPI_RESID_CAPTURE of launch_gemm_mxfp8 (mc_test_gemm_mxfp8_capture of the reference library)"""
    fn = H.ref_lib().mc_test_gemm_mxfp8_capture
    vp, i, l = C.c_void_p, C.c_int, C.c_long
    fn.restype, fn.argtypes = C.c_int, [vp, l, vp, l, vp, l, vp, l, vp, i, i, i, vp, l, vp, vp, l, vp, l, vp]
    M, K = aq.shape
    st = fn(P(aq), aq.stride(0), P(sa), sa.shape[1], P(wq), wq.stride(0), P(sw), sw.shape[1], P(bias), M, wq.shape[0], K,
            P(X), X.stride(0), P(gate), P(X0), X0.stride(0), P(R), R.stride(0), S())
    assert st == 0, f"launch_gemm_mxfp8: hipError_t {st}"


_ops = {}


def operands(M, N, K):
    """quantised operands of a shape, once: A with exactly M rows, and the same rows zero-padded to ceil256(M)"""
    if (M, N, K) not in _ops:
        a = rnd(M, K, seed=1000 + M, dtype=torch.bfloat16)
        a[:, 3] *= 30.0
        a_pad = torch.zeros(ceil256(M), K, dtype=torch.bfloat16, device=DEV)
        a_pad[:M] = a
        w = rnd(N, K, seed=7, scale=0.05, dtype=torch.bfloat16)
        _ops[(M, N, K)] = (a, H.quantize_rows_mx(a), H.quantize_rows_mx(a_pad), w, H.quantize_rows_mx(w), rnd(N, seed=3))
    return _ops[(M, N, K)]


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_partial_tile_equals_the_padded_launch_and_leaves_the_rows_behind_alone(M, N, K):
    a, (aq, sa), (aqp, sap), w, (wq, sw), bias = operands(M, N, K)
    Mp = ceil256(M)
    assert aq.shape[0] == M and sa.shape[1] == Mp and torch.equal(aqp[:M], aq)
    gate = rnd(N, seed=6)
    x_init = rnd(Mp, N, seed=5)
    x0 = rnd(Mp, N, seed=8, dtype=torch.bfloat16)

    # ---- bf16 store and GELU
    for epi in (EPI_BF16, EPI_GELU):
        whole, cb = guarded(M, N, torch.bfloat16, -7.0)
        H.gemm_mxfp8(aq, sa, wq, sw, bias, epi, Cb=cb)
        want = torch.zeros(Mp, N, dtype=torch.bfloat16, device=DEV)
        H.gemm_mxfp8(aqp, sap, wq, sw, bias, epi, Cb=want)
        assert torch.equal(cb, want[:M]), f"epilogue {epi}: rows < M differ from the padded launch"
        assert bool((whole[M:] == -7.0).all()), f"epilogue {epi}: rows >= M were written"

    # ---- fp32 store: against the padded launch and the fp64 product of the dequantised operands
    whole, out = guarded(M, N, torch.float32, -7.0)
    H.gemm_mxfp8(aq, sa, wq, sw, bias, EPI_F32, X=out)
    want = torch.zeros(Mp, N, device=DEV)
    H.gemm_mxfp8(aqp, sap, wq, sw, bias, EPI_F32, X=want)
    assert torch.equal(out, want[:M])
    assert bool((whole[M:] == -7.0).all())

    def deq(q, s, rows):
        e = H.mx_unpermute(s, rows).float() - 127.0
        return (q.view(torch.float8_e4m3fn).float().view(rows, -1, 32) * torch.exp2(e)[..., None]).view(rows, -1).double()
    ref = deq(aq, sa, M) @ deq(wq, sw, N).t() + bias.double()
    err = rel_l2(out, ref)
    print(f"M {M} N {N} K {K}: relative L2 vs the fp64 product of the dequantised operands {err:.2e}")
    assert err < 1e-4

    # ---- gated residual
    whole, x = guarded(M, N, torch.float32, -7.0, x_init[:M])
    H.gemm_mxfp8(aq, sa, wq, sw, bias, EPI_RESID, X=x, gate=gate)
    want = x_init.clone()
    H.gemm_mxfp8(aqp, sap, wq, sw, bias, EPI_RESID, X=want, gate=gate)
    assert torch.equal(x, want[:M]) and not torch.equal(x, x_init[:M])
    assert bool((whole[M:] == -7.0).all())

    # ---- gated residual + MagCache capture: X and R
    xw, x = guarded(M, N, torch.float32, -7.0, x_init[:M])
    rw, r = guarded(M, N, torch.float32, -9.0)
    capture(aq, sa, wq, sw, bias, x, gate, x0[:M], r)
    want_x, want_r = x_init.clone(), torch.zeros(Mp, N, device=DEV)
    capture(aqp, sap, wq, sw, bias, want_x, gate, x0, want_r)
    assert torch.equal(x, want_x[:M]) and torch.equal(r, want_r[:M])
    assert torch.equal(r, x - x0[:M].float())
    assert bool((xw[M:] == -7.0).all()) and bool((rw[M:] == -9.0).all())


def test_gelu_quantising_epilogue_over_a_partial_tile():
    """EPI_GELU_MXFP8 at M = 300: Cq / c_mx of rows < M are the bits of quantising epilogue 1's bf16 output (the equality of
    test_gemm_mxfp8_gelu_quant_epilogue_equals_quantising_the_bf16_output); the e4m3 rows and the scale bytes of rows >= M keep
    their sentinels."""
    M, N, K = 300, 512, 512
    a, (aq, sa), _, w, (wq, sw), bias = operands(M, N, K)
    Mp = ceil256(M)
    cb = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
    H.gemm_mxfp8(aq, sa, wq, sw, bias, EPI_GELU, Cb=cb)
    want_q, want_s = H.quantize_rows_mx(cb)
    whole, cq = guarded(M, N, torch.uint8, 0x55)
    cs = torch.full((N // 32, Mp), 0x7B, dtype=torch.uint8, device=DEV)
    H.T("gemm_mxfp8_gelu_quant", P(aq), aq.stride(0), P(sa), sa.shape[1], P(wq), wq.stride(0), P(sw), sw.shape[1], P(bias), M, N, K,
        P(cq), cq.stride(0), P(cs), Mp, S())
    assert torch.equal(cq, want_q)
    assert bool((whole[M:] == 0x55).all())
    got_s = H.mx_unpermute(cs, Mp)                     # [Mp, N / 32] in natural row order
    assert torch.equal(got_s[:M], H.mx_unpermute(want_s, M))
    assert bool((got_s[M:] == 0x7B).all())
    assert int((cs == 0x7B).sum()) == (Mp - M) * (N // 32)


def test_row_count_is_no_longer_a_condition_and_the_other_conditions_stay():
    a, (aq, sa), _, w, (wq, sw), bias = operands(255, 256, 512)
    out = torch.zeros(255, 256, device=DEV)
    H.gemm_mxfp8(aq, sa, wq, sw, bias, EPI_F32, X=out)                           # M = 255: runs
    with pytest.raises(H._lib.MagCacheHipError):                                 # a scale image shorter than ceil256(M)
        H.gemm_mxfp8(aq, sa[:, :192].contiguous(), wq, sw, bias, EPI_F32, X=out)
    with pytest.raises(H._lib.MagCacheHipError):                                 # N % 256
        H.gemm_mxfp8(aq, sa, wq[:128], sw, bias, EPI_F32, X=out)
    with pytest.raises(H._lib.MagCacheHipError):                                 # K < 512
        H.gemm_mxfp8(aq[:, :256], sa, wq[:, :256], sw, bias, EPI_F32, X=out)


def test_the_e4m3_row_quantiser_takes_the_argument_contract_of_the_other_formats():
    """mc_op_quantize_rows_mx at M = 4, K = 64, the smallest shape it accepts: rows that overlap (ldq < K, ldx < K), an x or q
    that is not 16-byte aligned (the kernel moves 16 bytes at a time) and a null q are MC_EINVAL and nothing is launched -- q and
    the scale image keep their sentinels; the same call with valid arguments gives the bits of hip_ops.mx_quantize_ref."""
    M, K, rows_pad = 4, 64, 64
    lib, bf16_dt, einval = H.L(), H._lib.MC_BF16, H._lib.MC_EINVAL
    x = rnd(M + 1, K, seed=41, dtype=torch.bfloat16)           # a spare row: every refused call would stay inside the buffers
    x[0, 5] *= 40.0
    x[2, 32:] = 0.0                                            # an all-zero block: scale byte 0
    q = torch.full((M + 1, K), 0x55, dtype=torch.uint8, device=DEV)
    s = torch.full((K // 32, rows_pad), 0xEE, dtype=torch.uint8, device=DEV)   # 2^111: no scale of these values
    assert x.data_ptr() % 16 == 0 and q.data_ptr() % 16 == 0

    def call(xp, ldx, qp, ldq):
        return lib.mc_op_quantize_rows_mx(C.c_void_p(xp), bf16_dt, ldx, M, K, C.c_void_p(qp), ldq, P(s), rows_pad, S())
    assert call(x.data_ptr(), K, q.data_ptr(), 48) == einval          # ldq < K (a multiple of 16: the old check passed it)
    assert call(x.data_ptr(), 56, q.data_ptr(), K) == einval          # ldx < K (a multiple of 8)
    assert call(x.data_ptr() + 8, K, q.data_ptr(), K) == einval       # x not 16-byte aligned
    assert call(x.data_ptr(), K, q.data_ptr() + 8, K) == einval       # q not 16-byte aligned
    assert call(x.data_ptr(), K, 0, K) == einval                      # null q
    torch.cuda.synchronize()
    assert bool((q == 0x55).all()) and bool((s == 0xEE).all())

    assert call(x.data_ptr(), K, q.data_ptr(), K) == 0
    want_q, want_s = H.mx_quantize_ref(x[:M])
    assert torch.equal(q[:M], want_q.view(torch.uint8)) and bool((q[M:] == 0x55).all())
    assert torch.equal(H.mx_unpermute(s, M), want_s)
    assert int(want_s[2, 1]) == 0 and int((s == 0xEE).sum()) == (rows_pad - M) * (K // 32)
