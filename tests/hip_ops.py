"""Test-side helpers: call the single-op C-ABI entry points (mc_op_*) on torch tensors."""
import contextlib
import ctypes as C
import os

import torch

from magcache_amd import _lib
from magcache_amd._lib import check


REF_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_ref", "libmagcache_hip_ref.so")
_ref = None
_active = None        # the library the helpers below call: None = the shipped one


def ref_lib():
    """tests/_ref/libmagcache_hip_ref.so: the shipped objects + gemm_bf16_big.hip (rounds 1-3's 8-wave 256 x 256 GEMM),
    built by magcache_amd.build.build_ref().  Test-only: the independent implementation gemm_bf16_v2 is compared with bit for
    bit.  A second copy of the library in the process (its own option globals, the same HIP runtime)."""
    global _ref
    if _ref is None:
        if not os.path.exists(REF_PATH):
            raise ImportError(f"{REF_PATH} not found: python -c 'from magcache_amd import build; build.build_ref()'")
        _lib.load()                                   # torch's HIP runtime first (see _lib.load)
        lib = C.CDLL(REF_PATH)
        for name, (res, args) in _lib.SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        _ref = lib
    return _ref


def L():
    """the library under test: the shipped one unless a gemm_kernel(2) block is open"""
    return _active if _active is not None else _lib.load()


@contextlib.contextmanager
def gemm_kernel(k):
    """force a GEMM kernel for the enclosed single-op calls: 0 by shape, 1 the 128^2 kernel, 4 gemm_bf16_v2 -- options of the
    shipped library --, 2 the 8-wave reference kernel, which only the reference library has"""
    global _active
    lib = ref_lib() if k == 2 else _lib.load()
    prev = _active
    _active = lib if k == 2 else None
    check_on(lib, lib.mc_set_option(b"gemm_kernel", k))
    try:
        yield lib
    finally:
        lib.mc_set_option(b"gemm_kernel", 0)
        _active = prev


def check_on(lib, status):
    if status != 0:
        raise _lib.MagCacheHipError(status, lib.mc_last_error().decode())


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def bf16(t):
    return t.to(torch.bfloat16).contiguous()


def gemm(A, W, bias, epi, Cb=None, X=None, gate=None, X0=None, R=None, X0out=None, m_valid=0):
    lib = L()
    M, K = A.shape
    N = W.shape[0]
    check(lib.mc_op_gemm_bf16(P(A), A.stride(0), P(W), W.stride(0), P(bias), M, N, K, epi,
                              P(Cb), Cb.stride(0) if Cb is not None else 0,
                              P(X), X.stride(0) if X is not None else 0, P(gate),
                              P(X0), X0.stride(0) if X0 is not None else 0,
                              P(R), R.stride(0) if R is not None else 0,
                              P(X0out), X0out.stride(0) if X0out is not None else 0, m_valid, S()))


def quantize_rows_fp8(x):
    """x [M, K] bf16 or fp32 -> (q uint8 [M, K], scale fp32 [M])"""
    lib = L()
    M, K = x.shape
    q = torch.empty(M, K, dtype=torch.uint8, device=x.device)
    s = torch.empty(M, dtype=torch.float32, device=x.device)
    check(lib.mc_op_quantize_rows_fp8(P(x), _lib.MC_BF16 if x.dtype == torch.bfloat16 else _lib.MC_F32, x.stride(0), M, K,
                                      P(q), q.stride(0), P(s), S()))
    return q, s


def quantize_rows_mx(x):
    """x [M, K] bf16 or fp32 -> (q uint8 [M, K] e4m3, scales uint8 [K/32, rows_pad] E8M0, block-major, rows interleaved
    16 x 4 inside groups of 64: see mx_unpermute)"""
    lib = L()
    M, K = x.shape
    rows_pad = (M + 255) // 256 * 256
    q = torch.empty(M, K, dtype=torch.uint8, device=x.device)
    s = torch.full((K // 32, rows_pad), 127, dtype=torch.uint8, device=x.device)
    check(lib.mc_op_quantize_rows_mx(P(x), _lib.MC_BF16 if x.dtype == torch.bfloat16 else _lib.MC_F32, x.stride(0), M, K,
                                     P(q), q.stride(0), P(s), rows_pad, S()))
    return q, s


def mx_perm(rows):
    """where the kernels keep the scale bytes of row `rows` (int tensor): mx_scale_row of csrc/quant.h, the rows of every
    group of 64 interleaved 16 x 4"""
    return (rows & ~63) | ((rows & 15) << 2) | ((rows >> 4) & 3)


def mx_unpermute(s, M):
    """scales [K/32, rows_pad] in the kernel's row order -> [M, K/32] in natural order"""
    return s[:, mx_perm(torch.arange(M, device=s.device))].t().contiguous()


def gemm_mxfp8(Aq, sa, Wq, sw, bias, epi, Cb=None, X=None, gate=None):
    lib = L()
    M, K = Aq.shape
    N = Wq.shape[0]
    check(lib.mc_op_gemm_mxfp8(P(Aq), Aq.stride(0), P(sa), sa.shape[1], P(Wq), Wq.stride(0), P(sw), sw.shape[1], P(bias),
                               M, N, K, epi, P(Cb), Cb.stride(0) if Cb is not None else 0,
                               P(X), X.stride(0) if X is not None else 0, P(gate), S()))


def gemm_fp8(Aq, sa, Wq, sw, bias, epi, Cb=None, X=None, gate=None):
    lib = L()
    M, K = Aq.shape
    N = Wq.shape[0]
    check(lib.mc_op_gemm_fp8(P(Aq), Aq.stride(0), P(sa), P(Wq), Wq.stride(0), P(sw), P(bias), M, N, K, epi,
                             P(Cb), Cb.stride(0) if Cb is not None else 0, P(X), X.stride(0) if X is not None else 0,
                             P(gate), S()))


def attention(Q, K, V, O, n_heads, shard_rows, shard_valid, n_shards, scale, k_shard_stride=0, v_shard_stride=0):
    lib = L()
    check(lib.mc_op_attention(P(Q), Q.stride(0), P(K), K.stride(0), k_shard_stride, P(V), V.stride(0),
                              v_shard_stride, P(O), O.stride(0), Q.shape[0], n_heads, shard_rows, shard_valid,
                              n_shards, scale, S()))


def attention_partial(Q, K, V, O, n_heads, shard_rows, shard_valid, n_shards, scale, shard_stride, skip_shard=-1,
                      lse_out=None, lse_in=None):
    lib = L()
    check(lib.mc_op_attention_partial(P(Q), Q.stride(0), P(K), K.stride(0), shard_stride, P(V), V.stride(0),
                                      shard_stride, P(O), O.stride(0), Q.shape[0], n_heads, shard_rows, shard_valid,
                                      n_shards, scale, skip_shard, P(lse_out), P(lse_in), S()))


def attn_merge(o_parts, lse_parts, out):
    """out = log-sum-exp weighted mean of the partial attention results (bf16 [rows, d] each, lse fp32 [heads, rows_pad] each)"""
    lib = L()
    n = len(o_parts)
    op = (C.c_void_p * n)(*[t.data_ptr() for t in o_parts])
    lp = (C.c_void_p * n)(*[t.data_ptr() for t in lse_parts])
    check(lib.mc_op_attn_merge(op, lp, n, P(out), out.stride(0), out.shape[0], lse_parts[0].shape[1], out.shape[1], S()))


def ln_modulate(x, sc, sh, mode, eps, out_bf16=None, out_f32=None, x0=None):
    lib = L()
    M, D = x.shape
    check(lib.mc_op_ln_modulate(P(x), x.stride(0), P(x0), x0.stride(0) if x0 is not None else 0, P(sc), P(sh), mode,
                                eps, P(out_bf16), out_bf16.stride(0) if out_bf16 is not None else 0, P(out_f32),
                                out_f32.stride(0) if out_f32 is not None else 0, M, D, S()))


def rmsnorm_rope(x, w, eps, cs, cs_row0=0, D=None):
    lib = L()
    check(lib.mc_op_rmsnorm_rope(P(x), x.stride(0), P(w), eps, P(cs), cs_row0, x.shape[0], D or x.shape[1], S()))


def rope_table(F_, Hp, Wp, tok0, n_tok):
    lib = L()
    cs = torch.empty(n_tok, 128, dtype=torch.float32)
    check(lib.mc_op_rope_table(F_, Hp, Wp, tok0, n_tok, C.c_void_p(cs.data_ptr())))
    return cs


def skip_add(x0, r, out):
    lib = L()
    check(lib.mc_op_skip_add(P(x0), x0.stride(0), P(r), r.stride(0), P(out), out.stride(0), r.shape[0], r.shape[1],
                             S()))


def residual_sub(x, x0, r):
    lib = L()
    check(lib.mc_op_residual_sub(P(x), x.stride(0), P(x0), x0.stride(0), P(r), r.stride(0), x.shape[0], x.shape[1],
                                 S()))


CALIB_SENTINEL = -7.0     # what sums / stats hold where calib_stats did not write them


def calib_stats(r, rp, n_blocks=2048, partial=None, want_stats=True, ldr=None, ldrp=None, M=None, D=None, out=None):
    """-> (stats fp32 [3], sums fp64 [4]) on the host.  n_blocks = 2048 is what both engines launch (32 waves per CU).
    partial: the caller's scratch of at least 4 * n_blocks + 1 doubles, in any state (the launcher clears the ticket);
    want_stats=False passes stats = NULL (the launch of a sequence-parallel rank: sums only); ldr / ldrp / M / D override
    what the tensors say; out = (sums, stats): device tensors to write to instead of fresh ones, which stay readable
    when the call is refused.  Whatever the call leaves unwritten holds CALIB_SENTINEL."""
    lib = L()
    if partial is None:
        # 4 partial sums per block + the arrival ticket
        partial = torch.zeros(4 * n_blocks + 1, dtype=torch.float64, device=r.device)
    assert partial.dtype == torch.float64 and partial.numel() >= 4 * n_blocks + 1
    if out is None:
        out = (torch.full((4,), CALIB_SENTINEL, dtype=torch.float64, device=r.device),
               torch.full((3,), CALIB_SENTINEL, dtype=torch.float32, device=r.device))
    sums, stats = out
    check(lib.mc_op_calib_stats(P(r), r.stride(0) if ldr is None else ldr, P(rp), rp.stride(0) if ldrp is None else ldrp,
                                r.shape[0] if M is None else M, r.shape[1] if D is None else D, P(partial), n_blocks,
                                P(sums), P(stats) if want_stats else None, S()))
    return stats.cpu(), sums.cpu()


def calib_finalize(sums):
    """launch_calib_finalize: stats fp32 [3] (host) from sums fp64 [4] on the device, as a rank of a sequence-parallel
    group computes them after the all-reduce of the sums"""
    stats = torch.full((3,), CALIB_SENTINEL, dtype=torch.float32, device=sums.device)
    T("calib_finalize", P(sums), P(stats), S())
    return stats.cpu()


# ----------------------------------------------------------------------------- test-only entry points (mc_test_*)
# magcache_amd/csrc/test_ops.cpp, linked into the REFERENCE library only: thin wrappers around the launchers of ops.h the
# shipped C ABI has no single-op call for.  The reference library links the shipped elementwise.hip.o / gemm_mxfp8.hip.o, so
# these run the shipped machine code.  Each returns the launcher's hipError_t (0 = hipSuccess, 1 = hipErrorInvalidValue).
HIP_INVALID_VALUE = 1
_vp, _i, _l, _f, _d, _sz = C.c_void_p, C.c_int, C.c_long, C.c_float, C.c_double, C.c_size_t
TEST_SIGNATURES = {
    "mc_test_headnorm_rope": [_vp, _l, _l, _vp, _vp, _f, _vp, _i, _i, _i, _vp],
    "mc_test_gemv_bf16w": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp],
    "mc_test_gemv_f32": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp],
    "mc_test_head_linear": [_vp, _l, _vp, _vp, _vp, _l, _i, _i, _i, _vp],
    "mc_test_ln_modulate": [_vp, _l, _vp, _l, _vp, _vp, _i, _f, _vp, _l, _vp, _l, _i, _i, _vp, _vp, _vp, _vp],
    "mc_test_ln_modulate_fp8": [_vp, _l, _vp, _vp, _i, _f, _vp, _l, _vp, _vp, _l, _i, _i, _vp, _vp, _vp, _vp],
    "mc_test_gemm_mxfp8_gelu_quant": [_vp, _l, _vp, _l, _vp, _l, _vp, _l, _vp, _i, _i, _i, _vp, _l, _vp, _l, _vp],
    "mc_test_gemm_fp8_capture": [_vp, _l, _vp, _vp, _l, _vp, _vp, _i, _i, _i, _vp, _l, _vp, _vp, _l, _vp, _l, _vp],
    "mc_test_calib_finalize": [_vp, _vp, _vp],
    "mc_test_token_t_prepare": [_vp, _i, _i, _i, _i, _vp, _vp, _vp],
    "mc_test_patchify": [_vp, _i, _i, _i, _i, _i, _i, _i, _vp, _l, _vp],
    "mc_test_unpatchify": [_vp, _l, _i, _i, _i, _i, _i, _i, _vp, _vp],
    "mc_test_cast_pad_bf16": [_vp, _l, _i, _i, _i, _vp, _l, _vp],
    "mc_test_cast_bf16": [_vp, _vp, _sz, _vp],
    "mc_test_add_bf16": [_vp, _vp, _sz, _vp],
    "mc_test_add_bcast": [_vp, _i, _vp, _vp, _i, _vp],
    "mc_test_sinusoid": [_vp, _d, _i, _vp, _vp],
    "mc_test_colmean": [_vp, _l, _i, _i, _vp, _vp],
    "mc_test_rope_table_from_cos_sin": [_vp, _vp, _l, _i, _vp, _vp],
    "mc_test_cfg_euler": [_vp, _vp, _f, _f, _vp, _vp, _sz, _vp],
    "mc_test_attn_merge": [_vp, _vp, _i, _vp, _l, _i, _i, _i, _vp],
}
_test_bound = False


class HipStatusError(RuntimeError):
    def __init__(self, name, status):
        super().__init__(f"{name}: hipError_t {status}")
        self.status = status


def T(name, *args):
    """call mc_test_<name> of the reference library; a non-zero hipError_t raises HipStatusError"""
    global _test_bound
    lib = ref_lib()
    if not _test_bound:
        for n, argtypes in TEST_SIGNATURES.items():
            fn = getattr(lib, n)
            fn.restype, fn.argtypes = C.c_int, argtypes
        _test_bound = True
    status = getattr(lib, "mc_test_" + name)(*args)
    if status != 0:
        raise HipStatusError(name, status)


def _ld(t):
    return t.stride(0) if t is not None else 0


def headnorm_rope(x, k_col0, wq, wk, eps, cs, cs_row0, n_heads, M=None):
    """in place on the q | k columns of x [M, ldx] bf16 (q at column 0, k at column k_col0)"""
    T("headnorm_rope", P(x), x.stride(0), k_col0, P(wq), P(wk), eps, P(cs), cs_row0, x.shape[0] if M is None else M, n_heads, S())


def gemv_bf16w(W, x, b, y, act_in=0, act_out=0, accumulate=0, N=None, K=None):
    T("gemv_bf16w", P(W), P(x), P(b), P(y), W.shape[0] if N is None else N, W.shape[1] if K is None else K, act_in, act_out,
      accumulate, S())


def gemv_f32(W, x, b, y, act_in=0, act_out=0, N=None, K=None):
    T("gemv_f32", P(W), P(x), P(b), P(y), W.shape[0] if N is None else N, W.shape[1] if K is None else K, act_in, act_out, S())


def head_linear(xn, W, b, out, M, N, K):
    T("head_linear", P(xn), xn.stride(0), P(W), P(b), P(out), out.stride(0), M, N, K, S())


def ln_modulate_sel(x, sc, sh, mode, eps, out_bf16=None, out_f32=None, x0=None, sc2=None, sh2=None, sel=None, M=None, D=None):
    """launch_ln_modulate with every argument (H.ln_modulate is the shipped mc_op_ln_modulate, which has no sc2 / sh2 / sel)"""
    T("ln_modulate", P(x), x.stride(0), P(x0), _ld(x0), P(sc), P(sh), mode, eps, P(out_bf16), _ld(out_bf16), P(out_f32),
      _ld(out_f32), x.shape[0] if M is None else M, x.shape[1] if D is None else D, P(sc2), P(sh2), P(sel), S())


def ln_modulate_fp8(x, sc, sh, mode, eps, mx, sc2=None, sh2=None, sel=None):
    """-> (q uint8 [M, D], per-row scales fp32 [M]) or, mx=True, (q, E8M0 scales uint8 [D/32, rows_pad] as quantize_rows_mx)"""
    M, D = x.shape
    q = torch.full((M, D), 0x55, dtype=torch.uint8, device=x.device)
    if mx:
        rows_pad = (M + 255) // 256 * 256
        s = torch.full((D // 32, rows_pad), 127, dtype=torch.uint8, device=x.device)
        T("ln_modulate_fp8", P(x), x.stride(0), P(sc), P(sh), mode, eps, P(q), q.stride(0), None, P(s), rows_pad, M, D, P(sc2),
          P(sh2), P(sel), S())
    else:
        s = torch.full((M,), -1.0, dtype=torch.float32, device=x.device)
        T("ln_modulate_fp8", P(x), x.stride(0), P(sc), P(sh), mode, eps, P(q), q.stride(0), P(s), None, 0, M, D, P(sc2), P(sh2),
          P(sel), S())
    return q, s


def gemm_mxfp8_gelu_quant(Aq, sa, Wq, sw, bias):
    """EPI_GELU_MXFP8 -> (Cq uint8 [M, N] e4m3, c_mx uint8 [N/32, rows_pad]): the A operand of the next MX GEMM"""
    M, K = Aq.shape
    N = Wq.shape[0]
    rows_pad = (M + 255) // 256 * 256
    cq = torch.full((M, N), 0x55, dtype=torch.uint8, device=Aq.device)
    cs = torch.full((N // 32, rows_pad), 127, dtype=torch.uint8, device=Aq.device)
    T("gemm_mxfp8_gelu_quant", P(Aq), Aq.stride(0), P(sa), sa.shape[1], P(Wq), Wq.stride(0), P(sw), sw.shape[1], P(bias), M, N, K,
      P(cq), cq.stride(0), P(cs), rows_pad, S())
    return cq, cs


def gemm_fp8_capture(Aq, sa, Wq, sw, bias, X, gate, X0, R):
    """EPI_RESID_CAPTURE of launch_gemm_fp8: X += gate * bf16(acc * sa * sw + bias), R = X_new - float(X0)"""
    M, K = Aq.shape
    T("gemm_fp8_capture", P(Aq), Aq.stride(0), P(sa), P(Wq), Wq.stride(0), P(sw), P(bias), M, Wq.shape[0], K, P(X), X.stride(0),
      P(gate), P(X0), X0.stride(0), P(R), R.stride(0), S())


def token_t_prepare(t, n_all, row0, n_rows, n_rows_pad, t2, sel):
    T("token_t_prepare", P(t), n_all, row0, n_rows, n_rows_pad, P(t2), P(sel), S())


def patchify(lat, tok0, n_tok, n_rows, out, dims=None):
    Cc, F_, Hh, Ww = dims or lat.shape
    T("patchify", P(lat), Cc, F_, Hh, Ww, tok0, n_tok, n_rows, P(out), out.stride(0), S())


def unpatchify(tok, tok0, n_tok, out, dims=None):
    Cc, F_, Hh, Ww = dims or out.shape
    T("unpatchify", P(tok), tok.stride(0), Cc, F_, Hh, Ww, tok0, n_tok, P(out), S())


def cast_pad_bf16(src, rows_valid, rows, cols, dst):
    T("cast_pad_bf16", P(src), src.stride(0), rows_valid, rows, cols, P(dst), dst.stride(0), S())


def cast_bf16(src, dst, n):
    T("cast_bf16", P(src), P(dst), n, S())


def add_bf16(a, b, n):
    T("add_bf16", P(a), P(b), n, S())


def add_bcast(a, b, out, n):
    T("add_bcast", P(a), a.numel(), P(b), P(out), n, S())


def sinusoid(t_dev, t_host, dim, out):
    T("sinusoid", P(t_dev), float(t_host), dim, P(out), S())


def colmean(x, n_rows, D, out):
    T("colmean", P(x), x.stride(0), n_rows, D, P(out), S())


def rope_table_from_cos_sin(cosv, sinv, n_rows, cs):
    T("rope_table_from_cos_sin", P(cosv), P(sinv), cosv.stride(0), n_rows, P(cs), S())


def cfg_euler(cond, uncond, g, dt, x, eps_out, n):
    T("cfg_euler", P(cond), P(uncond), g, dt, P(x), P(eps_out), n, S())


def attn_merge_raw(o_parts, lse_parts, out, rows, rows_pad, d):
    """launch_attn_merge with explicit rows / rows_pad / d (H.attn_merge takes them from the tensors)"""
    n = len(o_parts)
    op = (C.c_void_p * n)(*[t.data_ptr() for t in o_parts])
    lp = (C.c_void_p * n)(*[t.data_ptr() for t in lse_parts])
    T("attn_merge", op, lp, n, P(out), out.stride(0), rows, rows_pad, d, S())


# ----------------------------------------------------------------------------- helpers shared by the GPU test files
def mx_quantize_ref(x):
    """torch restatement of quantize_rows_mx: per (row, 32 k) block e = ceil(log2(amax / 448)) through frexp of
    amax * fl32(1/448), elements e4m3fn(x * 2^-e), scale byte e + 127."""
    M, K = x.shape
    xb = x.float().view(M, K // 32, 32)
    amax = xb.abs().amax(dim=-1)
    f, ex = torch.frexp(amax * torch.tensor(1.0 / 448.0, dtype=torch.float32, device=x.device))
    e = torch.where(f == 0.5, ex - 1, ex).clamp(-127, 127)
    e = torch.where(amax > 0, e, torch.full_like(e, -127))
    q = (xb * torch.exp2(-e.float())[..., None]).to(torch.float8_e4m3fn)
    return q.view(M, K), (e + 127).to(torch.uint8)


def fp8_rows_quantize_ref(x):
    """torch restatement of quantize_rows_fp8: per row s = amax * fl32(1/448) (1 for an all-zero row), elements
    e4m3fn(x * (1 / s))."""
    xf = x.float()
    amax = xf.abs().amax(dim=-1)
    s = torch.where(amax > 0, amax * torch.tensor(1.0 / 448.0, dtype=torch.float32, device=x.device), torch.ones_like(amax))
    return (xf * (1.0 / s)[:, None]).to(torch.float8_e4m3fn), s


def v2_sample_rows(M, device="cuda:0"):
    """>= 512 rows spread over M tiles of 256 at the start, the middle and the end of the row range (under the grouped,
    XCD-contiguous tile order these land in the first, middle and last persistent trips of different workgroups), and inside
    a tile the rows where a wave's strip / range-check arithmetic changes: 0..3, 104..131 (incl. 108-111 and 124-127, where the
    first lean epilogue addressed rows through the buffer soffset and was wrong: profiles/r04/NOTES.md 1.4), 250..255."""
    tiles = [0, 1, 2, 3, 31, 32, 37, 63, 64, 65, 95, 100, 125, 126, 127]
    inside = list(range(0, 4)) + list(range(104, 132)) + list(range(250, 256))
    rows = torch.tensor([t * 256 + r for t in tiles for r in inside if t * 256 + r < M])
    assert rows.numel() >= 512
    return rows.to(device)
