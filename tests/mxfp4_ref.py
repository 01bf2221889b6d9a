"""MXFP4 (OCP microscaling, e2m1 elements + one E8M0 scale byte per 32 consecutive k) restated in torch, independent of
csrc/quant.h: quantise, pack, unpack, dequantise, and the layout of the scale image.  Float64 throughout, so every step is
exact (an fp32 / bf16 value times a power of two has no rounding in float64).

  * code book: magnitudes 0, 0.5, 1, 1.5, 2, 3, 4, 6 = codes 0..7; bit 3 of a code is the sign (x's own sign bit);
  * exponent of a block: e = ceil(log2(amax / 6)) clamped to [-127, 127], -127 for an all-zero block.  Computed from the
    float's own mantissa: amax = f 2^ex with f in [0.5, 1) and 6 = 0.75 2^3, so e = ex - 3 if f <= 0.75 else ex - 2;
  * code: the code-book value nearest to |x| 2^-e; of two equally near ones the EVEN code (the even mantissa);
  * packing: two codes per byte, the even k in the low nibble;
  * scale image: byte e + 127 at s[kb, mx_perm(row)] of a [K / 32, rows_pad] image (rows of every group of 64 interleaved
    16 x 4, as the MX fp8 path stores them).

The GPU wrappers at the end call the shipped single ops on torch tensors."""
import ctypes as C

import torch

CODEBOOK = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
TIES = ((0.25, 0.0), (0.75, 1.0), (1.25, 1.0), (1.75, 2.0), (2.5, 2.0), (3.5, 4.0), (5.0, 4.0))   # (value, rounds to)


def exponent(amax):
    """amax: float tensor (>= 0) -> int64 tensor of block exponents"""
    a = amax.double()
    f, ex = torch.frexp(a)
    e = torch.where(f <= 0.75, ex - 3, ex - 2).to(torch.int64).clamp(-127, 127)
    return torch.where(a > 0, e, torch.full_like(e, -127))


def encode(v, negative):
    """v: float64 magnitudes already divided by the block scale; negative: bool -> uint8 codes"""
    cb = torch.tensor(CODEBOOK, dtype=torch.float64, device=v.device)
    d = (v[..., None] - cb).abs()
    near = d == d.amin(dim=-1, keepdim=True)                       # one code, or two neighbours at a tie
    even = torch.tensor([2, 1, 2, 1, 2, 1, 2, 1], device=v.device)  # prefer the even code
    mag = (near * even).argmax(dim=-1)
    return (mag | (negative.to(torch.int64) << 3)).to(torch.uint8)


def quantize(x):
    """x [M, K] fp32 or bf16 -> (codes uint8 [M, K], block exponents int64 [M, K / 32])"""
    M, K = x.shape
    xb = x.double().view(M, K // 32, 32)
    e = exponent(xb.abs().amax(dim=-1))
    v = xb.abs() * torch.exp2(-e.double())[..., None]
    return encode(v, torch.signbit(x).view(M, K // 32, 32)).view(M, K), e


def pack(codes):
    """codes uint8 [M, K] -> bytes uint8 [M, K / 2], the even k in the low nibble"""
    return (codes[:, 0::2] | (codes[:, 1::2] << 4)).contiguous()


def unpack(q):
    """bytes uint8 [M, K / 2] -> codes uint8 [M, K]"""
    out = torch.empty(q.shape[0], q.shape[1] * 2, dtype=torch.uint8, device=q.device)
    out[:, 0::2] = q & 15
    out[:, 1::2] = q >> 4
    return out


def code_values(codes):
    """codes uint8 -> float64 element values (without the block scale)"""
    cb = torch.tensor(CODEBOOK, dtype=torch.float64, device=codes.device)
    v = cb[(codes & 7).long()]
    return torch.where((codes & 8) != 0, -v, v)


def dequantize(codes, e):
    """codes [M, K], block exponents [M, K / 32] -> float64 [M, K]"""
    M, K = codes.shape
    return (code_values(codes).view(M, K // 32, 32) * torch.exp2(e.double())[..., None]).view(M, K)


def mx_perm(rows):
    """where the kernels keep the scale bytes of row `rows` (int tensor): rows of every group of 64 interleaved 16 x 4"""
    return (rows & ~63) | ((rows & 15) << 2) | ((rows >> 4) & 3)


def scale_image(e, rows_pad, fill=127):
    """block exponents [M, K / 32] -> the scale image uint8 [K / 32, rows_pad] (bytes of rows >= M: `fill`)"""
    M = e.shape[0]
    s = torch.full((e.shape[1], rows_pad), fill, dtype=torch.uint8, device=e.device)
    s[:, mx_perm(torch.arange(M, device=e.device))] = (e + 127).to(torch.uint8).t()
    return s


def scale_rows(s, M):
    """scale image [K / 32, rows_pad] -> block exponents int64 [M, K / 32] in natural row order"""
    return s[:, mx_perm(torch.arange(M, device=s.device))].t().long() - 127


def ceil256(m):
    return (m + 255) // 256 * 256


# ---------------------------------------------------------------- the shipped single ops on torch tensors (GPU)
def _h():
    import hip_ops
    return hip_ops


def op_quantize(x, q=None, s=None, rows_pad=None, M=None, K=None, ldx=None, ldq=None):
    """mc_op_quantize_rows_mxfp4 -> (q uint8 [M, K / 2] (or the caller's), scale image uint8 [K / 32, rows_pad])"""
    H = _h()
    M = x.shape[0] if M is None else M
    K = x.shape[1] if K is None else K
    rows_pad = ceil256(M) if rows_pad is None else rows_pad
    if q is None:
        q = torch.empty(M, K // 2, dtype=torch.uint8, device=x.device)
    if s is None:
        s = torch.full((K // 32, rows_pad), 127, dtype=torch.uint8, device=x.device)
    H.check(H.L().mc_op_quantize_rows_mxfp4(H.P(x), H._lib.MC_BF16 if x.dtype == torch.bfloat16 else H._lib.MC_F32,
                                            x.stride(0) if ldx is None else ldx, M, K, H.P(q),
                                            q.stride(0) if ldq is None else ldq, H.P(s), rows_pad, H.S()))
    return q, s


def op_gemm(Aq, sa, Wq, sw, bias, epi, Cb=None, X=None, gate=None, M=None, N=None, K=None, lda=None, ldw=None, rows_pad_a=None,
            rows_pad_w=None):
    """mc_op_gemm_mxfp4: Aq [M, K / 2], Wq [N, K / 2] packed bytes; sa / sw scale images"""
    H = _h()
    M = Aq.shape[0] if M is None else M
    N = Wq.shape[0] if N is None else N
    K = Aq.shape[1] * 2 if K is None else K
    H.check(H.L().mc_op_gemm_mxfp4(H.P(Aq), Aq.stride(0) if lda is None else lda, H.P(sa),
                                   sa.shape[1] if rows_pad_a is None else rows_pad_a, H.P(Wq),
                                   Wq.stride(0) if ldw is None else ldw, H.P(sw), sw.shape[1] if rows_pad_w is None else rows_pad_w,
                                   H.P(bias), M, N, K, epi, H.P(Cb), Cb.stride(0) if Cb is not None else 0,
                                   H.P(X), X.stride(0) if X is not None else 0, H.P(gate), H.S()))


def _capture(name, aq, sa, wq, sw, bias, X, gate, X0, R, K):
    H = _h()
    fn = getattr(H.ref_lib(), name)
    vp, i, l = C.c_void_p, C.c_int, C.c_long
    fn.restype, fn.argtypes = C.c_int, [vp, l, vp, l, vp, l, vp, l, vp, i, i, i, vp, l, vp, vp, l, vp, l, vp]
    st = fn(H.P(aq), aq.stride(0), H.P(sa), sa.shape[1], H.P(wq), wq.stride(0), H.P(sw), sw.shape[1], H.P(bias), aq.shape[0],
            wq.shape[0], K, H.P(X), X.stride(0), H.P(gate), H.P(X0), X0.stride(0), H.P(R), R.stride(0), H.S())
    assert st == 0, f"{name}: hipError_t {st}"


def gemm_mxfp4_capture(aq, sa, wq, sw, bias, X, gate, X0, R):
    """EPI_RESID_CAPTURE of launch_gemm_mxfp4 (no shipped single-op call has X0 / R: the reference library's wrapper, which
    links the shipped gemm_mxfp4 object)"""
    _capture("mc_test_gemm_mxfp4_capture", aq, sa, wq, sw, bias, X, gate, X0, R, aq.shape[1] * 2)


def gemm_mxfp8_capture(aq, sa, wq, sw, bias, X, gate, X0, R):
    _capture("mc_test_gemm_mxfp8_capture", aq, sa, wq, sw, bias, X, gate, X0, R, aq.shape[1])
