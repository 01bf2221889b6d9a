"""MXFP6 (OCP microscaling, e2m3 elements + one E8M0 scale byte per 32 consecutive k) restated in torch, independent of
csrc/quant.h: quantise, pack, unpack, dequantise, and the layout of the scale image.  Float64 throughout, so every step is
exact (an fp32 / bf16 value times a power of two has no rounding in float64).  Written from the words of
include/magcache_hip.h (mc_op_quantize_rows_mxfp6), not from the kernels.

  * code book: a code is sign (bit 5), two exponent bits E (bits 4..3, bias 1), three mantissa bits m (bits 2..0): magnitude
    m / 8 for E = 0 (subnormal) and (1 + m / 8) 2^(E - 1) otherwise -- 0 .. 0.875 by 0.125, 1 .. 1.875 by 0.125, 2 .. 3.75 by
    0.25, 4 .. 7.5 by 0.5;
  * exponent of a block: e = ceil(log2(amax / 7.5)) clamped to [-127, 127], -127 for an all-zero block.  Computed from the
    float's own mantissa: amax = f 2^ex with f in [0.5, 1) and 7.5 = 0.9375 2^3, so e = ex - 3 if f <= 0.9375 else ex - 2;
  * code: the code-book value nearest to |x| 2^-e; of two equally near ones the one with the EVEN mantissa (= the even code);
    magnitudes above 7.5 (they do not occur under the block's own exponent) take code 31; the sign bit is x's own;
  * packing: the 32 codes of a block are one little-endian bit stream of 24 bytes -- bit b of the 192 (bit b % 8 of byte
    b / 8) is bit b % 6 of the code of k = b / 6; a row of K elements is 3 K / 4 bytes;
  * scale image: byte e + 127 at s[kb, mx_perm(row)] of a [K / 32, rows_pad] image (rows of every group of 64 interleaved
    16 x 4, as the MX fp8 path stores them).

The GPU wrappers at the end call the shipped single ops on torch tensors."""
import ctypes as C

import torch

CODEBOOK = tuple((m / 8.0) if E == 0 else (1.0 + m / 8.0) * 2.0 ** (E - 1) for E in range(4) for m in range(8))
MAX = 7.5
# the 31 midpoints of neighbouring code-book values and the value each goes to (the neighbour with the even code)
TIES = tuple(((CODEBOOK[i] + CODEBOOK[i + 1]) / 2.0, CODEBOOK[i] if i % 2 == 0 else CODEBOOK[i + 1]) for i in range(31))


def exponent(amax):
    """amax: float tensor (>= 0) -> int64 tensor of block exponents"""
    a = amax.double()
    f, ex = torch.frexp(a)
    e = torch.where(f <= 0.9375, ex - 3, ex - 2).to(torch.int64).clamp(-127, 127)
    return torch.where(a > 0, e, torch.full_like(e, -127))


def encode(v, negative):
    """v: float64 magnitudes already divided by the block scale; negative: bool -> uint8 codes"""
    cb = torch.tensor(CODEBOOK, dtype=torch.float64, device=v.device)
    d = (v[..., None] - cb).abs()
    near = d == d.amin(dim=-1, keepdim=True)                       # one code, or two neighbours at a tie
    even = torch.tensor([2, 1] * 16, device=v.device)              # prefer the even code
    mag = (near * even).argmax(dim=-1)
    return (mag | (negative.to(torch.int64) << 5)).to(torch.uint8)


def quantize(x):
    """x [M, K] fp32 or bf16 -> (codes uint8 [M, K], block exponents int64 [M, K / 32])"""
    M, K = x.shape
    xb = x.double().view(M, K // 32, 32)
    e = exponent(xb.abs().amax(dim=-1))
    v = xb.abs() * torch.exp2(-e.double())[..., None]
    return encode(v, torch.signbit(x).view(M, K // 32, 32)).view(M, K), e


def pack(codes):
    """codes uint8 [M, K] -> bytes uint8 [M, 3 K / 4]: four codes c0..c3 (24 bits, c0 lowest) fill three bytes"""
    M, K = codes.shape
    c = codes.view(M, K // 4, 4).to(torch.int64)
    w = c[..., 0] | (c[..., 1] << 6) | (c[..., 2] << 12) | (c[..., 3] << 18)
    return torch.stack((w & 255, (w >> 8) & 255, (w >> 16) & 255), dim=-1).to(torch.uint8).view(M, K // 4 * 3).contiguous()


def unpack(q):
    """bytes uint8 [M, 3 K / 4] -> codes uint8 [M, K]"""
    M, B = q.shape
    b = q.reshape(M, B // 3, 3).to(torch.int64)
    w = b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16)
    return torch.stack(((w >> 0) & 63, (w >> 6) & 63, (w >> 12) & 63, (w >> 18) & 63), dim=-1).to(torch.uint8).view(M, B // 3 * 4)


def code_values(codes):
    """codes uint8 -> float64 element values (without the block scale)"""
    cb = torch.tensor(CODEBOOK, dtype=torch.float64, device=codes.device)
    v = cb[(codes & 31).long()]
    return torch.where((codes & 32) != 0, -v, v)


def dequantize(codes, e):
    """codes [M, K], block exponents [M, K / 32] -> float64 [M, K]"""
    M, K = codes.shape
    return (code_values(codes).view(M, K // 32, 32) * torch.exp2(e.double())[..., None]).view(M, K)


def fake_quant(x):
    """x -> the float64 values its MXFP6 codes stand for"""
    return dequantize(*quantize(x))


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
    """mc_op_quantize_rows_mxfp6 -> (q uint8 [M, 3 K / 4] (or the caller's), scale image uint8 [K / 32, rows_pad])"""
    H = _h()
    M = x.shape[0] if M is None else M
    K = x.shape[1] if K is None else K
    rows_pad = ceil256(M) if rows_pad is None else rows_pad
    if q is None:
        q = torch.empty(M, K // 4 * 3, dtype=torch.uint8, device=x.device)
    if s is None:
        s = torch.full((K // 32, rows_pad), 127, dtype=torch.uint8, device=x.device)
    H.check(H.L().mc_op_quantize_rows_mxfp6(H.P(x), H._lib.MC_BF16 if x.dtype == torch.bfloat16 else H._lib.MC_F32,
                                            x.stride(0) if ldx is None else ldx, M, K, H.P(q),
                                            q.stride(0) if ldq is None else ldq, H.P(s), rows_pad, H.S()))
    return q, s


def op_gemm(Aq, sa, Wq, sw, bias, epi, Cb=None, X=None, gate=None, M=None, N=None, K=None, lda=None, ldw=None, rows_pad_a=None,
            rows_pad_w=None):
    """mc_op_gemm_mxfp6: Aq [M, 3 K / 4], Wq [N, 3 K / 4] packed bytes; sa / sw scale images"""
    H = _h()
    M = Aq.shape[0] if M is None else M
    N = Wq.shape[0] if N is None else N
    K = Aq.shape[1] // 3 * 4 if K is None else K
    H.check(H.L().mc_op_gemm_mxfp6(H.P(Aq), Aq.stride(0) if lda is None else lda, H.P(sa),
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


def gemm_mxfp6_capture(aq, sa, wq, sw, bias, X, gate, X0, R):
    """EPI_RESID_CAPTURE of launch_gemm_mxfp6 (no shipped single-op call has X0 / R: the reference library's wrapper, which
    links the shipped gemm_mxfp6 object)"""
    _capture("mc_test_gemm_mxfp6_capture", aq, sa, wq, sw, bias, X, gate, X0, R, aq.shape[1] // 3 * 4)


def gemm_mxfp8_capture(aq, sa, wq, sw, bias, X, gate, X0, R):
    _capture("mc_test_gemm_mxfp8_capture", aq, sa, wq, sw, bias, X, gate, X0, R, aq.shape[1])
