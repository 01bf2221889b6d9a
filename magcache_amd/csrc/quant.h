// The arithmetic of the two fp8 (OCP e4m3) quantisers and of the MXFP4 (e2m1) and MXFP6 (e2m3) quantisers, defined once.  Every
// producer of quantised rows -- the stand-alone kernels (quantize_rows_fp8_kernel and the three quantize_rows_mx*_kernel, whose
// body is at the end of this file), the fused tails of the LayerNorm + modulate kernel (elementwise.hip), the EPI_GELU_MXFP8 /
// EPI_GELU_MXFP4 epilogues (gemm_mxfp8.hip, gemm_mxfp4.hip) -- goes through these helpers, so "the same bits as quantising the
// bf16 row" (ops.h) holds by construction.
#pragma once
#include "common.h"
#include "ops.h"

namespace mc {

// ---- per-row scale (fp8_linear = 1): s = max|row| / 448 (448 = the largest e4m3 value, so nothing saturates), 1 for an
// all-zero row; elements e4m3(x * (1 / s))
__device__ __forceinline__ float fp8_row_scale(float amax) { return amax > 0.f ? amax * (1.0f / 448.0f) : 1.0f; }

// ---- MX (fp8_linear = 2): one E8M0 scale per 32 consecutive k, exponent e = ceil(log2(amax / 448)) clamped to
// [-127, 127]; an all-zero block gets e = -127 (and zeros).  Exactly: frexp gives amax / 448 = f * 2^ex with f in [0.5, 1)
// -> ceil(log2) = ex unless f == 0.5 (a power of two), then ex - 1
__device__ __forceinline__ int mx_exponent(float amax) {
  int e = -127;
  if (amax > 0.f) {
    int ex;
    const float f = frexpf(amax * (1.0f / 448.0f), &ex);
    e = (f == 0.5f) ? ex - 1 : ex;
    e = max(-127, min(127, e));
  }
  return e;
}
// 2^-e, the factor of the elements (e in [-127, 127] -> exponent field 0..254).  (MC_NO_PK_F32, the attribute of its caller
// ln_modulate_kernel: without it that kernel's registers are allocated differently from the open-coded form; with it every
// caller's instruction stream is the open-coded one -- tools/isa_same.py)
MC_NO_PK_F32 __device__ __forceinline__ float mx_inv_scale(int e) { return __uint_as_float((uint32_t)(127 - e) << 23); }
// the stored E8M0 byte
__device__ __forceinline__ uint8_t mx_scale_byte(int e) { return (uint8_t)(e + 127); }
// Scale bytes are stored block-major, s[kb * rows_pad + mx_scale_row(row)], with the rows of every group of 64 interleaved
// 16 x 4: the four 16-row blocks a lane of the MX GEMM works on are then the four bytes of ONE dword (gemm_mxfp8.hip).
// (The macro form is for the EPI_GELU_MXFP8 epilogue alone: behind a call the compiler allocates that kernel's registers
// differently, and its instruction stream is held fixed -- tools/isa_same.py.)
#define MC_MX_SCALE_ROW(row) (((row) & ~63) | (((row) & 15) << 2) | (((row) >> 4) & 3))
__device__ __forceinline__ int mx_scale_row(int row) { return MC_MX_SCALE_ROW(row); }

// four values times the inverse scale -> four e4m3 bytes, a in the lowest (two v_cvt_pk_fp8_f32).  (The products are formed
// here, two in front of each conversion as the open-coded form had them: taken as four scaled arguments the LayerNorm
// tails are scheduled differently -- tools/isa_same.py)
__device__ __forceinline__ int pack4_e4m3(float a, float b, float c, float d, float inv) {
  const int w = __builtin_amdgcn_cvt_pk_fp8_f32(a * inv, b * inv, 0, false);
  return __builtin_amdgcn_cvt_pk_fp8_f32(c * inv, d * inv, w, true);
}

// ---- MXFP4 (both engines' option "mx_fp4"): OCP e2m1 elements, magnitudes {0, 0.5, 1, 1.5, 2, 3, 4, 6} = codes 0..7, bit
// 3 the sign, with the MX scale image above: one E8M0 byte e + 127 per 32 consecutive k at s[kb * rows_pad +
// mx_scale_row(row)].  e = ceil(log2(amax / 6)) clamped to [-127, 127] (6 = the largest e2m1 value, so nothing saturates;
// an all-zero block gets e = -127 and zeros) -- mx_exponent with 448 replaced by 6.
// Packing: two codes per byte, the EVEN k in the LOW nibble; a row of K elements is K / 2 bytes.  That is the order the matrix
// core reads (tools/ubench_mx_probe.cpp: an FP4 operand of v_mfma_scale_f32_16x16x128_f8f6f4 is 16 bytes per lane, nibble i
// of lane group g is k = 32 g + i, even i in the low nibble of byte i / 2).
__device__ __forceinline__ int mxfp4_exponent(float amax) {
  int e = -127;
  if (amax > 0.f) {
    int ex;
    const float f = frexpf(amax * (1.0f / 6.0f), &ex);
    e = (f == 0.5f) ? ex - 1 : ex;
    e = max(-127, min(127, e));
  }
  return e;
}
// one value times the inverse scale -> its e2m1 code, round to nearest, a tie to the even mantissa (= the even code: 0.25 -> 0,
// 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4); the sign bit is x's own (a negative that rounds to zero is -0).
// Coded, not v_cvt_scalef32_pk_fp4_f32: its rounding has not been probed in this project.  The product is exact (a power of two).
__device__ __forceinline__ uint32_t e2m1_code(float x, float inv) {
  const float a = fabsf(x * inv);
  const uint32_t mag = (uint32_t)(a > 0.25f) + (uint32_t)(a >= 0.75f) + (uint32_t)(a > 1.25f) + (uint32_t)(a >= 1.75f) +
                       (uint32_t)(a > 2.5f) + (uint32_t)(a >= 3.5f) + (uint32_t)(a > 5.0f);
  return mag | ((__float_as_uint(x) >> 28) & 8u);
}
// eight consecutive k times the inverse scale -> one dword of codes, v[0] in the lowest nibble
__device__ __forceinline__ uint32_t pack8_e2m1(const float* v, float inv) {
  uint32_t w = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) w |= e2m1_code(v[i], inv) << (4 * i);
  return w;
}
// four consecutive k (the first one even) -> 16 bits of codes, a in the lowest nibble: the packing width of the fused producers,
// whose lanes own four consecutive columns (the LayerNorm tail of elementwise.hip, the EPI_GELU_MXFP4 epilogue of gemm_mxfp4.hip)
__device__ __forceinline__ uint32_t pack4_e2m1(float a, float b, float c, float d, float inv) {
  return e2m1_code(a, inv) | (e2m1_code(b, inv) << 4) | (e2m1_code(c, inv) << 8) | (e2m1_code(d, inv) << 12);
}

// ---- MXFP6 (both engines' option "mx_fp6"): OCP e2m3 elements -- sign, two exponent bits (bias 1), three mantissa bits:
// magnitudes 0 .. 0.875 by 0.125 (codes 0..7, subnormal), 1 .. 1.875 by 0.125 (8..15), 2 .. 3.75 by 0.25 (16..23), 4 .. 7.5 by
// 0.5 (24..31), bit 5 the sign -- with the MX scale image above: one E8M0 byte e + 127 per 32 consecutive k at s[kb * rows_pad +
// mx_scale_row(row)].  e = ceil(log2(amax / 7.5)) clamped to [-127, 127] (7.5 = the largest e2m3 value, so nothing saturates;
// an all-zero block gets e = -127 and zeros) -- mx_exponent with 448 replaced by 7.5.
// Packing: the 32 codes of a block are ONE little-endian bit stream of 24 bytes: bit b of the 192 (bit b % 8 of byte b / 8) is
// bit b % 6 of the code of k = b / 6, so code i starts at bit 6 i and four codes fill three bytes; a row of K elements is
// 3 K / 4 bytes.  That is the order the matrix core reads (tools/ubench_mxfp6_probe.cpp, profiles/r14/mxfp6_probe.log: an FP6
// operand of v_mfma_scale_f32_16x16x128_f8f6f4, cbsz / blgp = 2, is the low 24 bytes of a lane's register argument, and bit b
// of lane group g is bit b % 6 of the code of k = 32 g + b / 6).
__device__ __forceinline__ int mxfp6_exponent(float amax) {
  int e = -127;
  if (amax > 0.f) {
    int ex;
    const float f = frexpf(amax * (1.0f / 7.5f), &ex);
    e = (f == 0.5f) ? ex - 1 : ex;
    e = max(-127, min(127, e));
  }
  return e;
}
// (amax * (1 / 7.5f) is one rounding away from amax / 7.5; at amax = 7.5 * 2^n the product must land on 2^n exactly for the
// f == 0.5 test: 7.5f * fl(1 / 7.5) rounds to 1.0f -- tests/test_mxfp6_cpu.py restates the rule in float64 and the GPU test
// compares the bits at and just above every such amax.)
// one value times the inverse scale -> its e2m3 code, round to nearest, a tie to the even mantissa; the sign bit is x's own (a
// negative that rounds to zero is -0).  CODED, not v_cvt_scalef32_pk*_fp6_*: the hardware conversion's rounding has not been
// probed in this project.  The product is exact (a power of two); the code book is uniform inside each binade -- steps of
// 1/8 below 2, 1/4 below 4, 1/2 above -- so the code is rint (to nearest even) of |x| in units of the binade's step plus the
// binade's first code less its first value in steps: rint(8 a) for a < 2 (0..16), 8 + rint(4 a) for a < 4, 16 + rint(2 a)
// above; the offsets are even, so an even integer is an even mantissa, and a value that rounds up to the next binade lands on
// that binade's first code.  Magnitudes above 7.5 (not produced by mxfp6_exponent's scale) clamp to code 31.
__device__ __forceinline__ uint32_t e2m3_code(float x, float inv) {
  const float a = fminf(fabsf(x * inv), 7.5f);
  const float q = a < 2.0f ? rintf(a * 8.0f) : a < 4.0f ? 8.0f + rintf(a * 4.0f) : 16.0f + rintf(a * 2.0f);
  return (uint32_t)q | ((__float_as_uint(x) >> 26) & 32u);
}
// sixteen consecutive k (the first one a multiple of 16) times the inverse scale -> 96 bits of codes, v[0] in the lowest six
__device__ __forceinline__ void pack16_e2m3(const float* v, float inv, uint32_t (&w)[3]) {
  uint64_t lo = 0;   // codes 0..9 and the low four bits of code 10
#pragma unroll
  for (int i = 0; i < 10; ++i) lo |= (uint64_t)e2m3_code(v[i], inv) << (6 * i);
  const uint32_t c10 = e2m3_code(v[10], inv);
  lo |= (uint64_t)(c10 & 15u) << 60;
  uint32_t hi = c10 >> 4;   // the high two bits of code 10, then codes 11..15
#pragma unroll
  for (int i = 11; i < 16; ++i) hi |= e2m3_code(v[i], inv) << (6 * i - 64);
  w[0] = (uint32_t)lo; w[1] = (uint32_t)(lo >> 32); w[2] = hi;
}

// ---- the stand-alone row quantisers of the element formats (ops.h: MxFormat), one body.  A format is its exponent rule and
// "pack the 32 scaled values of a block and store them": the block's mx_info().block_bytes at q_row + at in the packed row.
struct QuantE4m3 {
  static constexpr MxFormat format = MX_E4M3;
  static __device__ __forceinline__ int exponent(float amax) { return mx_exponent(amax); }
  static __device__ __forceinline__ void store_block(const float* v, float inv, uint8_t* q_row, int at) {
    uint32_t w[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) w[i] = (uint32_t)pack4_e4m3(v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3], inv);
    u32x4* dst = (u32x4*)(q_row + at);
    dst[0] = u32x4{w[0], w[1], w[2], w[3]};
    dst[1] = u32x4{w[4], w[5], w[6], w[7]};
  }
};
struct QuantE2m1 {
  static constexpr MxFormat format = MX_E2M1;
  static __device__ __forceinline__ int exponent(float amax) { return mxfp4_exponent(amax); }
  static __device__ __forceinline__ void store_block(const float* v, float inv, uint8_t* q_row, int at) {
    *(u32x4*)(q_row + at) = u32x4{pack8_e2m1(v, inv), pack8_e2m1(v + 8, inv), pack8_e2m1(v + 16, inv), pack8_e2m1(v + 24, inv)};
  }
};

// One wave per row, four rows per block of 256; lane b (+64, +128, ...) owns the 32-element block b: scale exponent
// e = F::exponent(amax), the codes of x * 2^-e stored by F, scale byte e + 127 at s[b * rows_pad + mx_scale_row(row)].
// The whole body of a kernel with the parameters (x, xf, ldx, M, K, q, ldq, s, rows_pad).  (A macro, not a function: inlined
// from a function the same IR reaches the back end with the predecessors of its blocks in another order, and the two input
// branches are laid out the other way round; the macro leaves the kernels' instruction streams as they were -- tools/isa_same.py.
// quantize_rows_mxfp6_kernel keeps a body of its own in gemm_mxfp6.hip: with its 24-byte store behind a trait the compiler
// threads the branches of e2m3_code differently, macro or not.)
#define MC_QUANTIZE_ROWS_MX_BODY(F)                                                                          \
  const int lane = threadIdx.x & 63;                                                                         \
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);                                                       \
  if (row >= M) return;                                                                                      \
  for (int b = lane; b < K / 32; b += 64) {                                                                  \
    float v[32];                                                                                             \
    if (xf) {                                                                                                \
      _Pragma("unroll") for (int i = 0; i < 8; ++i) {                                                        \
        const f32x4 t = *(const f32x4*)(xf + (size_t)row * ldx + b * 32 + i * 4);                            \
        v[4 * i] = t[0]; v[4 * i + 1] = t[1]; v[4 * i + 2] = t[2]; v[4 * i + 3] = t[3];                      \
      }                                                                                                      \
    } else {                                                                                                 \
      _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                        \
        const u32x4 t = *(const u32x4*)(x + (size_t)row * ldx + b * 32 + i * 8);                             \
        _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                                      \
          v[8 * i + 2 * j] = __uint_as_float(t[j] << 16);                                                    \
          v[8 * i + 2 * j + 1] = __uint_as_float(t[j] & 0xffff0000u);                                        \
        }                                                                                                    \
      }                                                                                                      \
    }                                                                                                        \
    float amax = 0.f;                                                                                        \
    _Pragma("unroll") for (int i = 0; i < 32; ++i) amax = fmaxf(amax, fabsf(v[i]));                          \
    const int e = F::exponent(amax);                                                                         \
    F::store_block(v, mx_inv_scale(e), q + (size_t)row * ldq, b * mx_info(F::format).block_bytes);           \
    s[(size_t)b * rows_pad + mx_scale_row(row)] = mx_scale_byte(e);                                          \
  }

// the launch of one of the three row-quantiser kernels, behind the argument contract of ops.h
template <auto Kernel>
inline hipError_t launch_quantize_rows_mx_kernel(MxFormat f, const bf16_t* x, const float* x_f32, long ldx, int M, int K, uint8_t* q,
                                                 long ldq, uint8_t* s, long rows_pad, hipStream_t stream) {
  if (!quantize_rows_mx_supported(f, x, x_f32, ldx, M, K, q, ldq, s, rows_pad)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(Kernel, dim3((M + 3) / 4), dim3(256), 0, stream, x, x_f32, ldx, M, K, q, ldq, s, rows_pad);
  return hipGetLastError();
}

}  // namespace mc
