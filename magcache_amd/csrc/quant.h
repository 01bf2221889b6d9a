// The arithmetic of the two fp8 (OCP e4m3) quantisers, defined once.  Every producer of quantised rows -- the stand-alone
// kernels (quantize_rows_fp8_kernel, quantize_rows_mx_kernel), the fused tails of the LayerNorm + modulate kernel
// (elementwise.hip) and the EPI_GELU_MXFP8 epilogue (gemm_mxfp8.hip) -- goes through these helpers, so "the same bits as
// quantising the bf16 row" (ops.h) holds by construction.
#pragma once
#include "common.h"

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

}  // namespace mc
