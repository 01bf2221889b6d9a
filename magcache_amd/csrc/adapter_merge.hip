// Adapter merge of every kind (ops.h: launch_adapter_merge): the live bf16 weight of a Linear part rebuilt from its pristine
// copy where the part carries a Kronecker (LoKr) or Hadamard (LoHa) term or a DoRA magnitude (host.cpp: WeightStore::lora_apply).
// A part whose terms are all low-rank pairs and that has no magnitude never comes here: it keeps lora_merge.hip's kernel.
// Not forward-path work: plain element-wise kernels over an fp32 image V [rows, K] in the caller's scratch.
//
//   1. the pairs: launch_lora_merge_f32 on a zeroed V, in place -- V = 0 + sum_j m_j (up_j down_j), exactly its delta
//   2. adapter_delta_kernel: one thread per 8 columns of a row adds the Kronecker and Hadamard terms to that delta and the
//      widened base element last; without a magnitude it rounds to bf16 and stores the 16 bytes of out, with one it stores V
//   3. adapter_dora_rows_kernel (magnitude only): one workgroup per row, the sum of squares in a fixed order, then the row
// Every product and sum is written out under contract(off): the results are defined bit for bit, and two applies agree.
// out may alias base: step 2 reads and writes an element in the same thread, step 3 reads V only.
#include <cstring>

#include "common.h"
#include "ops.h"

namespace mc {

namespace {

struct AdapterArgs {
  const bf16_t* base; long ld_base;
  bf16_t* out; long ld_out;
  float* v;   // [rows, K], pitch K
  int rows, K, n_kron, n_hada;
  int has_pairs;    // v holds the pairs' delta (else the delta starts from zero)
  int to_scratch;   // store V into v (a magnitude follows) instead of bf16(V) into out
  KronTerm kron[kLoraMaxTerms];
  HadaTerm hada[kLoraMaxTerms];
};

__global__ __launch_bounds__(256) void adapter_delta_kernel(AdapterArgs a) {
#pragma clang fp contract(off)
  const size_t chunks = (size_t)(a.K / 8);
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t row = idx / chunks;
  const int col = (int)(idx % chunks) * 8;
  if (row >= (size_t)a.rows || col >= a.K) return;
  float* vp = a.v + row * (size_t)a.K + col;
  float d[8];
  if (a.has_pairs) {
    const f32x4 lo = *reinterpret_cast<const f32x4*>(vp), hi = *reinterpret_cast<const f32x4*>(vp + 4);
#pragma unroll
    for (int q = 0; q < 4; ++q) { d[q] = lo[q]; d[q + 4] = hi[q]; }
  } else {
#pragma unroll
    for (int q = 0; q < 8; ++q) d[q] = 0.f;
  }
  for (int j = 0; j < a.n_kron; ++j) {
    const KronTerm t = a.kron[j];
    const float* w1r = t.w1 + (row / (size_t)t.r2) * (size_t)t.c1;
    const float* w2r = t.w2 + (row % (size_t)t.r2) * (size_t)t.c2;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int c = col + q;
      const float p = w1r[c / t.c2] * w2r[c % t.c2];
      const float term = t.scale * p;
      d[q] = d[q] + term;
    }
  }
  for (int j = 0; j < a.n_hada; ++j) {
    const HadaTerm t = a.hada[j];
    const float* u1r = t.u1 + row * (size_t)t.rank;
    const float* u2r = t.u2 + row * (size_t)t.rank;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int c = col + q;
      float s1 = 0.f, s2 = 0.f;
      for (int k = 0; k < t.rank; ++k) {
        const float p1 = u1r[k] * t.d1[(size_t)k * a.K + c];
        const float p2 = u2r[k] * t.d2[(size_t)k * a.K + c];
        s1 = s1 + p1;
        s2 = s2 + p2;
      }
      const float h = s1 * s2;
      const float term = t.scale * h;
      d[q] = d[q] + term;
    }
  }
  const u32x4 w = *reinterpret_cast<const u32x4*>(a.base + row * (size_t)a.ld_base + col);
  const bool any = a.has_pairs || a.n_kron > 0 || a.n_hada > 0;   // no term at all: V is the base element, its zero sign kept
  float v[8];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float lo = __uint_as_float(w[q] << 16), hi = __uint_as_float(w[q] & 0xffff0000u);
    v[2 * q] = any ? lo + d[2 * q] : lo;
    v[2 * q + 1] = any ? hi + d[2 * q + 1] : hi;
  }
  if (a.to_scratch) {
    *reinterpret_cast<f32x4*>(vp) = f32x4{v[0], v[1], v[2], v[3]};
    *reinterpret_cast<f32x4*>(vp + 4) = f32x4{v[4], v[5], v[6], v[7]};
  } else {
    u32x4 o;
#pragma unroll
    for (int q = 0; q < 4; ++q) o[q] = pack_bf16x2(v[2 * q], v[2 * q + 1]);
    *reinterpret_cast<u32x4*>(a.out + row * (size_t)a.ld_out + col) = o;
  }
}

// out[row, :] = bf16((g[row] / sqrt(sum_k V[row, k]^2)) * V[row, :]); one workgroup per row (grid == rows)
__global__ __launch_bounds__(256) void adapter_dora_rows_kernel(const float* v, const float* g, bf16_t* out, long ld_out, int rows,
                                                                int K) {
#pragma clang fp contract(off)
  __shared__ float part[256];
  const int tid = threadIdx.x;
  const size_t row = blockIdx.x;
  if (row >= (size_t)rows) return;   // the whole workgroup leaves: no barrier is left waiting
  const float* vr = v + row * (size_t)K;
  float acc = 0.f;
  for (int c = tid; c < K; c += 256) {
    const float x = vr[c];
    const float sq = x * x;
    acc = acc + sq;
  }
  part[tid] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) part[tid] = part[tid] + part[tid + s];
    __syncthreads();
  }
  const float sum = part[0];
  const float scale = sum > 0.f ? g[row] / sqrtf(sum) : 0.f;
  bf16_t* orow = out + row * (size_t)ld_out;
  for (int c = tid; c < K; c += 256) orow[c] = f32_to_bf16(scale * vr[c]);
}

__global__ __launch_bounds__(256) void widen_f32_kernel(const void* src, int src_f32, float* dst, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  dst[i] = src_f32 ? static_cast<const float*>(src)[i] : bf16_to_f32(static_cast<const bf16_t*>(src)[i]);
}

bool aligned(const void* p, uintptr_t a) { return p && (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

hipError_t launch_adapter_merge(const bf16_t* base, long ld_base, bf16_t* out, long ld_out, int rows, int K, const LoraTerm* pairs,
                                int n_pairs, const KronTerm* krons, int n_kron, const HadaTerm* hadas, int n_hada,
                                const float* magnitude, float* scratch, hipStream_t stream) {
  if (rows <= 0 || K <= 0 || (K % 8) != 0 || ld_base < K || ld_out < K || (ld_base % 8) != 0 || (ld_out % 8) != 0 ||
      !aligned(base, 16) || !aligned(out, 16) || !aligned(scratch, 16) || (magnitude && !aligned(magnitude, 4)))
    return hipErrorInvalidValue;
  if (n_pairs < 0 || n_kron < 0 || n_hada < 0 || n_pairs + n_kron + n_hada > kLoraMaxTerms || (n_pairs > 0 && !pairs) ||
      (n_kron > 0 && !krons) || (n_hada > 0 && !hadas))
    return hipErrorInvalidValue;
  AdapterArgs a;
  memset(&a, 0, sizeof(a));
  a.base = base; a.ld_base = ld_base; a.out = out; a.ld_out = ld_out; a.v = scratch; a.rows = rows; a.K = K;
  a.n_kron = n_kron; a.n_hada = n_hada; a.has_pairs = n_pairs > 0; a.to_scratch = magnitude != nullptr;
  for (int j = 0; j < n_pairs; ++j)   // what launch_lora_merge_f32 would refuse, before anything is launched
    if (!aligned(pairs[j].up, 16) || !aligned(pairs[j].down, 16) || pairs[j].rank_pad <= 0 || (pairs[j].rank_pad % kLoraRankStep) != 0)
      return hipErrorInvalidValue;
  for (int j = 0; j < n_kron; ++j) {
    const KronTerm& t = krons[j];
    if (!aligned(t.w1, 4) || !aligned(t.w2, 4) || t.r1 < 1 || t.c1 < 1 || t.r2 < 1 || t.c2 < 1 || (long)t.r1 * t.r2 != rows ||
        (long)t.c1 * t.c2 != K)
      return hipErrorInvalidValue;
    a.kron[j] = t;
  }
  for (int j = 0; j < n_hada; ++j) {
    const HadaTerm& t = hadas[j];
    if (!aligned(t.u1, 4) || !aligned(t.d1, 4) || !aligned(t.u2, 4) || !aligned(t.d2, 4) || t.rank < 1) return hipErrorInvalidValue;
    a.hada[j] = t;
  }
  const size_t threads = (size_t)rows * (size_t)(K / 8);
  const size_t blocks = (threads + 255) / 256;
  if (blocks > 0x7fffffffUL) return hipErrorInvalidValue;
  if (n_pairs > 0) {
    hipError_t err = hipMemsetAsync(scratch, 0, (size_t)rows * K * sizeof(float), stream);
    if (err != hipSuccess) return err;
    err = launch_lora_merge_f32(scratch, K, scratch, K, rows, K, pairs, n_pairs, stream);
    if (err != hipSuccess) return err;
  }
  hipLaunchKernelGGL(adapter_delta_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, a);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess || !magnitude) return err;
  hipLaunchKernelGGL(adapter_dora_rows_kernel, dim3((unsigned)rows), dim3(256), 0, stream, scratch, magnitude, out, ld_out, rows, K);
  return hipGetLastError();
}

hipError_t launch_widen_f32(const void* src, int src_f32, float* dst, size_t n, hipStream_t stream) {
  if (!src || !dst || n == 0 || (n + 255) / 256 > 0x7fffffffUL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(widen_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, src, src_f32, dst, n);
  return hipGetLastError();
}

}  // namespace mc
