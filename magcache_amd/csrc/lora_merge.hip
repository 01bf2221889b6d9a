// LoRA merge: out[rows, K] = bf16( base + sum_j scale_j * (up_j down_j) ), the live weight of a Linear rebuilt from its pristine
// copy whenever adapters or scales change (host.cpp: WeightStore::lora_apply).  Not a forward-path kernel.
// The same kernel with fp32 base and out (launch_lora_merge_f32: the Wan engine's fp32 matrices) ends in the fp32 add, with no
// rounding step; a chunk of 8 columns is then two 16-byte vectors, each inside or outside the matrix as a whole (K % 4 == 0).
// launch_param_delta, at the end of the file, is the additive rule of the parameters that are no matrices.
//
// Arithmetic (tests/test_lora_merge_gpu.py depends on it): per term an fp32 accumulator from zero on bf16 MFMAs over the
// rank, zero-padded to kLoraRankStep; the fp32 delta = sum_j scale_j * acc_j in term order (a multiply and an add, never contracted); ONE fp32
// add of the widened base element, last; ONE round-to-nearest-even to bf16.
//
// A streaming kernel: the base tile in and the output tile out are the traffic, the operands are small and stay in L2.  One
// workgroup = 128 x 128 outputs, wave w = rows 32w .. 32w+31 of it as four 32 x 32 MFMA blocks.  The operands are the store's
// own copies, so they are kept in the order the MFMA reads them (LoraTerm, launch_lora_pack): the 64 fragments of one
// 32x32x16 step are 1 KB of consecutive memory, one fully coalesced 16-byte load per lane and no LDS.  The MFMA runs with
// down as its A operand: a lane then holds, for ONE
// output row (lane & 31), 4 x 4 consecutive columns -- the transpose of what a coalesced store wants -- so the delta goes
// through a wave-private LDS image (64 columns at a time, rows padded by 4 floats against bank conflicts) and comes back as 8
// consecutive columns per lane: 16-byte base loads and output stores, 128 bytes of a row per 8 lanes.
// out may alias base: every element is read and written by the same lane.
#include "common.h"
#include "ops.h"

namespace mc {

namespace {

constexpr int kTile = 128;       // rows and columns of a workgroup's tile
constexpr int kHalf = 64;        // columns that pass through LDS at a time
constexpr int kPitch = kHalf + 4;

template <class T>   // bf16_t | float: the element of base and out
struct MergeArgs {
  const T* base; long ld_base;
  T* out; long ld_out;
  int rows, K, n_terms, tiles_n;
  LoraTerm t[kLoraMaxTerms];
};

// the fragments of 32-row block `blk`, step `ks` (zeros for a block outside the matrix): LoraTerm's layout
__device__ __forceinline__ bf16x8 frag(const bf16_t* m, int blk, int n_blocks, int ks, int n_steps, int lane) {
  u32x4 v = {0u, 0u, 0u, 0u};
  if (blk < n_blocks) v = *reinterpret_cast<const u32x4*>(m + (((size_t)blk * n_steps + ks) * 64 + lane) * 8);
  return __builtin_bit_cast(bf16x8, v);
}

// The operands of two steps of one wave: its row block of `up` and its four column blocks of `down`.  The rank loop keeps two
// of these, the one it multiplies and the next one in flight: with one step loaded and waited for at a time a rank-128 merge
// took 3 times a copy of the same bytes, with this 1.9 times (profiles/r11/LORA_MERGE.md).
struct Frags {
  bf16x8 u[2], dn[4][2];
};
__device__ __forceinline__ void load_frags(Frags& f, const LoraTerm& t, int rb, int row_blocks, int cb, int col_blocks, int ks,
                                           int n_steps, int lane) {
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const bool in = ks + s < n_steps;   // past the last step: zeros, which add nothing
    f.u[s] = frag(t.up, rb, in ? row_blocks : 0, ks + s, n_steps, lane);
#pragma unroll
    for (int b = 0; b < 4; ++b) f.dn[b][s] = frag(t.down, cb + b, in ? col_blocks : 0, ks + s, n_steps, lane);
  }
}

// kMulti = false: exactly one term, whose accumulators become the delta in place (64 registers fewer, more waves in flight)
template <bool kMulti, class T>
__global__ __launch_bounds__(256) void lora_merge_kernel(MergeArgs<T> a) {
  constexpr int kVecs = sizeof(T) / 2;      // 16-byte vectors of an 8-column chunk: 1 (bf16) | 2 (fp32)
  constexpr int kVecCols = 8 / kVecs;
  __shared__ float lds[4][32][kPitch];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = tid >> 6;
  const int h = lane >> 5, l31 = lane & 31;
  const int row0 = (blockIdx.x / a.tiles_n) * kTile + wv * 32;   // first row of this wave
  const int col0 = (blockIdx.x % a.tiles_n) * kTile;
  const int row_blocks = (a.rows + 31) / 32, col_blocks = (a.K + 31) / 32;

  // the base tile first: its 8 x 16 bytes per lane are in flight while the operands are fetched and multiplied.  Chunk
  // (hf, it) = 8 columns from 64 hf + 8 (lane & 7) of row 8 it + (lane >> 3), the order the epilogue stores in
  u32x4 w[2][4][kVecs];
#pragma unroll
  for (int hf = 0; hf < 2; ++hf)
#pragma unroll
    for (int it = 0; it < 4; ++it)
#pragma unroll
      for (int v = 0; v < kVecs; ++v) {
        const int row = row0 + it * 8 + (lane >> 3), col = col0 + kHalf * hf + (lane & 7) * 8 + v * kVecCols;
        w[hf][it][v] = u32x4{0u, 0u, 0u, 0u};
        if (row < a.rows && col < a.K) w[hf][it][v] = *reinterpret_cast<const u32x4*>(a.base + (size_t)row * a.ld_base + col);
      }

  f32x16 delta[4];
  const int n_terms = kMulti ? a.n_terms : 1;
  for (int j = 0; j < n_terms; ++j) {
    const LoraTerm t = a.t[j];
    f32x16 acc[4];
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[b][i] = 0.f;
    const int n_steps = t.rank_pad / kLoraRankStep;
    Frags cur, nxt;
    load_frags(cur, t, row0 / 32, row_blocks, col0 / 32, col_blocks, 0, n_steps, lane);
    load_frags(nxt, t, row0 / 32, row_blocks, col0 / 32, col_blocks, 2, n_steps, lane);
    for (int ks = 0; ks < n_steps; ks += 2) {
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int b = 0; b < 4; ++b)
          // D[i][n] = sum_k down[k][col i] * up[row n][k]: the output row on the lane, its columns in the registers
          acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(cur.dn[b][s], cur.u[s], acc[b], 0, 0, 0);
      cur = nxt;
      load_frags(nxt, t, row0 / 32, row_blocks, col0 / 32, col_blocks, ks + 4, n_steps, lane);
    }
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float term = __fmul_rn(t.scale, acc[b][i]);
        delta[b][i] = j == 0 ? term : __fadd_rn(delta[b][i], term);
      }
  }

  // register i of block b: column 32 b + (i & 3) + 8 (i >> 2) + 4 h of row l31
#pragma unroll
  for (int hf = 0; hf < 2; ++hf) {
#pragma unroll
    for (int bb = 0; bb < 2; ++bb)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x16& d = delta[2 * hf + bb];
        f32x4 v = {d[4 * g], d[4 * g + 1], d[4 * g + 2], d[4 * g + 3]};
        *reinterpret_cast<f32x4*>(&lds[wv][l31][32 * bb + 8 * g + 4 * h]) = v;
      }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int r = it * 8 + (lane >> 3), c = (lane & 7) * 8;
      const int row = row0 + r, col = col0 + kHalf * hf + c;
      if (row < a.rows && col < a.K) {   // bf16: K is a multiple of 8, a chunk is inside or outside as a whole
        const f32x4 d0 = *reinterpret_cast<const f32x4*>(&lds[wv][r][c]);
        const f32x4 d1 = *reinterpret_cast<const f32x4*>(&lds[wv][r][c + 4]);
        if constexpr (kVecs == 1) {
          u32x4 o;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float dl = q < 2 ? d0[2 * q] : d1[2 * q - 4], dh = q < 2 ? d0[2 * q + 1] : d1[2 * q - 3];
            const float lo = __fadd_rn(__uint_as_float(w[hf][it][0][q] << 16), dl);
            const float hi = __fadd_rn(__uint_as_float(w[hf][it][0][q] & 0xffff0000u), dh);
            o[q] = pack_bf16x2(lo, hi);
          }
          *reinterpret_cast<u32x4*>(a.out + (size_t)row * a.ld_out + col) = o;
        } else {   // fp32: K is a multiple of 4, the chunk's second vector may lie outside
#pragma unroll
          for (int v = 0; v < kVecs; ++v) {
            const f32x4 dv = v == 0 ? d0 : d1;
            u32x4 o;
#pragma unroll
            for (int q = 0; q < 4; ++q) o[q] = __float_as_uint(__fadd_rn(__uint_as_float(w[hf][it][v][q]), dv[q]));
            if (col + v * kVecCols < a.K) *reinterpret_cast<u32x4*>(a.out + (size_t)row * a.ld_out + col + v * kVecCols) = o;
          }
        }
      }
    }
    __syncthreads();
  }
}

// dst in LoraTerm's layout <- element (row, k) = src[row * rs + k * cs], zero for row >= n or k >= rank
__global__ __launch_bounds__(256) void lora_pack_kernel(const void* src, int src_f32, long rs, long cs, int n, int rank, int n_steps,
                                                        size_t total, bf16_t* dst) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int j = (int)(idx & 7), lane = (int)((idx >> 3) & 63);
  const size_t step = idx >> 9;
  const size_t row = (step / n_steps) * 32 + (lane & 31);
  const int k = (int)(step % n_steps) * kLoraRankStep + 8 * (lane >> 5) + j;
  bf16_t v = 0;
  if (row < (size_t)n && k < rank) {
    const size_t e = row * rs + (size_t)k * cs;
    v = src_f32 ? f32_to_bf16(static_cast<const float*>(src)[e]) : static_cast<const bf16_t*>(src)[e];
  }
  dst[idx] = v;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the checks and the launch of both element widths; kAlign = elements of a 16-byte vector, what K and the pitches are multiples of
template <class T>
hipError_t launch_merge(const T* base, long ld_base, T* out, long ld_out, int rows, int K, const LoraTerm* terms, int n_terms,
                        hipStream_t stream) {
  constexpr int kAlign = 16 / sizeof(T);
  if (!base || !out || rows <= 0 || K <= 0 || (K % kAlign) != 0 || ld_base < K || ld_out < K || (ld_base % kAlign) != 0 ||
      (ld_out % kAlign) != 0 || !aligned16(base) || !aligned16(out) || n_terms < 0 || n_terms > kLoraMaxTerms || (n_terms > 0 && !terms))
    return hipErrorInvalidValue;
  MergeArgs<T> a;
  a.base = base; a.ld_base = ld_base; a.out = out; a.ld_out = ld_out; a.rows = rows; a.K = K; a.n_terms = n_terms;
  for (int j = 0; j < n_terms; ++j) {
    const LoraTerm& t = terms[j];
    if (!t.up || !t.down || t.rank_pad <= 0 || (t.rank_pad % kLoraRankStep) != 0 || !aligned16(t.up) || !aligned16(t.down))
      return hipErrorInvalidValue;
    a.t[j] = t;
  }
  for (int j = n_terms; j < kLoraMaxTerms; ++j) a.t[j] = LoraTerm{nullptr, nullptr, 0, 0.f};
  const long tiles_m = (rows + kTile - 1) / kTile;
  a.tiles_n = (K + kTile - 1) / kTile;
  if (tiles_m * a.tiles_n > 0x7fffffffL) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(tiles_m * a.tiles_n));
  if (n_terms == 0) {   // no live term: the base rows as they are
    if (out == base) return hipSuccess;
    return hipMemcpy2DAsync(out, (size_t)ld_out * sizeof(T), base, (size_t)ld_base * sizeof(T), (size_t)K * sizeof(T), rows,
                            hipMemcpyDeviceToDevice, stream);
  }
  if (n_terms == 1) hipLaunchKernelGGL((lora_merge_kernel<false, T>), grid, dim3(256), 0, stream, a);
  else hipLaunchKernelGGL((lora_merge_kernel<true, T>), grid, dim3(256), 0, stream, a);
  return hipGetLastError();
}

// ---- out[i] = base[i] + sum_j scale_j * delta_j[i] (fp32): the delta sum from zero in term order, a multiply and an add per
// term, never contracted; ONE add of the base element last.  Thread t takes vector t of the body, then element t of the tail.
struct DeltaArgs {
  const float* base; float* out;
  size_t n_vec, tail0, n;   // 16-byte vectors of the body, first element of the scalar tail, elements
  int n_terms;
  const float* delta[kLoraMaxTerms];
  float scale[kLoraMaxTerms];
};

// The products and sums are written out under contract(off): the toolchain's __fmul_rn / __fadd_rn are a plain * and + that it
// is free to fuse into one fma, and this kernel's result is defined bit for bit.
__global__ __launch_bounds__(256) void param_delta_kernel(DeltaArgs a) {
#pragma clang fp contract(off)
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < a.n_vec) {
    f32x4 sum = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < a.n_terms; ++j) {
      const f32x4 dl = reinterpret_cast<const f32x4*>(a.delta[j])[i];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float term = a.scale[j] * dl[q];
        sum[q] = sum[q] + term;
      }
    }
    const f32x4 b = reinterpret_cast<const f32x4*>(a.base)[i];
    f32x4 o;
#pragma unroll
    for (int q = 0; q < 4; ++q) o[q] = b[q] + sum[q];
    reinterpret_cast<f32x4*>(a.out)[i] = o;
  }
  const size_t e = a.tail0 + i;
  if (e < a.n) {
    float sum = 0.f;
    for (int j = 0; j < a.n_terms; ++j) {
      const float term = a.scale[j] * a.delta[j][e];
      sum = sum + term;
    }
    a.out[e] = a.base[e] + sum;
  }
}

}  // namespace

hipError_t launch_lora_merge(const bf16_t* base, long ld_base, bf16_t* out, long ld_out, int rows, int K, const LoraTerm* terms,
                             int n_terms, hipStream_t stream) {
  return launch_merge<bf16_t>(base, ld_base, out, ld_out, rows, K, terms, n_terms, stream);
}

hipError_t launch_lora_merge_f32(const float* base, long ld_base, float* out, long ld_out, int rows, int K, const LoraTerm* terms,
                                 int n_terms, hipStream_t stream) {
  return launch_merge<float>(base, ld_base, out, ld_out, rows, K, terms, n_terms, stream);
}

hipError_t launch_param_delta(const float* base, float* out, size_t n, const float* const* deltas, const float* scales, int n_terms,
                              hipStream_t stream) {
  if (!base || !out || n == 0 || n_terms < 1 || n_terms > kLoraMaxTerms || !deltas || !scales ||
      ((reinterpret_cast<uintptr_t>(base) | reinterpret_cast<uintptr_t>(out)) & 3))
    return hipErrorInvalidValue;
  DeltaArgs a;
  a.base = base; a.out = out; a.n = n; a.n_terms = 0;
  bool vec = aligned16(base) && aligned16(out);   // one operand off a 16-byte boundary: every element goes through the tail
  for (int j = 0; j < n_terms; ++j) {
    if (!deltas[j] || (reinterpret_cast<uintptr_t>(deltas[j]) & 3)) return hipErrorInvalidValue;
    if (scales[j] == 0.f) continue;   // left out, as the merge's callers leave a term with multiplier 0 out
    vec = vec && aligned16(deltas[j]);
    a.delta[a.n_terms] = deltas[j]; a.scale[a.n_terms] = scales[j];
    ++a.n_terms;
  }
  for (int j = a.n_terms; j < kLoraMaxTerms; ++j) { a.delta[j] = nullptr; a.scale[j] = 0.f; }
  if (a.n_terms == 0) {   // no live term: base as it is
    if (out == base) return hipSuccess;
    return hipMemcpyAsync(out, base, n * sizeof(float), hipMemcpyDeviceToDevice, stream);
  }
  a.n_vec = vec ? n / 4 : 0;
  a.tail0 = a.n_vec * 4;
  const size_t threads = a.n_vec > n - a.tail0 ? a.n_vec : n - a.tail0;
  if ((threads + 255) / 256 > 0x7fffffffUL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(param_delta_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_lora_pack(const void* src, int src_f32, long row_stride, long col_stride, int n, int rank, int rank_pad, bf16_t* dst,
                            hipStream_t stream) {
  if (!src || !dst || n <= 0 || rank <= 0 || rank_pad < rank || (rank_pad % kLoraRankStep) != 0) return hipErrorInvalidValue;
  const size_t total = lora_packed_elems(n, rank_pad);
  hipLaunchKernelGGL(lora_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, src, src_f32, row_stride,
                     col_stride, n, rank, rank_pad / kLoraRankStep, total, dst);
  return hipGetLastError();
}

}  // namespace mc
