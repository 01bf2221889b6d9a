// MX fp8 self-attention for gfx950, head_dim 128: both products of a flash-style non-causal attention on
// v_mfma_scale_f32_32x32x64_f8f6f4 (e4m3 operands, E8M0 block scales multiplied inside the matrix core), twice the bf16 MFMA
// rate.  An OPTIONAL mode of the Wan engine (option "attn_mx8"), never a default and never the headline; attention_v5.hip is
// the default kernel.  Plain HIP with builtins, compiler-scheduled: not a variant of the generated v5 stream.
//
// Two launchers:
//   launch_attn_quantize_mx8   bf16 q, k, v columns (rows of "qkv", any ld % 8 == 0) -> the images of ops.h: AttnMx8Images.
//       Q^ = e4m3(q * scale * log2(e)) per (row, 32 channels): the scores come out of the MFMA in log2 units.  K^ the same
//       without the factor, rows >= valid zero with the unit scale.  V^T per head [128 channels][keys], one scale per
//       (channel, 32 key slots), rows >= valid counted as zero, the keys of every 64 stored in the order of mx8_slot_key
//       (quant.h).  The quantiser arithmetic is quant.h's (mx_exponent, mx_inv_scale, pack4_e4m3).
//   launch_attention_mx8       the images -> O bf16.
//
// The kernel.  One workgroup of 4 waves (one per SIMD) per (256 query rows, head); a wave owns 64 queries as two 32-column
// blocks and walks the keys 64 at a time:
//   S^T = K^ Q^T   keys are the rows (2 key blocks x 2 query blocks x 2 k steps of 64 channels = 8 MFMAs), so a lane owns
//                  one query column: the softmax reductions are in-lane plus one exchange with lane ^ 32.  Both operands
//                  carry their E8M0 scales in the MFMA's scale arguments; the Q^ fragments and scales stay in registers.
//   softmax        fp32, base 2, running maximum and sum, exact (the reference maximum moves with every tile: P <= 1 is what
//                  the e4m3 packing needs); the sum is taken from the fp32 probabilities; O is rescaled only in tiles
//                  where some row's maximum moved (wave-uniform; the factor is exactly 1 otherwise).
//   P              p = exp2(s - m) in [0, 1] packed as e4m3(256 p) (256 <= 448, 1.0 stays exact) with the constant scale 2^-8.
//   O^T += V^T P^T the 32 bytes a lane packs from its two S^T blocks ARE its B operand (4 channel blocks x 2 query blocks = 8
//                  MFMAs): no LDS round trip and no cross-lane move, because the pre-pass stored V^T's keys in the order
//                  the operand's k slots meet the accumulator rows (mx8_slot_key).
//   LDS            a tile is 8 KiB of K^ (64 rows x 128 B, 16-byte chunk c of row r at c ^ (r / 2 % 8)), 8 KiB of V^T (128
//                  rows x 64 B, chunk c of row r at c ^ (r / 4 % 4)) -- both make the 16-byte fragment reads of 16 lanes cover
//                  all 64 banks once -- and 512 B of scales, in a ring of three stages.  Tile t + 2 is fetched into registers
//                  (five loads per thread) before tile t's MFMAs and stored to the stage tile t - 1 left after them: one
//                  barrier per tile, the global latency under a whole tile of matrix work.
//   epilogue       O = O^T * 256 / l (l is summed in units of 2^-8) as bf16, transposed through LDS per wave, 16-byte stores.
#include "common.h"
#include "ops.h"
#include "quant.h"

namespace mc {

namespace {

typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(4))) int i32x4;

constexpr int QB = 256;                       // query rows per workgroup (4 waves x 64)
constexpr int KT = 64;                        // keys per tile
constexpr int HD = 128;                       // head dim
constexpr int K_TILE = KT * HD;               // bytes of a K^ tile
constexpr int V_TILE = HD * KT;               // bytes of a V^T tile
constexpr int SC_OFF = K_TILE + V_TILE;       // the tile's scale dwords: K^ (256 B), V^T (256 B)
constexpr int STAGE = SC_OFF + 512;
constexpr int NST = 3;                        // ring depth
constexpr int LDS_BYTES = NST * STAGE;
constexpr int O_ROW = 2 * HD + 16;            // bytes of a row of the epilogue's transpose (16 B pad)
constexpr int P_SCALE = 0x77777777;           // E8M0 127 - 8: the probabilities are packed as 256 p
constexpr float NEG_INF = -__builtin_huge_valf();
static_assert(4 * 32 * O_ROW <= LDS_BYTES, "the epilogue's transpose lives in the ring");

// the slots of a 64-key tile are a permutation of its keys, block by block
constexpr bool slot_key_is_permutation() {
  unsigned long long seen = 0;
  for (int s = 0; s < KT; ++s) {
    if (mx8_slot_key(s) / 32 != s / 32) return false;
    seen |= 1ull << mx8_slot_key(s);
  }
  return seen == ~0ull;
}
static_assert(slot_key_is_permutation(), "mx8_slot_key");

__device__ __forceinline__ i32x8 cat(i32x4 lo, i32x4 hi) { return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7); }

// 32 bf16 (four 16-byte loads) -> fp32 times f
__device__ __forceinline__ void load32_bf16(const bf16_t* p, float f, float (&v)[32]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const u32x4 t = *(const u32x4*)(p + i * 8);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[8 * i + 2 * j] = __uint_as_float(t[j] << 16) * f;
      v[8 * i + 2 * j + 1] = __uint_as_float(t[j] & 0xffff0000u) * f;
    }
  }
}

// 32 values -> their MX exponent and 32 e4m3 bytes (quant.h's arithmetic)
__device__ __forceinline__ int quantize32(const float (&v)[32], u32x4& lo, u32x4& hi) {
  float amax = 0.f;
#pragma unroll
  for (int i = 0; i < 32; ++i) amax = fmaxf(amax, fabsf(v[i]));
  const int e = mx_exponent(amax);
  const float inv = mx_inv_scale(e);
  uint32_t w[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) w[i] = (uint32_t)pack4_e4m3(v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3], inv);
  lo = u32x4{w[0], w[1], w[2], w[3]};
  hi = u32x4{w[4], w[5], w[6], w[7]};
  return e;
}

// ------------------------------------------------------------------ pre-pass: Q^ and K^
// One thread per (row, 32 channels).  Rows >= valid: zero bytes, the unit scale.
__global__ __launch_bounds__(256) void attn_quantize_rows_mx8_kernel(const bf16_t* __restrict__ x, long ld, int rows, int valid, int d,
                                                                      float premul, uint8_t* __restrict__ q, uint8_t* __restrict__ s) {
  const int nb = d / 32;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)rows * nb) return;
  const int row = (int)(idx / nb), b = (int)(idx - (long)row * nb);
  u32x4 lo = {0, 0, 0, 0}, hi = {0, 0, 0, 0};
  int e = 0;
  if (row < valid) {
    float v[32];
    load32_bf16(x + (size_t)row * ld + b * 32, premul, v);
    e = quantize32(v, lo, hi);
  }
  u32x4* dst = (u32x4*)(q + (size_t)row * d + b * 32);
  dst[0] = lo;
  dst[1] = hi;
  s[(size_t)(b >> 2) * rows * 4 + mx8_row_scale_index(row, b & 3)] = mx_scale_byte(e);
}

// ------------------------------------------------------------------ pre-pass: V^T
// One workgroup per (64-key tile, head): the tile's bf16 rows through LDS (rows >= valid as zeros, never read), then one
// thread per (channel, 32-slot block) gathers its 32 keys in slot order.
__global__ __launch_bounds__(256) void attn_quantize_vt_mx8_kernel(const bf16_t* __restrict__ v, long ld, int rows, int valid,
                                                                    uint8_t* __restrict__ vt, uint8_t* __restrict__ vs) {
  constexpr int ROW = HD + 8;   // bf16 elements of an LDS row
  __shared__ __attribute__((aligned(16))) bf16_t tile[KT * ROW];
  const int tid = threadIdx.x, t = blockIdx.x, head = blockIdx.y;
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int key = it * 16 + (tid >> 4), c = tid & 15;
    u32x4 w = {0, 0, 0, 0};
    if (t * KT + key < valid) w = *(const u32x4*)(v + (size_t)(t * KT + key) * ld + head * HD + c * 8);
    *(u32x4*)(tile + key * ROW + c * 8) = w;
  }
  __syncthreads();
  const int ch = tid & (HD - 1), sb = tid >> 7;
  float x[32];
#pragma unroll
  for (int j = 0; j < 32; ++j) x[j] = bf16_to_f32(tile[mx8_slot_key(32 * sb + j) * ROW + ch]);
  u32x4 lo, hi;
  const int e = quantize32(x, lo, hi);
  u32x4* dst = (u32x4*)(vt + (size_t)(head * HD + ch) * rows + t * KT + sb * 32);
  dst[0] = lo;
  dst[1] = hi;
  vs[(size_t)head * rows * 4 + mx8_v_scale_index(ch, 2 * t + sb)] = mx_scale_byte(e);
}

// ------------------------------------------------------------------ the kernel
template <int OA, int OB>
__device__ __forceinline__ f32x16 mma(i32x8 a, i32x8 b, f32x16 c, int sa, int sb) {
  return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, 0, 0, OA, sa, OB, sb);
}

__device__ __forceinline__ float max16(const f32x16& a) {
  float m0 = fmaxf(fmaxf(a[0], a[1]), fmaxf(a[2], a[3])), m1 = fmaxf(fmaxf(a[4], a[5]), fmaxf(a[6], a[7]));
  float m2 = fmaxf(fmaxf(a[8], a[9]), fmaxf(a[10], a[11])), m3 = fmaxf(fmaxf(a[12], a[13]), fmaxf(a[14], a[15]));
  return fmaxf(fmaxf(m0, m1), fmaxf(m2, m3));
}

// what a thread moves of a tile: two 16-byte chunks of K^, two of V^T, one scale dword (threads 0..127)
struct Staged {
  u32x4 k[2], v[2];
  uint32_t sc;
};

__global__ __launch_bounds__(256, 1) void attn_mx8_kernel(AttnMx8Images im, bf16_t* __restrict__ O, long ldo, int Lq_pad, int n_heads,
                                                          int rows, int valid, int nqb) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = lane >> 5;
  const int l31 = lane & 31;
  const int d = n_heads * HD;

  const int vb = xcd_remap(blockIdx.x, nqb * n_heads);
  const int head = vb / nqb;
  const int q0 = (vb - head * nqb) * QB + wv * 64;   // this wave's first query row

  // the two 16-byte chunks of a lane's operand: bytes 0..15 and 16..31 carry k = kc0 + 0..15 and kc1 + 0..15 of a 64-k step
  const int kc0 = mx8_operand_k(half, 0), kc1 = mx8_operand_k(half, 16);

  // ---- Q^ fragments [query block][k step] and their scales (bytes 2 qblk + ks of ONE dword): resident for the launch
  i32x8 qf[2][2];
  {
    const uint8_t* qp = im.q + (size_t)(q0 + l31) * d + head * HD;
#pragma unroll
    for (int qblk = 0; qblk < 2; ++qblk)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
        qf[qblk][ks] = cat(*(const i32x4*)(qp + (size_t)qblk * 32 * d + 64 * ks + kc0), *(const i32x4*)(qp + (size_t)qblk * 32 * d + 64 * ks + kc1));
  }
  const int qsc = *(const int*)(im.qs + (size_t)head * Lq_pad * 4 + (size_t)q0 * 4 + lane * 4);

  // ---- global -> LDS staging of a tile
  const int kr = tid >> 3, kc = tid & 7;     // K^: rows kr and kr + 32, chunk kc
  const int vr = tid >> 2, vc = tid & 3;     // V^T: channels vr and vr + 64, chunk vc
  const uint8_t* ksrc = im.k + (size_t)kr * d + head * HD + kc * 16;
  const uint8_t* vsrc = im.vt + (size_t)(head * HD + vr) * rows + vc * 16;
  const uint8_t* ssrc = (tid < 64 ? im.ks : im.vs) + (size_t)head * rows * 4 + (tid & 63) * 4;
  const int kdst = kr * 128 + ((kc ^ ((kr >> 1) & 7)) << 4);   // (kr + 32) / 2 % 8 == kr / 2 % 8
  const int vdst = K_TILE + vr * 64 + ((vc ^ ((vr >> 2) & 3)) << 4);
  auto fetch = [&](int t, Staged& g) {
    g.k[0] = *(const u32x4*)(ksrc + (size_t)t * KT * d);
    g.k[1] = *(const u32x4*)(ksrc + (size_t)t * KT * d + (size_t)32 * d);
    g.v[0] = *(const u32x4*)(vsrc + t * KT);
    g.v[1] = *(const u32x4*)(vsrc + (size_t)64 * rows + t * KT);
    if (tid < 128) g.sc = *(const uint32_t*)(ssrc + (size_t)t * 256);
  };
  auto stash = [&](int slot, const Staged& g) {
    char* st = smem + slot * STAGE;
    *(u32x4*)(st + kdst) = g.k[0];
    *(u32x4*)(st + kdst + 32 * 128) = g.k[1];
    *(u32x4*)(st + vdst) = g.v[0];
    *(u32x4*)(st + vdst + 64 * 64) = g.v[1];
    if (tid < 128) *(uint32_t*)(st + SC_OFF + tid * 4) = g.sc;
  };

  // ---- fragment read offsets inside a stage
  const int ksw = (l31 >> 1) & 7, vsw = (l31 >> 2) & 3;
  int koff[2][2];   // [k step][chunk]: row l31 (+ 32 kb), channels 64 ks + kc0 / kc1
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    koff[ks][0] = l31 * 128 + ((((64 * ks + kc0) >> 4) ^ ksw) << 4);
    koff[ks][1] = l31 * 128 + ((((64 * ks + kc1) >> 4) ^ ksw) << 4);
  }
  const int voff0 = K_TILE + l31 * 64 + (((kc0 >> 4) ^ vsw) << 4);   // row l31 (+ 32 cb), slots kc0 / kc1
  const int voff1 = K_TILE + l31 * 64 + (((kc1 >> 4) ^ vsw) << 4);

  f32x16 o[4][2];   // O^T [channel block][query block]
#pragma unroll
  for (int cb = 0; cb < 4; ++cb)
#pragma unroll
    for (int qblk = 0; qblk < 2; ++qblk)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[cb][qblk][r] = 0.f;
  float m_run[2] = {NEG_INF, NEG_INF}, l_run[2] = {0.f, 0.f};   // l in units of 2^-8, this lane's keys only
  const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

  const int ntiles = (valid + KT - 1) / KT;
  {
    Staged g;
    fetch(0, g);
    stash(0, g);
    if (ntiles > 1) {
      fetch(1, g);
      stash(1, g);
    }
  }
  __syncthreads();

  int slot = 0;
  for (int t = 0; t < ntiles; ++t) {
    Staged nxt;
    const bool more = t + 2 < ntiles;   // uniform
    if (more) fetch(t + 2, nxt);        // in flight under this tile's MFMAs
    const char* st = smem + slot * STAGE;
    const int ksc = *(const int*)(st + SC_OFF + lane * 4);         // bytes 2 kb + ks
    const int vsc = *(const int*)(st + SC_OFF + 256 + lane * 4);   // byte cb

    // ---- S^T = K^ Q^T
    f32x16 s[2][2];   // [key block][query block]
#define MC_QK(kb, ks)                                                                                                     \
  {                                                                                                                       \
    const i32x8 a = cat(*(const i32x4*)(st + (kb) * 32 * 128 + koff[ks][0]), *(const i32x4*)(st + (kb) * 32 * 128 + koff[ks][1])); \
    s[kb][0] = mma<2 * (kb) + (ks), (ks)>(a, qf[0][ks], (ks) ? s[kb][0] : zero16, ksc, qsc);                              \
    s[kb][1] = mma<2 * (kb) + (ks), 2 + (ks)>(a, qf[1][ks], (ks) ? s[kb][1] : zero16, ksc, qsc);                          \
  }
    MC_QK(0, 0) MC_QK(1, 0) MC_QK(0, 1) MC_QK(1, 1)
#undef MC_QK

    // keys >= valid of the tail tile: -inf before the maximum and the exponentials (uniform branch)
    const int nvalid = valid - t * KT;
    if (nvalid < KT) {
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (32 * kb + mfma32_acc_row(half, r) >= nvalid) {
            s[kb][0][r] = NEG_INF;
            s[kb][1][r] = NEG_INF;
          }
    }

    // ---- online softmax, P packed as the B operand
    i32x8 pw[2];
    float alpha[2];
#pragma unroll
    for (int qblk = 0; qblk < 2; ++qblk) {
      const float mx = half_swap_max(fmaxf(max16(s[0][qblk]), max16(s[1][qblk])));
      const float m_new = fmaxf(m_run[qblk], mx);
      alpha[qblk] = __builtin_amdgcn_exp2f(m_run[qblk] - m_new);   // first tile: exp2(-inf) = 0
      m_run[qblk] = m_new;
      const float mb = m_new - 8.0f;   // 256 p
      float sum0 = 0.f, sum1 = 0.f;
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
          s[kb][qblk][r] = __builtin_amdgcn_exp2f(s[kb][qblk][r] - mb);
          s[kb][qblk][r + 1] = __builtin_amdgcn_exp2f(s[kb][qblk][r + 1] - mb);
          sum0 += s[kb][qblk][r];
          sum1 += s[kb][qblk][r + 1];
        }
      l_run[qblk] = l_run[qblk] * alpha[qblk] + (sum0 + sum1);
      // byte 16 kb + r of the operand <- register r of key block kb (the order mx8_slot_key inverts)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const f32x16& sv = s[j >> 2][qblk];
        const int r = 4 * (j & 3);
        const int w = __builtin_amdgcn_cvt_pk_fp8_f32(sv[r], sv[r + 1], 0, false);
        pw[qblk][j] = __builtin_amdgcn_cvt_pk_fp8_f32(sv[r + 2], sv[r + 3], w, true);
      }
    }
    if (__any(alpha[0] != 1.0f || alpha[1] != 1.0f)) {
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) {
        o[cb][0] = o[cb][0] * alpha[0];
        o[cb][1] = o[cb][1] * alpha[1];
      }
    }

    // ---- O^T += V^T P^T
#define MC_PV(cb)                                                                                                        \
  {                                                                                                                      \
    const i32x8 a = cat(*(const i32x4*)(st + (cb) * 32 * 64 + voff0), *(const i32x4*)(st + (cb) * 32 * 64 + voff1));      \
    o[cb][0] = mma<(cb), 0>(a, pw[0], o[cb][0], vsc, P_SCALE);                                                            \
    o[cb][1] = mma<(cb), 0>(a, pw[1], o[cb][1], vsc, P_SCALE);                                                            \
  }
    MC_PV(0) MC_PV(1) MC_PV(2) MC_PV(3)
#undef MC_PV

    // tile t + 2 into the stage tile t - 1 left (every wave passed the last barrier after reading it)
    if (more) stash(slot == 0 ? NST - 1 : slot - 1, nxt);
    __syncthreads();
    slot = slot + 1 == NST ? 0 : slot + 1;
  }

  // ---- epilogue: O[q][ch] = O^T[ch][q] * 256 / l, a wave's 32 x 128 block at a time through its own LDS rows (the ring is
  // free: the loop ended with a barrier)
  char* ob = smem + wv * (32 * O_ROW);
#pragma unroll
  for (int qblk = 0; qblk < 2; ++qblk) {
    const float inv = 256.0f / half_swap_sum(l_run[qblk]);
#pragma unroll
    for (int cb = 0; cb < 4; ++cb)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x16& a = o[cb][qblk];
        const u32x2 w = {pack_bf16x2(a[4 * g] * inv, a[4 * g + 1] * inv), pack_bf16x2(a[4 * g + 2] * inv, a[4 * g + 3] * inv)};
        *(u32x2*)(ob + l31 * O_ROW + (32 * cb + mfma32_acc_row(half, 4 * g)) * 2) = w;
      }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int row = it * 4 + (lane >> 4), c = lane & 15;
      const u32x4 w = *(const u32x4*)(ob + row * O_ROW + c * 16);
      *(u32x4*)(O + (size_t)(q0 + 32 * qblk + row) * ldo + head * HD + c * 8) = w;
    }
    __builtin_amdgcn_wave_barrier();
  }
}

}  // namespace

bool attention_mx8_supports(const AttnParams& p, const AttnMx8Images& im) {
  auto al16 = [](const void* q) { return q && ((uintptr_t)q & 15) == 0; };
  if (!attention_shape_ok(p) || !attention_plain_form(p)) return false;
  const size_t d = (size_t)p.n_heads * HD;   // byte offsets into the e4m3 images are 32-bit
  if ((size_t)p.Lq_pad * d >= (1ull << 32) || (size_t)p.shard_rows * d >= (1ull << 32)) return false;
  return al16(im.q) && al16(im.qs) && al16(im.k) && al16(im.ks) && al16(im.vt) && al16(im.vs);
}

hipError_t launch_attn_quantize_mx8(const AttnParams& p, const AttnMx8Images& im, hipStream_t stream) {
  if (!attention_mx8_supports(p, im)) return hipErrorInvalidValue;
  const int d = p.n_heads * HD;
  const auto blocks = [&](int rows) { return dim3((unsigned)(((size_t)rows * (d / 32) + 255) / 256)); };
  hipLaunchKernelGGL(attn_quantize_rows_mx8_kernel, blocks(p.Lq_pad), dim3(256), 0, stream, p.Q, p.ldq, p.Lq_pad, p.Lq_pad, d,
                     p.scale * 1.4426950408889634f, im.q, im.qs);
  hipLaunchKernelGGL(attn_quantize_rows_mx8_kernel, blocks(p.shard_rows), dim3(256), 0, stream, p.K, p.ldk, p.shard_rows,
                     p.shard_valid, d, 1.0f, im.k, im.ks);
  hipLaunchKernelGGL(attn_quantize_vt_mx8_kernel, dim3(p.shard_rows / KT, p.n_heads), dim3(256), 0, stream, p.V, p.ldv,
                     p.shard_rows, p.shard_valid, im.vt, im.vs);
  return hipGetLastError();
}

hipError_t launch_attention_mx8(const AttnParams& p, const AttnMx8Images& im, hipStream_t stream) {
  if (!attention_mx8_supports(p, im)) return hipErrorInvalidValue;
  const int nqb = p.Lq_pad / QB;
  return launch_dynamic_lds<attn_mx8_kernel>(dim3(nqb * p.n_heads), dim3(256), LDS_BYTES, stream, im, p.O, p.ldo, p.Lq_pad, p.n_heads,
                                             p.shard_rows, p.shard_valid, nqb);
}

}  // namespace mc
