// The tile-mask predictor for gfx950: from a self-attention launch's own Q and K to the key-tile bitmap attention_sparse.hip
// walks, on the device, in two plain launches.  head_dim 128, bf16 operands, everything after the loads in fp32.
//
// The rule (one definition; include/magcache_hip.h: mc_op_attention_tile_predict, ops.h: AttnPredict).  Q [Lq_pad][ldq] and
// K [rows][ldk] as the attention kernels read them, the first `valid` rows of each are tokens; nqt = Lq_pad / 128,
// nkt = rows / 64, vk = ceil(valid / 64), words = (nkt + 31) / 32.  For every head h and query tile qt:
//   n_q(qt), n_k(kt)  the rows i of the tile with i < valid
//   q~[h][qt], k~[h][kt]  the fp32 mean of the tile's VALID rows (zero where there is none)
//   s[kt] = scale <q~, k~[kt]>,  w[kt] = n_k(kt) exp(s[kt] - max s),  p[kt] = w[kt] / sum w      for kt < vk
//   forced = {2 qt, 2 qt + 1} below vk: the key tiles that hold the query tile's own rows, always kept
//   theta  = the largest p[kt], kt not forced, with  sum_forced p + sum_{kt not forced, p[kt] >= theta} p[kt] >= mass;
//            the forced tiles alone reach mass: no other tile is kept; no theta reaches it (rounding only): every tile < vk
//   bit kt is set iff kt is forced or p[kt] >= theta -- ties at theta are all kept: a threshold, not a sort; bits at
//   kt >= vk are clear; a query tile without a valid row holds its forced bits only (possibly none).
// mass = 1 keeps every tile whose share the fp32 sums can still resolve, which need not be every tile.
// Output: uint32 [n_heads][nqt][words] -- mc_op_attention_sparse's layout and bit order with mask_heads == n_heads.
//
// Pass 1, pool (bandwidth: one read of Q and of K).  One workgroup of 4 waves per (row tile, head), Q tiles first, heads
// innermost so that neighbouring workgroups read neighbouring columns of the same rows.  A lane owns 8 channels (one 16-byte
// load) of the rows r = 4 wave + lane / 16 (mod 16): 16 lanes cover a head's 256-byte row, a wave four rows.  Only rows below
// the tile's valid count are loaded -- the tile with valid - 1 in it is handled by that count, padding rows are never data.
// The order of the sum is fixed: a lane adds its rows in ascending order, the four row slots of a wave meet in two butterfly
// steps (each a commutative add of the same pair, so every lane holds the same bits), the four waves through LDS in wave order.
//
// Pass 2, select.  One workgroup of 4 waves per (head, 4 query tiles), one wave per query tile.  The head's pooled k rows pass
// through LDS 64 tiles at a time (rows padded to 132 floats: a 16-byte read per lane is conflict-free), shared by the four
// waves; lane i of a wave takes tile c0 + i of the chunk and runs the 128 FMAs of its dot product in ascending channel order
// against the wave's q~ (LDS, broadcast reads).  PLAIN FMAs, no matrix instruction: the work is below 0.1 % of the
// attention's, one lane per score makes the order of every sum a property of the source text, and bf16 MFMAs would move the
// shares by ~1e-2, the size of the gaps the selection decides on.
// A wave keeps its scores, then its shares, in its own 8 KiB of LDS at [kt]: lane i only ever touches the entries kt = i
// (mod 64), so LDS is per-lane indexed storage here and no lane reads what another wrote; what crosses lanes goes through
// wave reductions (butterflies again: the same bits in every lane, the branch on them is wave-uniform).
// Softmax in base 2 like the attention kernels.  The threshold is found without a sort: positive fp32 values order like their
// bit patterns, so theta's pattern is built from bit 30 down -- 31 rounds of "would the shares with pattern >= candidate,
// plus the forced ones, still reach mass?", each a compare-add over the lane's entries and one wave sum.  The forced tiles'
// shares are added up first and then zeroed in place: they never compete.  Bits are assembled with one ballot per 64 tiles
// and stored as whole words by lanes 0 and 1 (vector stores); every word of the row is written.  No atomics.
//
// Limit: nkt <= kAttnPredictMaxNkt = 2048 (the per-wave share array); Wan2.1-14B 720p has nkt = 1182.
#include "common.h"
#include "ops.h"

namespace mc {

namespace {

constexpr int QT = 128;   // query rows per mask row
constexpr int KT = 64;    // keys per mask bit
constexpr int HD = 128;
constexpr int WAVES = 4;
constexpr int CHUNK = 64;        // pooled k rows staged per round: one per lane
constexpr int KROW = HD + 4;     // floats per staged row
constexpr int SELECT_LDS = (CHUNK * KROW + WAVES * HD + WAVES * kAttnPredictMaxNkt) * (int)sizeof(float);   // 67 KiB: two workgroups per CU
constexpr float LOG2E = 1.4426950408889634f;

struct PoolArgs {
  const bf16_t* Q; long ldq;
  const bf16_t* K; long ldk;
  int nqt, nkt, n_heads, valid;
  float *q_pool, *k_pool;
};

__global__ __launch_bounds__(256) void predict_pool_kernel(PoolArgs a) {
  __shared__ float part[WAVES][HD];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = tid >> 6;
  const int c8 = lane & 15;   // this lane's 8 channels
  // ---- the item: (Q | K, row tile, head)
  int item = blockIdx.x;
  const bool is_q = item < a.nqt * a.n_heads;
  if (!is_q) item -= a.nqt * a.n_heads;
  const int tile = item / a.n_heads;
  const int head = item - tile * a.n_heads;
  const int R = is_q ? QT : KT;
  const long ld = is_q ? a.ldq : a.ldk;
  const int n = min(max(a.valid - tile * R, 0), R);   // valid rows of the tile
  const bf16_t* src = (is_q ? a.Q : a.K) + (size_t)tile * R * ld + head * HD + c8 * 8;

  float acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = 0.f;
#pragma unroll 4
  for (int r = wv * 4 + (lane >> 4); r < n; r += 16) {
    const u32x4 v = *(const u32x4*)(src + (size_t)r * ld);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      acc[2 * i] += __uint_as_float(v[i] << 16);
      acc[2 * i + 1] += __uint_as_float(v[i] & 0xffff0000u);
    }
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    acc[i] += __shfl_xor(acc[i], 16, 64);
    acc[i] += __shfl_xor(acc[i], 32, 64);
  }
  if (lane < 16) {
#pragma unroll
    for (int i = 0; i < 8; ++i) part[wv][c8 * 8 + i] = acc[i];
  }
  __syncthreads();
  if (tid < HD) {
    const float sum = ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
    float* out = is_q ? a.q_pool + ((size_t)head * a.nqt + tile) * HD : a.k_pool + ((size_t)head * a.nkt + tile) * HD;
    out[tid] = n ? sum / (float)n : 0.f;
  }
}

struct SelectArgs {
  const float *q_pool, *k_pool;
  uint32_t* bits;
  int nqt, nkt, n_heads, valid, words;
  float scale2;   // scale * log2(e)
  float mass;
};

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

__global__ __launch_bounds__(256, 2) void predict_select_kernel(SelectArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* kst = (float*)smem;                  // [CHUNK][KROW]: the pooled k rows of the round
  float* qst = kst + CHUNK * KROW;            // [WAVES][HD]: each wave's q~
  float* shares = qst + WAVES * HD;           // [WAVES][kAttnPredictMaxNkt]: each wave's scores, then weights, then shares
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int groups = (a.nqt + WAVES - 1) / WAVES;
  const int head = blockIdx.x / groups;
  const int qt = (blockIdx.x - head * groups) * WAVES + wv;
  const bool live = qt < a.nqt;               // wave-uniform; a wave beyond the last query tile only helps to stage
  const int vk = (a.valid + KT - 1) / KT;     // <= nkt <= kAttnPredictMaxNkt
  float* my = shares + wv * kAttnPredictMaxNkt;
  const float* q = qst + wv * HD;

  if (live) {
    const float* qp = a.q_pool + ((size_t)head * a.nqt + qt) * HD;
    qst[wv * HD + lane] = qp[lane];
    qst[wv * HD + 64 + lane] = qp[64 + lane];
  }
  // ---- scores in log2 units: s2[kt] = scale log2(e) <q~, k~[kt]>
  const float* kp = a.k_pool + (size_t)head * a.nkt * HD;
  for (int c0 = 0; c0 < vk; c0 += CHUNK) {
    __syncthreads();   // every wave is past the rows of the round before (and, the first time, q~ has landed)
    const int nrow = min(CHUNK, vk - c0);
    for (int i = tid; i < nrow * (HD / 4); i += 256) {
      const int r = i >> 5, c4 = i & 31;
      *(f32x4*)(kst + r * KROW + c4 * 4) = *(const f32x4*)(kp + (size_t)(c0 + r) * HD + c4 * 4);
    }
    __syncthreads();
    if (live && lane < nrow) {
      const float* kr = kst + lane * KROW;
      float acc = 0.f;
#pragma unroll 8
      for (int c4 = 0; c4 < HD / 4; ++c4) {
        const f32x4 kv = *(const f32x4*)(kr + c4 * 4);
        const f32x4 qv = *(const f32x4*)(q + c4 * 4);
        acc = fmaf(qv[0], kv[0], acc);
        acc = fmaf(qv[1], kv[1], acc);
        acc = fmaf(qv[2], kv[2], acc);
        acc = fmaf(qv[3], kv[3], acc);
      }
      my[c0 + lane] = acc * a.scale2;
    }
  }
  if (!live) return;   // (no barrier below)

  // ---- this lane's entries: kt = 64 j + lane < vk
  const int nj = (vk + 63) >> 6;
  float m = -__builtin_huge_valf();
  for (int j = 0; j < nj; ++j) {
    const int kt = j * 64 + lane;
    if (kt < vk) m = fmaxf(m, my[kt]);
  }
  m = wave_max(m);
  // weights: the keys of a tile times exp2(s2 - max); the tile with valid - 1 in it counts its valid keys
  const int n_last = a.valid - (vk - 1) * KT;
  float wsum = 0.f;
  for (int j = 0; j < nj; ++j) {
    const int kt = j * 64 + lane;
    if (kt < vk) {
      const float w = (float)(kt == vk - 1 ? n_last : KT) * __builtin_amdgcn_exp2f(my[kt] - m);
      my[kt] = w;
      wsum += w;
    }
  }
  wsum = wave_sum(wsum);   // >= 1: the maximum's tile holds a key
  // shares; the forced tiles' are added up and leave the competition (0 in place)
  float forced = 0.f;
  for (int j = 0; j < nj; ++j) {
    const int kt = j * 64 + lane;
    if (kt < vk) {
      float p = my[kt] / wsum;
      if ((kt >> 1) == qt) {
        forced += p;
        p = 0.f;
      }
      my[kt] = p;
    }
  }
  forced = wave_sum(forced);   // at most two non-zero terms: exact whatever the order

  // ---- theta's bit pattern: the largest t with forced + sum{p : pattern(p) >= t} >= mass.  t = 0 keeps every tile below vk
  // (also where rounding leaves the whole sum short of mass); a pattern above every float keeps the forced tiles only.
  const int n_q = min(max(a.valid - qt * QT, 0), QT);
  uint32_t t = 0xffffffffu;
  if (n_q > 0 && !(forced >= a.mass)) {
    t = 0;
    for (int b = 30; b >= 0; --b) {
      const uint32_t cand = t | (1u << b);
      float g = 0.f;
      for (int j = 0; j < nj; ++j) {
        const int kt = j * 64 + lane;
        if (kt < vk) {
          const float p = my[kt];
          if (__float_as_uint(p) >= cand) g += p;
        }
      }
      if (forced + wave_sum(g) >= a.mass) t = cand;   // wave-uniform
    }
  }

  // ---- bits: one ballot per 64 tiles, lanes 0 and 1 store its two words; every word of the row, zeros behind vk
  uint32_t* row = a.bits + ((size_t)head * a.nqt + qt) * a.words;
  for (int j = 0; j < (a.nkt + 63) >> 6; ++j) {
    const int kt = j * 64 + lane;
    bool keep = false;
    if (kt < vk) keep = (kt >> 1) == qt || __float_as_uint(my[kt]) >= t;
    const unsigned long long b = __ballot(keep);
    const uint32_t word = (lane & 1) ? (uint32_t)(b >> 32) : (uint32_t)b;
    if (lane < 2 && 2 * j + lane < a.words) row[2 * j + lane] = word;
  }
}

}  // namespace

bool attention_predict_supports(const AttnPredict& p) {
  AttnParams shape = {};
  shape.Lq_pad = p.Lq_pad; shape.n_heads = p.n_heads; shape.shard_rows = p.rows; shape.shard_valid = p.valid; shape.n_shards = 1;
  shape.ldq = p.ldq; shape.ldk = p.ldk; shape.ldv = p.ldk;
  if (!attention_shape_ok(shape)) return false;
  const auto al16 = [](const void* q) { return q && ((uintptr_t)q & 15) == 0; };
  const size_t d = (size_t)p.n_heads * HD;
  if (!al16(p.Q) || !al16(p.K) || (size_t)p.ldq < d || (size_t)p.ldk < d) return false;
  if ((size_t)p.Lq_pad * p.ldq * 2 >= (1ull << 32) || (size_t)p.rows * p.ldk * 2 >= (1ull << 32)) return false;
  if (!(p.mass > 0.f && p.mass <= 1.f)) return false;   // (a NaN is refused too)
  if (!p.bits || ((uintptr_t)p.bits & 3) != 0 || !al16(p.scratch)) return false;
  if (p.rows / KT > kAttnPredictMaxNkt) return false;
  return (size_t)p.n_heads * ((size_t)p.Lq_pad / QT + (size_t)p.rows / KT) < (1ull << 31);
}

hipError_t launch_attention_predict(const AttnPredict& p, hipStream_t stream) {
  if (!attention_predict_supports(p)) return hipErrorInvalidValue;
  const int nqt = p.Lq_pad / QT, nkt = p.rows / KT;
  float* q_pool = (float*)p.scratch;
  float* k_pool = q_pool + (size_t)p.n_heads * nqt * HD;
  const PoolArgs pa = {p.Q, p.ldq, p.K, p.ldk, nqt, nkt, p.n_heads, p.valid, q_pool, k_pool};
  hipLaunchKernelGGL(predict_pool_kernel, dim3((nqt + nkt) * p.n_heads), dim3(256), 0, stream, pa);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  const SelectArgs sa = {q_pool, k_pool, p.bits, nqt, nkt, p.n_heads, p.valid, (nkt + 31) / 32, p.scale * LOG2E, p.mass};
  return launch_dynamic_lds<predict_select_kernel>(dim3(p.n_heads * ((nqt + WAVES - 1) / WAVES)), dim3(256), SELECT_LDS, stream, sa);
}

}  // namespace mc
