// Tile-sparse self-attention over key SHARDS for gfx950, with a log-sum-exp out and a merge in: the form a sequence-parallel
// engine needs.  head_dim 128, bf16 operands, fp32 online softmax in base 2.
//
// The argument contract is stated once, in ops.h (AttnShardMask, attention_sparse_shards_supports) and at
// include/magcache_hip.h: mc_op_attention_sparse_partial.  In short: AttnParams in its full form -- n_shards shards of shard_rows
// rows, k_shard_stride / v_shard_stride apart, the first shard_valid rows of each are keys, skip_shard_p1 leaves one out --
// and a mask row uint32 bits[mask_heads][Lq_pad / 128][row_words] of which THIS launch sees a slice: key tile t of shard s is
// bit bit0 + s * bit_shard_stride + t, for t < tps = ceil(shard_valid / 64).
//
// Work split and data movement are attention_sparse.hip's: one workgroup of 4 waves x 32 rows per (128 query rows, head), two
// workgroups per CU, 64 KiB of LDS as a ring of two (K image, V image) stages filled by LDS-DMA, tile t + 1 issued behind the
// barrier that opens tile t.  Tile images, Q fragments, fragment reads, the PV step and the O store are attention_tile.h's.
//
// What this kernel adds.
//
// The walk over bit RANGES.  A shard owns the bits [lo, lo + tps) of the row, lo = bit0 + s * bit_shard_stride: a range that
// starts and ends anywhere inside a word and may cross words.  The iterator is wave-uniform scalar state
// (shard, word index, word): the next tile is ctz(word), word &= word - 1 clears it, an exhausted word is replaced by the next
// word of the range (a scalar load through the constant address space), an exhausted range by the first word of the next
// shard that is not skipped.  The first word of a range is and-ed with ~0 << (lo & 31), the last with the bits up to
// (lo + tps - 1) & 31 -- both when the range lies in one word --, so a bit outside the ranges is never taken for a tile, and
// only words lo >> 5 .. (lo + tps - 1) >> 5 are loaded, which the host has checked to lie in [0, row_words).  The iterator
// runs one tile ahead of the compute ACROSS shard boundaries: what it hands the DMA is (shard, tile), and the base address is
// formed from both.
//
// Two classes of tile (a wave-uniform scalar branch): the tile tps - 1 of every shard when shard_valid % 64 != 0 takes one compare
// per score, -inf BEFORE the row maximum; every other visited tile takes none.  Every visited tile holds a valid key, so the
// first visited tile's row maximum is the softmax reference and there is no `seen` state (attention_sparse.hip).
//
// Log-sum-exp and merge.  lse = m_ref + log2(l) per row, written to lse_out by the lower lane half.  With lse_in, O already
// holds a normalised result over other keys: O = ca * O_prev + cb * O_own with the weights taken relative to
// mm = max(lse_prev, lse_own).  An EMPTY walk is ordinary here (a gather round in which a query tile sees nothing):
//   no lse_in        O = exact zeros, lse_out = -inf
//   lse_in           O is not touched, lse_out = lse_in
// and a row whose lse_in is -inf takes the kernel's own result alone (O_prev is not blended in: it may hold anything).  The
// epilogue branches on mm == -inf before it forms a weight, so no expression subtracts two infinities.
//
// Order: blockIdx.x indexes the optional table order[] of item ids qt * n_heads + head, clamped; null is the identity.  No
// xcd_remap below it (attention_sparse.hip says why).
// the LDS-DMA asm of attention_tile.h names m0 in its clobber list on purpose (reserved register: the compiler only warns)
#pragma clang diagnostic ignored "-Winline-asm"
#include "attention_tile.h"

namespace mc {

namespace {

constexpr int QT = 128;   // query rows per workgroup (4 waves x 32)
constexpr int STAGE_BYTES = 2 * TILE_BYTES;  // K tile, V tile
constexpr int LDS_BYTES = 2 * STAGE_BYTES;   // 64 KiB: two workgroups per CU

struct ShardBits {
  const uint32_t* bits;
  const int32_t* order;
  int mask_heads, nqt, row_words, bit0, bit_shard_stride;
};

// the set bits of one mask row inside the shards' bit ranges, shard by shard in ascending order; every member is wave-uniform
// (the row lives in the constant address space, for attention_sparse.hip's reason)
typedef const uint32_t __attribute__((address_space(4))) * MaskRow;
struct ShardWalk {
  MaskRow row;
  uint32_t word, last_keep;
  int s, wi, last_word, lo;            // the shard in hand, the word in hand, the last word of its range, its first bit
  int n_shards, skip, tps, bit0, stride;
  // the first word of shard sh's range, masked at both ends
  __device__ __forceinline__ void open(int sh) {
    s = sh;
    lo = bit0 + sh * stride;
    const int hi = lo + tps - 1;       // the last bit of the range
    wi = lo >> 5;
    last_word = hi >> 5;
    last_keep = (2u << (hi & 31)) - 1u;   // bits 0 .. hi & 31 (bit 31: 2u << 31 wraps to 0, minus one = all)
    word = row[wi] & (~0u << (lo & 31));
    if (wi == last_word) word &= last_keep;
  }
  __device__ __forceinline__ void start(const uint32_t* r, const AttnParams& p, const ShardBits& b) {
    row = (MaskRow)(uintptr_t)r;
    n_shards = p.n_shards; skip = p.skip_shard_p1 - 1;
    tps = (p.shard_valid + KT - 1) / KT;
    bit0 = b.bit0; stride = b.bit_shard_stride;
    word = 0; wi = last_word = 0; last_keep = 0; lo = 0;
    s = skip == 0 ? 1 : 0;
    if (s < n_shards) open(s);
  }
  // the next visible tile of shard `s` (the member, as it stands on return), -1 when every range is exhausted
  __device__ __forceinline__ int next() {
    for (;;) {
      if (s >= n_shards) return -1;
      if (word) break;
      if (wi < last_word) {
        ++wi;
        word = row[wi];
        if (wi == last_word) word &= last_keep;
      } else {
        int sh = s + 1;
        if (sh == skip) ++sh;
        if (sh >= n_shards) { s = n_shards; return -1; }
        open(sh);
      }
    }
    const int t = wi * 32 + __builtin_ctz(word) - lo;
    word &= word - 1;
    return t;
  }
};

__global__ __launch_bounds__(256, 2) void attn_sparse_shards_kernel(AttnParams p, ShardBits tm) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = lane >> 5;
  const int l31 = lane & 31;

  // ---- the item
  int item = tm.order ? tm.order[blockIdx.x] : (int)blockIdx.x;
  item = __builtin_amdgcn_readfirstlane(min(max(item, 0), tm.nqt * p.n_heads - 1));
  const int qt = item / p.n_heads;
  const int head = item - qt * p.n_heads;
  const int tail = (p.shard_valid % KT) ? (p.shard_valid - 1) / KT : -1;   // the tile of every shard that needs a compare per score
  ShardWalk walk;
  walk.start(tm.bits + ((size_t)(tm.mask_heads == 1 ? 0 : head) * tm.nqt + qt) * tm.row_words, p, tm);

  const int qrow = qt * QT + wv * 32 + l31;
  bf16_t* op = p.O + (size_t)qrow * p.ldo + head * HD + 4 * half;
  const size_t lse_at = (size_t)head * p.Lq_pad + qrow;

  int t_cur = walk.next(), s_cur = walk.s, t_next = -1, s_next = 0;
  if (t_cur < 0) {   // ---- an empty walk (workgroup-uniform): nothing is loaded
    if (p.lse_in) {  // O stays; the log-sum-exp is handed on
      if (p.lse_out && p.lse_out != p.lse_in && half == 0) p.lse_out[lse_at] = p.lse_in[lse_at];
      return;
    }
    const u32x2 zero = {0u, 0u};
#pragma unroll
    for (int db = 0; db < 4; ++db)
#pragma unroll
      for (int g = 0; g < 4; ++g) *(u32x2*)(op + db * 32 + 8 * g) = zero;
    if (p.lse_out && half == 0) p.lse_out[lse_at] = NEG_INF;
    return;
  }

  bf16x8 qf[8];
  MC_ATTN_LOAD_Q(p, qrow, head, half, qf)
  uint32_t srcK[4], srcV[4];  // this wave's 4 of the 16 pieces per operand tile: byte offsets from the tile's first row
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int row = (wv * 4 + j) * 4 + (lane >> 4);
    const int slot = lane & 15;
    srcK[j] = MC_ATTN_PIECE_SRC(row, p.ldk, head, MC_ATTN_K_SRC_CHUNK(slot, row));
    srcV[j] = MC_ATTN_PIECE_SRC(row, p.ldv, head, MC_ATTN_V_SRC_CHUNK(slot, row));
  }
  const uint32_t dma_lds = (uint32_t)(uintptr_t)MC_LDS_PTR(smem) + wv * 4096;  // this wave's 4 pieces inside a tile image
  auto dma_tile = [&](int s, int t, int stage) {
    const bf16_t* kp = p.K + (size_t)s * p.k_shard_stride + (size_t)t * KT * p.ldk;
    const bf16_t* vp = p.V + (size_t)s * p.v_shard_stride + (size_t)t * KT * p.ldv;
    const uint32_t dst = dma_lds + stage * STAGE_BYTES;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      dma_piece(kp, srcK[j], dst + j * 1024);
      dma_piece(vp, srcV[j], dst + TILE_BYTES + j * 1024);
    }
  };
  int koff[8], voff[4];
  MC_ATTN_FRAG_OFFSETS(lane, half, l31, TILE_BYTES, koff, voff)

  f32x16 o[4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[i][r] = 0.f;
  float l_run = 0.f;   // this lane's share of the row sum
  f32x16 c_init;       // -m_ref in every register: the accumulator a tile's first MFMA starts from
#pragma unroll
  for (int r = 0; r < 16; ++r) c_init[r] = 0.f;
  bool first = true;   // wave-uniform: the tile the reference is taken from

  auto tile = [&](int t, int stage) __attribute__((always_inline)) {
    const char* st = smem + stage * STAGE_BYTES;
    // ---- S^T = K Q^T - m_ref: lane holds query l31, keys (r&3) + 8*(r>>2) + 4*half of key block 0 (s0) and 1 (s1)
    f32x16 s0, s1;
#pragma unroll
    for (int ds = 0; ds < 8; ++ds) {
      const bf16x8 ka = *(const bf16x8*)(st + koff[ds]);
      const bf16x8 kb = *(const bf16x8*)(st + koff[ds] + 32 * 256);
      s0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ka, qf[ds], ds ? s0 : c_init, 0, 0, 0);
      s1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kb, qf[ds], ds ? s1 : c_init, 0, 0, 0);
    }
    if (t == tail) {
      const int key0 = t * KT + 4 * half;   // key of register 0, counted inside the shard
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int kk = (r & 3) + 8 * (r >> 2);
        if (key0 + kk >= p.shard_valid) s0[r] = NEG_INF;
        if (key0 + kk + 32 >= p.shard_valid) s1[r] = NEG_INF;
      }
    }
    // ---- reference: the first visited tile's maximum (finite: a visited tile holds a valid key), then only a maximum more
    // than 2^RTHR above it (wave-uniform, rare)
    const float mx = rowmax32(s0, s1);
    if (first || __any(mx > RTHR)) {
      const float d = first ? mx : fmaxf(mx, 0.f);
      const float alpha = first ? 0.f : __builtin_amdgcn_exp2f(-d);   // first: O = l = 0 and stay 0, never exp2 of a large -d
      l_run *= alpha;
#pragma unroll
      for (int i = 0; i < 4; ++i) o[i] = o[i] * alpha;
      s0 = s0 - d;   // -inf stays -inf
      s1 = s1 - d;
      c_init = c_init - d;
      first = false;
    }
    // ---- P = exp2(S): registers 2j, 2j+1 of key block kb -> the packed pair 8*kb + j (pv_step's operand words)
    uint32_t pk[16];
    float rs0 = 0.f, rs1 = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float a0 = __builtin_amdgcn_exp2f(s0[2 * j]), a1 = __builtin_amdgcn_exp2f(s0[2 * j + 1]);
      const float b0 = __builtin_amdgcn_exp2f(s1[2 * j]), b1 = __builtin_amdgcn_exp2f(s1[2 * j + 1]);
      rs0 += a0 + b0;
      rs1 += a1 + b1;
      pk[j] = pack_bf16x2(a0, a1);
      pk[8 + j] = pack_bf16x2(b0, b1);
    }
    l_run += rs0 + rs1;
    // ---- O^T += V^T P^T, micro-step i = 4*ks + db
#pragma unroll
    for (int i = 0; i < 16; ++i) pv_step(o, i, read_vt(st + voff[i & 3] + (i >> 2) * (16 * 256)), pk);
  };
  // one ring step: tile (s_cur, t_cur) has landed in `stage` for every wave and the other stage is free (every wave is past
  // the tile before it); the iterator moves on behind the barrier, one tile ahead of the compute, into the next shard if need be
  auto step = [&](int stage) __attribute__((always_inline)) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    t_next = walk.next();
    s_next = walk.s;
    if (t_next >= 0) dma_tile(s_next, t_next, stage ^ 1);
    tile(t_cur, stage);
    t_cur = t_next;
    s_cur = s_next;
  };

  dma_tile(s_cur, t_cur, 0);
  for (;;) {   // stages as compile-time constants
    step(0);
    if (t_cur < 0) break;
    step(1);
    if (t_cur < 0) break;
  }

  // ---- epilogue: O = O^T / l, the log2-sum-exp m_ref + log2(l), and the merge with what O already holds
  const float l_tot = half_swap_sum(l_run);   // > 0: the walk was not empty and every visited tile holds a valid key
  float inv = 1.0f / l_tot;
  if (p.lse_in || p.lse_out) {   // (uniform)
    float lse = __builtin_amdgcn_logf(l_tot) - c_init[0];   // v_log_f32 is log2; finite
    if (p.lse_in) {
      const float lse_prev = p.lse_in[lse_at];
      const float mm = fmaxf(lse, lse_prev);   // finite, since lse is: no weight below is formed from two infinities
      const float wa = __builtin_amdgcn_exp2f(lse_prev - mm), wb = __builtin_amdgcn_exp2f(lse - mm);
      const float rden = 1.0f / (wa + wb);
      const float ca = wa * rden, cb = wb * rden * inv;
      inv = 1.0f;
      lse = mm + __builtin_amdgcn_logf(wa + wb);
      const bool blend = lse_prev != NEG_INF;   // -inf: the rows of O_prev are not a result, the kernel's own is taken
#pragma unroll
      for (int db = 0; db < 4; ++db) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const u32x2 pv = *(const u32x2*)(op + db * 32 + 8 * g);
          const float p0 = blend ? __uint_as_float(pv[0] << 16) * ca : 0.f, p1 = blend ? __uint_as_float(pv[0] & 0xffff0000u) * ca : 0.f;
          const float p2 = blend ? __uint_as_float(pv[1] << 16) * ca : 0.f, p3 = blend ? __uint_as_float(pv[1] & 0xffff0000u) * ca : 0.f;
          o[db][4 * g] = o[db][4 * g] * cb + p0;
          o[db][4 * g + 1] = o[db][4 * g + 1] * cb + p1;
          o[db][4 * g + 2] = o[db][4 * g + 2] * cb + p2;
          o[db][4 * g + 3] = o[db][4 * g + 3] * cb + p3;
        }
      }
    }
    if (p.lse_out && half == 0) p.lse_out[lse_at] = lse;
  }
  MC_ATTN_STORE_O(op, o, inv)
}

}  // namespace

bool attention_sparse_shards_supports(const AttnParams& p, const AttnShardMask& m) {
  if (!attention_shape_ok(p)) return false;
  const auto al16 = [](const void* q) { return ((uintptr_t)q & 15) == 0; };
  const size_t d = (size_t)p.n_heads * 128;
  if (!p.Q || !p.K || !p.V || !p.O || !al16(p.Q) || !al16(p.K) || !al16(p.V) || !al16(p.O) || !al16(p.lse_in) || !al16(p.lse_out)) return false;
  if ((size_t)p.ldq < d || (size_t)p.ldk < d || (size_t)p.ldv < d || (size_t)p.ldo < d || (p.ldo % 8) != 0) return false;
  // a shard left to visit after the skip
  if (p.skip_shard_p1 < 0 || p.skip_shard_p1 > p.n_shards || p.n_shards - (p.skip_shard_p1 ? 1 : 0) < 1) return false;
  // shard bases stay 16-byte aligned, and the whole K / V span, like every row offset the contract promises, fits 32-bit bytes
  const long gaps = p.n_shards - 1;
  if (gaps && (p.k_shard_stride < 0 || p.v_shard_stride < 0 || (p.k_shard_stride % 8) != 0 || (p.v_shard_stride % 8) != 0)) return false;
  const size_t kspan = (gaps ? (size_t)gaps * p.k_shard_stride : 0) + (size_t)p.shard_rows * p.ldk;
  const size_t vspan = (gaps ? (size_t)gaps * p.v_shard_stride : 0) + (size_t)p.shard_rows * p.ldv;
  if (kspan * 2 >= (1ull << 32) || vspan * 2 >= (1ull << 32) || (size_t)p.Lq_pad * p.ldq * 2 >= (1ull << 32) ||
      (size_t)p.Lq_pad * p.ldo * 2 >= (1ull << 32))
    return false;
  if (!m.bits || ((uintptr_t)m.bits & 3) != 0 || ((uintptr_t)m.order & 3) != 0) return false;
  if (m.mask_heads != 1 && m.mask_heads != p.n_heads) return false;
  // every addressed bit below 32 * row_words: the range of the last shard that is visited ends the highest
  if (m.row_words < 1 || m.bit0 < 0 || m.bit_shard_stride < 0) return false;
  const long last = p.skip_shard_p1 == p.n_shards ? p.n_shards - 2 : p.n_shards - 1;
  const long tps = (p.shard_valid + KT - 1) / KT;
  if ((long)m.bit0 + last * m.bit_shard_stride + tps > 32l * m.row_words) return false;
  return (size_t)(p.Lq_pad / QT) * p.n_heads < (1ull << 31);
}

hipError_t launch_attention_sparse_shards(const AttnParams& p, const AttnShardMask& m, hipStream_t stream) {
  if (!attention_sparse_shards_supports(p, m)) return hipErrorInvalidValue;
  const int nqt = p.Lq_pad / QT;
  const ShardBits tm = {m.bits, m.order, m.mask_heads, nqt, m.row_words, m.bit0, m.bit_shard_stride};
  return launch_dynamic_lds<attn_sparse_shards_kernel>(dim3(nqt * p.n_heads), dim3(256), LDS_BYTES, stream, p, tm);
}

}  // namespace mc
