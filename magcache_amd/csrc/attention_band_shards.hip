// Frame-block causal / windowed self-attention over key SHARDS for gfx950, with a log-sum-exp out and a merge in: the form a
// sequence-parallel engine needs.  head_dim 128, bf16 operands, fp32 online softmax in base 2.
//
// The band in GLOBAL tokens (one definition; ops.h: AttnBandShards, include/magcache_hip.h: mc_op_attention_band_partial).
// AttnParams in its full form -- n_shards shards of shard_rows rows, k_shard_stride / v_shard_stride apart, the first shard_valid
// rows of each are keys, skip_shard_p1 leaves one out.  Query row i stands at global token gq = q_tok0 + min(i, q_valid - 1), in
// block b = gq / block_tokens; key row j of shard s stands at global token key_tok0 + s * key_tok_stride + j and is seen iff
//   lo(b) <= that token < hi(b),   hi(b) = (b + 1) block_tokens,   lo(b) = window_blocks ? max(0, b - window_blocks + 1) block_tokens : 0.
// No mask exists in memory: every bound below is arithmetic on six integers passed by value.
//
// Work split and data movement are attention_band.hip's: one workgroup of 4 waves x 32 rows per (128 query rows, head), two
// workgroups per CU, 64 KiB of LDS as a ring of two (K image, V image) stages filled by LDS-DMA, tile t + 1 issued behind the
// barrier that opens tile t.  Tile images, Q fragments, fragment reads, the PV step and the O store are attention_tile.h's.
//
// What shards change.
//
// Bounds per shard.  lo and hi are monotonic in the row, so an item, a wave and a row each keep ONE pair of global bounds
// (unsigned 32-bit: b * block_tokens <= gq < 2^31 and block_tokens < 2^31, so hi < 2^32).  Opening shard s translates a pair into
// the shard's rows, x -> clamp(x - (key_tok0 + s key_tok_stride), 0, shard_valid), in 64-bit scalar arithmetic (the lane's own
// pair: 64-bit vector arithmetic, once per shard).  A translated interval may be EMPTY (lo == hi): every compare below then fails
// by itself, nothing asks whether a shard lies before or behind a row.
//
// The walk.  Per item and visited shard: the tiles [lo of the item's first row / 64, (hi of its last row - 1) / 64] of the
// translated, clipped interval; an empty interval -- every shard of a later rank under a causal band, every shard behind the
// window -- costs no load and no barrier.  The iterator is wave-uniform scalar state (shard, tile, last tile) and runs one tile
// ahead of the compute ACROSS shard boundaries: what it hands the DMA is (shard, tile).  The compute re-translates the wave's and
// the lane's bounds when the tile it is handed belongs to another shard than the one before (a wave-uniform branch, once per
// shard).
//
// Three classes of (wave, key tile), wave-uniform scalar branches, on the translated bounds:
//   wholly visible    tile within [lo, hi) of the wave's first AND last row: the plain stream, no compare instruction
//   wholly invisible  tile above hi of the last row or below lo of the first: no MFMA, no softmax; the wave still moves its
//                     pieces of the next tile and meets the barrier
//   partial           (unsigned)(key - lo_row) < hi_row - lo_row per element, -inf BEFORE the row maximum.  hi is clipped to
//                     shard_valid, so the tail tile of a shard (shard_valid % 64 != 0) is partial and its padding keys never count.
//
// Softmax state and the -inf hazard: attention_band.hip's rule.  m_ref is always finite (0 until the row's first visible key), a
// row carries `seen`, its O and l are exactly 0 until then, and no expression subtracts two infinities.  Unlike there a row may
// end the launch unseen (another rank's keys are all it may see); the epilogue gives it, per row, the contract of
// attention_sparse_shards.hip:
//   no lse_in        O = exact zeros, lse_out = -inf
//   lse_in           O keeps its value (blended with weight exactly 1 and 0), lse_out = lse_in
// and a row whose lse_in is -inf takes the kernel's own result alone (zeros and -inf if that is empty too).  A workgroup whose
// whole walk is empty does the same without loading anything.
//
// Order: heavy first on the item's visited-tile count SUMMED over the visited shards.  Causal (window 0): lo = 0 and hi never
// falls with the row, so the count never falls with the query tile in any shard: the order is the reverse, no table.  With a
// window every workgroup counts and ranks the query tiles in LDS before its first load, ties to the higher tile (nq * shards
// range computations and nq^2 compares spread over 256 threads).  blockIdx.x = rank * n_heads + head, no xcd_remap below it
// (attention_band.hip says why).  The result does not depend on the order.
// the LDS-DMA asm of attention_tile.h names m0 in its clobber list on purpose (reserved register: the compiler only warns)
#pragma clang diagnostic ignored "-Winline-asm"
#include "attention_tile.h"

namespace mc {

namespace {

constexpr int QT = 128;   // query rows per workgroup (4 waves x 32)
constexpr int STAGE_BYTES = 2 * TILE_BYTES;  // K tile, V tile
constexpr int LDS_BYTES = 2 * STAGE_BYTES;   // 64 KiB: two workgroups per CU
constexpr int MAX_RANKED = LDS_BYTES / 4 - 1;  // query tiles the window form can rank in LDS

struct BandShards {
  int bt, win, q_tok0, q_valid, key_tok0, key_stride;
  int valid, n_shards, skip;   // of AttnParams: shard_valid, n_shards, skip_shard_p1 - 1
  __device__ __forceinline__ int block(int row) const { return (q_tok0 + min(row, q_valid - 1)) / bt; }
  __device__ __forceinline__ uint32_t lo(int b) const { return win ? (uint32_t)max(0, b - win + 1) * (uint32_t)bt : 0u; }
  __device__ __forceinline__ uint32_t hi(int b) const { return ((uint32_t)b + 1u) * (uint32_t)bt; }
  // a global token bound as a row bound of shard s, clipped to the shard's keys
  __device__ __forceinline__ int local(uint32_t g, int s) const {
    const long x = (long)g - ((long)key_tok0 + (long)s * key_stride);
    return (int)min(max(x, 0l), (long)valid);
  }
  // first and last key tile of shard s for rows whose global bounds are [glo, ghi); t1 < t0: none
  __device__ __forceinline__ void tiles(uint32_t glo, uint32_t ghi, int s, int& t0, int& t1) const {
    const int a = local(glo, s), b = local(ghi, s);
    t0 = a / KT;
    t1 = b > a ? (b - 1) / KT : t0 - 1;
  }
  __device__ __forceinline__ int first_shard() const { return skip == 0 ? 1 : 0; }
  __device__ __forceinline__ int next_shard(int s) const { return s + 1 == skip ? s + 2 : s + 1; }
  // visited tiles of the query tile j, summed over the visited shards
  __device__ __forceinline__ int count(int j) const {
    const uint32_t glo = lo(block(j * QT)), ghi = hi(block(j * QT + QT - 1));
    int c = 0;
    for (int s = first_shard(); s < n_shards; s = next_shard(s)) {
      int a, b;
      tiles(glo, ghi, s, a, b);
      c += b - a + 1;
    }
    return c;
  }
};

// the tiles an item visits, shard by shard in ascending order; every member is wave-uniform
struct BandWalk {
  uint32_t glo, ghi;
  int s, t, t1;
  __device__ __forceinline__ void start(const BandShards& bs, uint32_t lo_, uint32_t hi_) {
    glo = lo_; ghi = hi_;
    s = bs.first_shard();
    t = 0; t1 = -1;
    if (s < bs.n_shards) bs.tiles(glo, ghi, s, t, t1);
  }
  // the next visited tile of shard `s` (the member, as it stands on return), -1 when every shard is exhausted
  __device__ __forceinline__ int next(const BandShards& bs) {
    for (;;) {
      if (s >= bs.n_shards) return -1;
      if (t <= t1) return t++;
      s = bs.next_shard(s);
      if (s >= bs.n_shards) return -1;
      bs.tiles(glo, ghi, s, t, t1);
    }
  }
};

__global__ __launch_bounds__(256, 2) void attn_band_shards_kernel(AttnParams p, BandShards bs, int nqt) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = lane >> 5;
  const int l31 = lane & 31;

  // ---- the item: blockIdx.x is the rank in descending visited-tile count (ties: the higher tile first), heads innermost
  const int qrank = blockIdx.x / p.n_heads;
  const int head = blockIdx.x - qrank * p.n_heads;
  int qt = nqt - 1 - qrank;   // causal: the count never falls with the tile index
  if (bs.win != 0) {
    int* cnt = (int*)smem;
    for (int j = tid; j < nqt; j += 256) cnt[j] = bs.count(j);
    __syncthreads();
    for (int j = tid; j < nqt; j += 256) {
      const int cj = cnt[j];
      int before = 0;
      for (int k = 0; k < nqt; ++k) {
        const int ck = cnt[k];
        before += (ck > cj || (ck == cj && k > j)) ? 1 : 0;
      }
      if (before == qrank) cnt[nqt] = j;   // the ranks are a permutation: exactly one thread writes
    }
    __syncthreads();
    qt = cnt[nqt];
    __syncthreads();   // the ring's first load overwrites the table
  }
  qt = min(max(__builtin_amdgcn_readfirstlane(qt), 0), nqt - 1);   // (a permutation by construction; never an address out of range)
  BandWalk walk;
  walk.start(bs, __builtin_amdgcn_readfirstlane(bs.lo(bs.block(qt * QT))), __builtin_amdgcn_readfirstlane(bs.hi(bs.block(qt * QT + QT - 1))));

  const int wrow = qt * QT + wv * 32;
  const int qrow = wrow + l31;
  bf16_t* op = p.O + (size_t)qrow * p.ldo + head * HD + 4 * half;
  const size_t lse_at = (size_t)head * p.Lq_pad + qrow;

  int t_cur = walk.next(bs), s_cur = walk.s, t_next = -1, s_next = 0;
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

  // ---- the global bounds of this wave's first and last row (scalar: the three classes) and of this lane's row (the partial
  // class); their translation into the rows of the shard in hand
  const int w_bf = __builtin_amdgcn_readfirstlane(bs.block(wrow)), w_bl = __builtin_amdgcn_readfirstlane(bs.block(wrow + 31));
  const uint32_t wg_lo_min = bs.lo(w_bf), wg_lo_max = bs.lo(w_bl), wg_hi_min = bs.hi(w_bf), wg_hi_max = bs.hi(w_bl);
  const int r_blk = bs.block(qrow);
  const uint32_t rg_lo = bs.lo(r_blk), rg_hi = bs.hi(r_blk);
  int s_bound = -1, w_lo_min = 0, w_lo_max = 0, w_hi_min = 0, w_hi_max = 0, r_lo = 0;
  unsigned r_span = 0;   // 0: the row sees no key of the shard

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
  bool seen = false;   // has this row met a visible key?  (the same in both halves: mx is the row's)
  f32x16 c_init;       // -m_ref (log2 units, finite) in every register: the accumulator a tile's first MFMA starts from
#pragma unroll
  for (int r = 0; r < 16; ++r) c_init[r] = 0.f;

  auto tile = [&](int s, int t, int stage) __attribute__((always_inline)) {
    if (s != s_bound) {   // (wave-uniform) another shard: translate the bounds into its rows
      s_bound = s;
      w_lo_min = bs.local(wg_lo_min, s); w_lo_max = bs.local(wg_lo_max, s);
      w_hi_min = bs.local(wg_hi_min, s); w_hi_max = bs.local(wg_hi_max, s);
      r_lo = bs.local(rg_lo, s);
      r_span = (unsigned)(bs.local(rg_hi, s) - r_lo);
    }
    const int k0 = t * KT;
    if (k0 >= w_hi_max || k0 + KT <= w_lo_min) return;   // wholly invisible to this wave
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
    if (!(k0 >= w_lo_max && k0 + KT <= w_hi_min)) {   // partial: some row of the wave does not see some key of the tile
      const int rel = k0 + 4 * half - r_lo;           // (key of register 0) - lo of this lane's row
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int kk = (r & 3) + 8 * (r >> 2);
        if ((unsigned)(rel + kk) >= r_span) s0[r] = NEG_INF;
        if ((unsigned)(rel + kk + 32) >= r_span) s1[r] = NEG_INF;
      }
    }
    // ---- reference: first visible key of a row, or a maximum more than 2^RTHR above it (wave-uniform, rare)
    const float mx = rowmax32(s0, s1);
    const bool fresh = mx > NEG_INF;   // this tile holds a visible key of the row
    if (__any(seen ? mx > RTHR : fresh)) {
      // unseen rows: O = l = 0 and stay 0 (factor 0, never exp2 of a large -d); m_ref is finite before and after
      const float d = seen ? fmaxf(mx, 0.f) : (fresh ? mx : 0.f);
      const float alpha = seen ? __builtin_amdgcn_exp2f(-d) : 0.f;
      l_run *= alpha;
#pragma unroll
      for (int i = 0; i < 4; ++i) o[i] = o[i] * alpha;
      s0 = s0 - d;   // -inf stays -inf
      s1 = s1 - d;
      c_init = c_init - d;
      seen = seen || fresh;
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
    t_next = walk.next(bs);
    s_next = walk.s;
    if (t_next >= 0) dma_tile(s_next, t_next, stage ^ 1);
    tile(s_cur, t_cur, stage);
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

  // ---- epilogue: O = O^T / l, the log2-sum-exp m_ref + log2(l), and the merge with what O already holds.  An unseen row has
  // O^T = l = 0 exactly: its factor is 0 (never 1 / 0) and its log-sum-exp -inf
  const float l_tot = half_swap_sum(l_run);
  float inv = seen ? 1.0f / l_tot : 0.f;
  if (p.lse_in || p.lse_out) {   // (uniform)
    float lse = seen ? __builtin_amdgcn_logf(l_tot) - c_init[0] : NEG_INF;   // v_log_f32 is log2
    if (p.lse_in) {
      const float lse_prev = p.lse_in[lse_at];
      const float mm = fmaxf(lse, lse_prev);
      const bool none = mm == NEG_INF;               // neither side holds a key: zeros and -inf
      const float ref = none ? 0.f : mm;             // finite: no weight below is formed from two infinities
      const float wa = __builtin_amdgcn_exp2f(lse_prev - ref), wb = __builtin_amdgcn_exp2f(lse - ref);   // (-inf: 0)
      const float rden = none ? 0.f : 1.0f / (wa + wb);
      // an unseen row hands on what it found, exactly: weight 1 for O_prev, lse_in for the log-sum-exp
      const float ca = seen ? wa * rden : 1.0f, cb = wb * rden * inv;
      lse = none ? NEG_INF : seen ? mm + __builtin_amdgcn_logf(wa + wb) : lse_prev;
      inv = 1.0f;
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

bool attention_band_shards_supports(const AttnParams& p, const AttnBandShards& b) {
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
  if (b.block_tokens < 1 || b.window_blocks < 0 || b.q_valid < 1 || b.q_valid > p.Lq_pad || b.q_tok0 < 0 || b.key_tok0 < 0 ||
      b.key_tok_stride < 0)
    return false;
  // every global token below 2^31: the last valid query row, the last key of the last shard
  if ((long)b.q_tok0 + b.q_valid - 1 >= (1l << 31) || (long)b.key_tok0 + gaps * b.key_tok_stride + p.shard_valid - 1 >= (1l << 31)) return false;
  const size_t nqt = p.Lq_pad / QT;
  return nqt * p.n_heads < (1ull << 31) && (b.window_blocks == 0 || nqt <= (size_t)MAX_RANKED);
}

hipError_t launch_attention_band_shards(const AttnParams& p, const AttnBandShards& b, hipStream_t stream) {
  if (!attention_band_shards_supports(p, b)) return hipErrorInvalidValue;
  const int nqt = p.Lq_pad / QT;
  const BandShards bs = {b.block_tokens, b.window_blocks, b.q_tok0, b.q_valid, b.key_tok0, b.key_tok_stride,
                         p.shard_valid, p.n_shards, p.skip_shard_p1 - 1};
  return launch_dynamic_lds<attn_band_shards_kernel>(dim3(nqt * p.n_heads), dim3(256), LDS_BYTES, stream, p, bs, nqt);
}

}  // namespace mc
