// Frame-block causal / windowed self-attention for gfx950, head_dim 128, bf16 operands, fp32 online softmax in base 2.
//
// The band (one definition; ops.h: AttnBand, include/magcache_hip.h: mc_op_attention_band).  Over one key shard of `valid` keys,
// query row i belongs to block b = min(i, valid - 1) / block_tokens and sees the keys lo(b) <= j < hi(b),
//   hi(b) = min((b + 1) block_tokens, valid),   lo(b) = window_blocks ? max(0, b - window_blocks + 1) block_tokens : 0.
// Every row sees at least its own block; padding rows (i >= valid) are rows of the last valid block; block_tokens >= valid is
// plain attention.  No mask exists in memory: every bound below is arithmetic on the two parameters.
//
// Work split.  One workgroup of 4 waves per (128 query rows, head), TWO workgroups per CU (64 KiB of LDS and <= 256 VGPRs each).
// A wave owns 32 query rows.  A workgroup walks only the 64-key tiles first .. last of the union of its rows' intervals.
//   * 128 rows, not attention_v3's 256: an item's K/V walk is as long as its LAST row needs, so the rows above it pay for
//     tiles they cannot see; halving the height halves that triangle (and the partial tiles at a block edge) and doubles the
//     number of items the heavy-first order has to balance with.  It re-reads K/V twice as often -- from L2, where the items
//     that run side by side on an XCD are neighbours in the same head (below).
//   * the two co-resident workgroups replace v3's in-wave software pipeline: with three classes of tile the instruction
//     stream of a tile is not fixed, so nothing can be pinned between MFMAs by hand; instead one workgroup's softmax (VALU)
//     runs beside the other's MFMAs on the same SIMD, and their barriers do not meet.
//   * heavy first: blockIdx.x = rank in DESCENDING key-tile count, rank = q_rank * n_heads + head.  Hardware hands block b
//     to XCD b % 8, so every XCD walks the same descending list with stride 8: its share of the work is the same to within
//     one item per level, the tail of the launch is made of the shortest items on every XCD, and an XCD sees the heads
//     congruent to it modulo gcd(8, n_heads) only (3 of 12, 5 of 40).  xcd_remap (contiguous chunks of the virtual order per
//     XCD) would hand the heaviest eighth of a triangular list to ONE XCD -- that is why it is not applied here; the locality it
//     exists for comes from the head residue.  Causal (window 0): the count grows with the tile index, the order is the
//     reverse.  With a window the count is not monotonic (a tile that straddles a block edge sees one block more): every
//     workgroup ranks the query tiles in LDS before its first load (nq^2 / 256 compares per thread, ~1 us at nq = 256).
//
// Three classes of (wave, key tile), wave-uniform scalar branches:
//   wholly visible    tile within [lo, hi) of the wave's first AND last row: the plain stream, no compare instruction
//   wholly invisible  tile above hi of the last row or below lo of the first: no MFMA, no softmax; the wave still moves its
//                     pieces of the next tile and meets the barrier
//   partial           (unsigned)(key - lo_row) < hi_row - lo_row per element, -inf BEFORE the row maximum: a masked score
//                     enters neither the maximum, nor the row sum, nor P
//
// Softmax state and the -inf hazard.  As in v3 the scores leave the MFMA relative to a per-row reference m_ref (the accumulator
// starts at -m_ref, q carries scale * log2 e), P = exp2(S) directly, and O, l are rescaled only when some row's tile maximum
// exceeds the reference by more than 2^RTHR.  v3 takes its reference from tile 0; here a row may have seen NO key in the tiles
// visited so far (a window's lower edge, two blocks in one wave), so:
//   * m_ref is always FINITE (0 until the row's first visible key): no expression subtracts two infinities;
//   * a row carries `seen`.  Unseen, its O and l are exactly 0 (P = exp2(-inf) = 0); its first finite tile maximum mx becomes
//     the reference whatever its sign (d = mx), with the rescale factor forced to 0 instead of exp2(-d), which may overflow
//     to +inf and make 0 * inf;
//   * a tile whose maximum is -inf for an unseen row moves nothing (d = 0) and contributes P = 0.
//
// Data movement.  Q fragments, tile images, fragment reads, the PV step and the O store are attention_tile.h's, shared with
// attention_v3.hip.  K/V: LDS-DMA into a ring of two 32 KiB stages (a K image, the V image behind it); tile t + 1 is issued
// right after the barrier that opens tile t and waited for (vmcnt(0)) before the next barrier: one barrier per tile, a whole
// tile of matrix work over the latency.
// the LDS-DMA asm of attention_tile.h names m0 in its clobber list on purpose (reserved register: the compiler only warns)
#pragma clang diagnostic ignored "-Winline-asm"
#include "attention_tile.h"

namespace mc {

namespace {

constexpr int QT = 128;   // query rows per workgroup (4 waves x 32)
constexpr int STAGE_BYTES = 2 * TILE_BYTES;  // K tile, V tile
constexpr int LDS_BYTES = 2 * STAGE_BYTES;   // 64 KiB: two workgroups per CU
constexpr int MAX_RANKED = LDS_BYTES / 4 - 1;  // query tiles the window form can rank in LDS

struct Band {
  int bt, win, valid;
  __device__ __forceinline__ int block(int row) const { return min(row, valid - 1) / bt; }
  __device__ __forceinline__ int lo(int b) const { return win ? max(0, b - win + 1) * bt : 0; }   // <= b * bt < valid
  __device__ __forceinline__ int hi(int b) const { return (int)min((long)(b + 1) * bt, (long)valid); }
  // first and last key tile of the rows [row0, row0 + n)
  __device__ __forceinline__ void tiles(int row0, int n, int& t0, int& t1) const {
    t0 = lo(block(row0)) / KT;
    t1 = (hi(block(row0 + n - 1)) - 1) / KT;
  }
};

__global__ __launch_bounds__(256, 2) void attn_band_kernel(AttnParams p, Band band, int nqt) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = lane >> 5;
  const int l31 = lane & 31;

  // ---- the item: blockIdx.x is the rank in descending key-tile count (ties: the higher tile first), heads innermost
  const int qrank = blockIdx.x / p.n_heads;
  const int head = blockIdx.x - qrank * p.n_heads;
  int qt = nqt - 1 - qrank;   // causal: the count never falls with the tile index
  if (band.win != 0) {
    int* cnt = (int*)smem;
    for (int j = tid; j < nqt; j += 256) {
      int a, b;
      band.tiles(j * QT, QT, a, b);
      cnt[j] = b - a;
    }
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
  int t0, t1;
  band.tiles(qt * QT, QT, t0, t1);
  t0 = __builtin_amdgcn_readfirstlane(t0);
  t1 = __builtin_amdgcn_readfirstlane(t1);

  // ---- the bounds of this wave's rows (scalar: the three classes) and of this lane's row (the partial class)
  const int wrow = qt * QT + wv * 32;
  const int w_bf = band.block(wrow), w_bl = band.block(wrow + 31);
  const int w_lo_min = band.lo(w_bf), w_lo_max = band.lo(w_bl), w_hi_min = band.hi(w_bf), w_hi_max = band.hi(w_bl);
  const int qrow = wrow + l31;
  const int r_blk = band.block(qrow);
  const int r_lo = band.lo(r_blk);
  const unsigned r_span = (unsigned)(band.hi(r_blk) - r_lo);   // >= 1

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
  auto dma_tile = [&](int t, int stage) {
    const bf16_t* kp = p.K + (size_t)t * KT * p.ldk;
    const bf16_t* vp = p.V + (size_t)t * KT * p.ldv;
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
  float m_ref = 0.f, l_run = 0.f;   // the reference (log2 units, finite) and this lane's share of the row sum
  bool seen = false;                // has this row met a visible key?  (the same in both halves: mx is the row's)
  f32x16 c_init;                    // -m_ref in every register: the accumulator a tile's first MFMA starts from
#pragma unroll
  for (int r = 0; r < 16; ++r) c_init[r] = 0.f;

  auto tile = [&](int t, int stage) __attribute__((always_inline)) {
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
      m_ref += d;
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
  // one ring step: tile t has landed in `stage` for every wave and the other stage is free (every wave is past tile t - 1)
  auto step = [&](int t, int stage) __attribute__((always_inline)) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (t < t1) dma_tile(t + 1, stage ^ 1);
    tile(t, stage);
  };

  dma_tile(t0, 0);
  for (int t = t0; t <= t1; t += 2) {   // stages as compile-time constants
    step(t, 0);
    if (t < t1) step(t + 1, 1);
  }

  // ---- epilogue: O = O^T / l.  Every row has seen its own block: l > 0
  const float inv = 1.0f / half_swap_sum(l_run);
  bf16_t* op = p.O + (size_t)qrow * p.ldo + head * HD + 4 * half;
  MC_ATTN_STORE_O(op, o, inv)
}

}  // namespace

bool attention_band_supports(const AttnParams& p, const AttnBand& b) {
  if (!attention_shape_ok(p) || !attention_plain_form(p) || b.block_tokens < 1 || b.window_blocks < 0) return false;
  // a lane's K / V offset inside a tile is 32-bit, and so is every row offset the contract promises
  if ((size_t)p.shard_rows * p.ldk * 2 >= (1ull << 32) || (size_t)p.shard_rows * p.ldv * 2 >= (1ull << 32) ||
      (size_t)p.Lq_pad * p.ldq * 2 >= (1ull << 32) || (size_t)p.Lq_pad * p.ldo * 2 >= (1ull << 32))
    return false;
  const size_t nqt = p.Lq_pad / QT;
  return nqt * p.n_heads < (1ull << 31) && (b.window_blocks == 0 || nqt <= (size_t)MAX_RANKED);
}

hipError_t launch_attention_band(const AttnParams& p, const AttnBand& b, hipStream_t stream) {
  if (!attention_band_supports(p, b)) return hipErrorInvalidValue;
  const int nqt = p.Lq_pad / QT;
  const Band band = {b.block_tokens, b.window_blocks, p.shard_valid};
  return launch_dynamic_lds<attn_band_kernel>(dim3(nqt * p.n_heads), dim3(256), LDS_BYTES, stream, p, band, nqt);
}

}  // namespace mc
