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
// Data movement.  Q: 8 fragments in registers for the launch.  K/V: LDS-DMA (global_load_lds_dwordx4, the technique and the
// bank swizzles of attention_v3.hip) into a ring of two 32 KiB stages; tile t + 1 is issued right after the barrier that opens
// tile t and waited for (vmcnt(0)) before the next barrier: one barrier per tile, a whole tile of matrix work over the latency.
// O: O^T accumulators scaled by 1 / l, 8-byte stores, as v3.
// the LDS-DMA asm below names m0 in its clobber list on purpose (reserved register: the compiler only warns)
#pragma clang diagnostic ignored "-Winline-asm"
#include "common.h"
#include "ops.h"

namespace mc {

namespace {

constexpr int QT = 128;   // query rows per workgroup (4 waves x 32)
constexpr int KT = 64;    // keys per tile
constexpr int HD = 128;   // head dim
constexpr int TILE_BYTES = KT * HD * 2;      // 16 KiB: one operand's tile
constexpr int STAGE_BYTES = 2 * TILE_BYTES;  // K tile, V tile
constexpr int LDS_BYTES = 2 * STAGE_BYTES;   // 64 KiB: two workgroups per CU
constexpr int MAX_RANKED = LDS_BYTES / 4 - 1;  // query tiles the window form can rank in LDS
constexpr float NEG_INF = -__builtin_huge_valf();
constexpr float RTHR = 4.0f;  // rescale threshold in log2 units: P <= 2^4

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

__device__ __forceinline__ float max3(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }

// row maximum over a lane's 32 scores and the other half's
__device__ __forceinline__ float rowmax32(const f32x16& a, const f32x16& b) {
  float m0 = max3(a[0], a[1], a[2]), m1 = max3(a[3], a[4], a[5]);
  float m2 = max3(a[6], a[7], a[8]), m3 = max3(a[9], a[10], a[11]);
  m0 = max3(m0, a[12], a[13]); m1 = max3(m1, a[14], a[15]);
  m2 = max3(m2, b[0], b[1]);   m3 = max3(m3, b[2], b[3]);
  m0 = max3(m0, b[4], b[5]);   m1 = max3(m1, b[6], b[7]);
  m2 = max3(m2, b[8], b[9]);   m3 = max3(m3, b[10], b[11]);
  m0 = max3(m0, b[12], b[13]); m1 = max3(m1, b[14], b[15]);
  return half_swap_max(fmaxf(fmaxf(m0, m1), fmaxf(m2, m3)));
}

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

  // ---- Q fragments (B operand of the S^T MFMA): lane -> query row l31, d = ds*16 + 8*half + 0..7, times scale * log2(e)
  const float c = p.scale * 1.4426950408889634f;
  bf16x8 qf[8];
  {
    const bf16_t* qp = p.Q + (size_t)qrow * p.ldq + head * HD + 8 * half;
#pragma unroll
    for (int ds = 0; ds < 8; ++ds) {
      const bf16x8 raw = *(const bf16x8*)(qp + ds * 16);
#pragma unroll
      for (int i = 0; i < 8; ++i) qf[ds][i] = (__bf16)((float)raw[i] * c);
    }
  }

  // ---- LDS-DMA: 16 pieces of 1 KiB per operand tile, 4 per wave.  piece g = rows 4g..4g+3, lane -> (row = 4g + lane/16,
  // slot = lane%16); the 16-byte source chunk of a slot is K: slot ^ (row&15), V: slot ^ ((row&3)<<2) (v3's swizzles)
  uint32_t srcK[4], srcV[4];  // byte offsets from the tile's first row
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int row = (wv * 4 + j) * 4 + (lane >> 4);
    const int slot = lane & 15;
    srcK[j] = (uint32_t)(row * (int)p.ldk + head * HD + (slot ^ (row & 15)) * 8) * 2u;
    srcV[j] = (uint32_t)(row * (int)p.ldv + head * HD + (slot ^ ((row & 3) << 2)) * 8) * 2u;
  }
  const uint32_t dma_lds = (uint32_t)(uintptr_t)MC_LDS_PTR(smem) + wv * 4096;  // this wave's 4 pieces inside a tile image
  // one 1 KiB piece.  saddr form: uniform 64-bit base + 32-bit lane offset; M0 = LDS byte address of the piece; s_nop covers
  // the SALU-write-M0 -> LDS-DMA hazard
  auto dma1 = [&](const bf16_t* base, uint32_t off, uint32_t lds) {
    asm volatile(
        "s_mov_b32 m0, %1\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %0, %2"
        :
        : "v"(off), "s"(lds), "s"(base)
        : "memory", "m0");
  };
  auto dma_tile = [&](int t, int stage) {
    const bf16_t* kp = p.K + (size_t)t * KT * p.ldk;
    const bf16_t* vp = p.V + (size_t)t * KT * p.ldv;
    const uint32_t dst = dma_lds + stage * STAGE_BYTES;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      dma1(kp, srcK[j], dst + j * 1024);
      dma1(vp, srcV[j], dst + TILE_BYTES + j * 1024);
    }
  };

  // ---- K fragment read: row = kb*32 + l31, chunk (2*ds + half) ^ (row & 15), row&15 == lane&15
  int koff[8];
#pragma unroll
  for (int ds = 0; ds < 8; ++ds) koff[ds] = l31 * 256 + (((2 * ds + half) ^ (lane & 15)) << 4);
  // ---- V^T fragment (transposing read): key = ks*16 + 4*half + r (+8 for the second read), r = (lane&15)>>2;
  //   d = db*32 + dg*16 + 4*c, dg = (lane>>4)&1, c = lane&3; 64-B chunk (= db) ^= (key&3) = r
  const int vr = (lane & 15) >> 2;
  const int vbase = TILE_BYTES + (4 * half + vr) * 256 + ((lane >> 4) & 1) * 32 + (lane & 3) * 8;
  int voff[4];
#pragma unroll
  for (int db = 0; db < 4; ++db) voff[db] = vbase + ((db ^ vr) << 6);

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
    // ---- P = exp2(S): registers 2j, 2j+1 of key block kb -> the packed pair 8*kb + j, word j%4 of the B operand of key
    // step ks = 2*kb + j/4 (the accumulator layout of S^T IS that operand: both products agree on the key order)
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
    for (int i = 0; i < 16; ++i) {
      const char* vp = st + voff[i & 3] + (i >> 2) * (16 * 256);
      const bf16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4*)(vp));
      const bf16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4*)(vp + 8 * 256));
      const bf16x8 vf = __builtin_shufflevector(v0, v1, 0, 1, 2, 3, 4, 5, 6, 7);
      const int ks = i >> 2;
      const u32x4 pw = {pk[4 * ks], pk[4 * ks + 1], pk[4 * ks + 2], pk[4 * ks + 3]};
      o[i & 3] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, __builtin_bit_cast(bf16x8, pw), o[i & 3], 0, 0, 0);
    }
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

  // ---- epilogue: O[q][d] = O^T[d][q] / l ; lane holds d = db*32 + 8*g + 4*half + 0..3.  Every row has seen its own block: l > 0
  const float inv = 1.0f / half_swap_sum(l_run);
  bf16_t* op = p.O + (size_t)qrow * p.ldo + head * HD + 4 * half;
#pragma unroll
  for (int db = 0; db < 4; ++db) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      u32x2 w = {pack_bf16x2(o[db][4 * g] * inv, o[db][4 * g + 1] * inv),
                 pack_bf16x2(o[db][4 * g + 2] * inv, o[db][4 * g + 3] * inv)};
      *(u32x2*)(op + db * 32 + 8 * g) = w;
    }
  }
}

}  // namespace

bool attention_band_supports(const AttnParams& p, const AttnBand& b) {
  auto al16 = [](const void* q) { return q && ((uintptr_t)q & 15) == 0; };
  if (p.n_shards != 1 || p.skip_shard_p1 != 0 || p.lse_in || p.lse_out) return false;
  if (p.Lq_pad <= 0 || (p.Lq_pad % 256) != 0 || p.shard_rows <= 0 || (p.shard_rows % KT) != 0 || p.shard_valid < 1 ||
      p.shard_valid > p.shard_rows || p.n_heads <= 0)
    return false;
  if (b.block_tokens < 1 || b.window_blocks < 0) return false;
  if ((p.ldq % 8) || (p.ldk % 8) || (p.ldv % 8) || (p.ldo % 8)) return false;
  const size_t d = (size_t)p.n_heads * HD;
  if ((size_t)p.ldq < d || (size_t)p.ldk < d || (size_t)p.ldv < d || (size_t)p.ldo < d) return false;
  // a lane's K / V offset inside a tile is 32-bit, and so is every row offset the contract promises
  if ((size_t)p.shard_rows * p.ldk * 2 >= (1ull << 32) || (size_t)p.shard_rows * p.ldv * 2 >= (1ull << 32) ||
      (size_t)p.Lq_pad * p.ldq * 2 >= (1ull << 32) || (size_t)p.Lq_pad * p.ldo * 2 >= (1ull << 32))
    return false;
  const size_t nqt = p.Lq_pad / QT;
  if (nqt * p.n_heads >= (1ull << 31) || (b.window_blocks != 0 && nqt > (size_t)MAX_RANKED)) return false;
  return al16(p.Q) && al16(p.K) && al16(p.V) && al16(p.O);
}

hipError_t launch_attention_band(const AttnParams& p, const AttnBand& b, hipStream_t stream) {
  if (!attention_band_supports(p, b)) return hipErrorInvalidValue;
  const int nqt = p.Lq_pad / QT;
  const Band band = {b.block_tokens, b.window_blocks, p.shard_valid};
  return launch_dynamic_lds<attn_band_kernel>(dim3(nqt * p.n_heads), dim3(256), LDS_BYTES, stream, p, band, nqt);
}

}  // namespace mc
