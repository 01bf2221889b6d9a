// Tile-sparse self-attention for gfx950, head_dim 128, bf16 operands, fp32 online softmax in base 2.
//
// The mask (one definition; ops.h: AttnTileMask, include/magcache_hip.h: mc_op_attention_sparse).  Over one key shard of `rows`
// rows of which the first `valid` are keys, with nqt = Lq_pad / 128, nkt = rows / 64, words = (nkt + 31) / 32:
//   uint32 tile_mask[mask_heads][nqt][words] in device memory, mask_heads 1 or n_heads;
//   query row i of head h sees key j iff j < valid and bit (j / 64) & 31 of word (j / 64) >> 5 of row
//   [mask_heads == 1 ? 0 : h][i / 128] is set.
// Bits at key tiles >= nkt and at tiles whose first key is >= valid are ignored.  A query tile that sees no key writes O = 0
// for its 128 rows.  All bits set is plain attention.
//
// Work split.  attention_band.hip's item: one workgroup of 4 waves x 32 rows per (128 query rows, head), two workgroups per CU
// (64 KiB of LDS and <= 256 VGPRs each), K/V by LDS-DMA into a ring of two 32 KiB stages.  Tile images, Q fragments, fragment
// reads, the PV step and the O store are attention_tile.h's.
//
// The walk is compacted -- what this kernel adds.  A workgroup visits the SET BITS of its mask row and nothing else; the
// iteration is wave-uniform scalar arithmetic on (current word, word index):
//   tile = 32 * index + ctz(word),  word &= word - 1;  an exhausted word is replaced by the next one of the row (a scalar load:
//   the row's address is uniform), zero words cost one compare each.
// The word that holds tile t_last = (valid - 1) / 64 is masked when it is fetched so that no bit above t_last survives, and no
// word behind it is ever read: padding bits and bits beyond nkt never reach the walk.  The iterator runs one tile ahead of the
// compute: the LDS-DMA of tile t_next is issued right after the barrier that opens t_cur, as band's ring does with t + 1 -- the
// next word's load, when one is due, hides under the same tile of matrix work.
// Band's "wholly invisible" class does not exist: all 128 rows of an item share one mask row, every wave computes every
// visited tile, so a scattered pattern costs what it visits.
//
// Two classes of tile (a wave-uniform scalar branch):
//   full   no compare instruction
//   tail   the tile that holds valid - 1, when valid % 64 != 0: key < valid per score, -inf BEFORE the row maximum
//
// Softmax.  Every row of an item sees the same tiles and the tail tile holds at least one valid key, so after the FIRST visited
// tile every row has met a key: no `seen` state.  The reference m_ref is the first visited tile's row maximum, whatever its
// sign (O = l = 0 before it: nothing to rescale, and no exp2 of a large -d); afterwards O and l are rescaled only where some
// row's tile maximum exceeds the reference by more than 2^RTHR, as in attention_v3.hip.  An empty walk skips to the store with
// factor 0 on a zero accumulator: no division by l = 0, no expression on two infinities.
//
// Heavy first.  blockIdx.x indexes an optional device table order[nqt * n_heads] of item ids qt * n_heads + head (the engine
// builds it once per mask on the host: descending visited-tile count, ties to the higher tile, heads innermost); null: the
// item id is blockIdx.x.  The table is trusted but clamped -- an address is never out of range -- and an item's result does not
// depend on where it runs, so any order gives the same bits.  No xcd_remap below it, for band's reason: contiguous chunks of a
// sorted list would hand the heaviest eighth to one XCD, while hardware's block b -> XCD b % 8 deals every XCD the same
// descending list with stride 8.
// the LDS-DMA asm of attention_tile.h names m0 in its clobber list on purpose (reserved register: the compiler only warns)
#pragma clang diagnostic ignored "-Winline-asm"
#include "attention_tile.h"

namespace mc {

namespace {

constexpr int QT = 128;   // query rows per workgroup (4 waves x 32)
constexpr int STAGE_BYTES = 2 * TILE_BYTES;  // K tile, V tile
constexpr int LDS_BYTES = 2 * STAGE_BYTES;   // 64 KiB: two workgroups per CU

struct TileMask {
  const uint32_t* bits;
  const int32_t* order;
  int mask_heads, nqt, words;
};

// the set bits of one mask row below tile t_last + 1, in ascending order; every member is wave-uniform
// (the row lives in the constant address space: nothing writes the mask while the kernel runs, and only from there does the
// compiler fetch a uniform address through the scalar cache when LDS-DMA asm with a memory clobber sits in the same loop)
typedef const uint32_t __attribute__((address_space(4))) * MaskRow;
struct Walk {
  MaskRow row;
  uint32_t word;
  int wi, last_word;
  uint32_t last_keep;
  __device__ __forceinline__ uint32_t fetch(int i) const { return i == last_word ? row[i] & last_keep : row[i]; }
  __device__ __forceinline__ void start(const uint32_t* r, int t_last) {
    row = (MaskRow)(uintptr_t)r;
    last_word = t_last >> 5;
    last_keep = (2u << (t_last & 31)) - 1u;   // bits 0 .. t_last & 31 (bit 31: 2u << 31 wraps to 0, minus one = all)
    wi = 0;
    word = fetch(0);
  }
  // the next visible tile, -1 when the row is exhausted
  __device__ __forceinline__ int next() {
    while (word == 0) {
      if (wi >= last_word) return -1;
      word = fetch(++wi);
    }
    const int t = wi * 32 + __builtin_ctz(word);
    word &= word - 1;
    return t;
  }
};

__global__ __launch_bounds__(256, 2) void attn_sparse_kernel(AttnParams p, TileMask tm) {
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
  const int t_last = (p.shard_valid - 1) / KT;
  const int tail = (p.shard_valid % KT) ? t_last : -1;   // the one tile that needs a compare per score
  Walk walk;
  walk.start(tm.bits + ((size_t)(tm.mask_heads == 1 ? 0 : head) * tm.nqt + qt) * tm.words, t_last);

  const int qrow = qt * QT + wv * 32 + l31;
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
      const int key0 = t * KT + 4 * half;   // key of register 0
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
  // one ring step: tile t_cur has landed in `stage` for every wave and the other stage is free (every wave is past the tile
  // before it); the iterator moves on behind the barrier, one tile ahead of the compute
  int t_cur = walk.next(), t_next = -1;
  auto step = [&](int stage) __attribute__((always_inline)) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    t_next = walk.next();
    if (t_next >= 0) dma_tile(t_next, stage ^ 1);
    tile(t_cur, stage);
    t_cur = t_next;
  };

  const bool empty = t_cur < 0;
  if (!empty) {
    dma_tile(t_cur, 0);
    for (;;) {   // stages as compile-time constants
      step(0);
      if (t_cur < 0) break;
      step(1);
      if (t_cur < 0) break;
    }
  }

  // ---- epilogue: O = O^T / l; an empty walk stores 0 * 0
  const float inv = empty ? 0.f : 1.0f / half_swap_sum(l_run);
  bf16_t* op = p.O + (size_t)qrow * p.ldo + head * HD + 4 * half;
  MC_ATTN_STORE_O(op, o, inv)
}

}  // namespace

bool attention_sparse_supports(const AttnParams& p, const AttnTileMask& m) {
  if (!attention_shape_ok(p) || !attention_plain_form(p)) return false;
  // a lane's K / V offset inside a tile is 32-bit, and so is every row offset the contract promises
  if ((size_t)p.shard_rows * p.ldk * 2 >= (1ull << 32) || (size_t)p.shard_rows * p.ldv * 2 >= (1ull << 32) ||
      (size_t)p.Lq_pad * p.ldq * 2 >= (1ull << 32) || (size_t)p.Lq_pad * p.ldo * 2 >= (1ull << 32))
    return false;
  if (!m.bits || ((uintptr_t)m.bits & 3) != 0 || ((uintptr_t)m.order & 3) != 0) return false;
  if (m.mask_heads != 1 && m.mask_heads != p.n_heads) return false;
  return (size_t)(p.Lq_pad / QT) * p.n_heads < (1ull << 31);
}

hipError_t launch_attention_sparse(const AttnParams& p, const AttnTileMask& m, hipStream_t stream) {
  if (!attention_sparse_supports(p, m)) return hipErrorInvalidValue;
  const int nqt = p.Lq_pad / QT, nkt = p.shard_rows / KT;
  const TileMask tm = {m.bits, m.order, m.mask_heads, nqt, (nkt + 31) / 32};
  return launch_dynamic_lds<attn_sparse_kernel>(dim3(nqt * p.n_heads), dim3(256), LDS_BYTES, stream, p, tm);
}

}  // namespace mc
