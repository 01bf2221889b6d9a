// Tile-sparse JOINT attention for gfx950 (MM-DiT: text and image rows in one sequence), head_dim 128, bf16 operands, fp32 online
// softmax in base 2.  attention_sparse.hip's bitmap walk with the rule for the joint text rows inside the kernel and inside its
// item order, so that no caller's mask has to know where the text rows sit or that a tile boundary falls among them.
//
// The visibility rule (one definition; repeated verbatim in include/magcache_mmdit.h at mc_op_attention_joint_sparse).  Let
// nqt = Lq_pad / 128, nkt = rows / 64, words = (nkt + 31) / 32.  Two half-open tile ranges are passed by value:
// qdense = [q0, q1) in query tiles and kalways = [k0, k1) in key tiles.  Either may be empty.
//   Query row i of head h sees key j iff j < valid and at least one of these holds:
//   - i / 128 in qdense,
//   - j / 64 in kalways,
//   - bit (j/64) & 31 of word (j/64) >> 5 of mask row [mask_heads == 1 ? 0 : h][i / 128] is set.
// Bits at tiles >= nkt are ignored, and so are bits at tiles whose first key is >= valid.  A query tile that sees no key stores
// O = 0.  All bits set, or qdense covering every tile, is plain attention.
//
// Work split, tile images, Q fragments, fragment reads, the PV step and the O store: attention_sparse.hip's and
// attention_tile.h's -- one workgroup of 4 waves x 32 rows per (128 query rows, head), two workgroups per CU (64 KiB of LDS and
// <= 256 VGPRs each), K/V by LDS-DMA into a ring of two 32 KiB stages, two tile classes (full; the one tail tile with key <
// valid per score before the row maximum), the first visited tile gives the softmax reference, an empty walk stores 0 * 0.
//
// What this kernel adds.
//   The word.  The iterator still walks (current word, word index) with ctz and word &= word - 1, one tile ahead of the
//   compute, but the word it fetches is
//       ((in_qdense ? ~0u : row[i]) | always_word(i)) & (i == last_word ? last_keep : ~0u)
//   always_word(i) = the bits of [k0, k1) that fall into tiles [32 i, 32 i + 32): two clamps and two shifts on scalars, no
//   memory.  A dense query tile never reads the bitmap (its pointer may be null when qdense covers every tile); a row whose
//   words are all zero still visits kalways; the keep mask of the word that holds (valid - 1) / 64 clips both sources alike.
//   The item order.  A dense item costs 1 / density of a typical one, and in HunyuanVideo's row order [image ; text] the dense
//   text query tiles are the LAST block indices: launched in memory order they would run alone as the tail of the launch.  So
//   block b maps to its item by arithmetic, dense items first:
//       b <  (q1 - q0) n_heads:  query tile q0 + b / n_heads
//       otherwise, r = b - (q1 - q0) n_heads, t = r / n_heads:  query tile t < q0 ? t : t + (q1 - q0)
//   heads innermost, no table, no memory.  An optional device table order[nqt * n_heads] of item ids qt * n_heads + head
//   (attention_sparse.hip's contract: trusted but clamped, the result does not depend on it) overrides this when non-null.
// the LDS-DMA asm of attention_tile.h names m0 in its clobber list on purpose (reserved register: the compiler only warns)
#pragma clang diagnostic ignored "-Winline-asm"
#include "attention_tile.h"

namespace mc {

namespace {

constexpr int QT = 128;   // query rows per workgroup (4 waves x 32)
constexpr int STAGE_BYTES = 2 * TILE_BYTES;  // K tile, V tile
constexpr int LDS_BYTES = 2 * STAGE_BYTES;   // 64 KiB: two workgroups per CU

struct JointMask {
  const uint32_t* bits;
  const int32_t* order;
  int mask_heads, nqt, words;
  int q0, q1, k0, k1;
};

// the visible key tiles of one item below tile t_last + 1, in ascending order; every member is wave-uniform
// (the row lives in the constant address space, as in attention_sparse.hip: a uniform address fetched through the scalar cache)
typedef const uint32_t __attribute__((address_space(4))) * MaskRow;
struct JointWalk {
  MaskRow row;
  uint32_t word;
  int wi, last_word, k0, k1;
  uint32_t last_keep;
  bool dense;
  // bits of the key tiles [k0, k1) inside word i
  __device__ __forceinline__ uint32_t always_word(int i) const {
    const int lo = max(k0 - 32 * i, 0), hi = min(k1 - 32 * i, 32);
    if (hi <= lo) return 0u;
    const uint32_t below_hi = hi == 32 ? ~0u : (1u << hi) - 1u;   // lo < hi <= 32: lo <= 31
    return below_hi & ~((1u << lo) - 1u);
  }
  __device__ __forceinline__ uint32_t fetch(int i) const {
    uint32_t w = always_word(i);
    if (dense) w = ~0u;
    else w |= row[i];
    return i == last_word ? w & last_keep : w;
  }
  __device__ __forceinline__ void start(const uint32_t* r, bool in_qdense, int k0_, int k1_, int t_last) {
    row = (MaskRow)(uintptr_t)r;
    dense = in_qdense; k0 = k0_; k1 = k1_;
    last_word = t_last >> 5;
    last_keep = (2u << (t_last & 31)) - 1u;   // bits 0 .. t_last & 31 (bit 31: 2u << 31 wraps to 0, minus one = all)
    wi = 0;
    word = fetch(0);
  }
  // the next visible tile, -1 when the item is exhausted
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

__global__ __launch_bounds__(256, 2) void attn_joint_kernel(AttnParams p, JointMask jm) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = lane >> 5;
  const int l31 = lane & 31;

  // ---- the item: the table, or dense items first by arithmetic
  int qt, head;
  if (jm.order) {
    int item = jm.order[blockIdx.x];
    item = __builtin_amdgcn_readfirstlane(min(max(item, 0), jm.nqt * p.n_heads - 1));
    qt = item / p.n_heads;
    head = item - qt * p.n_heads;
  } else {
    const int nd = jm.q1 - jm.q0;
    const int b = (int)blockIdx.x, r = b - nd * p.n_heads;
    const int t = (r < 0 ? b : r) / p.n_heads;
    head = (r < 0 ? b : r) - t * p.n_heads;
    qt = r < 0 ? jm.q0 + t : (t < jm.q0 ? t : t + nd);
    qt = min(qt, jm.nqt - 1);   // (the launcher's ranges keep it there; an address is never out of range)
  }
  const bool in_qdense = qt >= jm.q0 && qt < jm.q1;
  const int t_last = (p.shard_valid - 1) / KT;
  const int tail = (p.shard_valid % KT) ? t_last : -1;   // the one tile that needs a compare per score
  JointWalk walk;
  walk.start(jm.bits + ((size_t)(jm.mask_heads == 1 ? 0 : head) * jm.nqt + qt) * jm.words, in_qdense, jm.k0, jm.k1, t_last);

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

bool attention_joint_supports(const AttnParams& p, const AttnTileMask& m, const AttnJointRanges& r) {
  if (!attention_shape_ok(p) || !attention_plain_form(p)) return false;
  // a lane's K / V offset inside a tile is 32-bit, and so is every row offset the contract promises
  if ((size_t)p.shard_rows * p.ldk * 2 >= (1ull << 32) || (size_t)p.shard_rows * p.ldv * 2 >= (1ull << 32) ||
      (size_t)p.Lq_pad * p.ldq * 2 >= (1ull << 32) || (size_t)p.Lq_pad * p.ldo * 2 >= (1ull << 32))
    return false;
  const int nqt = p.Lq_pad / QT, nkt = p.shard_rows / KT;
  if (r.q0 < 0 || r.q0 > r.q1 || r.q1 > nqt || r.k0 < 0 || r.k0 > r.k1 || r.k1 > nkt) return false;
  if (!m.bits && !(r.q0 == 0 && r.q1 == nqt)) return false;   // only an all-dense launch never reads the bitmap
  if (((uintptr_t)m.bits & 3) != 0 || ((uintptr_t)m.order & 3) != 0) return false;
  if (m.mask_heads != 1 && m.mask_heads != p.n_heads) return false;
  return (size_t)nqt * p.n_heads < (1ull << 31);
}

hipError_t launch_attention_joint(const AttnParams& p, const AttnTileMask& m, const AttnJointRanges& r, hipStream_t stream) {
  if (!attention_joint_supports(p, m, r)) return hipErrorInvalidValue;
  const int nqt = p.Lq_pad / QT, nkt = p.shard_rows / KT;
  const JointMask jm = {m.bits, m.order, m.mask_heads, nqt, (nkt + 31) / 32, r.q0, r.q1, r.k0, r.k1};
  return launch_dynamic_lds<attn_joint_kernel>(dim3(nqt * p.n_heads), dim3(256), LDS_BYTES, stream, p, jm);
}

}  // namespace mc
