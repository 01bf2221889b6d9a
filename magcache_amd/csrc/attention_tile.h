// The bf16 tile geometry attention_v3.hip and attention_band.hip share: head_dim 128, 64-key K / V tiles as swizzled LDS images
// filled by LDS-DMA, 32 query rows per wave on v_mfma_f32_32x32x16_bf16.  Each kernel keeps its own ring, schedule and softmax
// state; what one tile looks like in LDS and in registers is stated here, once.  (attention_mx8.hip has another MFMA shape and
// other images: quant.h.)
//
// A tile image is 64 rows (keys) x 256 bytes = 16 chunks of 16 bytes per row, 16 KiB.  It is written as 16 pieces of 1 KiB (rows
// 4g .. 4g + 3), one global_load_lds_dwordx4 each: lane -> (row = 4g + lane / 16, slot = lane % 16), and slot s of a row receives
// the row's SOURCE chunk
//     K:  s ^ (row & 15)            V:  s ^ ((row & 3) << 2)
// so that the fragment reads below are free of bank conflicts.  THE SWIZZLE PAIR: piece_src_offsets (the source side) and
// frag_offsets (the read side) are the two halves of these formulas and must change together -- a chunk c of a row lives in slot
// c ^ (row & 15) (K), c ^ ((row & 3) << 2) (V), whichever side asks.
#pragma once
#include "common.h"
#include "ops.h"

namespace mc {

constexpr int KT = 64;    // keys per tile
constexpr int HD = 128;   // head dim
constexpr int TILE_BYTES = KT * HD * 2;  // 16 KiB: one operand's tile image
constexpr float NEG_INF = -__builtin_huge_valf();
constexpr float RTHR = 4.0f;  // rescale threshold in log2 units: P <= 2^4

__device__ __forceinline__ float max3(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }

// row maximum over a lane's 32 scores (two S^T accumulators) and the other lane half's
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

// Q fragments (B operand of the S^T = K Q^T MFMA): lane -> query row qrow (l31 of the wave's 32), d = ds*16 + 8*half + 0..7.
// Q is pre-multiplied by c = scale * log2(e) (one extra bf16 rounding of q, 2^-9 relative: below the rounding q and k already
// carry), so the MFMA delivers scores in log2 units and, with the accumulator initialised to minus the softmax reference,
// P = exp2(S) needs no multiply-add per element.  qf: bf16x8[8].  (A macro for the reason given at MC_ATTN_K_SRC_CHUNK.)
#define MC_ATTN_LOAD_Q(p, qrow, head, half, qf)                                               \
  {                                                                                           \
    const float c_ = (p).scale * 1.4426950408889634f;                                         \
    const bf16_t* qp_ = (p).Q + (size_t)(qrow) * (p).ldq + (head) * HD + 8 * (half);          \
    _Pragma("unroll") for (int ds_ = 0; ds_ < 8; ++ds_) {                                     \
      const bf16x8 raw_ = *(const bf16x8*)(qp_ + ds_ * 16);                                   \
      _Pragma("unroll") for (int i_ = 0; i_ < 8; ++i_) qf[ds_][i_] = (__bf16)((float)raw_[i_] * c_); \
    }                                                                                         \
  }

// One 1 KiB piece by LDS-DMA (inline asm so hipcc's waitcnt pass does not serialise ds_reads behind it; the including file
// silences -Winline-asm: m0 is a reserved register and the compiler only warns).  saddr form: uniform 64-bit base + 32-bit
// lane offset; M0 = LDS byte address of the piece; s_nop covers the SALU-write-M0 -> LDS-DMA hazard.
__device__ __forceinline__ void dma_piece(const bf16_t* base, uint32_t off, uint32_t lds) {
  asm volatile(
      "s_mov_b32 m0, %1\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %0, %2"
      :
      : "v"(off), "s"(lds), "s"(base)
      : "memory", "m0");
}

// SOURCE side of the swizzle pair: the source chunk that slot `slot` of row `row` of an image receives.  A wave that moves N
// pieces per operand tile (8 waves x 2 in v3, 4 waves x 4 in band) moves pieces wv * N .. wv * N + N - 1; the byte offset of its
// lane's chunk from the tile's first row (head 0, column 0) is MC_ATTN_PIECE_SRC of that.
// These, the fragment offsets, the Q load and the O store are macros, not functions: behind a call (even a __forceinline__ one,
// even one that returns slot ^ (row & 15)) the compiler folds the index arithmetic in another order and allocates a kernel's
// registers differently; the macros leave both instruction streams as they were (tools/isa_same.py), like MC_GROUPED_TILE of
// common.h.  The N-piece loop around them stays in each kernel: v3 names the two chunks before it forms the offsets, band
// does not, and either text changes the other kernel's registers (DESIGN.md has what isa_same printed).
#define MC_ATTN_K_SRC_CHUNK(slot, row) ((slot) ^ ((row) & 15))
#define MC_ATTN_V_SRC_CHUNK(slot, row) ((slot) ^ (((row) & 3) << 2))
#define MC_ATTN_PIECE_SRC(row, ld, head, chunk) ((uint32_t)((row) * (int)(ld) + (head) * HD + (chunk) * 8) * 2u)

//
// READ side of the swizzle pair: byte offsets of this lane's fragments (half = lane >> 5, l31 = lane & 31), koff[8] from a K
// image, voff[4] from the same base with the V image v_image bytes behind that K image.
//   K fragment of d-step ds (A operand of S^T): row = kb*32 + l31 (kb: + 32 * 256 bytes), chunk 2*ds + half, in slot
//     (2*ds + half) ^ (row & 15), row & 15 == lane & 15
//   V^T fragment of micro-step i = 4*ks + db (read_vt at voff[db] + ks * 16 * 256): key = ks*16 + 4*half + r (+8 for the second
//     read), r = (lane&15)>>2; d = db*32 + dg*16 + 4*c, dg = (lane>>4)&1, c = lane&3; the 64-byte group db sits at db ^ r:
//     chunk 4*db + .. in slot (4*db + ..) ^ ((key & 3) << 2), key & 3 == r
#define MC_ATTN_FRAG_OFFSETS(lane, half, l31, v_image, koff, voff)                                               \
  {                                                                                                              \
    _Pragma("unroll") for (int ds_ = 0; ds_ < 8; ++ds_)                                                          \
      koff[ds_] = (l31) * 256 + (((2 * ds_ + (half)) ^ ((lane) & 15)) << 4);                                     \
    const int vr_ = ((lane) & 15) >> 2;                                                                          \
    const int vbase_ = (v_image) + (4 * (half) + vr_) * 256 + (((lane) >> 4) & 1) * 32 + ((lane) & 3) * 8;       \
    _Pragma("unroll") for (int db_ = 0; db_ < 4; ++db_) voff[db_] = vbase_ + ((db_ ^ vr_) << 6);                 \
  }

// the V^T fragment at vp: two transposing reads, keys .. and .. + 8
__device__ __forceinline__ bf16x8 read_vt(const char* vp) {
  const bf16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4*)(vp));
  const bf16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4*)(vp + 8 * 256));
  return __builtin_shufflevector(v0, v1, 0, 1, 2, 3, 4, 5, 6, 7);
}

// PV micro-step i = 4*ks + db: O^T[db] += V^T fragment x P^T.  pk[8*kb + j] is the packed bf16 pair exp2(S[kb][2j]),
// exp2(S[kb][2j+1]); words 4*ks .. 4*ks + 3 are the B operand of key step ks = 2*kb + j/4 (the accumulator layout of S^T IS
// that operand: an MFMA's contraction index may be permuted if both operands agree on the key order)
__device__ __forceinline__ void pv_step(f32x16 (&o)[4], int i, const bf16x8& vf, const uint32_t (&pk)[16]) {
  const int ks = i >> 2;
  const u32x4 pw = {pk[4 * ks], pk[4 * ks + 1], pk[4 * ks + 2], pk[4 * ks + 3]};
  o[i & 3] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, __builtin_bit_cast(bf16x8, pw), o[i & 3], 0, 0, 0);
}

// epilogue: O[q][d] = O^T[d][q] * inv, 8-byte stores; op = the row's head columns + 4*half: the lane holds
// d = db*32 + 8*g + 4*half + 0..3 in o[db][4g .. 4g + 3].  o: f32x16[4]
#define MC_ATTN_STORE_O(op, o, inv)                                                              \
  _Pragma("unroll") for (int db_ = 0; db_ < 4; ++db_) {                                          \
    _Pragma("unroll") for (int g_ = 0; g_ < 4; ++g_) {                                           \
      u32x2 w_ = {pack_bf16x2(o[db_][4 * g_] * (inv), o[db_][4 * g_ + 1] * (inv)),               \
                  pack_bf16x2(o[db_][4 * g_ + 2] * (inv), o[db_][4 * g_ + 3] * (inv))};          \
      *(u32x2*)((op) + db_ * 32 + 8 * g_) = w_;                                                  \
    }                                                                                            \
  }

}  // namespace mc
