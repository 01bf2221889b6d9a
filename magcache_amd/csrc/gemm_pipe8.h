// The shared skeleton of the 8-wave 256x256 LDS-DMA GEMMs: gemm_bf16_big.hip (bf16, the test-only reference kernel),
// gemm_fp8_big.hip (per-row-scaled fp8), gemm_mxfp8.hip (MX fp8) and gemm_mxfp4.hip (MXFP4).  What they have in common lives here once; the
// interval schedules, wait counts, fragment structs, MFMAs and epilogues differ and stay with each kernel.
//
// Geometry
//   * workgroup = 8 waves (2 along M x 4 along N), one 256x256 output tile; wave tile 128(M) x 64(N).
//   * a K tile is 128 BYTES of every row (64 bf16, 128 fp8 or 256 fp4), and each operand's K tile is split into two 16 KiB
//     "halves" by WHEN a wave needs them:
//        Am0 / Am1 : for each wave row wr, rows wr*128 + [0,64) / [64,128) of the A tile
//        Wn0 / Wn1 : for each wave col wc, rows wc*64  + [0,32) / [32,64)  of the W tile
//     LDS = 2 stages x 4 halves x 16 KiB.  Each half is 16 pieces of 1 KiB (8 rows x 128 B); a wave moves 2 pieces per
//     half with global_load_lds_dwordx4 (HBM/L2 -> LDS, no VGPR round trip).
//   * LDS rows are 128 B; the image is XOR-swizzled, chunk' = chunk ^ ((row >> 1) & 7), applied to the SOURCE address
//     (LDS-DMA writes lane-linear) and to the ds_read_b128 address.
// The pipeline itself (four intervals per K tile, counted vmcnt waits) is described in gemm_bf16_big.hip.
#pragma once
#include "common.h"

namespace mc {
namespace pipe8 {

constexpr int TB = 256;                      // tile edge (M and N)
constexpr int ROW_BYTES = 128;               // bytes of K per row of a K tile
constexpr int HALF_BYTES = 128 * ROW_BYTES;  // 16 KiB
constexpr int STAGE_BYTES = 4 * HALF_BYTES;  // Am0 | Am1 | Wn0 | Wn1
constexpr int OFF_AM0 = 0, OFF_AM1 = HALF_BYTES, OFF_WN0 = 2 * HALF_BYTES, OFF_WN1 = 3 * HALF_BYTES;

// tile rasterisation (MC_GROUPED_TILE, common.h): group_m M-tiles x all N-tiles per group.  Measured (kbench, M = 32768): 8 for
// N = 4608 (QKV: 1176 vs 1168 TF), 4 for N = 8960 (FFN-1: 1138 vs 1096 TF), no difference for N = 1536.
#define MC_GROUP_M_OF(tilesN) ((tilesN) >= 32 ? 4 : 8)

// end-of-interval wait: at most n LDS-DMA instructions of this wave still in flight.  (ds_reads need
// no wait here: a region is re-filled two barriers after its last read, and every read has been
// consumed by an MFMA -- i.e. waited for -- one barrier earlier.)
#define MC_WAIT_(n) asm volatile("s_waitcnt vmcnt(" #n ")" ::: "memory")
// interval boundary: nothing (MFMAs included -- they are register-only and would otherwise drift
// across the asm statements) is scheduled across it
#define MC_BARRIER()                              \
  do {                                            \
    asm volatile("s_barrier" ::: "memory");       \
    __builtin_amdgcn_sched_barrier(0);            \
  } while (0)
#define MC_PIN() __builtin_amdgcn_sched_barrier(0)

// LDS-DMA sources.  Piece g (0..15) of a half = image rows 8g..8g+7; wave wv owns pieces 2wv, 2wv+1 (j = 0, 1);
// lane -> (image row = 8g + lane/8, slot = lane%8), source chunk (16 bytes) = slot ^ ((row>>1)&7).
// Image row r of Am<h> is tile row (r>>6)*128 + h*64 + (r&63); of Wn<h>: (r>>5)*64 + h*32 + (r&31).
// (Macros, not functions: behind a call the compiler folds this index arithmetic in another order and allocates the
// kernels' registers differently; the macros leave every instruction stream as it was -- tools/isa_same.py.)
#define MC_PIECE_ROW(wv, j, lane) (((wv) * 2 + (j)) * 8 + ((lane) >> 3))
#define MC_PIECE_CHUNK(r, lane) (((lane) & 7) ^ (((r) >> 1) & 7))
#define MC_A_TILE_ROW(r, h) (((r) >> 6) * 128 + (h) * 64 + ((r) & 63))
#define MC_W_TILE_ROW(r, h) (((r) >> 5) * 64 + (h) * 32 + ((r) & 31))

// LDS-DMA issue in inline asm: hipcc's waitcnt pass makes every ds_read that follows a
// __builtin_amdgcn_global_load_lds wait for it (vmcnt(0) in the loop); an asm DMA is invisible to
// that pass and ordered only by the counted waits of the kernel.  One 1 KiB piece per call.  saddr form: 64-bit
// uniform base in SGPRs + one 32-bit byte offset per lane; M0 = LDS byte address of the piece
// (wave-uniform); s_nop covers the SALU-write-M0 -> LDS-DMA hazard.
// M0 is clobbered, not saved: nothing the compiler emits in these kernels reads it.  (It is a reserved register, so the
// compiler warns about the clobber: the including files silence -Winline-asm.)
__device__ __forceinline__ void dma_piece(const void* base, uint32_t off, uint32_t lds) {
  asm volatile(
      "s_mov_b32 m0, %1\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %0, %2"
      :
      : "v"(off), "s"(lds), "s"(base)
      : "memory", "m0");
}

}  // namespace pipe8
}  // namespace mc
