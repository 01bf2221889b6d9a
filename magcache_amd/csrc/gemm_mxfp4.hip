// MXFP4 block-scaled GEMM for gfx950 on v_mfma_scale_f32_16x16x128_f8f6f4 with both operands declared FP4 (cbsz:4 blgp:4):
//   C[M,N] = sum over 32-element K blocks kb of 2^(sa[m][kb] - 127) 2^(sw[n][kb] - 127) (A_q[m, kb] . W_q[n, kb])
//            (+ the fused epilogues of gemm_epilogue.h, and EPI_GELU_MXFP4: GELU rows leave as the next MXFP4 GEMM's A operand)
// A_q, W_q: OCP e2m1 codes, two per byte, K contiguous, the even k in the low nibble (a row of K elements is K / 2 bytes; lda /
// ldw count bytes); sa, sw: E8M0 scale bytes, one per (row, 32 consecutive k), in the scale image of the MX fp8 GEMM:
// block-major, s[kb * rows_pad + mx_scale_row(row)] (quant.h).  W4A4: an OPTIONAL mode of both engines (option "mx_fp4" on
// top of mc_config.fp8_linear = 2 | 3), coarser than MX fp8, never a default.
//
// What the instruction does with FP4 operands was probed on the hardware first (tools/ubench_mx_probe.cpp,
// profiles/r12/mx_probe_fp4.log): an FP4 operand is 16 bytes per lane (the low four dwords; nothing else is read); lane l holds
// row l % 16, and nibble i (even i = the low nibble of byte i / 2) of lane group g = l / 16 is k = 32 g + i -- 32 CONSECUTIVE k
// per lane, unlike the e4m3 operand's two stacked halves (gemm_mxfp8.hip); the scale byte of lane group g (op_sel picks one of
// the VGPR's four) multiplies exactly those 32 codes; code book 0 0.5 1 1.5 2 3 4 6, bit 3 the sign; the first operand's rows
// are D's rows; C/D layout as every 16x16 MFMA.
//
// The kernel is gemm_mxfp8.hip's on the 8-wave LDS-DMA pipeline of gemm_pipe8.h with a K tile of 256 FP4 = the same 128-byte
// LDS rows, so per K tile the same LDS and HBM traffic buys twice the k:
//   * 8 waves (2 x 4), wave tile 128(M) x 64(N), one interval = one 64 x 32 quadrant x 256 k = 16 MFMAs of 16x16x128 (two k
//     steps of 128; the second step of a block comes 8 MFMAs behind the first, so no MFMA waits for its accumulator);
//   * a fragment is the same two ds_read_b128 per 16 rows: the 16-byte chunks kgrp and 4 + kgrp of the 128-byte row ARE the
//     lane's operands of k step 0 and k step 1 (k = 128 step + 32 kgrp + 0..31);
//   * scales: per K tile 8 k blocks x 256 rows of each operand = 4 KiB; TWO global_load_lds_dword per wave per K tile (k
//     blocks wv % 4 and 4 + wv % 4 of A, waves 0..3, or W, waves 4..7); a lane reads one dword per k step at
//     [4 step + kgrp][64-row group][lane % 16] and the MFMA's op_sel picks the 16-row block's byte.
//   Every wave issues 10 LDS-DMA instructions per K tile (2 scale + 8 data): counted waits 12 / 8 / 14 / 12 (at MC_TILE).
// K: a multiple of 256 elements, at least 512 (an odd number of K tiles runs one more steady-state tile before the two tail
// tiles).  N: a multiple of 256.
//
// Rows: any M > 0, the contract of gemm_mxfp8.hip.  tilesM = ceil(M / 256); a partial last tile clamps the A rows its LDS-DMA
// reads to M - 1, per half and piece (no byte of A behind row M - 1 is read), reads scale bytes up to the next multiple of 256
// (contract: mx_rows_a >= ceil256(M), whatever those bytes hold) and every epilogue skips the rows m >= M.  Every output row
// depends on its own A row and that row's scale bytes only, so rows >= M of A and their scale bytes never reach a stored value,
// and a launch over M rows gives rows [0, M) the bits a launch over ceil256(M) rows gives them.
// the LDS-DMA asm (below and in gemm_pipe8.h) names m0 in its clobber list on purpose (reserved register: the compiler only warns)
#pragma clang diagnostic ignored "-Winline-asm"
#include "common.h"
#include "gemm_epilogue.h"
#include "gemm_pipe8.h"
#include "ops.h"
#include "quant.h"

namespace mc {

namespace {

typedef __attribute__((ext_vector_type(4))) int i32x4v;

using namespace pipe8;

constexpr int BKE = 256;                         // elements of K per tile = 128 bytes of a packed row
constexpr int BKB = BKE / 2;
constexpr int SC_KSTRIDE = 320;                  // bytes between the k blocks of a scale image (256 rows + 64 pad: banks)
constexpr int SC_OPND = 8 * SC_KSTRIDE;          // one operand's scales of a K tile: 8 k blocks
constexpr int SC_STAGE = 2 * SC_OPND;            // A | W
constexpr int SC_BASE = 2 * STAGE_BYTES;         // scale images behind the two data stages
constexpr int LDS_TOTAL = SC_BASE + 2 * SC_STAGE;

struct FragA {   // one A half of a wave: 64 rows x 256 k = 4 m blocks of 16, per k step 16 bytes per lane each
  i32x4v v[4][2];   // [m block][k step]
  uint32_t s[2];    // E8M0 scales of the 4 blocks (byte mb), k block 4 step + kgrp
};
struct FragW {   // one W half of a wave: 32 rows x 256 k = 2 n blocks
  i32x4v v[2][2];
};
struct ScaleW {  // scales of the wave's 4 n blocks (byte 2 nh + nb) of one K tile: both W halves use the same dwords
  uint32_t s[2];
};

template <int EPI>
__global__ __launch_bounds__(512, 2) void gemm_mxfp4_kernel(GemmParams p, int tilesM, int tilesN, int GROUP_M) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15;
  const int kgrp = lane >> 4;
  const int wr = wv >> 2, wc = wv & 3;

  const int v = xcd_remap(blockIdx.x, tilesM * tilesN);
  int m0, n0;
  MC_GROUPED_TILE(v, tilesM, tilesN, GROUP_M, TB, m0, n0);

  // ---- LDS-DMA sources of the data halves: the pieces, image rows and swizzled chunks of gemm_pipe8.h; the row guard of
  // gemm_mxfp8.hip: the first row of a piece is clamped to M - 1 and the lane part to lim = (rows of the 8 that exist - 1) *
  // lda + 112, so a lane whose row is behind M - 1 reads chunk 7 of the last row that exists (lda >= K / 2 >= 256 > 112, so
  // every lane part of an existing row is <= lim and of a missing row > lim).  No byte behind row M - 1 is read.
  const uint8_t* Aq = (const uint8_t*)p.A;
  const uint8_t* Wq = (const uint8_t*)p.W;
  uint32_t srcA[2], srcW[2];
  size_t baseA[2][2];   // [half][piece] byte offset of the piece's first row
  uint32_t limA[2][2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int r0 = MC_PIECE_ROW(wv, j, 0);   // the piece's first image row
    const int r = r0 + (lane >> 3);
    const int chunk = MC_PIECE_CHUNK(r, lane);
    srcA[j] = (uint32_t)(lane >> 3) * (uint32_t)p.lda + chunk * 16;
    srcW[j] = (uint32_t)(n0 + MC_W_TILE_ROW(r, 0)) * (uint32_t)p.ldw + chunk * 16;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int row = __builtin_amdgcn_readfirstlane(min(m0 + MC_A_TILE_ROW(r0, h), p.M - 1));
      baseA[h][j] = (size_t)row * p.lda;
      limA[h][j] = (uint32_t)(min(p.M - row, 8) - 1) * (uint32_t)p.lda + 112;
    }
  }
  const size_t halfW = (size_t)32 * p.ldw;
  const uint32_t lds0 = (uint32_t)(uintptr_t)MC_LDS_PTR(smem);
  const uint32_t dma_lds = lds0 + wv * 2048;
  // ---- the scale pieces of this wave: waves 0..3 the A scales of k blocks wv and 4 + wv, waves 4..7 the W scales of k blocks
  // wv - 4 and wv; 256 rows = 64 lanes x 4 bytes.  Source: s[(8 kt + kb) * rows_pad + tile row 0 + 4 lane]
  const int sc_kb = wv & 3;
  const size_t sc_rows = (size_t)(wv < 4 ? p.mx_rows_a : p.mx_rows_w);
  const uint8_t* sc_src = (wv < 4 ? p.a_mx + m0 : p.w_mx + n0) + (size_t)sc_kb * sc_rows;
  const size_t sc_step = 8 * sc_rows;   // bytes per K tile
  const uint32_t sc_off = lane * 4;
  const uint32_t sc_lds = lds0 + SC_BASE + (wv < 4 ? 0 : SC_OPND) + sc_kb * SC_KSTRIDE;

  // ---- fragment read offsets: image row = blk*16 + l15 (+ wave base); chunk kgrp of the row (XOR-swizzled) = k step 0, chunk
  // 4 + kgrp = k step 1: its address is the first one's ^ 64
  const int sw = l15 >> 1;
  int foa[2], fow[2];   // [stage], chunk kgrp
#pragma unroll
  for (int st = 0; st < 2; ++st) {
    const int fo = l15 * 128 + ((kgrp ^ sw) << 4);
    foa[st] = fo + wr * (64 * 128) + st * STAGE_BYTES;
    fow[st] = fo + wc * (32 * 128) + st * STAGE_BYTES;
  }
  // scale dwords: [stage][operand][k block 4 step + kgrp][64-row group][l15] -> bytes = the group's four 16-row blocks.
  // A half h of wave row wr = group 2 wr + h; the W rows of wave column wc = group wc (byte 2 nh + nb)
  const int sb = kgrp * SC_KSTRIDE + l15 * 4;
  const int soa_u = SC_BASE + wr * 128, sow_u = SC_BASE + SC_OPND + wc * 64;   // wave-uniform parts (+ st * SC_STAGE)

  f32x4 acc[2][4][2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int d = 0; d < 2; ++d)
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[a][b][c][d][r] = 0.f;

  const int nk = p.K / BKE;

  // A pieces: dma_piece (gemm_pipe8.h) with the row clamp in front of the load (inside the asm: gemm_mxfp8.hip says why)
  auto dma_a1 = [&](int kt, int st, int h, int j) {
    uint32_t off;
    asm volatile(
        "s_mov_b32 m0, %2\n\t"
        "v_min_u32 %0, %4, %1\n\t"
        "global_load_lds_dwordx4 %0, %3"
        : "=&v"(off)
        : "v"(srcA[j]), "s"(dma_lds + st * STAGE_BYTES + (h ? OFF_AM1 : OFF_AM0) + j * 1024),
          "s"(Aq + (size_t)kt * BKB + baseA[h][j]), "s"(limA[h][j])
        : "memory", "m0");
  };
  auto dma_w1 = [&](int kt, int st, int h, int j) {
    dma_piece(Wq + (size_t)kt * BKB + (h ? halfW : 0), srcW[j], dma_lds + st * STAGE_BYTES + (h ? OFF_WN1 : OFF_WN0) + j * 1024);
  };
  auto dma_a = [&](int kt, int st, int h) { dma_a1(kt, st, h, 0); dma_a1(kt, st, h, 1); };
  auto dma_w = [&](int kt, int st, int h) { dma_w1(kt, st, h, 0); dma_w1(kt, st, h, 1); };
  auto dma_sc1 = [&](int kt, int st, int half) {   // 256 scale bytes of K tile kt: k block sc_kb + 4 half
    asm volatile(
        "s_mov_b32 m0, %1\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dword %0, %2"
        :
        : "v"(sc_off), "s"(sc_lds + st * SC_STAGE + half * 4 * SC_KSTRIDE), "s"(sc_src + (size_t)kt * sc_step + (size_t)half * 4 * sc_rows)
        : "memory", "m0");
  };
  auto dma_sc = [&](int kt, int st) { dma_sc1(kt, st, 0); dma_sc1(kt, st, 1); };
  // k step ks (0, 1) of fragment i (0..3) of this wave's A half h: one 16-byte read; with (0, 0) the two scale dwords
  // (st_sc: the stage of the scale image, st everywhere but in the prologue)
  auto read_a1 = [&](int st, int h, int i, int ks, FragA& f, int st_sc) {
    const char* b = smem + (h ? OFF_AM1 : OFF_AM0) + i * (16 * 128);
    f.v[i][ks] = *(const i32x4v*)(b + (ks ? foa[st] ^ 64 : foa[st]));
    if (i == 0 && ks == 0) {
      f.s[0] = *(const uint32_t*)(smem + (soa_u + st_sc * SC_STAGE + h * 64) + sb);
      f.s[1] = *(const uint32_t*)(smem + (soa_u + st_sc * SC_STAGE + h * 64 + 4 * SC_KSTRIDE) + sb);
    }
  };
  auto read_w1 = [&](int st, int h, int i, int ks, FragW& f) {
    const char* b = smem + (h ? OFF_WN1 : OFF_WN0) + i * (16 * 128);
    f.v[i][ks] = *(const i32x4v*)(b + (ks ? fow[st] ^ 64 : fow[st]));
  };
  auto read_ws = [&](int st, ScaleW& f) {
    f.s[0] = *(const uint32_t*)(smem + (sow_u + st * SC_STAGE) + sb);
    f.s[1] = *(const uint32_t*)(smem + (sow_u + st * SC_STAGE + 4 * SC_KSTRIDE) + sb);
  };
  // MFMA i (0..15) of an interval: k step i / 8, m block (i % 8) / 2, n block i % 2.  asm with the accumulator pinned (why:
  // gemm_bf16_big.hip, mma1); first operand = weight rows (D rows = n), its scale first; op_sel / op_sel_hi = low / high bit of
  // the scale byte index of (first, second) operand: W byte 2 nh + nb, A byte mb.
#define MC_MX4_MFMA(SEL)                                                                                 \
  asm volatile("v_mfma_scale_f32_16x16x128_f8f6f4 %0, %1, %2, %0, %3, %4 " SEL " cbsz:4 blgp:4"          \
               : "+v"(c[mb][nh][nb])                                                                     \
               : "v"(w.v[nb][ks]), "v"(a.v[mb][ks]), "v"(ws.s[ks]), "v"(a.s[ks]))
  auto mma1 = [&](int i, const FragW& w, const ScaleW& ws, const FragA& a, f32x4 (&c)[4][2][2], int nh) {
    const int ks = i >> 3, mb = (i & 7) >> 1, nb = i & 1;
    switch ((2 * nh + nb) * 4 + mb) {   // constant after unrolling
      case 0: MC_MX4_MFMA("op_sel:[0,0,0] op_sel_hi:[0,0,0]"); break;
      case 1: MC_MX4_MFMA("op_sel:[0,1,0] op_sel_hi:[0,0,0]"); break;
      case 2: MC_MX4_MFMA("op_sel:[0,0,0] op_sel_hi:[0,1,0]"); break;
      case 3: MC_MX4_MFMA("op_sel:[0,1,0] op_sel_hi:[0,1,0]"); break;
      case 4: MC_MX4_MFMA("op_sel:[1,0,0] op_sel_hi:[0,0,0]"); break;
      case 5: MC_MX4_MFMA("op_sel:[1,1,0] op_sel_hi:[0,0,0]"); break;
      case 6: MC_MX4_MFMA("op_sel:[1,0,0] op_sel_hi:[0,1,0]"); break;
      case 7: MC_MX4_MFMA("op_sel:[1,1,0] op_sel_hi:[0,1,0]"); break;
      case 8: MC_MX4_MFMA("op_sel:[0,0,0] op_sel_hi:[1,0,0]"); break;
      case 9: MC_MX4_MFMA("op_sel:[0,1,0] op_sel_hi:[1,0,0]"); break;
      case 10: MC_MX4_MFMA("op_sel:[0,0,0] op_sel_hi:[1,1,0]"); break;
      case 11: MC_MX4_MFMA("op_sel:[0,1,0] op_sel_hi:[1,1,0]"); break;
      case 12: MC_MX4_MFMA("op_sel:[1,0,0] op_sel_hi:[1,0,0]"); break;
      case 13: MC_MX4_MFMA("op_sel:[1,1,0] op_sel_hi:[1,0,0]"); break;
      case 14: MC_MX4_MFMA("op_sel:[1,0,0] op_sel_hi:[1,1,0]"); break;
      default: MC_MX4_MFMA("op_sel:[1,1,0] op_sel_hi:[1,1,0]"); break;
    }
  };

  // ---- prologue: per tile the issue order of the steady state: Wn0, Am0, scales (2), Wn1, Am1.  The K tiles run in pairs
  // (stages 0, 1; the W fragments change roles from tile to tile with period 2), so an ODD number of tiles starts in the
  // middle of a pair: tile 0 goes to stage 1, and its first fragments into the registers the second tile of a pair works on.
  // Both register sets are filled here (the same LDS reads twice), so that the prologue needs no branch; the fragment offsets
  // of the two stages change places around these reads (the lambdas index them with a constant), the scale stage is passed.
  const int odd = nk & 1;
  dma_w(0, odd, 0); dma_a(0, odd, 0); dma_sc(0, odd); dma_w(0, odd, 1); dma_a(0, odd, 1);
  dma_w(1, 1 - odd, 0); dma_a(1, 1 - odd, 0); dma_sc(1, 1 - odd); dma_w(1, 1 - odd, 1); dma_a(1, 1 - odd, 1);
  MC_WAIT_(12);   // 20 issued; Wn0(0), Am0(0), scales(0), Wn1(0) = the first 8 have landed
  MC_BARRIER();
  FragA A0, A1;
  FragW W0, W1, W2;
  ScaleW S0, S2;
  if (odd) { const int t = foa[0]; foa[0] = foa[1]; foa[1] = t; const int u = fow[0]; fow[0] = fow[1]; fow[1] = u; }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (i < 2) {
      read_w1(0, 0, i, 0, W0); read_w1(0, 0, i, 1, W0);
      read_w1(0, 0, i, 0, W2); read_w1(0, 0, i, 1, W2);
    }
    read_a1(0, 0, i, 0, A0, odd); read_a1(0, 0, i, 1, A0, odd);
  }
  read_ws(odd, S0);
  read_ws(odd, S2);
  if (odd) { const int t = foa[0]; foa[0] = foa[1]; foa[1] = t; const int u = fow[0]; fow[0] = fow[1]; fow[1] = u; }
  MC_BARRIER();   // every wave has issued its reads of Wn0(0) before the first interval re-fills it

  // One interval = 16 MFMA slots: k step 0 of the quadrant's 8 blocks, then k step 1.  The LDS-DMA pieces of the half this
  // interval re-fills in slots 3 and 5, the wave's two scale pieces (q2 only) in slot 1.  The NEXT interval's fragments are
  // read in the second half, a k step at a time: the registers of this interval's k step 0 operands are free by then, so an
  // A fragment is never held twice in full (two whole A fragments + three W fragments + the accumulators do not fit 256 VGPRs).
  //   RDA: A k step 0 of m block i in slot 8 + i (+ the scales in slot 8), k step 1 in slot 12 + i;
  //   RDW: W k step 0 of n block i in slot 8 + i, k step 1 in slot 12 + i (+ the next tile's W scales in slot 10).
#define MC_INTERVAL(WF, WS, AF, MH, NH, READ_STMT, DS, D0, D1)                 \
  _Pragma("unroll") for (int i_ = 0; i_ < 16; ++i_) {                          \
    mma1(i_, WF, WS, AF, acc[MH], NH);                                         \
    READ_STMT;                                                                 \
    if (i_ == 1) { DS; }                                                       \
    if (i_ == 3) { D0; }                                                       \
    if (i_ == 5) { D1; }                                                       \
    MC_PIN();                                                                  \
  }
#define MC_RD_W(COND, ST_, H_, DST)                                                                  \
  if ((COND) && i_ >= 8 && (i_ & 3) < 2) read_w1(ST_, H_, i_ & 3, (i_ >> 2) & 1, DST)
#define MC_RD_WS(COND, ST_, DST) if ((COND) && i_ == 10) read_ws(ST_, DST)
#define MC_RD_A(COND, ST_, H_, DST) if ((COND) && i_ >= 8) read_a1(ST_, H_, i_ & 3, (i_ >> 2) & 1, DST, ST_)

  // The scale image of stage ST (tile kt) is read until q1(kt) (the scales of Am1(kt)), so it is re-filled from q2(kt).
  // A wave's LDS-DMA stream per K tile: [Wn0 a, b] in q0, [Am0 a, b] in q1, [scales a, b, Wn1 a, b] in q2, [Am1 a, b] in q3 =
  // 10 instructions, each tile's issued two tiles ahead.  At the end of an interval whatever is read in the NEXT interval
  // must have landed:
  //   end of q0(kt): Am1(kt), issued in q3(kt-2); issued since: tile kt-1's 10 + q0's 2                         -> vmcnt(12)
  //   end of q1(kt): Wn0(kt+1) (q0(kt-1)) AND scales(kt+1) (q2(kt-1), read first in q2(kt)); since the scales:
  //                  Wn1 2 + Am1 2 + q0(kt) 2 + q1(kt) 2                                                        -> vmcnt(8)
  //   end of q2(kt): Am0(kt+1), issued in q1(kt-1); since: 4 + 2 + 2 + 2 + 4                                    -> vmcnt(14)
  //   end of q3(kt): Wn1(kt+1), issued in q2(kt-1) behind the scales; since: 2 + 10                             -> vmcnt(12)
  // Tile nk-2 issues nothing: 10, 4, 4 (6 would do), 2; tile nk-1: 0 once.
  // (the reads of an interval come after its own LDS-DMA issues, which the counts above place at its end: a read only needs
  // what the wait at the end of the PREVIOUS interval covered.)
#define MC_TILE(TAIL, kt, ST, W0, W2, S0, S2)                                                                 \
  {                                                                                                           \
    MC_INTERVAL(W0, S0, A0, 0, 0, MC_RD_W(true, ST, 1, W1), ,                                                 \
                if (TAIL == 0) dma_w1((kt) + 2, ST, 0, 0), if (TAIL == 0) dma_w1((kt) + 2, ST, 0, 1))         \
    if (TAIL == 0) MC_WAIT_(12); else if (TAIL == 1) MC_WAIT_(10); else MC_WAIT_(0);                          \
    MC_BARRIER();                                                                                             \
    MC_INTERVAL(W1, S0, A0, 0, 1, MC_RD_A(true, ST, 1, A1), ,                                                 \
                if (TAIL == 0) dma_a1((kt) + 2, ST, 0, 0), if (TAIL == 0) dma_a1((kt) + 2, ST, 0, 1))         \
    if (TAIL == 0) MC_WAIT_(8); else if (TAIL == 1) MC_WAIT_(4);                                              \
    MC_BARRIER();                                                                                             \
    MC_INTERVAL(W1, S0, A1, 1, 1, MC_RD_W(TAIL != 2, 1 - ST, 0, W2); MC_RD_WS(TAIL != 2, 1 - ST, S2),         \
                if (TAIL == 0) dma_sc((kt) + 2, ST),                                                          \
                if (TAIL == 0) dma_w1((kt) + 2, ST, 1, 0), if (TAIL == 0) dma_w1((kt) + 2, ST, 1, 1))         \
    if (TAIL == 0) MC_WAIT_(14); else if (TAIL == 1) MC_WAIT_(4);                                             \
    MC_BARRIER();                                                                                             \
    MC_INTERVAL(W0, S0, A1, 1, 0, MC_RD_A(TAIL != 2, 1 - ST, 0, A0), ,                                        \
                if (TAIL == 0) dma_a1((kt) + 2, ST, 1, 0), if (TAIL == 0) dma_a1((kt) + 2, ST, 1, 1))         \
    if (TAIL == 0) MC_WAIT_(12); else if (TAIL == 1) MC_WAIT_(2);                                             \
    MC_BARRIER();                                                                                             \
  }

  // nk odd: the second tile of a pair first (tile 0, in stage 1; nk >= 3, so it is a steady-state tile); then pairs of
  // steady-state tiles while two more tiles follow the pair; then the last two tiles
  int kt = 0;
  if (odd) {
    MC_TILE(0, 0, 1, W2, W0, S2, S0);
    kt = 1;
  }
  for (; kt < nk - 2; kt += 2) {
    MC_TILE(0, kt, 0, W0, W2, S0, S2);
    MC_TILE(0, kt + 1, 1, W2, W0, S2, S0);
  }
  MC_TILE(1, kt, 0, W0, W2, S0, S2);
  MC_TILE(2, kt + 1, 1, W2, W0, S2, S0);
#undef MC_TILE
#undef MC_INTERVAL
#undef MC_RD_W
#undef MC_RD_WS
#undef MC_RD_A
#undef MC_MX4_MFMA
  asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");   // XDL write -> VALU read of the accumulators (asm MFMAs)

  // ---- epilogue: the accumulator layout of gemm_mxfp8.hip (same MFMA shape, same wave tile); rows m >= M of a partial last
  // tile are skipped
#pragma unroll
  for (int mh = 0; mh < 2; ++mh) {
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) {
      const int m = m0 + wr * 128 + mh * 64 + mb * 16 + l15;
      if (m >= p.M) continue;
#pragma unroll
      for (int nh = 0; nh < 2; ++nh) {
        if constexpr (EPI == EPI_GELU_MXFP4) {
          // The 32 columns n0 + wc*64 + nh*32 .. +31 of row m are ONE block of the next GEMM's A operand (the position of
          // EPI_GELU_MXFP8 in gemm_mxfp8.hip): 2 x 4 consecutive columns in this lane (nb = 0, 1), the rest in the lanes ^ 16
          // and ^ 32 -- same l15 = same row, so they skip rows m >= M together and every shuffle stays among active lanes.
          // Values as the bf16 epilogue would store them; exponent, codes and scale row by quant.h.  A lane's codes are 16
          // bits per nb at byte nb * 8 + 2 kgrp of the block's 16; the pair kgrp ^ 1 trades one half so that each lane stores
          // ONE dword: an even kgrp the nb = 0 columns of both, an odd kgrp the nb = 1 columns.
          const int nblk0 = n0 + wc * 64 + nh * 32;
          float y[8];
          float amax = 0.f;
#pragma unroll
          for (int nb = 0; nb < 2; ++nb) {
            const int n = nblk0 + nb * 16 + 4 * kgrp;
            f32x4 b = {0.f, 0.f, 0.f, 0.f};
            if (p.bias) b = *(const f32x4*)(p.bias + n);
            const f32x4 val = acc[mh][mb][nh][nb] + b;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              y[4 * nb + i] = bf16_round(gelu_tanh_fast(bf16_round(val[i])));
              amax = fmaxf(amax, fabsf(y[4 * nb + i]));
            }
          }
          amax = fmaxf(amax, __shfl_xor(amax, 16, 64));
          amax = fmaxf(amax, __shfl_xor(amax, 32, 64));
          const int ex = mxfp4_exponent(amax);
          const float inv = mx_inv_scale(ex);
          const uint32_t c0 = pack4_e2m1(y[0], y[1], y[2], y[3], inv), c1 = pack4_e2m1(y[4], y[5], y[6], y[7], inv);
          const uint32_t got = __shfl_xor((kgrp & 1) ? c0 : c1, 16, 64);
          const uint32_t w = (kgrp & 1) ? (got | (c1 << 16)) : (c0 | (got << 16));
          *(uint32_t*)(p.Cq + (size_t)m * p.ldcq + (nblk0 >> 1) + (kgrp & 1) * 8 + (kgrp & 2) * 2) = w;
          if (kgrp == 0) p.c_mx[(size_t)(nblk0 >> 5) * p.mx_rows_c + mx_scale_row(m)] = mx_scale_byte(ex);
          continue;
        }
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
          const int n = n0 + wc * 64 + nh * 32 + nb * 16 + 4 * kgrp;
          f32x4 b = {0.f, 0.f, 0.f, 0.f};
          if (p.bias) b = *(const f32x4*)(p.bias + n);
          if constexpr (EPI != EPI_GELU_MXFP4) gemm_epilogue_quad<EPI>(p, m, n, acc[mh][mb][nh][nb] + b);
        }
      }
    }
  }
}

template <int EPI>
hipError_t launch_mx4_t(const GemmParams& p, hipStream_t stream) {
  const int tilesM = (p.M + TB - 1) / TB, tilesN = p.N / TB;
  return launch_dynamic_lds<gemm_mxfp4_kernel<EPI>>(dim3(tilesM * tilesN), dim3(512), LDS_TOTAL, stream, p, tilesM, tilesN,
                                                    MC_GROUP_M_OF(tilesN));
}

// ------------------------------------------------------------------ MXFP4 quantisation of rows
// quant.h's body with this format's exponent and packing
__global__ __launch_bounds__(256) void quantize_rows_mxfp4_kernel(const bf16_t* __restrict__ x, const float* __restrict__ xf,
                                                                  long ldx, int M, int K, uint8_t* __restrict__ q, long ldq,
                                                                  uint8_t* __restrict__ s, long rows_pad) {
  MC_QUANTIZE_ROWS_MX_BODY(QuantE2m1)
}

}  // namespace

hipError_t launch_gemm_mxfp4(const GemmParams& p, int epi, hipStream_t stream) {
  if (!gemm_mx_supported(MX_E2M1, p)) return hipErrorInvalidValue;
  switch (epi) {
    case EPI_BF16: return p.Cb ? launch_mx4_t<EPI_BF16>(p, stream) : hipErrorInvalidValue;
    case EPI_GELU_BF16: return p.Cb ? launch_mx4_t<EPI_GELU_BF16>(p, stream) : hipErrorInvalidValue;
    case EPI_RESID_GATE: return p.X ? launch_mx4_t<EPI_RESID_GATE>(p, stream) : hipErrorInvalidValue;
    case EPI_RESID_CAPTURE: return p.X ? launch_mx4_t<EPI_RESID_CAPTURE>(p, stream) : hipErrorInvalidValue;
    case EPI_F32: return p.X ? launch_mx4_t<EPI_F32>(p, stream) : hipErrorInvalidValue;
    case EPI_GELU_MXFP4:
      if (!p.Cq || !p.c_mx || ((uintptr_t)p.Cq & 3) != 0 || (p.ldcq % 16) != 0 || p.ldcq < p.N / 2 || (p.mx_rows_c % 64) != 0 ||
          p.mx_rows_c < (long)((p.M + TB - 1) / TB) * TB)
        return hipErrorInvalidValue;
      return launch_mx4_t<EPI_GELU_MXFP4>(p, stream);
    default: return hipErrorInvalidValue;   // EPI_GELU_MXFP8 included: its bytes are e4m3
  }
}

hipError_t launch_quantize_rows_mxfp4(const bf16_t* x, const float* x_f32, long ldx, int M, int K, uint8_t* q, long ldq,
                                      uint8_t* s, long rows_pad, hipStream_t stream) {
  return launch_quantize_rows_mx_kernel<quantize_rows_mxfp4_kernel>(MX_E2M1, x, x_f32, ldx, M, K, q, ldq, s, rows_pad, stream);
}

}  // namespace mc
