// 256x256 fp8 (OCP e4m3) GEMM for gfx950 on v_mfma_scale_f32_32x32x64_f8f6f4 with unit E8M0 block scales; per-row
// activation scales and per-output-channel weight scales (fp32) are applied to the fp32 accumulator in the epilogue:
//   C[M,N] = (A_q[M,K] * W_q[N,K]^T) * a_scale[m] * w_scale[n]  (+ the fused epilogues of gemm_epilogue.h)
// An OPTIONAL speed / quality mode of the engine (mc_config.fp8_linear = 1), never the default and never the headline.
// p.A / p.W point to bytes, lda / ldw / K count fp8 elements.
//
// The 8-wave LDS-DMA pipeline of gemm_pipe8.h (geometry, LDS image, XOR swizzle, DMA pieces) with a K tile of 128 fp8 and
// the 32x32 accumulator layout: one interval multiplies one 64(m) x 32(n) quadrant of the wave tile over the 128 k of
// the tile = 4 MFMAs of 32x32x64 in the even ones of 8 issue slots; the fragment reads (ds_read_b128) and the two
// LDS-DMA pieces of the half an interval re-fills sit between them.  Intervals, what each reads and re-fills, and the
// wait counts: at MC_TILE below.
// the LDS-DMA asm (gemm_pipe8.h) names m0 in its clobber list on purpose (reserved register: the compiler only warns)
#pragma clang diagnostic ignored "-Winline-asm"
#include "common.h"
#include "gemm_epilogue.h"
#include "gemm_pipe8.h"
#include "ops.h"

namespace mc {

namespace {

using namespace pipe8;

constexpr int BK = 128;                // fp8 elements (= bytes) of K per tile
constexpr int GROUP_M = 8;
// E8M0 block scale 127 = 2^0 in all four bytes: the MX-scaled MFMA with unit scales
#define MC_F8_UNIT_SCALE 0x7f7f7f7f
typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(4))) int i32x4;

struct Frag4 {  // one 32-row block x 128 k: four 16-byte reads per lane, two per 32x32x64 MFMA operand
  bf16x8 v[4];
};

template <int EPI>
__global__ __launch_bounds__(512, 2) void gemm_fp8_kernel(GemmParams p, int tilesM, int tilesN) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = lane >> 5;
  const int l31 = lane & 31;
  const int wr = wv >> 2, wc = wv & 3;

  // ---- tile mapping: XCD-contiguous, grouped along M so neighbouring tiles share W panels in L2
  const int v = xcd_remap(blockIdx.x, tilesM * tilesN);
  int m0, n0;
  MC_GROUPED_TILE(v, tilesM, tilesN, GROUP_M, TB, m0, n0);

  // ---- LDS-DMA sources (pieces, image rows and swizzled chunks: gemm_pipe8.h); a partial last M tile re-reads row M-1
  uint32_t srcA[2][2], srcW[2][2];  // [half][piece] BYTE offsets from p.A / p.W (without k)
#pragma unroll
  for (int h = 0; h < 2; ++h) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int r = MC_PIECE_ROW(wv, j, lane);
      const int chunk = MC_PIECE_CHUNK(r, lane);
      const int ra = min(m0 + MC_A_TILE_ROW(r, h), p.M - 1);
      const int rw = n0 + MC_W_TILE_ROW(r, h);
      srcA[h][j] = (uint32_t)ra * (uint32_t)p.lda + chunk * 16;
      srcW[h][j] = (uint32_t)rw * (uint32_t)p.ldw + chunk * 16;
    }
  }
  // LDS byte address (M0 value) of this wave's two pieces inside half 0 of stage 0
  const uint32_t dma_lds = (uint32_t)(uintptr_t)MC_LDS_PTR(smem) + wv * 2048;

  // ---- fragment read offsets inside a half: image row = blk*32 + l31 (+64 for wave row 1 of an
  // A half / + wc*32 for W), 16-B chunk ^ ((row>>1)&7); (row>>1)&7 == (lane>>1)&7
  const int sw = (lane >> 1) & 7;
  int fo[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    // fragments (2s, 2s+1) = the 32 bytes of k-substep s (64 k) that this lane half owns, chunks 4s + 2*half + {0, 1}
    const int chunk = 4 * (ks >> 1) + 2 * half + (ks & 1);
    fo[ks] = l31 * 128 + ((chunk ^ sw) << 4);
  }
  // per-wave bases folded into the lane offsets: every ds_read below is base VGPR + immediate
  // (one set per stage: the second stage starts at 64 KiB, beyond the 16-bit DS offset field)
  int foa[2][4], fow[2][4];
#pragma unroll
  for (int st = 0; st < 2; ++st) {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      foa[st][ks] = fo[ks] + wr * (64 * 128) + st * STAGE_BYTES;  // + ms*32*128
      fow[st][ks] = fo[ks] + wc * (32 * 128) + st * STAGE_BYTES;
    }
  }

  f32x16 acc[2][2][2];  // [m half][ms][n half]
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[a][b][c][r] = 0.f;

  const int nk = p.K / BK;

  // piece j (0/1) of half h of K tile kt into stage st (= kt & 1)
  auto dma_a1 = [&](int kt, int st, int h, int j) {
    dma_piece((const char*)p.A + (size_t)kt * BK, srcA[h][j], dma_lds + st * STAGE_BYTES + (h ? OFF_AM1 : OFF_AM0) + j * 1024);
  };
  auto dma_w1 = [&](int kt, int st, int h, int j) {
    dma_piece((const char*)p.W + (size_t)kt * BK, srcW[h][j], dma_lds + st * STAGE_BYTES + (h ? OFF_WN1 : OFF_WN0) + j * 1024);
  };
  auto dma_a = [&](int kt, int st, int h) { dma_a1(kt, st, h, 0); dma_a1(kt, st, h, 1); };  // prologue
  auto dma_w = [&](int kt, int st, int h) { dma_w1(kt, st, h, 0); dma_w1(kt, st, h, 1); };
  // fragment i = 4*ms + ks of this wave's A half h / fragment ks of its W half h
  auto read_a1 = [&](int st, int h, int i, Frag4 (&f)[2]) {
    f[i >> 2].v[i & 3] =
        *(const bf16x8*)(smem + (h ? OFF_AM1 : OFF_AM0) + (i >> 2) * (32 * 128) + foa[st][i & 3]);
  };
  auto read_w1 = [&](int st, int h, int ks, Frag4& f) {
    f.v[ks] = *(const bf16x8*)(smem + (h ? OFF_WN1 : OFF_WN0) + fow[st][ks]);
  };
  auto read_a = [&](int st, int h, Frag4 (&f)[2]) {  // prologue
#pragma unroll
    for (int i = 0; i < 8; ++i) read_a1(st, h, i, f);
  };
  auto read_w = [&](int st, int h, Frag4& f) {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) read_w1(st, h, ks, f);
  };
  // issue slot i (0..7) of an interval.  Slots 0, 2, 4, 6 hold an MFMA: k-substep s = i/4 (64 k), 32-row block (i/2)%2 ->
  // two rotating accumulators; the odd slots are empty
  auto mma1 = [&](int i, const Frag4& w, const Frag4 (&a)[2], f32x16 (&c0), f32x16 (&c1)) {
    if ((i & 1) == 0) {
      const int s2 = (i >> 2) * 2, blk = (i >> 1) & 1;
      const i32x8 wv = __builtin_shufflevector(__builtin_bit_cast(i32x4, w.v[s2]), __builtin_bit_cast(i32x4, w.v[s2 + 1]),
                                               0, 1, 2, 3, 4, 5, 6, 7);
      const i32x8 av = __builtin_shufflevector(__builtin_bit_cast(i32x4, a[blk].v[s2]),
                                               __builtin_bit_cast(i32x4, a[blk].v[s2 + 1]), 0, 1, 2, 3, 4, 5, 6, 7);
      f32x16& c = blk ? c1 : c0;
      c = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wv, av, c, 0, 0, 0, MC_F8_UNIT_SCALE, 0, MC_F8_UNIT_SCALE);
    }
  };

  // ---- prologue: K tiles 0 and 1 in the steady-state issue order; Wn0(0), Am0(0), Wn1(0) landed
  dma_w(0, 0, 0); dma_a(0, 0, 0); dma_w(0, 0, 1); dma_a(0, 0, 1);
  dma_w(1, 1, 0); dma_a(1, 1, 0); dma_w(1, 1, 1); dma_a(1, 1, 1);
  MC_WAIT_(10);
  MC_BARRIER();
  // A0/A1: this wave's m0/m1 halves; W0/W1: n0/n1 of the current tile, W2: n0 of the next (W0 is
  // still live when it is read, so W0/W2 ping-pong by renaming; A0 is dead by then and is reused)
  Frag4 A0[2], A1[2], W0, W1, W2;
  read_w(0, 0, W0);
  read_a(0, 0, A0);
  // Wn0 of stage 0 is re-filled (K tile 2) by the FIRST interval below: every wave must have issued its reads of
  // Wn0(0) before any wave issues that DMA.  (Steady state has two barriers between the last read of a half and its
  // refill; this is the one place where the prologue had none -- a WAR window of a few hundred cycles that only a
  // wave delayed by that much behind its workgroup could hit.)
  MC_BARRIER();

  // TAIL 0: steady state (tile kt+2 exists); 1: kt == nk-2; 2: kt == nk-1.  ST = kt & 1, a literal.
  // Wait counts: at the end of an interval the half that is read in the NEXT interval must have
  // landed.  Steady state: 6 halves (12 DMAs) issued since, the oldest must be done -> vmcnt(10).
  // Tile nk-2 issues nothing: 4,3,2,1 halves may stay in flight -> 8,6,4,2; tile nk-1: 0 once.
#define MC_TILE(TAIL, kt, ST, W0, W2) \
  { \
    /* q0: (m0,n0); reads Wn1(kt); DMA Wn0(kt+2) */ \
    mma1(0, W0, A0, acc[0][0][0], acc[0][1][0]); \
    read_w1(ST, 1, 0, W1); \
    MC_PIN(); \
    mma1(1, W0, A0, acc[0][0][0], acc[0][1][0]); \
    MC_PIN(); \
    mma1(2, W0, A0, acc[0][0][0], acc[0][1][0]); \
    read_w1(ST, 1, 1, W1); \
    if (TAIL == 0) dma_w1((kt) + 2, ST, 0, 0); \
    MC_PIN(); \
    mma1(3, W0, A0, acc[0][0][0], acc[0][1][0]); \
    MC_PIN(); \
    mma1(4, W0, A0, acc[0][0][0], acc[0][1][0]); \
    read_w1(ST, 1, 2, W1); \
    MC_PIN(); \
    mma1(5, W0, A0, acc[0][0][0], acc[0][1][0]); \
    if (TAIL == 0) dma_w1((kt) + 2, ST, 0, 1); \
    MC_PIN(); \
    mma1(6, W0, A0, acc[0][0][0], acc[0][1][0]); \
    read_w1(ST, 1, 3, W1); \
    MC_PIN(); \
    mma1(7, W0, A0, acc[0][0][0], acc[0][1][0]); \
    MC_PIN(); \
    if (TAIL == 0) MC_WAIT_(10); else if (TAIL == 1) MC_WAIT_(8); else MC_WAIT_(0); \
    MC_BARRIER(); \
    /* q1: (m0,n1); reads Am1(kt); DMA Am0(kt+2) */ \
    mma1(0, W1, A0, acc[0][0][1], acc[0][1][1]); \
    read_a1(ST, 1, 0, A1); \
    MC_PIN(); \
    mma1(1, W1, A0, acc[0][0][1], acc[0][1][1]); \
    read_a1(ST, 1, 1, A1); \
    MC_PIN(); \
    mma1(2, W1, A0, acc[0][0][1], acc[0][1][1]); \
    read_a1(ST, 1, 2, A1); \
    if (TAIL == 0) dma_a1((kt) + 2, ST, 0, 0); \
    MC_PIN(); \
    mma1(3, W1, A0, acc[0][0][1], acc[0][1][1]); \
    read_a1(ST, 1, 3, A1); \
    MC_PIN(); \
    mma1(4, W1, A0, acc[0][0][1], acc[0][1][1]); \
    read_a1(ST, 1, 4, A1); \
    MC_PIN(); \
    mma1(5, W1, A0, acc[0][0][1], acc[0][1][1]); \
    read_a1(ST, 1, 5, A1); \
    if (TAIL == 0) dma_a1((kt) + 2, ST, 0, 1); \
    MC_PIN(); \
    mma1(6, W1, A0, acc[0][0][1], acc[0][1][1]); \
    read_a1(ST, 1, 6, A1); \
    MC_PIN(); \
    mma1(7, W1, A0, acc[0][0][1], acc[0][1][1]); \
    read_a1(ST, 1, 7, A1); \
    MC_PIN(); \
    if (TAIL == 0) MC_WAIT_(10); else if (TAIL == 1) MC_WAIT_(6); \
    MC_BARRIER(); \
    /* q2: (m1,n1); reads Wn0(kt+1); DMA Wn1(kt+2) */ \
    mma1(0, W1, A1, acc[1][0][1], acc[1][1][1]); \
    if (TAIL != 2) read_w1(1 - ST, 0, 0, W2); \
    MC_PIN(); \
    mma1(1, W1, A1, acc[1][0][1], acc[1][1][1]); \
    MC_PIN(); \
    mma1(2, W1, A1, acc[1][0][1], acc[1][1][1]); \
    if (TAIL != 2) read_w1(1 - ST, 0, 1, W2); \
    if (TAIL == 0) dma_w1((kt) + 2, ST, 1, 0); \
    MC_PIN(); \
    mma1(3, W1, A1, acc[1][0][1], acc[1][1][1]); \
    MC_PIN(); \
    mma1(4, W1, A1, acc[1][0][1], acc[1][1][1]); \
    if (TAIL != 2) read_w1(1 - ST, 0, 2, W2); \
    MC_PIN(); \
    mma1(5, W1, A1, acc[1][0][1], acc[1][1][1]); \
    if (TAIL == 0) dma_w1((kt) + 2, ST, 1, 1); \
    MC_PIN(); \
    mma1(6, W1, A1, acc[1][0][1], acc[1][1][1]); \
    if (TAIL != 2) read_w1(1 - ST, 0, 3, W2); \
    MC_PIN(); \
    mma1(7, W1, A1, acc[1][0][1], acc[1][1][1]); \
    MC_PIN(); \
    if (TAIL == 0) MC_WAIT_(10); else if (TAIL == 1) MC_WAIT_(4); \
    MC_BARRIER(); \
    /* q3: (m1,n0); reads Am0(kt+1); DMA Am1(kt+2) */ \
    mma1(0, W0, A1, acc[1][0][0], acc[1][1][0]); \
    if (TAIL != 2) read_a1(1 - ST, 0, 0, A0); \
    MC_PIN(); \
    mma1(1, W0, A1, acc[1][0][0], acc[1][1][0]); \
    if (TAIL != 2) read_a1(1 - ST, 0, 1, A0); \
    MC_PIN(); \
    mma1(2, W0, A1, acc[1][0][0], acc[1][1][0]); \
    if (TAIL != 2) read_a1(1 - ST, 0, 2, A0); \
    if (TAIL == 0) dma_a1((kt) + 2, ST, 1, 0); \
    MC_PIN(); \
    mma1(3, W0, A1, acc[1][0][0], acc[1][1][0]); \
    if (TAIL != 2) read_a1(1 - ST, 0, 3, A0); \
    MC_PIN(); \
    mma1(4, W0, A1, acc[1][0][0], acc[1][1][0]); \
    if (TAIL != 2) read_a1(1 - ST, 0, 4, A0); \
    MC_PIN(); \
    mma1(5, W0, A1, acc[1][0][0], acc[1][1][0]); \
    if (TAIL != 2) read_a1(1 - ST, 0, 5, A0); \
    if (TAIL == 0) dma_a1((kt) + 2, ST, 1, 1); \
    MC_PIN(); \
    mma1(6, W0, A1, acc[1][0][0], acc[1][1][0]); \
    if (TAIL != 2) read_a1(1 - ST, 0, 6, A0); \
    MC_PIN(); \
    mma1(7, W0, A1, acc[1][0][0], acc[1][1][0]); \
    if (TAIL != 2) read_a1(1 - ST, 0, 7, A0); \
    MC_PIN(); \
    if (TAIL == 0) MC_WAIT_(10); else if (TAIL == 1) MC_WAIT_(2); \
    MC_BARRIER(); \
  }

  // nk is even (checked by the launcher): steady pairs, then the two tail tiles
  int kt = 0;
  for (; kt < nk - 2; kt += 2) {
    MC_TILE(0, kt, 0, W0, W2);
    MC_TILE(0, kt + 1, 1, W2, W0);
  }
  MC_TILE(1, kt, 0, W0, W2);
  MC_TILE(2, kt + 1, 1, W2, W0);
#undef MC_TILE

  // ---- every MFMA retires HERE, in front of the row guard of the epilogue.  The guard is a divergent branch, and hipcc sank
  // the last MFMAs of an accumulator into the block that stores it.  An MFMA reads its operands from all 64 lanes whatever
  // EXEC says, but a fragment register the compiler had spilled was reloaded inside the block, under the block's EXEC: only
  // in the lanes of rows < M.  With fewer than 32 valid rows in a 32-row block of the last M tile the other lanes fed stale
  // registers to that MFMA, and one 64-k chunk of half the columns of those rows was wrong (M = 1, 257, 2309 at K = 512;
  // tests/test_fp8_gemm_rows_gpu.py).  An empty asm that takes each accumulator as an in/out operand costs no instruction
  // and cannot be crossed by the MFMA that writes it.
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int c = 0; c < 2; ++c) asm volatile("" : "+v"(acc[a][b][c]));

  // ---- epilogue. acc[mh][ms][nh][r] = C[m][n], m = m0 + wr*128 + mh*64 + ms*32 + l31,
  //      n = n0 + wc*64 + nh*32 + (r&3) + 8*(r>>2) + 4*half  -> 4 consecutive n per (r>>2)
#pragma unroll
  for (int mh = 0; mh < 2; ++mh) {
#pragma unroll
    for (int ms = 0; ms < 2; ++ms) {
      const int m = m0 + wr * 128 + mh * 64 + ms * 32 + l31;
      if (m >= p.M) continue;
      const float sa = p.a_scale[m];
#pragma unroll
      for (int nh = 0; nh < 2; ++nh) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int n = n0 + wc * 64 + nh * 32 + 8 * g + 4 * half;
          f32x4 val;
          f32x4 b = {0.f, 0.f, 0.f, 0.f};
          if (p.bias) b = *(const f32x4*)(p.bias + n);
          const f32x4 sw4 = *(const f32x4*)(p.w_scale + n);
#pragma unroll
          for (int i = 0; i < 4; ++i) val[i] = acc[mh][ms][nh][4 * g + i] * (sa * sw4[i]) + b[i];
          gemm_epilogue_quad<EPI>(p, m, n, val);
        }
      }
    }
  }
}

template <int EPI>
hipError_t launch_fp8_t(const GemmParams& p, hipStream_t stream) {
  const int tilesM = (p.M + TB - 1) / TB, tilesN = p.N / TB;
  return launch_dynamic_lds<gemm_fp8_kernel<EPI>>(dim3(tilesM * tilesN), dim3(512), 2 * STAGE_BYTES, stream, p, tilesM, tilesN);
}

}  // namespace

// K in fp8 elements, two K tiles of 128 per loop trip
bool gemm_fp8_supported(const GemmParams& p) {
  return p.M > 0 && p.N > 0 && (p.N % TB) == 0 && (p.K % (2 * BK)) == 0 && p.K >= 4 * BK && (p.lda % 16) == 0 &&
         (p.ldw % 16) == 0 && p.a_scale && p.w_scale && (size_t)p.M * (size_t)p.lda < (1ull << 32) &&
         (size_t)p.N * (size_t)p.ldw < (1ull << 32);
}

hipError_t launch_gemm_fp8(const GemmParams& p, int epi, hipStream_t stream) {
  if (!gemm_fp8_supported(p)) return hipErrorInvalidValue;
  switch (epi) {
    case EPI_BF16: return launch_fp8_t<EPI_BF16>(p, stream);
    case EPI_GELU_BF16: return launch_fp8_t<EPI_GELU_BF16>(p, stream);
    case EPI_RESID_GATE: return launch_fp8_t<EPI_RESID_GATE>(p, stream);
    case EPI_RESID_CAPTURE: return launch_fp8_t<EPI_RESID_CAPTURE>(p, stream);
    case EPI_F32: return launch_fp8_t<EPI_F32>(p, stream);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace mc
