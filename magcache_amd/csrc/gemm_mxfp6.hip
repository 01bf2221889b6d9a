// MXFP6 block-scaled GEMM for gfx950 on v_mfma_scale_f32_16x16x128_f8f6f4 with both operands declared FP6 e2m3 (cbsz:2 blgp:2):
//   C[M,N] = sum over 32-element K blocks kb of 2^(sa[m][kb] - 127) 2^(sw[n][kb] - 127) (A_q[m, kb] . W_q[n, kb])
//            (+ the fused epilogues of gemm_epilogue.h that the MX fp8 GEMM has, EPI_RESID_CAPTURE included)
// A_q, W_q: OCP e2m3 codes, 32 consecutive k per 24 bytes as ONE little-endian bit stream (code i of a block starts at bit 6 i:
// quant.h), K contiguous: a row of K elements is 3 K / 4 bytes, and lda / ldw count bytes; sa, sw: E8M0 scale bytes, one per
// (row, 32 consecutive k), in the scale image of the MX fp8 GEMM: block-major, s[kb * rows_pad + mx_scale_row(row)] (quant.h).
// W6A6: an OPTIONAL mode of both engines (option "mx_fp6" on top of fp8_linear = 2 | 3), never a default.
// Measured (profiles/r14/NOTES.md): MX fp8's accuracy and MX fp8's speed -- 0.93-1.06 x gemm_mxfp8.hip over twelve shapes, not the
// FP4 rate: a 96-byte K tile of a row is not a whole number of 64-byte sectors, so the bytes fetched are the e4m3 kernel's.
//
// What the instruction does with FP6 operands was probed on the hardware first (tools/ubench_mxfp6_probe.cpp,
// profiles/r14/mxfp6_probe.log): an FP6 operand is the low 24 bytes (six dwords) of a lane's register argument; lane l holds
// row l % 16, and its 24 bytes are the 32 CONSECUTIVE k = 32 g + 0..31 of lane group g = l / 16 in exactly the packed order
// above, so 24 contiguous bytes of a packed row ARE a lane's operand; the scale byte of lane group g (op_sel picks one of the
// VGPR's four) multiplies exactly those 32 codes; the first operand's rows are D's rows; C/D layout as every 16x16 MFMA.
// The same probe found what shapes the LDS image: global_load_lds_dwordx3 writes lane l's 12 bytes at M0 + 16 l -- the lane
// stride of _dwordx4, bytes 12..15 of every 16 untouched -- so a 96-byte row moved by eight _dwordx3 lanes would still take 128
// bytes of LDS.  The kernel therefore moves its rows with global_load_lds_dwordx4: the LDS image of a group of rows is lane-linear
// and DENSE, 96 bytes per row, and since 16 divides 96 every lane's 16 bytes lie inside one row: lane l of the j-th
// instruction of a 32-row group carries bytes [P % 96, + 16) of row P / 96, P = 1024 j + 16 l; three instructions = 32 rows.
//
// The kernel (its own pipeline, not gemm_pipe8.h's, whose 128-byte LDS rows and 16-byte-aligned fragment reads do not fit):
//   * workgroup = 8 waves (2 along M x 4 along N), one 256 x 256 output tile, wave tile 128(M) x 64(N): the geometry, tile
//     rasterisation and epilogue positions of the other MX kernels.  K tile = 128 elements = one MFMA k step = 96 bytes of a row.
//   * LDS: 3 stages x (A 256 rows | W 256 rows) x 96 bytes = 144 KiB + 3 x the scale image of a K tile; the dense rows are what
//     lets a third stage fit the 160 KiB.  Wave wv moves rows 32 wv .. 32 wv + 31 of A and of W: 3 + 3 LDS-DMA instructions.
//   * a fragment = a lane's 24 bytes at row * 96 + 24 g: 8-byte aligned, three ds_read_b64 straight into the six VGPRs the MFMA
//     reads.  No swizzle: ds_read_b64 is served 32 lanes at a time with banks = (address / 4) mod 64, and a row is 24 dwords,
//     so of the 16 rows of a block only r and r + 8 meet on the same banks (2-way, on a read that runs at 256 bytes a clock).
//     The reads are volatile so that they STAY ds_read_b64: the compiler pairs neighbouring ones into ds_read2_b64, which is
//     banked mod 32 in groups of 16 lanes -- four rows of a block per bank -- and that version measured 0.63 x this one (profiles/r14/NOTES.md 2).
//   * scales: per K tile 4 k blocks x 256 rows of each operand = 1 KiB; ONE global_load_lds_dword per wave per K tile (k block
//     wv % 4 of A, waves 0..3, or of W, waves 4..7); a lane reads one dword at [k block g][64-row group][lane % 16] and the
//     MFMA's op_sel picks the 16-row block's byte.
//   * pipeline: tiles kt + 1 and kt + 2 are in flight while tile kt is multiplied.  Per K tile: s_waitcnt vmcnt(7) (this wave's
//     7 LDS-DMA instructions of tile kt have landed, those of tile kt + 1 may be under way; vmcnt(0) on the last tile),
//     lgkmcnt(0) (its reads of tile kt - 1 have returned), s_barrier (both hold for every wave), issue tile kt + 2 into the
//     stage tile kt - 1 was read from, then 12 fragments and 32 MFMAs of tile kt.  MFMAs through the builtin, so the compiler
//     schedules the reads against them and keeps the hazards.
// K: a multiple of 256 elements, at least 512 (the contract of gemm_mxfp4; the loop itself steps by 128).  N: a multiple of 256.
//
// Rows: any M > 0, the contract of gemm_mxfp8.hip.  tilesM = ceil(M / 256); a partial last tile clamps the A rows its LDS-DMA
// reads to M - 1, per lane (no byte of A behind row M - 1 is read), reads scale bytes up to the next multiple of 256
// (contract: mx_rows_a >= ceil256(M), whatever those bytes hold) and every epilogue skips the rows m >= M.  Every output row
// depends on its own A row and that row's scale bytes only, so rows >= M of A and their scale bytes never reach a stored value,
// and a launch over M rows gives rows [0, M) the bits a launch over ceil256(M) rows gives them.
// the LDS-DMA asm names m0 in its clobber list on purpose (reserved register: the compiler only warns)
#pragma clang diagnostic ignored "-Winline-asm"
#include "common.h"
#include "gemm_epilogue.h"
#include "ops.h"
#include "quant.h"

namespace mc {

namespace {

typedef __attribute__((ext_vector_type(8))) int i32x8v;

constexpr int TB = 256;                          // tile edge (M and N)
constexpr int BKE = 128;                         // elements of K per tile
constexpr int BKB = BKE * 3 / 4;                 // = 96 bytes of a packed row
constexpr int ROW_LDS = BKB;                     // bytes of LDS per row of a K tile: dense
constexpr int OPND_BYTES = TB * ROW_LDS;         // 24 KiB
constexpr int STAGE_BYTES = 2 * OPND_BYTES;      // A | W
constexpr int NSTAGE = 3;
constexpr int SC_KSTRIDE = 320;                  // bytes between the k blocks of a scale image (256 rows + 64 pad: banks)
constexpr int SC_OPND = 4 * SC_KSTRIDE;          // one operand's scales of a K tile: 4 k blocks
constexpr int SC_STAGE = 2 * SC_OPND;            // A | W
constexpr int SC_BASE = NSTAGE * STAGE_BYTES;    // scale images behind the data stages
constexpr int LDS_TOTAL = SC_BASE + NSTAGE * SC_STAGE;
static_assert(LDS_TOTAL <= 160 * 1024, "the three stages fit the CU's LDS");
#define MC_GROUP_M_OF6(tilesN) ((tilesN) >= 32 ? 4 : 8)   // the rasterisation of gemm_pipe8.h

template <int EPI>
__global__ __launch_bounds__(512, 2) void gemm_mxfp6_kernel(GemmParams p, int tilesM, int tilesN, int GROUP_M) {
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

  // ---- LDS-DMA sources.  This wave's 32 rows of an operand = 3 instructions; lane -> byte P = 1024 j + 16 lane of the group's
  // dense image = row P / 96, bytes [P % 96, + 16).  The row guard of gemm_mxfp8.hip, per lane: an A row behind M - 1 is replaced
  // by row M - 1 (its bytes land in the missing row's place and reach no stored value).  No byte behind row M - 1 is read.
  // (32-bit offsets: M * lda and N * ldw are below 2^32, gemm_mx_supported.)
  const uint8_t* Aq = (const uint8_t*)p.A;
  const uint8_t* Wq = (const uint8_t*)p.W;
  uint32_t srcA[3], srcW[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int P = 1024 * j + 16 * lane;
    const int row = 32 * wv + P / BKB, col = P % BKB;
    srcA[j] = (uint32_t)min(m0 + row, p.M - 1) * (uint32_t)p.lda + col;
    srcW[j] = (uint32_t)(n0 + row) * (uint32_t)p.ldw + col;
  }
  const uint32_t lds0 = (uint32_t)(uintptr_t)MC_LDS_PTR(smem);
  const uint32_t dma_lds = lds0 + wv * (32 * ROW_LDS);
  // ---- the scale piece of this wave: waves 0..3 the A scales of k block wv, waves 4..7 the W scales of k block wv - 4;
  // 256 rows = 64 lanes x 4 bytes.  Source: s[(4 kt + kb) * rows_pad + tile row 0 + 4 lane]
  const int sc_kb = wv & 3;
  const size_t sc_rows = (size_t)(wv < 4 ? p.mx_rows_a : p.mx_rows_w);
  const uint8_t* sc_src = (wv < 4 ? p.a_mx + m0 : p.w_mx + n0) + (size_t)sc_kb * sc_rows;
  const size_t sc_step = 4 * sc_rows;   // bytes per K tile
  const uint32_t sc_off = lane * 4;
  const uint32_t sc_lds = lds0 + SC_BASE + (wv < 4 ? 0 : SC_OPND) + sc_kb * SC_KSTRIDE;

  auto dma_x4 = [&](const void* base, uint32_t off, uint32_t lds) {
    asm volatile(
        "s_mov_b32 m0, %1\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %0, %2"
        :
        : "v"(off), "s"(lds), "s"(base)
        : "memory", "m0");
  };
  auto dma_tile = [&](int kt, int st) {   // this wave's 7 LDS-DMA instructions of K tile kt
    const uint32_t lds = dma_lds + st * STAGE_BYTES;
#pragma unroll
    for (int j = 0; j < 3; ++j) dma_x4(Wq + (size_t)kt * BKB, srcW[j], lds + OPND_BYTES + j * 1024);
    asm volatile(
        "s_mov_b32 m0, %1\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dword %0, %2"
        :
        : "v"(sc_off), "s"(sc_lds + st * SC_STAGE), "s"(sc_src + (size_t)kt * sc_step)
        : "memory", "m0");
#pragma unroll
    for (int j = 0; j < 3; ++j) dma_x4(Aq + (size_t)kt * BKB, srcA[j], lds + j * 1024);
  };

  // ---- fragment read offsets: row = 16 blk + l15 (+ the wave's first row); the lane's 24 bytes start at 24 g of the row
  const int fo = l15 * ROW_LDS + 24 * kgrp;
  const int foa = fo + wr * (128 * ROW_LDS);
  const int fow = fo + OPND_BYTES + wc * (64 * ROW_LDS);
  // scale dwords: [stage][operand][k block g][64-row group][l15] -> bytes = the group's four 16-row blocks.  The A rows of wave
  // row wr = groups 2 wr, 2 wr + 1; the W rows of wave column wc = group wc
  const int sb = kgrp * SC_KSTRIDE + l15 * 4;
  const int soa = SC_BASE + wr * 128 + sb, sow = SC_BASE + SC_OPND + wc * 64 + sb;

  // (volatile, so that the three reads stay single ds_read_b64 -- see the top of the file; in the LDS address space by name:
  // a volatile access through a generic pointer would be a flat load)
  typedef const volatile __attribute__((address_space(3))) u32x2* lds_u32x2;
  const auto lds = (const __attribute__((address_space(3))) char*)smem;
  auto read_frag = [&](int off) {
    const u32x2 a = *(lds_u32x2)(lds + off), b = *(lds_u32x2)(lds + off + 8), c = *(lds_u32x2)(lds + off + 16);
    return i32x8v{(int)a[0], (int)a[1], (int)b[0], (int)b[1], (int)c[0], (int)c[1], 0, 0};
  };

  f32x4 acc[8][4];
#pragma unroll
  for (int a = 0; a < 8; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[a][b][r] = 0.f;

  const int nk = p.K / BKE;
  // stage of tile kt = kt % 3: st_rd is read now, st_fill (the stage read last) is re-filled now
  int st_rd = 0, st_fill = 2;
  dma_tile(0, 0);
  dma_tile(1, 1);
  for (int kt = 0; kt < nk; ++kt) {
    // tile kt has landed (this wave's part: at most tile kt + 1's 7 instructions are still in flight) and this wave's reads
    // of tile kt - 1 have returned; behind the barrier both hold for every wave: the stage of tile kt may be read and the
    // stage of tile kt - 1 re-filled
    if (kt + 1 < nk) asm volatile("s_waitcnt vmcnt(7) lgkmcnt(0)\n\ts_barrier" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    if (kt + 2 < nk) dma_tile(kt + 2, st_fill);
    const int so = st_rd * STAGE_BYTES, ss = st_rd * SC_STAGE;
    st_fill = st_rd;
    st_rd = st_rd == NSTAGE - 1 ? 0 : st_rd + 1;
    i32x8v w[4];
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) w[nb] = read_frag(fow + so + nb * (16 * ROW_LDS));
    const int ws = *(const int*)(smem + sow + ss);
    const int as0 = *(const int*)(smem + soa + ss), as1 = *(const int*)(smem + soa + ss + 64);
    // first operand = weight rows (D rows = n), its scale first; the scale byte of n block nb / m block mb % 4
#define MC_MX6_MFMA(MB, NB, AS)                                                                                              \
  acc[MB][NB] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(w[NB], a, acc[MB][NB], 2, 2, NB, ws, (MB) & 3, AS)
#define MC_MX6_ROW(MB, AS)                                                \
  {                                                                       \
    const i32x8v a = read_frag(foa + so + (MB) * (16 * ROW_LDS));         \
    MC_MX6_MFMA(MB, 0, AS); MC_MX6_MFMA(MB, 1, AS); MC_MX6_MFMA(MB, 2, AS); MC_MX6_MFMA(MB, 3, AS); \
  }
    MC_MX6_ROW(0, as0) MC_MX6_ROW(1, as0) MC_MX6_ROW(2, as0) MC_MX6_ROW(3, as0)
    MC_MX6_ROW(4, as1) MC_MX6_ROW(5, as1) MC_MX6_ROW(6, as1) MC_MX6_ROW(7, as1)
#undef MC_MX6_ROW
#undef MC_MX6_MFMA
  }

  // ---- epilogue: the accumulator positions of gemm_mxfp8.hip (same MFMA shape, same wave tile); rows m >= M of a partial
  // last tile are skipped
#pragma unroll
  for (int mb = 0; mb < 8; ++mb) {
    const int m = m0 + wr * 128 + mb * 16 + l15;
    if (m >= p.M) continue;
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) {
      const int n = n0 + wc * 64 + nb * 16 + 4 * kgrp;
      f32x4 b = {0.f, 0.f, 0.f, 0.f};
      if (p.bias) b = *(const f32x4*)(p.bias + n);
      gemm_epilogue_quad<EPI>(p, m, n, acc[mb][nb] + b);
    }
  }
}

template <int EPI>
hipError_t launch_mx6_t(const GemmParams& p, hipStream_t stream) {
  const int tilesM = (p.M + TB - 1) / TB, tilesN = p.N / TB;
  return launch_dynamic_lds<gemm_mxfp6_kernel<EPI>>(dim3(tilesM * tilesN), dim3(512), LDS_TOTAL, stream, p, tilesM, tilesN,
                                                    MC_GROUP_M_OF6(tilesN));
}

// ------------------------------------------------------------------ MXFP6 quantisation of rows
// One wave per row; lane b (+64, +128, ...) owns the 32-element block b: scale exponent e = mxfp6_exponent(amax), codes
// e2m3(x * 2^-e) packed into 24 bytes, scale byte e + 127 at s[b * rows_pad + mx_scale_row(row)] (all of it quant.h).
__global__ __launch_bounds__(256) void quantize_rows_mxfp6_kernel(const bf16_t* __restrict__ x, const float* __restrict__ xf,
                                                                  long ldx, int M, int K, uint8_t* __restrict__ q, long ldq,
                                                                  uint8_t* __restrict__ s, long rows_pad) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  for (int b = lane; b < K / 32; b += 64) {
    float v[32];
    if (xf) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const f32x4 t = *(const f32x4*)(xf + (size_t)row * ldx + b * 32 + i * 4);
        v[4 * i] = t[0]; v[4 * i + 1] = t[1]; v[4 * i + 2] = t[2]; v[4 * i + 3] = t[3];
      }
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const u32x4 t = *(const u32x4*)(x + (size_t)row * ldx + b * 32 + i * 8);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          v[8 * i + 2 * j] = __uint_as_float(t[j] << 16);
          v[8 * i + 2 * j + 1] = __uint_as_float(t[j] & 0xffff0000u);
        }
      }
    }
    float amax = 0.f;
#pragma unroll
    for (int i = 0; i < 32; ++i) amax = fmaxf(amax, fabsf(v[i]));
    const int e = mxfp6_exponent(amax);
    const float inv = mx_inv_scale(e);
    uint32_t w0[3], w1[3];
    pack16_e2m3(v, inv, w0);
    pack16_e2m3(v + 16, inv, w1);
    u32x2* dst = (u32x2*)(q + (size_t)row * ldq + b * 24);   // 8-byte aligned: ldq % 16 == 0
    dst[0] = u32x2{w0[0], w0[1]};
    dst[1] = u32x2{w0[2], w1[0]};
    dst[2] = u32x2{w1[1], w1[2]};
    s[(size_t)b * rows_pad + mx_scale_row(row)] = mx_scale_byte(e);
  }
}

}  // namespace

hipError_t launch_gemm_mxfp6(const GemmParams& p, int epi, hipStream_t stream) {
  if (!gemm_mx_supported(MX_E2M3, p)) return hipErrorInvalidValue;
  switch (epi) {
    case EPI_BF16: return p.Cb ? launch_mx6_t<EPI_BF16>(p, stream) : hipErrorInvalidValue;
    case EPI_GELU_BF16: return p.Cb ? launch_mx6_t<EPI_GELU_BF16>(p, stream) : hipErrorInvalidValue;
    case EPI_RESID_GATE: return p.X ? launch_mx6_t<EPI_RESID_GATE>(p, stream) : hipErrorInvalidValue;
    case EPI_RESID_CAPTURE: return p.X ? launch_mx6_t<EPI_RESID_CAPTURE>(p, stream) : hipErrorInvalidValue;
    case EPI_F32: return p.X ? launch_mx6_t<EPI_F32>(p, stream) : hipErrorInvalidValue;
    default: return hipErrorInvalidValue;   // no fused quantising epilogue in this format
  }
}

hipError_t launch_quantize_rows_mxfp6(const bf16_t* x, const float* x_f32, long ldx, int M, int K, uint8_t* q, long ldq,
                                      uint8_t* s, long rows_pad, hipStream_t stream) {
  return launch_quantize_rows_mx_kernel<quantize_rows_mxfp6_kernel>(MX_E2M3, x, x_f32, ldx, M, K, q, ldq, s, rows_pad, stream);
}

}  // namespace mc
