// Internal launch API of the HIP kernels (C++ side, below the C-ABI in include/magcache_hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

namespace mc {

typedef uint16_t bf16_t;

// ---------------------------------------------------------------- GEMM (gemm_bf16.hip)
// C[M,N] = A[M,K] * W[N,K]^T  (bf16 inputs, fp32 MFMA accumulate), fused epilogues.
enum GemmEpi {
  EPI_BF16 = 0,          // Cb = bf16(acc + bias)
  EPI_GELU_BF16 = 1,     // Cb = bf16(gelu_tanh(bf16(acc + bias)))
  EPI_RESID_GATE = 2,    // X += gate[n] * bf16(acc + bias)         (gate == null -> 1)
  EPI_RESID_CAPTURE = 3, // as 2, then R = X_new - X0               (MagCache residual capture)
  EPI_EMBED = 4,         // X = bf16(acc + bias) (as fp32), X0out = same (bf16)
  EPI_F32 = 5,           // X = acc + bias (fp32 store)
  EPI_GELU_ERF_BF16 = 6, // Cb = bf16(gelu_erf(bf16(acc + bias)))   (128x128 kernel only)
  EPI_SILU_BF16 = 7,     // Cb = bf16(silu(bf16(acc + bias)))       (128x128 kernel only; HunyuanVideo token refiner)
  EPI_BF16_GELU_SPLIT = 10, // columns [0, n_split): Cb = bf16(acc + bias); columns [n_split, N): Cb2[m][n - n_split] =
                         // bf16(gelu_tanh(bf16(acc + bias))) -- two Linears over the same rows as ONE launch (the single block's
                         // q|k|v and MLP-in of an MM-DiT: 216 + 288 tiles are 2 + 2 trips of 256 CUs apart, 2 together)
  EPI_RESID_GATE_SEL = 11,    // (internal, gemm_bf16_v2) EPI_RESID_GATE / _CAPTURE with per-row gates: the launcher picks them
  EPI_RESID_CAPTURE_SEL = 12, // when gate_sel != null, so that the form without per-token gates keeps its code
  EPI_SPLITK_PARTIAL = 9,// (internal, gemm_bf16_v2 split-K) the fp32 accumulators of one K slice of a tile -> splitk_ws
  EPI_GELU_MXFP8 = 8,    // as 1, then MX-quantised in the epilogue: Cq = e4m3 bytes, c_mx = E8M0 block scales -- the A
                         // operand of the next MX GEMM, the bits launch_quantize_rows_mxfp8 would make of Cb (gemm_mxfp8 only)
  EPI_GELU_MXFP4 = 13,   // as 1, then MXFP4-quantised in the epilogue: Cq = packed e2m1 codes (column n at byte n / 2), c_mx =
                         // E8M0 block scales -- the A operand of the next MXFP4 GEMM, the bits launch_quantize_rows_mxfp4 would
                         // make of Cb (gemm_mxfp4 only)
};

struct GemmParams {
  const bf16_t* A; long lda;
  const bf16_t* W; long ldw;
  const float* bias;
  int M, N, K;
  bf16_t* Cb; long ldc;
  float* X; long ldx;
  const float* gate;
  const bf16_t* X0; long ldx0;
  float* R; long ldr;
  bf16_t* X0out; long ldx0out;
  int m_valid;  // EPI_EMBED: rows >= m_valid are written as zeros (sequence padding)
  // per-token modulation (Wan2.2 TI2V: two timestep values per forward): rows with gate_sel[m] != 0 use gate2
  const float* gate2;
  const uint8_t* gate_sel;
  // table form (gate_stride != 0, with gate_sel): gate is the first of gate_sets (1..64) vectors gate_stride floats apart and
  // row m takes vector min(gate_sel[m], gate_sets - 1) -- the byte is clamped before it forms an address; gate2 is ignored
  long gate_stride; int gate_sets;
  // split-K scratch (gemm_bf16_v2 only, optional): when a shape's 256 x 256 tiles fill less than half of the CUs and K is
  // long, launch_gemm_bf16 cuts K into S slices, every (tile, slice) workgroup parks its fp32 accumulators here and a second
  // launch sums the slices in index order and applies the epilogue (deterministic; not bit-identical to the unsplit sum).
  // null / too small: no split.  Must not be shared by GEMMs that may run concurrently.
  float* splitk_ws; size_t splitk_ws_bytes;
  // row-split operands (m_split > 0): rows >= m_split use W_b / bias_b / gate_b instead of W / bias / gate -- two Linears with
  // the same shapes over two row ranges of the same buffers as ONE launch (the image and the text stream of an MM-DiT double
  // block are row ranges of the joint buffers).  One gemm_bf16_v2 launch when m_split is a multiple of 256 and the epilogue is
  // bf16 / GELU / gated residual (+ capture); two launches through the normal dispatch otherwise.  Same bits either way.
  int m_split; const bf16_t* W_b; const float* bias_b; const float* gate_b;
  // EPI_BF16_GELU_SPLIT: first GELU column (a multiple of 256) and the GELU half's destination
  int n_split; bf16_t* Cb2; long ldc2;
  // fp8 GEMM (launch_gemm_fp8): A / W point to OCP e4m3 bytes, C = (A W^T) * a_scale[m] * w_scale[n] + bias
  const float* a_scale;
  const float* w_scale;
  // MX fp8 GEMM (launch_gemm_mxfp8): A / W point to e4m3 bytes (lda / ldw in bytes), a_mx / w_mx to E8M0 scale bytes,
  // block-major: scale of (row, k block kb of 32) at [kb * mx_rows + mx_scale_row(row)] (quant.h)
  const uint8_t* a_mx; long mx_rows_a;
  const uint8_t* w_mx; long mx_rows_w;
  // EPI_GELU_MXFP8: e4m3 output rows (ldcq bytes) and their block scales, c_mx[(n / 32) * mx_rows_c + mx_scale_row(m)] (quant.h);
  // EPI_GELU_MXFP4: packed e2m1 output rows, Cq[m * ldcq + n / 2], the same scale image
  uint8_t* Cq; long ldcq;
  uint8_t* c_mx; long mx_rows_c;
};

// the table form's operands (gate_stride != 0): a selector, a table, 1..64 rows at least N floats (a multiple of 4) apart
inline bool gemm_gate_table_ok(const GemmParams& p) {
  return p.gate_sel && p.gate && p.gate_sets >= 1 && p.gate_sets <= 64 && p.gate_stride >= p.N && (p.gate_stride % 4) == 0;
}
// The argument contract of the bf16 GEMM, stated once: launch_gemm_bf16 (before any dispatch) and the launchers of the shipped
// kernels (_small, _v2, _v2_splitk) return hipErrorInvalidValue, with nothing launched and nothing written, unless it holds.
//   shape     M > 0, N > 0 and % 4 == 0 (an epilogue handles a quad of 4 columns), K > 0 and % 64 == 0
//   operands  A [M, K] and W [N, K] (W_b too when m_split > 0) non-null and 16-byte aligned, lda and ldw >= K and % 8 == 0:
//             every kernel fetches them 16 bytes at a time.  Only rows [0, M) / [0, N) and columns [0, K) are read.
//   vectors   bias, bias_b, gate, gate2, gate_b: null or 16-byte aligned (read as one 16-byte quad per 4 columns); a gate table
//             as gemm_gate_table_ok; gate_sel with a gate and no table needs gate2
//   per epilogue, what it reads and writes -- non-null, a leading dimension >= N and % 4 == 0, and the quad's alignment:
//             EPI_BF16, _GELU_BF16, _GELU_ERF_BF16, _SILU_BF16   Cb (8 bytes: a quad of bf16)
//             EPI_RESID_GATE, EPI_F32                             X (16 bytes: a quad of fp32)
//             EPI_RESID_CAPTURE                                   X, X0 (8), R (16)
//             EPI_EMBED                                           X, X0out (8)
//             EPI_BF16_GELU_SPLIT                                 0 < n_split < N and % 4 == 0; Cb with ldc >= n_split, Cb2 with
//                                                                 ldc2 >= N - n_split (8 each)
//             anything else (the internal values included)        refused
//   Nothing outside rows [0, M) x columns [0, N) (of the widths above) of an output is written, whatever its leading dimension.
// gemm_bf16_v2 stores bf16 rows 16 bytes at a time (its row-major epilogues): a Cb / Cb2 that is not 16-byte aligned or whose
// leading dimension is no multiple of 8 is legal and runs on the 128x128 kernel instead (gemm_bf16_v2_epi_ok), like every
// other form that kernel lacks.  A split-K workspace that is not 16-byte aligned is not used.
inline bool gemm_bf16_args_ok(const GemmParams& p, int epi) {
  auto al = [](const void* q, uintptr_t a) { return ((uintptr_t)q & (a - 1)) == 0; };
  auto out = [&](const void* q, long ld, long width, uintptr_t a) { return q && al(q, a) && ld >= width && (ld % 4) == 0; };
  if (p.M <= 0 || p.N <= 0 || p.K <= 0 || (p.N % 4) != 0 || (p.K % 64) != 0) return false;
  if (!p.A || !p.W || !al(p.A, 16) || !al(p.W, 16) || (p.lda % 8) != 0 || (p.ldw % 8) != 0 || p.lda < p.K || p.ldw < p.K) return false;
  if (!al(p.bias, 16) || !al(p.gate, 16) || !al(p.gate2, 16)) return false;
  if (p.m_split > 0 && (!p.W_b || !al(p.W_b, 16) || !al(p.bias_b, 16) || !al(p.gate_b, 16))) return false;
  if (p.gate_stride != 0 ? !gemm_gate_table_ok(p) : (p.gate_sel && p.gate && !p.gate2)) return false;
  switch (epi) {
    case EPI_BF16: case EPI_GELU_BF16: case EPI_GELU_ERF_BF16: case EPI_SILU_BF16: return out(p.Cb, p.ldc, p.N, 8);
    case EPI_RESID_GATE: case EPI_F32: return out(p.X, p.ldx, p.N, 16);
    case EPI_RESID_CAPTURE: return out(p.X, p.ldx, p.N, 16) && out(p.X0, p.ldx0, p.N, 8) && out(p.R, p.ldr, p.N, 16);
    case EPI_EMBED: return out(p.X, p.ldx, p.N, 16) && out(p.X0out, p.ldx0out, p.N, 8);
    case EPI_BF16_GELU_SPLIT:
      return p.n_split > 0 && p.n_split < p.N && (p.n_split % 4) == 0 && out(p.Cb, p.ldc, p.n_split, 8) &&
             out(p.Cb2, p.ldc2, p.N - p.n_split, 8);
    default: return false;
  }
}
hipError_t launch_gemm_bf16(const GemmParams& p, int epi, hipStream_t stream);        // picks a kernel
int gemm_bf16_kernel_for(const GemmParams& p, int epi);                               // ... this one: 1 small, 2 8-wave 256^2, 4 v2
hipError_t launch_gemm_bf16_small(const GemmParams& p, int epi, hipStream_t stream);  // 128x128 tiles
// 256x256 tiles, 8 waves (rounds 1-3's kernel): NOT in libmagcache_hip.so since round 6 -- gemm_bf16_big.hip is built into
// the test-only libmagcache_hip_ref.so (MC_WITH_REF_GEMM), where gemm_kernel = 2 selects it as the independent
// implementation gemm_bf16_v2 is compared with bit for bit
hipError_t launch_gemm_bf16_big(const GemmParams& p, int epi, hipStream_t stream);
bool gemm_bf16_big_supported(const GemmParams& p);
bool gemm_bf16_big_linked();   // is this the reference library?  (gemm_bf16.hip is the one file built both ways)
hipError_t launch_gemm_bf16_v2(const GemmParams& p, int epi, hipStream_t stream);     // 256x256 tiles, 4 waves, generated stream
bool gemm_bf16_v2_supported(const GemmParams& p);
bool gemm_bf16_v2_epi_ok(const GemmParams& p, int epi);         // this epilogue on these operands?
bool gemm_bf16_v2_rowsplit_ok(const GemmParams& p, int epi);   // m_split > 0: can this be ONE gemm_bf16_v2 launch?
extern int g_gemm_defer;   // (libraries whose gemm_v2 stream was generated with --defer 1 only; the shipped one is not) 0: epilogues in place
// split-K (gemm_bf16_v2.hip): slices launch_gemm_bf16 would cut this problem's K into (1 = no split) given p.splitk_ws_bytes;
// bytes of scratch the split it would choose with unlimited scratch needs (0 = it would not split)
int gemm_splitk_slices(const GemmParams& p, int epi);
size_t gemm_splitk_ws_need(int M, int N, int K, int epi);
hipError_t launch_gemm_bf16_v2_splitk(const GemmParams& p, int epi, int slices, hipStream_t stream);
extern int g_gemm_v2_max_grid;  // 0 = grid of gemm_bf16_v2 = CUs; n = at most n persistent workgroups (probe: two forwards side by side)
extern int g_gemm_splitk;  // mc_set_option("gemm_splitk"): 1 = by shape (default), 0 = never, 2..16 = force that many slices where valid
extern int g_gemm_kernel;  // 0 by shape, 1 small, 2 big where supported (reference library only), 4: generation 2 where supported
// fp8 (e4m3) operands, 256x256 tiles, v_mfma_f32_32x32x64_f8f6f4; K (fp8 elements) a multiple of 256
hipError_t launch_gemm_fp8(const GemmParams& p, int epi, hipStream_t stream);
bool gemm_fp8_supported(const GemmParams& p);
// row-wise fp8 quantisation: q[m, :] = e4m3(x[m, :] / s[m]), s[m] = max|x[m, :]| / 448 (1 for an all-zero row); the
// arithmetic itself, shared with the fused producers of elementwise.hip: quant.h.
// x bf16 (x_f32 null) or fp32.  Used for activations (per token) and for weights (per output channel).
hipError_t launch_quantize_rows_fp8(const bf16_t* x, const float* x_f32, long ldx, int M, int K, uint8_t* q, long ldq,
                                    float* scale, hipStream_t stream);

// ---------------------------------------------------------------- MX block-scaled Linears: the element formats
// One E8M0 scale per (row, 32 k) on v_mfma_scale_f32_16x16x128_f8f6f4, in one scale image (quant.h: mx_scale_row) for every
// element format.  MxFormat is what the host asks "which format" with: a Linear, a weight slot and an engine hold ONE value of
// it.  The table holds facts about a format only; which producers an engine fuses is that engine's own predicate.
enum MxFormat { MX_E4M3, MX_E2M3, MX_E2M1 };
struct MxInfo {
  const char* name;     // as the error texts spell it
  const char* option;   // the mc_set_option key that selects it at create time; null: the default
  int block_bytes;      // bytes of 32 consecutive k in a packed row
  int gelu_epi;         // the quantising GELU epilogue of its GEMM, -1: it has none
};
constexpr MxInfo kMxInfo[] = {{"MX fp8", nullptr, 32, EPI_GELU_MXFP8}, {"MXFP6", "mx_fp6", 24, -1}, {"MXFP4", "mx_fp4", 16, EPI_GELU_MXFP4}};
constexpr const MxInfo& mx_info(MxFormat f) { return kMxInfo[f]; }
// bytes of k elements (a multiple of 32) in a packed row: every lda / ldw / ldq below is at least this and % 16 == 0
constexpr long mx_row_bytes(MxFormat f, long k) { return k / 32 * mx_info(f).block_bytes; }

// The operand contract of all three GEMMs: M > 0 (rows m >= M of a partial tile are guarded), N % 256 == 0, K a multiple of
// 256 elements and >= 512, 16-byte aligned packed rows of at least mx_row_bytes within 32-bit byte offsets, scale images with
// mx_rows_a >= ceil256(M), mx_rows_w >= N, both % 64 == 0.
inline bool gemm_mx_supported(MxFormat f, const GemmParams& p) {
  const long rb = mx_row_bytes(f, p.K);
  return p.M > 0 && p.N > 0 && (p.N % 256) == 0 && p.K >= 512 && (p.K % 256) == 0 && (p.lda % 16) == 0 && (p.ldw % 16) == 0 &&
         p.lda >= rb && p.ldw >= rb && p.A && p.W && (((uintptr_t)p.A | (uintptr_t)p.W) & 15) == 0 &&
         (size_t)p.M * (size_t)p.lda < (1ull << 32) && (size_t)p.N * (size_t)p.ldw < (1ull << 32) && p.a_mx && p.w_mx &&
         (((uintptr_t)p.a_mx | (uintptr_t)p.w_mx) & 3) == 0 && p.mx_rows_a >= (long)((p.M + 255) / 256) * 256 &&
         p.mx_rows_w >= p.N && (p.mx_rows_a % 64) == 0 && (p.mx_rows_w % 64) == 0;
}
// The argument contract of all three row quantisers: x bf16 (x_f32 null) or fp32, any M > 0, K % 32 == 0, ldx % 8 == 0 and
// >= K, ldq (bytes) % 16 == 0 and >= mx_row_bytes, x and q 16-byte aligned, rows_pad % 64 == 0 and >= ceil64(M).
inline bool quantize_rows_mx_supported(MxFormat f, const bf16_t* x, const float* x_f32, long ldx, int M, int K, const uint8_t* q,
                                       long ldq, const uint8_t* s, long rows_pad) {
  return (x || x_f32) && q && s && M > 0 && K > 0 && (K % 32) == 0 && (ldx % 8) == 0 && ldx >= K && (ldq % 16) == 0 &&
         ldq >= mx_row_bytes(f, K) && rows_pad >= ((M + 63) / 64) * 64 && (rows_pad % 64) == 0 &&
         (((uintptr_t)x | (uintptr_t)x_f32 | (uintptr_t)q) & 15) == 0;
}

// The per-format launchers (gemm_mxfp8.hip, gemm_mxfp4.hip, gemm_mxfp6.hip); lda / ldw / ldq / ldcq in BYTES of packed rows.
//   e4m3: one byte per element; the epilogues of gemm_epilogue.h and EPI_GELU_MXFP8.
//   e2m1: two codes per byte, the even k in the low nibble; the same epilogues with EPI_GELU_MXFP4 in its place (ldcq % 16 == 0
//         and >= N / 2, mx_rows_c % 64 == 0 and >= ceil256(M); rows m >= M store nothing).
//   e2m3: 32 consecutive k per 24 bytes, one little-endian bit stream with code i at bit 6 i; EPI_BF16, _GELU_BF16, _RESID_GATE,
//         _RESID_CAPTURE, _F32, no quantising epilogue.
hipError_t launch_gemm_mxfp8(const GemmParams& p, int epi, hipStream_t stream);
hipError_t launch_gemm_mxfp4(const GemmParams& p, int epi, hipStream_t stream);
hipError_t launch_gemm_mxfp6(const GemmParams& p, int epi, hipStream_t stream);
// q[m, block kb] = the 32 codes of x * 2^-e, e = ceil(log2(max|block| / the format's largest value: 448 | 6 | 7.5)), scale byte
// e + 127 at s[kb * rows_pad + mx_scale_row(m)]; exponent, packing and scale row are quant.h's, as in every fused producer
hipError_t launch_quantize_rows_mxfp8(const bf16_t* x, const float* x_f32, long ldx, int M, int K, uint8_t* q, long ldq,
                                      uint8_t* s, long rows_pad, hipStream_t stream);
hipError_t launch_quantize_rows_mxfp4(const bf16_t* x, const float* x_f32, long ldx, int M, int K, uint8_t* q, long ldq,
                                      uint8_t* s, long rows_pad, hipStream_t stream);
hipError_t launch_quantize_rows_mxfp6(const bf16_t* x, const float* x_f32, long ldx, int M, int K, uint8_t* q, long ldq,
                                      uint8_t* s, long rows_pad, hipStream_t stream);

// ... and the one place that maps a format to them
inline hipError_t launch_gemm_mx(MxFormat f, const GemmParams& p, int epi, hipStream_t s) {
  switch (f) {
    case MX_E4M3: return launch_gemm_mxfp8(p, epi, s);
    case MX_E2M3: return launch_gemm_mxfp6(p, epi, s);
    case MX_E2M1: return launch_gemm_mxfp4(p, epi, s);
  }
  return hipErrorInvalidValue;
}
inline hipError_t launch_quantize_rows_mx(MxFormat f, const bf16_t* x, const float* x_f32, long ldx, int M, int K, uint8_t* q,
                                          long ldq, uint8_t* s, long rows_pad, hipStream_t stream) {
  switch (f) {
    case MX_E4M3: return launch_quantize_rows_mxfp8(x, x_f32, ldx, M, K, q, ldq, s, rows_pad, stream);
    case MX_E2M3: return launch_quantize_rows_mxfp6(x, x_f32, ldx, M, K, q, ldq, s, rows_pad, stream);
    case MX_E2M1: return launch_quantize_rows_mxfp4(x, x_f32, ldx, M, K, q, ldq, s, rows_pad, stream);
  }
  return hipErrorInvalidValue;
}

// ---------------------------------------------------------------- LoRA merge (lora_merge.hip)
// out[rows, K] = bf16(base + sum_j scale_j * (up_j down_j)), up_j [rows, rank], down_j [rank, K].  Per term an fp32 accumulator
// from zero on bf16 MFMAs, the fp32 delta summed in term order, one fp32 add of the widened base element last, one
// round-to-nearest-even.  out may alias base; nothing outside [rows, K] is written (ld_out > K is legal).
// The operands are copies launch_lora_pack makes, bf16 in the order the kernel's 32x32x16 MFMAs read them: the rank zero-padded
// to a multiple of kLoraRankStep, the rows (of up; the columns of down) to a multiple of 32, and element (row, k) at
//   [((row / 32) * (rank_pad / 16) + k / 16) * 64 + 32 * ((k % 16) / 8) + row % 32][k % 8]
// -- per 32 rows and 16 rank elements the 64 lanes' 8-element fragments, consecutive.  lora_packed_elems: elements of one.
// hipErrorInvalidValue, and nothing launched, for more than kLoraMaxTerms terms, a rank_pad that is no positive multiple of
// kLoraRankStep, K or a leading dimension that is no multiple of 8, or a pointer that is not 16-byte aligned.  n_terms == 0
// copies base to out.
constexpr int kLoraMaxTerms = 8;
constexpr int kLoraRankStep = 16;
struct LoraTerm {
  const bf16_t* up;     // rows x rank_pad, packed
  const bf16_t* down;   // K x rank_pad (down transposed), packed
  int rank_pad;
  float scale;
};
inline size_t lora_packed_elems(size_t n, size_t rank_pad) { return (n + 31) / 32 * 32 * rank_pad; }
hipError_t launch_lora_merge(const bf16_t* base, long ld_base, bf16_t* out, long ld_out, int rows, int K, const LoraTerm* terms,
                             int n_terms, hipStream_t stream);
// The same merge into an fp32 matrix (the Wan engine's time MLP, time projection and head): out = base + delta, the ONE fp32 add
// last and no rounding step; same terms, same tiling.  K and the leading dimensions are multiples of 4 here.
hipError_t launch_lora_merge_f32(const float* base, long ld_base, float* out, long ld_out, int rows, int K, const LoraTerm* terms,
                                 int n_terms, hipStream_t stream);
// out[i] = base[i] + sum_j scales[j] * deltas[j][i], fp32, i < n (any n > 0): the sum from zero in term order, a multiply and an
// add per term (never contracted), one add of the base element last.  A term whose scale is 0 is left out; with no live term
// out is a copy of base.  out may alias base.  16-byte vectors where base, out and every live delta are 16-byte aligned, single
// elements for the tail (and for everything, where one of them is not).  hipErrorInvalidValue, and nothing launched, for
// n == 0, fewer than 1 or more than kLoraMaxTerms terms, a null pointer or one that is not 4-byte aligned.
hipError_t launch_param_delta(const float* base, float* out, size_t n, const float* const* deltas, const float* scales, int n_terms,
                              hipStream_t stream);
// dst (lora_packed_elems(n, rank_pad) elements) <- element (row, k) of an [n, rank] matrix at src[row * row_stride + k * col_stride],
// fp32 (src_f32) or bf16: `up` as given (strides rank, 1), `down` [rank, K] transposed (strides 1, K)
hipError_t launch_lora_pack(const void* src, int src_f32, long row_stride, long col_stride, int n, int rank, int rank_pad, bf16_t* dst,
                            hipStream_t stream);

// ---------------------------------------------------------------- adapter merge of every kind (adapter_merge.hip)
// out[rows, K] (bf16) from a bf16 base, any mix of low-rank pairs, Kronecker (LoKr) and Hadamard (LoHa) terms and an optional
// DoRA magnitude.  fp32 throughout, in `scratch` (rows * K floats, 16-byte aligned, owned by the caller):
//   delta  = the pairs as launch_lora_merge_f32 forms them on a zero base (bf16 operands, fp32 MFMA accumulation, term order)
//   delta += m_j * (w1_j[r / r2, c / c2] * w2_j[r % r2, c % c2])     one multiply for the product, one for m_j, one add
//   delta += m_j * ((u1_j d1_j)[r, c] * (u2_j d2_j)[r, c])           two rank-long dot products in k order, then as above
//   V      = fp32(base) + delta                                      ONE add of the base element, last
//   out    = bf16(V)                                                 magnitude == null
//   out    = bf16((g[r] / sqrt(sum_k V[r, k]^2)) * V[r, k])          magnitude g [rows]: thread t of the row's workgroup sums
//            columns t, t + 256, ... in that order and a fixed tree adds the 256 partial sums; a row whose V is all zero stays zero
// No product is contracted into an fma.  Kinds in the order above, terms of a kind in array order.  Element-wise launches, every
// thread guarded on its row and its 8-column chunk; nothing outside [rows, K] of out is written; out may alias base.  Not a
// forward-path launch.  hipErrorInvalidValue, and nothing launched, for what launch_lora_merge refuses, more than kLoraMaxTerms
// terms in all, r1 * r2 != rows, c1 * c2 != K, a rank < 1, a null or misaligned operand or scratch.
struct KronTerm {
  const float* w1;   // [r1, c1]
  const float* w2;   // [r2, c2]
  int r1, c1, r2, c2;
  float scale;
};
struct HadaTerm {
  const float *u1, *d1, *u2, *d2;   // u [rows, rank], d [rank, K]
  int rank;
  float scale;
};
hipError_t launch_adapter_merge(const bf16_t* base, long ld_base, bf16_t* out, long ld_out, int rows, int K, const LoraTerm* pairs,
                                int n_pairs, const KronTerm* krons, int n_kron, const HadaTerm* hadas, int n_hada,
                                const float* magnitude, float* scratch, hipStream_t stream);
// dst[i] = fp32(src[i]), i < n: src fp32 (a copy) or bf16 (widened exactly)
hipError_t launch_widen_f32(const void* src, int src_f32, float* dst, size_t n, hipStream_t stream);

// ---------------------------------------------------------------- attention (attention.hip)
struct AttnParams {
  const bf16_t* Q; long ldq;
  const bf16_t* K; long ldk; long k_shard_stride;
  const bf16_t* V; long ldv; long v_shard_stride;
  bf16_t* O; long ldo;
  int Lq_pad;       // query rows, multiple of 256
  int n_heads;      // head_dim is fixed at 128
  int shard_rows;   // rows per KV shard in memory (multiple of 64)
  int shard_valid;  // valid keys at the start of every shard
  int n_shards;
  float scale;      // softmax scale (1/sqrt(128))
  // Two-phase attention (sequence parallel: the local K/V shard is attended while the other shards are still in
  // flight over xGMI, the rest afterwards).  All three default to "off" when the struct is zero-filled.
  int skip_shard_p1;    // k + 1: shard k is left out of the key sequence; 0: none
  float* lse_out;       // [n_heads][Lq_pad] log2-sum-exp of the scaled scores of the keys visited, or null
  const float* lse_in;  // not null: O already holds the normalised result over OTHER keys whose log2-sum-exp is
                        // lse_in; the kernel merges both and writes the combined O (and lse_out if given)
};
// K/V rows in [shard_valid, shard_rows) are read (and masked) but must hold finite values.
hipError_t launch_attention(const AttnParams& p, hipStream_t stream);     // picks a kernel
hipError_t launch_attention_v5(const AttnParams& p, hipStream_t stream);  // 4 waves x 64 rows, one wave per SIMD, hand-scheduled (round 3)
bool attention_v5_supports(const AttnParams& p);                          // K / V span within 32-bit byte offsets
hipError_t launch_attention_v3(const AttnParams& p, hipStream_t stream);  // 8 waves x 32 rows, pipelined, 32x32x16 MFMA (round 1)
extern int g_attn_kernel;  // 0: by support (see launch_attention), 3: attention_v3.hip, 5: attention_v5.hip where it applies

// ---------------------------------------------------------------- token-wise ops (elementwise.hip)
// out[m,:] = bf16( LN(x[m,:]) * a + b ),  a = 1+scale (modulate) or weight (affine)
//   mode 0: a = 1 + sc[d], b = sh[d]      (AdaLN modulate; sc/sh fp32 vectors)
//   mode 1: a = sc[d],     b = sh[d]      (affine LayerNorm: weight / bias)
// If x0 != null the row is x0[m,:] (bf16) + x[m,:] (fp32): the fused MagCache skip path.
// sel != null: rows with sel[m] != 0 take (sc2, sh2) instead of (sc, sh) -- per-token modulation (Wan2.2 TI2V)
// set_stride != 0 (with sel and n_sets in 1..64): row m takes sc + k * set_stride and sh + k * set_stride, k = min(sel[m],
// n_sets - 1) -- a table of modulation sets; sc2 / sh2 are ignored.  The same for the quantising forms below.
hipError_t launch_ln_modulate(const float* x, long ldx, const bf16_t* x0, long ldx0, const float* sc,
                              const float* sh, int mode, float eps, bf16_t* out, long ldo, float* out_f32,
                              long ldof, int M, int D, hipStream_t stream, const float* sc2 = nullptr,
                              const float* sh2 = nullptr, const uint8_t* sel = nullptr, long set_stride = 0, int n_sets = 0);
// The same row, quantised for an fp8 GEMM instead of stored as bf16: e4m3 bytes q[m, :] relative to one scale per row
// (row_scale != null; launch_quantize_rows_fp8's arithmetic) or to one E8M0 scale per 32 elements (mx != null;
// launch_quantize_rows_mxfp8's arithmetic and scale layout) -- bit-identical to quantising the bf16 row launch_ln_modulate
// writes, without that row's round trip through memory.
hipError_t launch_ln_modulate_fp8(const float* x, long ldx, const float* sc, const float* sh, int mode, float eps,
                                  uint8_t* q, long ldq, float* row_scale, uint8_t* mx, long mx_rows, int M, int D,
                                  hipStream_t stream, const float* sc2 = nullptr, const float* sh2 = nullptr,
                                  const uint8_t* sel = nullptr, long set_stride = 0, int n_sets = 0);
// The same row as MXFP4: packed e2m1 codes q[m, d / 2] (ldq in bytes, % 16 == 0, >= D / 2) and one E8M0 scale per 32 elements in
// mx (mx_rows % 64 == 0, >= ceil64(M)) -- bit-identical to launch_quantize_rows_mxfp4 of the bf16 row launch_ln_modulate writes.
hipError_t launch_ln_modulate_mxfp4(const float* x, long ldx, const float* sc, const float* sh, int mode, float eps, uint8_t* q,
                                    long ldq, uint8_t* mx, long mx_rows, int M, int D, hipStream_t stream,
                                    const float* sc2 = nullptr, const float* sh2 = nullptr, const uint8_t* sel = nullptr,
                                    long set_stride = 0, int n_sets = 0);
// Wan2.2 TI2V per-token timesteps (at most two distinct values per forward): t2[0] = max, t2[1] = min of t[0, n_all);
// sel[i] = 1 where t[row0 + i] == min and min != max (rows >= n_rows: 0); t2[2] = number of tokens that are neither
hipError_t launch_token_t_prepare(const float* t, int n_all, int row0, int n_rows, int n_rows_pad, float* t2, uint8_t* sel,
                                  hipStream_t stream);
// Up to cap (1..kMaxTokenSets) distinct per-token timesteps: vals[0, cap) = the distinct values of t[0, n_all) in DESCENDING
// order (set 0 = the maximum, as above), padded with the last one found; sel[i] = the index of t[row0 + i] in vals (rows >=
// n_rows: 0); a token whose value has no set -- more than cap values, or NaN -- selects cap - 1.  t2[0] = max, t2[1] = min over
// all tokens, t2[2] = number of tokens without a set, t2[3] = sets in use.  -0.0 and 0.0 are one value.  One launch, one block.
constexpr int kMaxTokenSets = 64;
hipError_t launch_token_t_sets(const float* t, int n_all, int row0, int n_rows, int n_rows_pad, int cap, float* t2, float* vals,
                               uint8_t* sel, hipStream_t stream);

// in-place RMSNorm over D (all heads) + optional 3-D RoPE on bf16 rows.
//   y = bf16(x * rsqrt(mean(x^2)+eps)) * w ; rope pairs (2i,2i+1) with cs[token][64] (cos,sin)
hipError_t launch_rmsnorm_rope(bf16_t* x, long ldx, const float* w, float eps, const float* cs, int cs_row0,
                               int M, int D, hipStream_t stream);

// MM-DiT (FLUX / HunyuanVideo) q and k of one [M, >= 2*n_heads*128] bf16 block, in place:
//   per head RMSNorm over the 128 channels (y = bf16(x * rsqrt(mean(x^2)+eps)) * w[128]), then RoPE on the pairs
//   (2i,2i+1) with cs[cs_row0 + row][64] (cos,sin).  q = columns [0, H*128) with wq, k = [k_col0, k_col0+H*128)
//   with wk.  wq/wk null: no norm; cs null: no RoPE.
hipError_t launch_headnorm_rope(bf16_t* x, long ldx, long k_col0, const float* wq, const float* wk, float eps,
                                const float* cs, int cs_row0, int M, int n_heads, hipStream_t stream);
// y[n] = (accumulate ? y[n] : 0) + act_out( dot(W[n,:] (bf16), act_in(x) (fp32)) + b[n] ), act: 0 none, 1 silu
hipError_t launch_gemv_bf16w(const bf16_t* W, const float* x, const float* b, float* y, int N, int K, int act_in,
                             int act_out, int accumulate, hipStream_t stream);
// out[c] = mean over rows [0, n_rows) of x[r, c]  (HunyuanVideo token refiner: masked mean of the text states)
hipError_t launch_colmean(const float* x, long ldx, int n_rows, int D, float* out, hipStream_t stream);
// rows [0, n_rows) of a bf16 [., D] block <- fp32 (optionally (cos,sin)-interleaving two [n, 128] tables, see mmdit)
hipError_t launch_rope_table_from_cos_sin(const float* cosv, const float* sinv, long ld, int n_rows, float* cs,
                                          hipStream_t stream);
// Wan's 3-D RoPE for head_dim 128 (upstream rope_params / rope_apply): 22 complex pairs turn with the frame index, 21 with the
// height and 21 with the width index of a token
constexpr int kRopePairsT = 22, kRopePairsHW = 21;
// cs [n_rows][64][(cos,sin)] <- the per-axis pairs `axes` (F x 22 frame | Hp x 21 height | Wp x 21 width, mc_op_rope_axes):
// row r < n_tok is global token tok0 + r = (f, h, w) of the grid and copies pair i from the axis it belongs to; rows >= n_tok
// and tokens >= F Hp Wp get the identity (1, 0).  hipErrorInvalidValue for a null pointer, a non-positive size, tok0 < 0,
// n_tok > n_rows, a grid of more than 2^31 - 1 tokens or a cs that is not 16-byte aligned.
hipError_t launch_rope_expand(const float* axes, int F, int Hp, int Wp, int tok0, int n_tok, int n_rows, float* cs,
                              hipStream_t stream);

// latent fp32 [C,F,H,W] -> im2col bf16 tokens [L_pad, C*pt*ph*pw] for patch (1,2,2)
hipError_t launch_patchify(const float* lat, int C, int F, int H, int W, int tok0, int n_tok, int n_rows,
                           bf16_t* out, long ldo, hipStream_t stream);
// head output [L, 4*C] fp32 -> out [C,F,H,W] fp32 (unpatchify, patch (1,2,2))
hipError_t launch_unpatchify(const float* tok, long ldt, int C, int F, int H, int W, int tok0, int n_tok,
                             float* out, hipStream_t stream);
// y[n] = act_out( dot(W[n,:], act_in(x)) + b[n] ), fp32 GEMV. act: 0 none, 1 silu
hipError_t launch_gemv_f32(const float* W, const float* x, const float* b, float* y, int N, int K, int act_in,
                           int act_out, hipStream_t stream);
// sinusoidal_embedding_1d(dim, t) in float64 -> fp32; t read from device (t_dev) or host value
hipError_t launch_sinusoid(const float* t_dev, double t_host, int dim, float* out, hipStream_t stream);
// out[i] = a[i % na] + b[i]   (modulation + e0 broadcast)
hipError_t launch_add_bcast(const float* a, int na, const float* b, float* out, int n, hipStream_t stream);
// The same three over R (1..kMaxTokenSets) rows at once, ONE launch each whatever R is; every output row holds the bits the
// single-row launcher gives for that row alone (the same expressions in the same order).
//   sinusoid: out + r * ldo <- the embedding of t_dev[r]
//   gemv:     y + r * ldy <- W (x + r * ldx) + b; a wave owns a weight row, reads it from memory once and keeps it in registers
//             for all R right-hand sides (K <= 8192)
//   add:      out[r * ld_set + j * n + i] = a[r * lda + i % na] + b[j][i] for j < n_b, i < n -- b: HOST array of n_b device pointers
hipError_t launch_sinusoid_rows(const float* t_dev, int R, int dim, float* out, long ldo, hipStream_t stream);
hipError_t launch_gemv_f32_rows(const float* W, const float* x, long ldx, const float* b, float* y, long ldy, int R, int N, int K,
                                int act_in, int act_out, hipStream_t stream);
hipError_t launch_add_bcast_rows(const float* a, long lda, int R, int na, const float* const* b, int n_b, int n, float* out,
                                 long ld_set, hipStream_t stream);
// fp32 -> bf16 cast with zero padding of rows >= rows_valid
hipError_t launch_cast_pad_bf16(const float* src, long lds, int rows_valid, int rows, int cols, bf16_t* dst,
                                long ldd, hipStream_t stream);
hipError_t launch_cast_bf16(const float* src, bf16_t* dst, size_t n, hipStream_t stream);
// out[row, head] = log-sum-exp weighted mean of n (1..9) normalised partial attention results over disjoint key sets:
// o_parts[i] bf16 [rows][ldo], lse_parts[i] fp32 [d / 128][rows_pad] (log2 units) -- sequence parallel, see elementwise.hip
hipError_t launch_attn_merge(const bf16_t* const* o_parts, const float* const* lse_parts, int n, bf16_t* out, long ldo, int rows,
                             int rows_pad, int d, hipStream_t stream);
// a[i] = bf16(float(a[i]) + float(b[i]))   (sum of two attention outputs, Wan I2V cross-attention)
hipError_t launch_add_bf16(bf16_t* a, const bf16_t* b, size_t n, hipStream_t stream);
// x[m, :] += s[m, :] for m < rows (x fp32; s fp32 or bf16 -- s_bf16 -- contiguous [rows, D], widened exactly): a ControlNet
// sample added to rows of the residual stream, bitwise x + float(s).  r != null, a second destination in the same pass:
// r[m, :] += s[m, :], or with x0 != null r[m, :] = x_new[m, :] - x0[m, :] (x0 bf16): the MagCache residual taken after the
// add.  hipErrorInvalidValue for D % 8 != 0 or a pointer that is not 16-byte aligned.
hipError_t launch_add_rows(float* x, long ldx, const void* s, int s_bf16, float* r, long ldr, const bf16_t* x0, long ldx0,
                           int rows, int D, hipStream_t stream);
// IP-Adapter cross-attention of the FLUX double block (ip_attention.hip): one adapter's keys and values of one block, rows of
// [K | V] bf16 ([.., 2 * heads * 128], leading dimension ld), the first `valid` (1..kIpMaxKeys) of them keys, and its scale
constexpr int kIpMaxAdapters = 4, kIpMaxKeys = 256;
struct IpKeys {
  const bf16_t* kv;
  long ld;
  int valid;
  float scale;
};
// out[m, head] = sum_j scale_j softmax(q_n[m, head] K_j[head]^T / sqrt(128)) V_j[head] for m < rows, bf16 [rows, heads * 128];
// q: the RAW q columns (launch_headnorm_rope has not run), normalised per head as that kernel does without a table,
// q_n = bf16(bf16(q rstd) wq); softmax per adapter, fp32 sum over the adapters, one bf16 rounding.  Rows of a cache past `valid`
// are never read; an adapter with scale 0 is skipped (all of them: zeros).  hipErrorInvalidValue for 0 or more than
// kIpMaxAdapters adapters, a key count outside 1..kIpMaxKeys, a pointer that is not 16-byte aligned, a leading dimension that
// is no multiple of 8 or too short.
hipError_t launch_ip_attention(const bf16_t* q, long ldq, const float* wq, float eps, const IpKeys* adapters, int n_adapters,
                               bf16_t* out, long ldo, int rows, int heads, hipStream_t stream);
// test entry (mc_test_ip_qnorm): out = q_n as launch_ip_attention forms it, the same kernel stopped after its first step
hipError_t launch_ip_attention_qnorm(const bf16_t* q, long ldq, const float* wq, float eps, bf16_t* out, long ldo, int rows, int heads,
                                     hipStream_t stream);
// head: out[m, n] = dot(xn[m,:], W[n,:]) + b[n], fp32, N <= 256 (64 columns per block)
hipError_t launch_head_linear(const float* xn, long ldx, const float* W, const float* b, float* out, long ldo,
                              int M, int N, int K, hipStream_t stream);
// sampler: eps = u + g (c - u);  x = x + dt * eps  (flow-matching Euler step)
hipError_t launch_cfg_euler(const float* cond, const float* uncond, float g, float dt, float* x, float* eps_out,
                            size_t n, hipStream_t stream);

// Qwen-Image true-CFG + flow-Euler step on token rows (fp32, in place on x): comb = u + g (c - u), v = comb * |c| / |comb|
// (row norms over the C <= 256 channels; v = 0 where |comb| == 0), x += dt * v, rows [0, n_rows) only
hipError_t launch_cfg_norm_euler(const float* cond, const float* uncond, long ldp, float g, float dt, float* x, long ldx,
                                 int n_rows, int C, hipStream_t stream);
// weighted row RMSNorm fp32 -> bf16: out[m] = bf16(x[m] * rsqrt(mean(x[m]^2) + eps) * w) for m < rows_valid, zero rows
// [rows_valid, rows)  (Qwen-Image txt_norm)
hipError_t launch_rmsnorm_rows_bf16(const float* x, long ldx, const float* w, float eps, bf16_t* out, long ldo,
                                    int rows_valid, int rows, int D, hipStream_t stream);

// out[i] = sum_j coef[j] * xs[j][i], 1 <= k <= 6 fp32 operands (host arrays of k pointers / coefficients);
// out may alias an operand.  The multistep flow solvers (sampler.py) are built from this.
hipError_t launch_lincomb(const float* const* xs, const float* coef, int k, float* out, size_t n, hipStream_t stream);

// ---------------------------------------------------------------- MagCache ops (magcache_ops.hip)
// hipErrorInvalidValue, and nothing launched, for D % 8, ldx0 % 8, an fp32 leading dimension % 4, an x0 that is not 8-byte
// aligned or an fp32 pointer that is not 16-byte aligned (8-byte bf16 and 16-byte fp32 accesses), M * D/4 >= 2^31.
// out = x0 (bf16) + r (fp32)     -- the skipped-step path (reference :294-295)
hipError_t launch_skip_add(const bf16_t* x0, long ldx0, const float* r, long ldr, float* out, long ldo, int M,
                           int D, hipStream_t stream);
// r = x (fp32) - x0 (bf16)       -- residual capture (reference :299)
hipError_t launch_residual_sub(const float* x, long ldx, const bf16_t* x0, long ldx0, float* r, long ldr, int M,
                               int D, hipStream_t stream);
// calibration statistics (reference :167-169): per token rho = |r|/|rp|, cos; then
// stats[0]=mean(rho) stats[1]=std(rho, unbiased) stats[2]=mean(1-cos). partial = workspace of
// 4*n_blocks doubles; sums[4] (double) receives (sum rho, sum rho^2, sum (1-cos), count) for
// multi-rank reduction.  hipErrorInvalidValue, and nothing launched or written, for M < 2, D % 4, n_blocks < 1, a leading
// dimension that is shorter than D or no multiple of 4, r / rp not 16-byte aligned (the kernel reads 16 bytes at a time).
hipError_t launch_calib_stats(const float* r, long ldr, const float* rp, long ldrp, int M, int D, double* partial,
                              int n_blocks, double* sums, float* stats, hipStream_t stream);
hipError_t launch_calib_finalize(const double* sums, float* stats, hipStream_t stream);

}  // namespace mc
