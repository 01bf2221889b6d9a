// The single-op C entry points of include/magcache_hip.h (mc_op_*: one launcher of ops.h each, for callers that bring their
// own buffers -- the sampler, the parity tests, the A/B tools), mc_set_option, mc_last_error and mc_version.
#include <string>

#include "host.h"

using mc::bf16_t;
using mc::fail;

// operands and shape of a GEMM over the caller's buffers
static mc::GemmParams gp(const bf16_t* A, long lda, const bf16_t* W, long ldw, const float* bias, int M, int N, int K) {
  mc::GemmParams p;
  memset(&p, 0, sizeof(p));
  p.A = A; p.lda = lda; p.W = W; p.ldw = ldw; p.bias = bias; p.M = M; p.N = N; p.K = K;
  return p;
}

extern "C" {

const char* mc_last_error(void) { return mc::last_error(); }
const char* mc_version(void) { return "magcache_hip 0.8 (gfx950; 0.7.1 + token_timestep_sets + adapter_kinds)"; }

// split-K scratch of the single-op entry point (mc_op_set_splitk_workspace): the engines carry their own in their workspace
static float* g_op_splitk_ws = nullptr;
static size_t g_op_splitk_bytes = 0;

mc_status mc_op_gemm_bf16(const void* A, long lda, const void* W, long ldw, const float* bias, int M, int N, int K,
                          int epi, void* Cb, long ldc, float* X, long ldx, const float* gate, const void* X0,
                          long ldx0, float* R, long ldr, void* X0out, long ldx0out, int m_valid, mc_stream s) {
  mc::GemmParams p = gp((const bf16_t*)A, lda, (const bf16_t*)W, ldw, bias, M, N, K);
  p.Cb = (bf16_t*)Cb; p.ldc = ldc; p.X = X; p.ldx = ldx; p.gate = gate;
  p.X0 = (const bf16_t*)X0; p.ldx0 = ldx0; p.R = R; p.ldr = ldr;
  p.X0out = (bf16_t*)X0out; p.ldx0out = ldx0out; p.m_valid = m_valid;
  p.splitk_ws = g_op_splitk_ws; p.splitk_ws_bytes = g_op_splitk_bytes;
  hipError_t err = mc::launch_gemm_bf16(p, epi, (hipStream_t)s);
  if (err == hipErrorInvalidValue) return fail(MC_EINVAL, "gemm: unsupported shape M=%d N=%d K=%d epi=%d", M, N, K, epi);
  HIP_TRY(err);
  return MC_OK;
}

mc_status mc_op_gemm_bf16_resid_sel(const void* A, long lda, const void* W, long ldw, const float* bias, int M, int N, int K,
                                    int capture, float* X, long ldx, const float* gate, const float* gate2,
                                    const unsigned char* gate_sel, const void* X0, long ldx0, float* R, long ldr, mc_stream s) {
  mc::GemmParams p = gp((const bf16_t*)A, lda, (const bf16_t*)W, ldw, bias, M, N, K);
  p.X = X; p.ldx = ldx; p.gate = gate; p.gate2 = gate2; p.gate_sel = gate_sel;
  p.X0 = (const bf16_t*)X0; p.ldx0 = ldx0; p.R = R; p.ldr = ldr;
  if (!gate || !gate2 || !gate_sel) return fail(MC_EINVAL, "gemm (per-token gates): gate, gate2 and gate_sel are required");
  hipError_t err = mc::launch_gemm_bf16(p, capture ? mc::EPI_RESID_CAPTURE : mc::EPI_RESID_GATE, (hipStream_t)s);
  if (err == hipErrorInvalidValue) return fail(MC_EINVAL, "gemm (per-token gates): unsupported shape M=%d N=%d K=%d", M, N, K);
  HIP_TRY(err);
  return MC_OK;
}

mc_status mc_op_gemm_bf16_resid_sets(const void* A, long lda, const void* W, long ldw, const float* bias, int M, int N, int K,
                                     int capture, float* X, long ldx, const float* gates, long gate_stride, int n_sets,
                                     const unsigned char* sel, const void* X0, long ldx0, float* R, long ldr, mc_stream s) {
  mc::GemmParams p = gp((const bf16_t*)A, lda, (const bf16_t*)W, ldw, bias, M, N, K);
  p.X = X; p.ldx = ldx; p.gate = gates; p.gate_sel = sel; p.gate_stride = gate_stride; p.gate_sets = n_sets;
  p.X0 = (const bf16_t*)X0; p.ldx0 = ldx0; p.R = R; p.ldr = ldr;
  if (!mc::gemm_gate_table_ok(p))
    return fail(MC_EINVAL, "gemm (gate table): a table, a selector, n_sets 1..64 (%d) and gate_stride >= N, %% 4 == 0 (%ld) are required",
                n_sets, gate_stride);
  hipError_t err = mc::launch_gemm_bf16(p, capture ? mc::EPI_RESID_CAPTURE : mc::EPI_RESID_GATE, (hipStream_t)s);
  if (err == hipErrorInvalidValue) return fail(MC_EINVAL, "gemm (gate table): unsupported shape M=%d N=%d K=%d", M, N, K);
  HIP_TRY(err);
  return MC_OK;
}

mc_status mc_op_gemm_bf16_rowsplit(const void* A, long lda, const void* W, const void* W_b, long ldw, const float* bias,
                                   const float* bias_b, int M, int N, int K, int m_split, int epi, void* Cb, long ldc, float* X,
                                   long ldx, const float* gate, const float* gate_b, mc_stream s) {
  mc::GemmParams p = gp((const bf16_t*)A, lda, (const bf16_t*)W, ldw, bias, M, N, K);
  p.Cb = (bf16_t*)Cb; p.ldc = ldc; p.X = X; p.ldx = ldx; p.gate = gate;
  p.m_split = m_split; p.W_b = (const bf16_t*)W_b; p.bias_b = bias_b; p.gate_b = gate_b;
  p.splitk_ws = g_op_splitk_ws; p.splitk_ws_bytes = g_op_splitk_bytes;
  if (epi != mc::EPI_BF16 && epi != mc::EPI_GELU_BF16 && epi != mc::EPI_RESID_GATE)
    return fail(MC_EINVAL, "gemm (row split): epi %d (0 bf16, 1 gelu, 2 gated residual)", epi);
  hipError_t err = mc::launch_gemm_bf16(p, epi, (hipStream_t)s);
  if (err == hipErrorInvalidValue)
    return fail(MC_EINVAL, "gemm (row split): unsupported shape M=%d N=%d K=%d m_split=%d epi=%d", M, N, K, m_split, epi);
  HIP_TRY(err);
  return MC_OK;
}

mc_status mc_op_gemm_bf16_gelu_split(const void* A, long lda, const void* W, long ldw, const float* bias, int M, int N, int K,
                                     int n_split, void* Cb, long ldc, void* Cb2, long ldc2, mc_stream s) {
  mc::GemmParams p = gp((const bf16_t*)A, lda, (const bf16_t*)W, ldw, bias, M, N, K);
  p.Cb = (bf16_t*)Cb; p.ldc = ldc; p.n_split = n_split; p.Cb2 = (bf16_t*)Cb2; p.ldc2 = ldc2;
  hipError_t err = mc::launch_gemm_bf16(p, mc::EPI_BF16_GELU_SPLIT, (hipStream_t)s);
  if (err == hipErrorInvalidValue)
    return fail(MC_EINVAL, "gemm (bf16 | gelu split): unsupported shape M=%d N=%d K=%d n_split=%d", M, N, K, n_split);
  HIP_TRY(err);
  return MC_OK;
}

int mc_op_gemm_bf16_kernel(int M, int N, int K, int epi) {
  mc::GemmParams p = gp(nullptr, K, nullptr, K, nullptr, M, N, K);
  p.ldc = N; p.ldx = N;
  if (M <= 0 || N <= 0 || K <= 0 || (K % 64) != 0 || (N % 4) != 0) return 0;
  // the operands an epilogue form needs, as the engines pass them (never dereferenced here): the dispatch asks whether
  // gemm_bf16_v2 can run THIS form (gemm_bf16_v2_epi_ok), not only the shape
  alignas(16) static char dummy[16];
  if (epi == mc::EPI_RESID_CAPTURE) { p.X0 = (const bf16_t*)dummy; p.ldx0 = N; p.R = (float*)dummy; p.ldr = N; }
  if (epi == mc::EPI_BF16_GELU_SPLIT) { p.n_split = N > 256 ? (N / 2) / 256 * 256 : 0; p.Cb2 = (bf16_t*)dummy; p.ldc2 = N; }
  return mc::gemm_bf16_kernel_for(p, epi);
}

int mc_op_gemm_bf16_splitk(int M, int N, int K, int epi) {
  mc::GemmParams p = gp(nullptr, K, nullptr, K, nullptr, M, N, K);
  p.ldc = N; p.ldx = N;
  p.splitk_ws = g_op_splitk_ws; p.splitk_ws_bytes = g_op_splitk_bytes;
  if (M <= 0 || N <= 0 || K <= 0 || (mc::g_gemm_kernel != 0 && mc::g_gemm_kernel != 4)) return 1;
  return mc::gemm_splitk_slices(p, epi);
}

size_t mc_op_gemm_splitk_need(int M, int N, int K, int epi) { return mc::gemm_splitk_ws_need(M, N, K, epi); }

mc_status mc_op_set_splitk_workspace(void* ws_dev, size_t bytes) {
  g_op_splitk_ws = (float*)ws_dev;
  g_op_splitk_bytes = ws_dev ? bytes : 0;
  return MC_OK;
}

mc_status mc_op_attention(const void* Q, long ldq, const void* K, long ldk, long kss, const void* V, long ldv,
                          long vss, void* O, long ldo, int Lq_pad, int n_heads, int shard_rows, int shard_valid,
                          int n_shards, float scale, mc_stream s) {
  mc::AttnParams a;
  memset(&a, 0, sizeof(a));
  a.Q = (const bf16_t*)Q; a.ldq = ldq; a.K = (const bf16_t*)K; a.ldk = ldk; a.k_shard_stride = kss;
  a.V = (const bf16_t*)V; a.ldv = ldv; a.v_shard_stride = vss; a.O = (bf16_t*)O; a.ldo = ldo;
  a.Lq_pad = Lq_pad; a.n_heads = n_heads; a.shard_rows = shard_rows; a.shard_valid = shard_valid;
  a.n_shards = n_shards; a.scale = scale;
  hipError_t err = mc::launch_attention(a, (hipStream_t)s);
  if (err == hipErrorInvalidValue) return fail(MC_EINVAL, "attention: unsupported shape");
  HIP_TRY(err);
  return MC_OK;
}

mc_status mc_op_quantize_rows_fp8(const void* x, mc_dtype dtype, long ldx, int M, int K, void* q, long ldq, float* scale,
                                  mc_stream s) {
  hipError_t err = mc::launch_quantize_rows_fp8(dtype == MC_BF16 ? (const bf16_t*)x : nullptr,
                                                dtype == MC_F32 ? (const float*)x : nullptr, ldx, M, K, (uint8_t*)q, ldq,
                                                scale, (hipStream_t)s);
  if (err == hipErrorInvalidValue) return fail(MC_EINVAL, "quantize_rows_fp8: K, ldx, ldq must be multiples of 4");
  HIP_TRY(err);
  return MC_OK;
}

mc_status mc_op_gemm_fp8(const void* A, long lda, const float* a_scale, const void* W, long ldw, const float* w_scale,
                         const float* bias, int M, int N, int K, int epi, void* Cb, long ldc, float* X, long ldx,
                         const float* gate, mc_stream s) {
  mc::GemmParams p = gp((const bf16_t*)A, lda, (const bf16_t*)W, ldw, bias, M, N, K);
  p.a_scale = a_scale; p.w_scale = w_scale;
  p.Cb = (bf16_t*)Cb; p.ldc = ldc; p.X = X; p.ldx = ldx; p.gate = gate;
  hipError_t err = mc::launch_gemm_fp8(p, epi, (hipStream_t)s);
  if (err == hipErrorInvalidValue)
    return fail(MC_EINVAL, "gemm_fp8: needs N %% 256 == 0, K %% 256 == 0, K >= 512, lda/ldw %% 16 == 0, both scale vectors");
  HIP_TRY(err);
  return MC_OK;
}

// the three MX row quantisers and the three MX GEMMs of the C ABI: one body each, the format's own words in the refusal
static mc_status quantize_rows_mx_op(mc::MxFormat fmt, const char* refusal, const void* x, mc_dtype dtype, long ldx, int M, int K,
                                     void* q, long ldq, void* scales, long rows_pad, mc_stream s) {
  hipError_t err = mc::launch_quantize_rows_mx(fmt, dtype == MC_BF16 ? (const bf16_t*)x : nullptr,
                                               dtype == MC_F32 ? (const float*)x : nullptr, ldx, M, K, (uint8_t*)q, ldq,
                                               (uint8_t*)scales, rows_pad, (hipStream_t)s);
  if (err == hipErrorInvalidValue) return fail(MC_EINVAL, "%s", refusal);
  HIP_TRY(err);
  return MC_OK;
}

static mc_status gemm_mx_op(mc::MxFormat fmt, const char* refusal, const void* A, long lda, const void* a_scales, long rows_pad_a,
                            const void* W, long ldw, const void* w_scales, long rows_pad_w, const float* bias, int M, int N, int K,
                            int epi, void* Cb, long ldc, float* X, long ldx, const float* gate, mc_stream s) {
  mc::GemmParams p = gp((const bf16_t*)A, lda, (const bf16_t*)W, ldw, bias, M, N, K);
  p.a_mx = (const uint8_t*)a_scales; p.mx_rows_a = rows_pad_a; p.w_mx = (const uint8_t*)w_scales; p.mx_rows_w = rows_pad_w;
  p.Cb = (bf16_t*)Cb; p.ldc = ldc; p.X = X; p.ldx = ldx; p.gate = gate;
  hipError_t err = mc::launch_gemm_mx(fmt, p, epi, (hipStream_t)s);
  if (err == hipErrorInvalidValue) return fail(MC_EINVAL, "%s", refusal);
  HIP_TRY(err);
  return MC_OK;
}

mc_status mc_op_quantize_rows_mx(const void* x, mc_dtype dtype, long ldx, int M, int K, void* q, long ldq, void* scales,
                                 long rows_pad, mc_stream s) {
  return quantize_rows_mx_op(mc::MX_E4M3, "quantize_rows_mx: K % 32 == 0, ldx % 8 == 0, ldq % 16 == 0, rows_pad >= M", x, dtype, ldx, M, K,
                             q, ldq, scales, rows_pad, s);
}

mc_status mc_op_gemm_mxfp8(const void* A, long lda, const void* a_scales, long rows_pad_a, const void* W, long ldw,
                           const void* w_scales, long rows_pad_w, const float* bias, int M, int N, int K, int epi, void* Cb,
                           long ldc, float* X, long ldx, const float* gate, mc_stream s) {
  return gemm_mx_op(mc::MX_E4M3, "gemm_mxfp8: needs N % 256 == 0, K % 256 == 0, K >= 512, lda/ldw % 16 == 0, block scales with "
                                 "rows_pad_a >= M rounded up to 256, rows_pad_w >= N, both multiples of 4",
                    A, lda, a_scales, rows_pad_a, W, ldw, w_scales, rows_pad_w, bias, M, N, K, epi, Cb, ldc, X, ldx, gate, s);
}

mc_status mc_op_quantize_rows_mxfp4(const void* x, mc_dtype dtype, long ldx, int M, int K, void* q, long ldq, void* scales,
                                    long rows_pad, mc_stream s) {
  if (dtype != MC_BF16 && dtype != MC_F32) return fail(MC_EINVAL, "quantize_rows_mxfp4: x is bf16 or fp32");
  return quantize_rows_mx_op(mc::MX_E2M1, "quantize_rows_mxfp4: M, K > 0, K % 32 == 0, ldx % 8 == 0 and >= K, ldq (bytes) % 16 == 0 and >= K / 2, "
                                          "16-byte aligned pointers, rows_pad % 64 == 0 and >= M",
                             x, dtype, ldx, M, K, q, ldq, scales, rows_pad, s);
}

mc_status mc_op_gemm_mxfp4(const void* A, long lda, const void* a_scales, long rows_pad_a, const void* W, long ldw,
                           const void* w_scales, long rows_pad_w, const float* bias, int M, int N, int K, int epi, void* Cb,
                           long ldc, float* X, long ldx, const float* gate, mc_stream s) {
  const char* refusal = "gemm_mxfp4: needs M > 0, N % 256 == 0, K % 256 == 0 (elements), K >= 512, lda/ldw (bytes) % 16 == 0 and "
                        ">= K / 2, 16-byte aligned operands, block scales with rows_pad_a >= M rounded up to 256, rows_pad_w >= N, "
                        "both multiples of 64, epilogue 0, 1, 2 or 5 with its output";
  if (epi == mc::EPI_RESID_CAPTURE) return fail(MC_EINVAL, "%s", refusal);   // no X0 / R arguments here
  return gemm_mx_op(mc::MX_E2M1, refusal, A, lda, a_scales, rows_pad_a, W, ldw, w_scales, rows_pad_w, bias, M, N, K, epi, Cb, ldc, X, ldx, gate, s);
}

mc_status mc_op_quantize_rows_mxfp6(const void* x, mc_dtype dtype, long ldx, int M, int K, void* q, long ldq, void* scales,
                                    long rows_pad, mc_stream s) {
  if (dtype != MC_BF16 && dtype != MC_F32) return fail(MC_EINVAL, "quantize_rows_mxfp6: x is bf16 or fp32");
  return quantize_rows_mx_op(mc::MX_E2M3, "quantize_rows_mxfp6: M, K > 0, K % 32 == 0, ldx % 8 == 0 and >= K, ldq (bytes) % 16 == 0 and >= 3 K / 4, "
                                          "16-byte aligned pointers, rows_pad % 64 == 0 and >= M",
                             x, dtype, ldx, M, K, q, ldq, scales, rows_pad, s);
}

mc_status mc_op_gemm_mxfp6(const void* A, long lda, const void* a_scales, long rows_pad_a, const void* W, long ldw,
                           const void* w_scales, long rows_pad_w, const float* bias, int M, int N, int K, int epi, void* Cb,
                           long ldc, float* X, long ldx, const float* gate, mc_stream s) {
  const char* refusal = "gemm_mxfp6: needs M > 0, N % 256 == 0, K % 256 == 0 (elements), K >= 512, lda/ldw (bytes) % 16 == 0 and "
                        ">= 3 K / 4, 16-byte aligned operands, block scales with rows_pad_a >= M rounded up to 256, rows_pad_w >= N, "
                        "both multiples of 64, epilogue 0, 1, 2 or 5 with its output";
  if (epi == mc::EPI_RESID_CAPTURE) return fail(MC_EINVAL, "%s", refusal);   // no X0 / R arguments here
  return gemm_mx_op(mc::MX_E2M3, refusal, A, lda, a_scales, rows_pad_a, W, ldw, w_scales, rows_pad_w, bias, M, N, K, epi, Cb, ldc, X, ldx, gate, s);
}

mc_status mc_op_attention_partial(const void* Q, long ldq, const void* K, long ldk, long kss, const void* V, long ldv,
                                  long vss, void* O, long ldo, int Lq_pad, int n_heads, int shard_rows,
                                  int shard_valid, int n_shards, float scale, int skip_shard, float* lse_out,
                                  const float* lse_in, mc_stream s) {
  mc::AttnParams a;
  memset(&a, 0, sizeof(a));
  a.Q = (const bf16_t*)Q; a.ldq = ldq; a.K = (const bf16_t*)K; a.ldk = ldk; a.k_shard_stride = kss;
  a.V = (const bf16_t*)V; a.ldv = ldv; a.v_shard_stride = vss; a.O = (bf16_t*)O; a.ldo = ldo;
  a.Lq_pad = Lq_pad; a.n_heads = n_heads; a.shard_rows = shard_rows; a.shard_valid = shard_valid;
  a.n_shards = n_shards; a.scale = scale;
  a.skip_shard_p1 = skip_shard >= 0 ? skip_shard + 1 : 0; a.lse_out = lse_out; a.lse_in = lse_in;
  hipError_t err = mc::launch_attention(a, (hipStream_t)s);
  if (err == hipErrorInvalidValue) return fail(MC_EINVAL, "attention: unsupported shape / shard selection");
  HIP_TRY(err);
  return MC_OK;
}

mc_status mc_op_attn_merge(const void* const* o_parts, const float* const* lse_parts, int n, void* out, long ldo, int rows,
                           int rows_pad, int d, mc_stream s) {
  if (!o_parts || !lse_parts || !out) return fail(MC_EINVAL, "attn_merge: null argument");
  hipError_t err = mc::launch_attn_merge((const bf16_t* const*)o_parts, lse_parts, n, (bf16_t*)out, ldo, rows, rows_pad, d,
                                         (hipStream_t)s);
  if (err == hipErrorInvalidValue) return fail(MC_EINVAL, "attn_merge: 1..9 parts, d a multiple of 128, 16-byte rows");
  HIP_TRY(err);
  return MC_OK;
}

mc_status mc_op_ln_modulate(const float* x, long ldx, const void* x0, long ldx0, const float* sc, const float* sh,
                            int mode, float eps, void* out, long ldo, float* out_f32, long ldof, int M, int D,
                            mc_stream s) {
  hipError_t err = mc::launch_ln_modulate(x, ldx, (const bf16_t*)x0, ldx0, sc, sh, mode, eps, (bf16_t*)out, ldo,
                                          out_f32, ldof, M, D, (hipStream_t)s);
  if (err == hipErrorInvalidValue) return fail(MC_EINVAL, "ln_modulate: unsupported D=%d", D);
  HIP_TRY(err);
  return MC_OK;
}

mc_status mc_op_rmsnorm_rope(void* x, long ldx, const float* w, float eps, const float* cs, int cs_row0, int M, int D,
                             mc_stream s) {
  hipError_t err = mc::launch_rmsnorm_rope((bf16_t*)x, ldx, w, eps, cs, cs_row0, M, D, (hipStream_t)s);
  if (err == hipErrorInvalidValue) return fail(MC_EINVAL, "rmsnorm_rope: unsupported D=%d", D);
  HIP_TRY(err);
  return MC_OK;
}

mc_status mc_op_skip_add(const void* x0, long ldx0, const float* r, long ldr, float* out, long ldo, int M, int D,
                         mc_stream s) {
  hipError_t err = mc::launch_skip_add((const bf16_t*)x0, ldx0, r, ldr, out, ldo, M, D, (hipStream_t)s);
  if (err == hipErrorInvalidValue) return fail(MC_EINVAL, "skip_add: needs D %% 8 == 0, ldx0 %% 8 == 0, ldr/ldo %% 4 == 0, x0 8-byte and r/out 16-byte aligned");
  HIP_TRY(err);
  return MC_OK;
}

mc_status mc_op_residual_sub(const float* x, long ldx, const void* x0, long ldx0, float* r, long ldr, int M, int D,
                             mc_stream s) {
  hipError_t err = mc::launch_residual_sub(x, ldx, (const bf16_t*)x0, ldx0, r, ldr, M, D, (hipStream_t)s);
  if (err == hipErrorInvalidValue) return fail(MC_EINVAL, "residual_sub: needs D %% 8 == 0, ldx0 %% 8 == 0, ldx/ldr %% 4 == 0, x0 8-byte and x/r 16-byte aligned");
  HIP_TRY(err);
  return MC_OK;
}

mc_status mc_op_calib_stats(const float* r, long ldr, const float* rp, long ldrp, int M, int D, double* partial,
                            int n_blocks, double* sums, float* stats, mc_stream s) {
  hipError_t err = mc::launch_calib_stats(r, ldr, rp, ldrp, M, D, partial, n_blocks, sums, stats, (hipStream_t)s);
  if (err == hipErrorInvalidValue) return fail(MC_EINVAL, "calib_stats: needs M >= 2, D %% 4 == 0, n_blocks >= 1, ldr/ldrp >= D and %% 4 == 0, r/rp 16-byte aligned");
  HIP_TRY(err);
  return MC_OK;
}

mc_status mc_op_cfg_euler(const float* cond, const float* uncond, float guide, float dt, float* x, float* eps_out,
                          size_t n, mc_stream s) {
  HIP_TRY(mc::launch_cfg_euler(cond, uncond, guide, dt, x, eps_out, n, (hipStream_t)s));
  return MC_OK;
}

mc_status mc_op_cfg_norm_euler(const float* cond, const float* uncond, long ld_pred, float guide, float dt, float* x, long ldx,
                               int n_rows, int C, mc_stream s) {
  if (!cond || !uncond || !x) return fail(MC_EINVAL, "null argument");
  hipError_t err = mc::launch_cfg_norm_euler(cond, uncond, ld_pred, guide, dt, x, ldx, n_rows, C, (hipStream_t)s);
  if (err == hipErrorInvalidValue) return fail(MC_EINVAL, "cfg_norm_euler: 0 < C <= 256, ld_pred / ldx >= C, n_rows >= 0");
  HIP_TRY(err);
  return MC_OK;
}

mc_status mc_op_rmsnorm_rows_bf16(const float* x, long ldx, const float* w, float eps, void* out, long ldo, int rows_valid,
                                  int rows, int D, mc_stream s) {
  if (!x || !w || !out) return fail(MC_EINVAL, "null argument");
  hipError_t err = mc::launch_rmsnorm_rows_bf16(x, ldx, w, eps, (bf16_t*)out, ldo, rows_valid, rows, D, (hipStream_t)s);
  if (err == hipErrorInvalidValue) return fail(MC_EINVAL, "rmsnorm_rows_bf16: D, ldx, ldo multiples of 4, 0 <= rows_valid <= rows");
  HIP_TRY(err);
  return MC_OK;
}

mc_status mc_op_lincomb(const float* const* xs_dev, const float* coef, int k, float* out_dev, size_t n, mc_stream s) {
  if (!xs_dev || !coef) return fail(MC_EINVAL, "null argument");
  hipError_t err = mc::launch_lincomb(xs_dev, coef, k, out_dev, n, (hipStream_t)s);
  if (err == hipErrorInvalidValue) return fail(MC_EINVAL, "lincomb: 1..6 operands, non-empty output");
  HIP_TRY(err);
  return MC_OK;
}

mc_status mc_op_rope_expand(const float* axes_dev, int F, int Hp, int Wp, int tok0, int n_tok, int n_rows, float* cs_dev,
                            mc_stream stream) {
  hipError_t err = mc::launch_rope_expand(axes_dev, F, Hp, Wp, tok0, n_tok, n_rows, cs_dev, (hipStream_t)stream);
  if (err == hipErrorInvalidValue)
    return fail(MC_EINVAL, "rope_expand: non-null pointers, positive F / Hp / Wp / n_tok / n_rows, tok0 >= 0, n_tok <= n_rows, cs_dev 16-byte aligned");
  HIP_TRY(err);
  return MC_OK;
}

mc_status mc_op_add_rows(float* x, long ldx, const void* s, mc_dtype s_dtype, float* r, long ldr, const void* x0, long ldx0,
                         int rows, int D, mc_stream stream) {
  if (s_dtype != MC_F32 && s_dtype != MC_BF16) return fail(MC_EINVAL, "add_rows: the sample is fp32 or bf16");
  hipError_t err = mc::launch_add_rows(x, ldx, s, s_dtype == MC_BF16, r, ldr, (const bf16_t*)x0, ldx0, rows, D, (hipStream_t)stream);
  if (err == hipErrorInvalidValue)
    return fail(MC_EINVAL, "add_rows: D a multiple of 8, 16-byte aligned pointers, ldx / ldr >= D multiples of 4, ldx0 of 8, x0 needs r");
  HIP_TRY(err);
  return MC_OK;
}

mc_status mc_op_ip_attention(const void* q, long ldq, const float* wq, float eps, const mc_ip_keys* adapters, int n_adapters,
                             void* out, long ldo, int rows, int heads, mc_stream stream) {
  mc::IpKeys keys[mc::kIpMaxAdapters] = {};
  static_assert(mc::kIpMaxAdapters == MC_IP_MAX_ADAPTERS && mc::kIpMaxKeys == MC_IP_MAX_KEYS, "header and kernel limits");
  hipError_t err = hipErrorInvalidValue;
  if (adapters && n_adapters >= 1 && n_adapters <= mc::kIpMaxAdapters) {
    for (int j = 0; j < n_adapters; ++j) keys[j] = {(const bf16_t*)adapters[j].kv, adapters[j].ld, adapters[j].valid, adapters[j].scale};
    err = mc::launch_ip_attention((const bf16_t*)q, ldq, wq, eps, keys, n_adapters, (bf16_t*)out, ldo, rows, heads, (hipStream_t)stream);
  }
  if (err == hipErrorInvalidValue)
    return fail(MC_EINVAL, "ip_attention: 1..%d adapters of 1..%d keys, rows >= 1, 16-byte aligned pointers, ldq / ldo >= heads * 128 and "
                           "ld >= 2 * heads * 128, all multiples of 8", mc::kIpMaxAdapters, mc::kIpMaxKeys);
  HIP_TRY(err);
  return MC_OK;
}

// One low-rank pair of a merge op in scratch memory: the packed bf16 copies of up [rows, rank] and down [rank, K] the kernels
// read (ops.h: launch_lora_pack), each from a 256-byte boundary.  Advances *off by the bytes of both; ws != null: packs them at
// ws + *off first and writes the kernel's term.
static hipError_t pack_pair(const void* down, const void* up, int rank, float scale, int rows, int K, char* ws, size_t* off,
                            mc::LoraTerm* term, hipStream_t stream) {
  const int rank_pad = (int)mc::align_up(rank, mc::kLoraRankStep);
  const size_t up_bytes = mc::align_up(mc::lora_packed_elems(rows, rank_pad) * 2, 256), at = *off;
  *off += up_bytes + mc::align_up(mc::lora_packed_elems(K, rank_pad) * 2, 256);
  if (!ws) return hipSuccess;
  *term = mc::LoraTerm{(bf16_t*)(ws + at), (bf16_t*)(ws + at + up_bytes), rank_pad, scale};
  hipError_t err = mc::launch_lora_pack(up, 0, rank, 1, rows, rank, rank_pad, (bf16_t*)(ws + at), stream);
  if (err == hipSuccess) err = mc::launch_lora_pack(down, 0, 1, K, K, rank, rank_pad, (bf16_t*)(ws + at + up_bytes), stream);
  return err;
}

size_t mc_op_lora_merge_scratch(int rows, int K, const mc_lora_term* terms, int n_terms) {
  size_t bytes = 0;
  for (int j = 0; terms && j < n_terms; ++j) {
    if (terms[j].rank < 1 || rows < 1 || K < 1) return 0;
    (void)pack_pair(nullptr, nullptr, terms[j].rank, 0.f, rows, K, nullptr, &bytes, nullptr, nullptr);   // sizes only
  }
  return bytes;
}

// both element widths of the merge: kAlign = elements of a 16-byte vector (8 bf16, 4 fp32)
static mc_status op_lora_merge(bool f32, const void* base, long ld_base, void* out, long ld_out, int rows, int K,
                               const mc_lora_term* terms, int n_terms, void* scratch, size_t scratch_bytes, mc_stream s) {
  hipStream_t stream = (hipStream_t)s;
  const int kAlign = f32 ? 4 : 8;
  if (!base || !out || rows <= 0 || K <= 0 || n_terms < 0 || (n_terms > 0 && !terms)) return fail(MC_EINVAL, "lora_merge: null or empty operand");
  if (n_terms > MC_LORA_MAX_TERMS) return fail(MC_EINVAL, "lora_merge: %d terms, at most %d", n_terms, MC_LORA_MAX_TERMS);
  for (int j = 0; j < n_terms; ++j)
    if (!terms[j].down || !terms[j].up || terms[j].rank < 1) return fail(MC_EINVAL, "lora_merge: term %d has rank %d or a null matrix", j, terms[j].rank);
  if ((K % kAlign) != 0 || ld_base < K || ld_out < K || (ld_base % kAlign) != 0 || (ld_out % kAlign) != 0 || (((uintptr_t)base | (uintptr_t)out) & 15))
    return fail(MC_EINVAL, "lora_merge: K and the pitches are multiples of %d, pitch >= K, base and out 16-byte aligned", kAlign);
  const size_t need = mc_op_lora_merge_scratch(rows, K, terms, n_terms);
  char* ws = (char*)scratch;
  if (ws && (scratch_bytes < need || ((uintptr_t)ws & 255)))
    return fail(MC_EINVAL, "lora_merge: scratch of %zu bytes, %zu needed, 256-byte aligned", scratch_bytes, need);
  bool own = false;
  if (!ws && need) {
    hipError_t err = hipMalloc((void**)&ws, need);
    if (err != hipSuccess) return fail(MC_ENOMEM, "hipMalloc(%zu) failed: %s", need, hipGetErrorString(err));
    own = true;
  }
  mc::LoraTerm t[MC_LORA_MAX_TERMS];
  hipError_t err = hipSuccess;
  size_t off = 0;
  for (int j = 0; j < n_terms && err == hipSuccess; ++j)
    err = pack_pair(terms[j].down, terms[j].up, terms[j].rank, terms[j].scale, rows, K, ws, &off, &t[j], stream);
  if (err == hipSuccess)
    err = f32 ? mc::launch_lora_merge_f32((const float*)base, ld_base, (float*)out, ld_out, rows, K, t, n_terms, stream)
              : mc::launch_lora_merge((const bf16_t*)base, ld_base, (bf16_t*)out, ld_out, rows, K, t, n_terms, stream);
  if (own) {
    if (err == hipSuccess) err = hipStreamSynchronize(stream);
    (void)hipFree(ws);
  }
  HIP_TRY(err);
  return MC_OK;
}

mc_status mc_op_lora_merge(const void* base, long ld_base, void* out, long ld_out, int rows, int K, const mc_lora_term* terms,
                           int n_terms, void* scratch, size_t scratch_bytes, mc_stream s) {
  return op_lora_merge(false, base, ld_base, out, ld_out, rows, K, terms, n_terms, scratch, scratch_bytes, s);
}

mc_status mc_op_lora_merge_f32(const float* base, long ld_base, float* out, long ld_out, int rows, int K, const mc_lora_term* terms,
                               int n_terms, void* scratch, size_t scratch_bytes, mc_stream s) {
  return op_lora_merge(true, base, ld_base, out, ld_out, rows, K, terms, n_terms, scratch, scratch_bytes, s);
}

// the fp32 image of the part first, then the packed copies of the pairs in term order
size_t mc_op_adapter_merge_scratch(int rows, int K, const mc_adapter_term* terms, int n_terms) {
  if (rows < 1 || K < 1) return 0;
  size_t bytes = mc::align_up((size_t)rows * (size_t)K * sizeof(float), 256);
  for (int j = 0; terms && j < n_terms; ++j) {
    if (terms[j].kind != MC_ADAPTER_PAIR) continue;
    if (terms[j].rank < 1) return 0;
    (void)pack_pair(nullptr, nullptr, terms[j].rank, 0.f, rows, K, nullptr, &bytes, nullptr, nullptr);   // sizes only
  }
  return bytes;
}

mc_status mc_op_adapter_merge(const void* base, long ld_base, void* out, long ld_out, int rows, int K, const mc_adapter_term* terms,
                              int n_terms, const float* magnitude, void* scratch, size_t scratch_bytes, mc_stream s) {
  hipStream_t stream = (hipStream_t)s;
  static_assert(mc::kLoraMaxTerms == MC_LORA_MAX_TERMS, "header and kernel limits");
  if (!base || !out || rows <= 0 || K <= 0 || n_terms < 0 || (n_terms > 0 && !terms)) return fail(MC_EINVAL, "adapter_merge: null or empty operand");
  if (n_terms > MC_LORA_MAX_TERMS) return fail(MC_EINVAL, "adapter_merge: %d terms, at most %d", n_terms, MC_LORA_MAX_TERMS);
  for (int j = 0; j < n_terms; ++j) {
    const mc_adapter_term& t = terms[j];
    if (t.kind == MC_ADAPTER_PAIR) {
      if (!t.a || !t.b || t.rank < 1) return fail(MC_EINVAL, "adapter_merge: term %d (pair) has rank %d or a null matrix", j, t.rank);
    } else if (t.kind == MC_ADAPTER_KRON) {
      if (!t.a || !t.b || t.r1 < 1 || t.c1 < 1 || t.r2 < 1 || t.c2 < 1 || (long)t.r1 * t.r2 != rows || (long)t.c1 * t.c2 != K)
        return fail(MC_EINVAL, "adapter_merge: term %d: [%d, %d] (x) [%d, %d] is no factorisation of [%d, %d], or a null factor", j, t.r1,
                    t.c1, t.r2, t.c2, rows, K);
    } else if (t.kind == MC_ADAPTER_HADA) {
      if (!t.a || !t.b || !t.c || !t.d || t.rank < 1) return fail(MC_EINVAL, "adapter_merge: term %d (hada) has rank %d or a null matrix", j, t.rank);
    } else {
      return fail(MC_EINVAL, "adapter_merge: term %d has the unknown kind %d", j, t.kind);
    }
    if (t.kind != MC_ADAPTER_PAIR && (((uintptr_t)t.a | (uintptr_t)t.b | (uintptr_t)t.c | (uintptr_t)t.d) & 3))
      return fail(MC_EINVAL, "adapter_merge: term %d: fp32 factors are 4-byte aligned", j);
  }
  if ((uintptr_t)magnitude & 3) return fail(MC_EINVAL, "adapter_merge: the magnitude is 4-byte aligned");
  if ((K % 8) != 0 || ld_base < K || ld_out < K || (ld_base % 8) != 0 || (ld_out % 8) != 0 || (((uintptr_t)base | (uintptr_t)out) & 15))
    return fail(MC_EINVAL, "adapter_merge: K and the pitches are multiples of 8, pitch >= K, base and out 16-byte aligned");
  const size_t need = mc_op_adapter_merge_scratch(rows, K, terms, n_terms);
  char* ws = (char*)scratch;
  if (ws && (scratch_bytes < need || ((uintptr_t)ws & 255)))
    return fail(MC_EINVAL, "adapter_merge: scratch of %zu bytes, %zu needed, 256-byte aligned", scratch_bytes, need);
  bool own = false;
  if (!ws) {
    hipError_t err = hipMalloc((void**)&ws, need);
    if (err != hipSuccess) return fail(MC_ENOMEM, "hipMalloc(%zu) failed: %s", need, hipGetErrorString(err));
    own = true;
  }
  mc::LoraTerm pairs[MC_LORA_MAX_TERMS];
  mc::KronTerm krons[MC_LORA_MAX_TERMS];
  mc::HadaTerm hadas[MC_LORA_MAX_TERMS];
  int np = 0, nk = 0, nh = 0;
  hipError_t err = hipSuccess;
  size_t off = mc::align_up((size_t)rows * (size_t)K * sizeof(float), 256);
  for (int j = 0; j < n_terms && err == hipSuccess; ++j) {
    const mc_adapter_term& t = terms[j];
    if (t.kind == MC_ADAPTER_KRON) {
      krons[nk++] = mc::KronTerm{(const float*)t.a, (const float*)t.b, t.r1, t.c1, t.r2, t.c2, t.scale};
    } else if (t.kind == MC_ADAPTER_HADA) {
      hadas[nh++] = mc::HadaTerm{(const float*)t.a, (const float*)t.b, (const float*)t.c, (const float*)t.d, t.rank, t.scale};
    } else {   // a = down [rank, K], b = up [rows, rank], bf16
      err = pack_pair(t.a, t.b, t.rank, t.scale, rows, K, ws, &off, &pairs[np++], stream);
    }
  }
  if (err == hipSuccess)
    err = mc::launch_adapter_merge((const bf16_t*)base, ld_base, (bf16_t*)out, ld_out, rows, K, pairs, np, krons, nk, hadas, nh, magnitude,
                                   (float*)ws, stream);
  if (own) {
    if (err == hipSuccess) err = hipStreamSynchronize(stream);
    (void)hipFree(ws);
  }
  if (err == hipErrorInvalidValue) return fail(MC_EINVAL, "adapter_merge: a misaligned operand (factors and magnitude 4-byte, pairs 16-byte aligned)");
  HIP_TRY(err);
  return MC_OK;
}

mc_status mc_op_param_delta(const float* base, float* out, size_t n, const float* const* deltas, const float* scales, int n_terms,
                            mc_stream s) {
  if (!base || !out || n == 0 || !deltas || !scales) return fail(MC_EINVAL, "param_delta: null or empty operand");
  if (n_terms < 1 || n_terms > MC_LORA_MAX_TERMS) return fail(MC_EINVAL, "param_delta: %d terms, 1 to %d", n_terms, MC_LORA_MAX_TERMS);
  for (int j = 0; j < n_terms; ++j)
    if (!deltas[j] || ((uintptr_t)deltas[j] & 3)) return fail(MC_EINVAL, "param_delta: delta %d is null or not 4-byte aligned", j);
  if (((uintptr_t)base | (uintptr_t)out) & 3) return fail(MC_EINVAL, "param_delta: base and out are 4-byte aligned");
  HIP_TRY(mc::launch_param_delta(base, out, n, deltas, scales, n_terms, (hipStream_t)s));
  return MC_OK;
}

mc_status mc_op_cast_bf16(const float* src, void* dst, size_t n, mc_stream s) {
  HIP_TRY(mc::launch_cast_bf16(src, (bf16_t*)dst, n, (hipStream_t)s));
  return MC_OK;
}

mc_status mc_set_option(const char* key, int value) {
  if (!key) return fail(MC_EINVAL, "null key");
  const std::string k(key);
  if (k == "gemm_kernel") {
    if ((value < 0 || value > 2) && value != 4)
      return fail(MC_EINVAL, "gemm_kernel must be 0 (by shape), 1 (128x128), 2 (256x256, 8 waves) or 4 (256x256, 4 waves, generated stream)");
    if (value == 2 && !mc::gemm_bf16_big_linked())
      return fail(MC_EINVAL, "gemm_kernel 2: the 8-wave reference kernel is not in this library (round 6: it lives in the "
                             "test-only libmagcache_hip_ref.so, magcache_amd.build.build_ref())");
    mc::g_gemm_kernel = value;
  } else if (k == "sp_attn_partials") {
    if (value < 0 || value > 2)
      return fail(MC_EINVAL, "sp_attn_partials must be 0 (chain on one stream), 1 (independent launches on two streams + merge where a launch "
                             "does not fill the chip in whole waves) or 2 (always)");
    mc::g_sp_attn_partials = value;
  } else if (k == "gemm_splitk") {
    if (value < 0 || value > 16) return fail(MC_EINVAL, "gemm_splitk must be 0 (never), 1 (by shape) or 2..16 (that many K slices wherever valid)");
    mc::g_gemm_splitk = value;
  } else if (k == "gemm_v2_max_grid") {
    if (value < 0 || value > 4096) return fail(MC_EINVAL, "gemm_v2_max_grid must be 0 (= the CUs) or a workgroup count");
    mc::g_gemm_v2_max_grid = value;
  } else if (k == "gemm_defer") {
    if (value != 0 && value != 1) return fail(MC_EINVAL, "gemm_defer must be 0 (residual epilogues in place) or 1 (deferred into the next tile's main loop)");
    mc::g_gemm_defer = value;
  } else if (k == "fp8_fused_quant") {
    if (value != 0 && value != 1) return fail(MC_EINVAL, "fp8_fused_quant must be 0 (separate quantise passes) or 1 (fused into the producers)");
    mc::g_fp8_fused_quant = value;
  } else if (k == "mx_fp4") {
    if (value != 0 && value != 1) return fail(MC_EINVAL, "mx_fp4 must be 0 (MX fp8 Linears) or 1 (MXFP4 Linears where fp8_linear is 2 or 3; read when an engine is created)");
    mc::g_mx_fp4 = value;
  } else if (k == "mx_fp6") {
    if (value != 0 && value != 1) return fail(MC_EINVAL, "mx_fp6 must be 0 (MX fp8 Linears) or 1 (MXFP6 Linears where fp8_linear is 2 or 3; read when an engine is created)");
    mc::g_mx_fp6 = value;
  } else if (k == "attn_kernel") {
    if (value != 0 && value != 3 && value != 5)
      return fail(MC_EINVAL, "attn_kernel must be 0 (default), 3 (8 waves x 32 rows) or 5 (4 waves x 64 rows, hand-scheduled)");
    mc::g_attn_kernel = value;
  } else if (k == "mmdit_two_streams") {
    if (value < -1 || value > 6) return fail(MC_EINVAL, "mmdit_two_streams must be -1 (by shape), 0, 1 or a diagnostic mode 2..6");
    mc::g_mmdit_two_streams = value;
  } else {
    return fail(MC_EINVAL, "unknown option '%s'", key);
  }
  return MC_OK;
}

mc_status mc_get_option(const char* key, int* value) {
  if (!key || !value) return fail(MC_EINVAL, "null argument");
  const std::string k(key);
  if (k == "gemm_kernel") *value = mc::g_gemm_kernel;
  else if (k == "sp_attn_partials") *value = mc::g_sp_attn_partials;
  else if (k == "gemm_splitk") *value = mc::g_gemm_splitk;
  else if (k == "gemm_v2_max_grid") *value = mc::g_gemm_v2_max_grid;
  else if (k == "gemm_defer") *value = mc::g_gemm_defer;
  else if (k == "fp8_fused_quant") *value = mc::g_fp8_fused_quant;
  else if (k == "mx_fp4") *value = mc::g_mx_fp4;
  else if (k == "mx_fp6") *value = mc::g_mx_fp6;
  else if (k == "attn_kernel") *value = mc::g_attn_kernel;
  else if (k == "mmdit_two_streams") *value = mc::g_mmdit_two_streams;
  else return fail(MC_EINVAL, "unknown option '%s'", key);
  return MC_OK;
}

}  // extern "C"
