// Test-only entry points (mc_test_*) to the launchers of ops.h that the shipped C ABI has no single-op call for.  Linked
// ONLY into tests/_ref/libmagcache_hip_ref.so (magcache_amd/build.py: REF_EXTRA) -- libmagcache_hip.so does not contain this
// file and include/*.h do not declare it.  Every wrapper passes its arguments through unchanged and returns the launcher's
// hipError_t as an int (hipSuccess = 0, hipErrorInvalidValue = 1): no logic lives here, so what the tests exercise is the
// launcher's own host checks and the kernel objects (elementwise.hip.o, gemm_mxfp8.hip.o, gemm_fp8_big.hip.o,
// magcache_ops.hip.o) the shipped library links too.
#include "ops.h"

using mc::bf16_t;

extern "C" {

int mc_test_headnorm_rope(void* x, long ldx, long k_col0, const float* wq, const float* wk, float eps, const float* cs,
                          int cs_row0, int M, int n_heads, void* s) {
  return (int)mc::launch_headnorm_rope((bf16_t*)x, ldx, k_col0, wq, wk, eps, cs, cs_row0, M, n_heads, (hipStream_t)s);
}

int mc_test_ip_qnorm(const void* q, long ldq, const float* wq, float eps, void* out, long ldo, int rows, int heads, void* s) {
  return (int)mc::launch_ip_attention_qnorm((const bf16_t*)q, ldq, wq, eps, (bf16_t*)out, ldo, rows, heads, (hipStream_t)s);
}

int mc_test_gemv_bf16w(const void* W, const float* x, const float* b, float* y, int N, int K, int act_in, int act_out,
                       int accumulate, void* s) {
  return (int)mc::launch_gemv_bf16w((const bf16_t*)W, x, b, y, N, K, act_in, act_out, accumulate, (hipStream_t)s);
}

int mc_test_gemv_f32(const float* W, const float* x, const float* b, float* y, int N, int K, int act_in, int act_out, void* s) {
  return (int)mc::launch_gemv_f32(W, x, b, y, N, K, act_in, act_out, (hipStream_t)s);
}

int mc_test_head_linear(const float* xn, long ldx, const float* W, const float* b, float* out, long ldo, int M, int N, int K,
                        void* s) {
  return (int)mc::launch_head_linear(xn, ldx, W, b, out, ldo, M, N, K, (hipStream_t)s);
}

int mc_test_ln_modulate(const float* x, long ldx, const void* x0, long ldx0, const float* sc, const float* sh, int mode,
                        float eps, void* out, long ldo, float* out_f32, long ldof, int M, int D, const float* sc2,
                        const float* sh2, const unsigned char* sel, void* s) {
  return (int)mc::launch_ln_modulate(x, ldx, (const bf16_t*)x0, ldx0, sc, sh, mode, eps, (bf16_t*)out, ldo, out_f32, ldof, M, D,
                                     (hipStream_t)s, sc2, sh2, sel);
}

int mc_test_ln_modulate_fp8(const float* x, long ldx, const float* sc, const float* sh, int mode, float eps, unsigned char* q,
                            long ldq, float* row_scale, unsigned char* mx, long mx_rows, int M, int D, const float* sc2,
                            const float* sh2, const unsigned char* sel, void* s) {
  return (int)mc::launch_ln_modulate_fp8(x, ldx, sc, sh, mode, eps, q, ldq, row_scale, mx, mx_rows, M, D, (hipStream_t)s, sc2,
                                         sh2, sel);
}

// EPI_GELU_MXFP8: the one epilogue of launch_gemm_mxfp8 that mc_op_gemm_mxfp8 cannot name (it has no Cq / c_mx arguments)
int mc_test_gemm_mxfp8_gelu_quant(const void* A, long lda, const void* a_mx, long mx_rows_a, const void* W, long ldw,
                                  const void* w_mx, long mx_rows_w, const float* bias, int M, int N, int K, void* Cq, long ldcq,
                                  void* c_mx, long mx_rows_c, void* s) {
  mc::GemmParams p = {};
  p.A = (const bf16_t*)A; p.lda = lda; p.W = (const bf16_t*)W; p.ldw = ldw; p.bias = bias;
  p.M = M; p.N = N; p.K = K;
  p.a_mx = (const uint8_t*)a_mx; p.mx_rows_a = mx_rows_a; p.w_mx = (const uint8_t*)w_mx; p.mx_rows_w = mx_rows_w;
  p.Cq = (uint8_t*)Cq; p.ldcq = ldcq; p.c_mx = (uint8_t*)c_mx; p.mx_rows_c = mx_rows_c;
  return (int)mc::launch_gemm_mxfp8(p, mc::EPI_GELU_MXFP8, (hipStream_t)s);
}

// EPI_RESID_CAPTURE of launch_gemm_mxfp8: mc_op_gemm_mxfp8 has no X0 / R arguments
int mc_test_gemm_mxfp8_capture(const void* A, long lda, const void* a_mx, long mx_rows_a, const void* W, long ldw,
                               const void* w_mx, long mx_rows_w, const float* bias, int M, int N, int K, float* X, long ldx,
                               const float* gate, const void* X0, long ldx0, float* R, long ldr, void* s) {
  mc::GemmParams p = {};
  p.A = (const bf16_t*)A; p.lda = lda; p.W = (const bf16_t*)W; p.ldw = ldw; p.bias = bias;
  p.M = M; p.N = N; p.K = K;
  p.a_mx = (const uint8_t*)a_mx; p.mx_rows_a = mx_rows_a; p.w_mx = (const uint8_t*)w_mx; p.mx_rows_w = mx_rows_w;
  p.X = X; p.ldx = ldx; p.gate = gate; p.X0 = (const bf16_t*)X0; p.ldx0 = ldx0; p.R = R; p.ldr = ldr;
  return (int)mc::launch_gemm_mxfp8(p, mc::EPI_RESID_CAPTURE, (hipStream_t)s);
}

int mc_test_ln_modulate_mxfp4(const float* x, long ldx, const float* sc, const float* sh, int mode, float eps, unsigned char* q,
                              long ldq, unsigned char* mx, long mx_rows, int M, int D, const float* sc2, const float* sh2,
                              const unsigned char* sel, void* s) {
  return (int)mc::launch_ln_modulate_mxfp4(x, ldx, sc, sh, mode, eps, q, ldq, mx, mx_rows, M, D, (hipStream_t)s, sc2, sh2, sel);
}

// EPI_GELU_MXFP4: the one epilogue of launch_gemm_mxfp4 that mc_op_gemm_mxfp4 cannot name (it has no Cq / c_mx arguments)
int mc_test_gemm_mxfp4_gelu_quant(const void* A, long lda, const void* a_mx, long mx_rows_a, const void* W, long ldw,
                                  const void* w_mx, long mx_rows_w, const float* bias, int M, int N, int K, void* Cq, long ldcq,
                                  void* c_mx, long mx_rows_c, void* s) {
  mc::GemmParams p = {};
  p.A = (const bf16_t*)A; p.lda = lda; p.W = (const bf16_t*)W; p.ldw = ldw; p.bias = bias;
  p.M = M; p.N = N; p.K = K;
  p.a_mx = (const uint8_t*)a_mx; p.mx_rows_a = mx_rows_a; p.w_mx = (const uint8_t*)w_mx; p.mx_rows_w = mx_rows_w;
  p.Cq = (uint8_t*)Cq; p.ldcq = ldcq; p.c_mx = (uint8_t*)c_mx; p.mx_rows_c = mx_rows_c;
  return (int)mc::launch_gemm_mxfp4(p, mc::EPI_GELU_MXFP4, (hipStream_t)s);
}

// EPI_RESID_CAPTURE of launch_gemm_mxfp4: mc_op_gemm_mxfp4 has no X0 / R arguments
int mc_test_gemm_mxfp4_capture(const void* A, long lda, const void* a_mx, long mx_rows_a, const void* W, long ldw,
                               const void* w_mx, long mx_rows_w, const float* bias, int M, int N, int K, float* X, long ldx,
                               const float* gate, const void* X0, long ldx0, float* R, long ldr, void* s) {
  mc::GemmParams p = {};
  p.A = (const bf16_t*)A; p.lda = lda; p.W = (const bf16_t*)W; p.ldw = ldw; p.bias = bias;
  p.M = M; p.N = N; p.K = K;
  p.a_mx = (const uint8_t*)a_mx; p.mx_rows_a = mx_rows_a; p.w_mx = (const uint8_t*)w_mx; p.mx_rows_w = mx_rows_w;
  p.X = X; p.ldx = ldx; p.gate = gate; p.X0 = (const bf16_t*)X0; p.ldx0 = ldx0; p.R = R; p.ldr = ldr;
  return (int)mc::launch_gemm_mxfp4(p, mc::EPI_RESID_CAPTURE, (hipStream_t)s);
}

// EPI_RESID_CAPTURE of launch_gemm_mxfp6: mc_op_gemm_mxfp6 has no X0 / R arguments
int mc_test_gemm_mxfp6_capture(const void* A, long lda, const void* a_mx, long mx_rows_a, const void* W, long ldw,
                               const void* w_mx, long mx_rows_w, const float* bias, int M, int N, int K, float* X, long ldx,
                               const float* gate, const void* X0, long ldx0, float* R, long ldr, void* s) {
  mc::GemmParams p = {};
  p.A = (const bf16_t*)A; p.lda = lda; p.W = (const bf16_t*)W; p.ldw = ldw; p.bias = bias;
  p.M = M; p.N = N; p.K = K;
  p.a_mx = (const uint8_t*)a_mx; p.mx_rows_a = mx_rows_a; p.w_mx = (const uint8_t*)w_mx; p.mx_rows_w = mx_rows_w;
  p.X = X; p.ldx = ldx; p.gate = gate; p.X0 = (const bf16_t*)X0; p.ldx0 = ldx0; p.R = R; p.ldr = ldr;
  return (int)mc::launch_gemm_mxfp6(p, mc::EPI_RESID_CAPTURE, (hipStream_t)s);
}

// EPI_RESID_CAPTURE of launch_gemm_fp8 (per-row / per-channel scales): mc_op_gemm_fp8 has no X0 / R arguments
int mc_test_gemm_fp8_capture(const void* A, long lda, const float* a_scale, const void* W, long ldw, const float* w_scale,
                             const float* bias, int M, int N, int K, float* X, long ldx, const float* gate, const void* X0,
                             long ldx0, float* R, long ldr, void* s) {
  mc::GemmParams p = {};
  p.A = (const bf16_t*)A; p.lda = lda; p.W = (const bf16_t*)W; p.ldw = ldw; p.bias = bias;
  p.M = M; p.N = N; p.K = K;
  p.a_scale = a_scale; p.w_scale = w_scale;
  p.X = X; p.ldx = ldx; p.gate = gate; p.X0 = (const bf16_t*)X0; p.ldx0 = ldx0; p.R = R; p.ldr = ldr;
  return (int)mc::launch_gemm_fp8(p, mc::EPI_RESID_CAPTURE, (hipStream_t)s);
}

// the finalize launch of the multi-rank calibration path: stats[3] from sums[4] that the caller reduced over the ranks
int mc_test_calib_finalize(const double* sums, float* stats, void* s) {
  return (int)mc::launch_calib_finalize(sums, stats, (hipStream_t)s);
}

int mc_test_token_t_prepare(const float* t, int n_all, int row0, int n_rows, int n_rows_pad, float* t2, unsigned char* sel,
                            void* s) {
  return (int)mc::launch_token_t_prepare(t, n_all, row0, n_rows, n_rows_pad, t2, sel, (hipStream_t)s);
}

// ---- the table forms of an engine with token_timestep_sets (tests/test_token_sets_ops_gpu.py)
int mc_test_token_t_sets(const float* t, int n_all, int row0, int n_rows, int n_rows_pad, int cap, float* t2, float* vals,
                         unsigned char* sel, void* s) {
  return (int)mc::launch_token_t_sets(t, n_all, row0, n_rows, n_rows_pad, cap, t2, vals, sel, (hipStream_t)s);
}

int mc_test_sinusoid_rows(const float* t_dev, int R, int dim, float* out, long ldo, void* s) {
  return (int)mc::launch_sinusoid_rows(t_dev, R, dim, out, ldo, (hipStream_t)s);
}

int mc_test_gemv_f32_rows(const float* W, const float* x, long ldx, const float* b, float* y, long ldy, int R, int N, int K,
                          int act_in, int act_out, void* s) {
  return (int)mc::launch_gemv_f32_rows(W, x, ldx, b, y, ldy, R, N, K, act_in, act_out, (hipStream_t)s);
}

// b: a HOST array of n_b device pointers
int mc_test_add_bcast_rows(const float* a, long lda, int R, int na, const float* const* b, int n_b, int n, float* out,
                           long ld_set, void* s) {
  return (int)mc::launch_add_bcast_rows(a, lda, R, na, b, n_b, n, out, ld_set, (hipStream_t)s);
}

int mc_test_ln_modulate_sets(const float* x, long ldx, const void* x0, long ldx0, const float* sc, const float* sh, int mode,
                             float eps, void* out, long ldo, float* out_f32, long ldof, int M, int D,
                             const unsigned char* sel, long set_stride, int n_sets, void* s) {
  return (int)mc::launch_ln_modulate(x, ldx, (const bf16_t*)x0, ldx0, sc, sh, mode, eps, (bf16_t*)out, ldo, out_f32, ldof, M, D,
                                     (hipStream_t)s, nullptr, nullptr, sel, set_stride, n_sets);
}

int mc_test_ln_modulate_fp8_sets(const float* x, long ldx, const float* sc, const float* sh, int mode, float eps,
                                 unsigned char* q, long ldq, float* row_scale, unsigned char* mx, long mx_rows, int M, int D,
                                 const unsigned char* sel, long set_stride, int n_sets, void* s) {
  return (int)mc::launch_ln_modulate_fp8(x, ldx, sc, sh, mode, eps, q, ldq, row_scale, mx, mx_rows, M, D, (hipStream_t)s,
                                         nullptr, nullptr, sel, set_stride, n_sets);
}

int mc_test_ln_modulate_mxfp4_sets(const float* x, long ldx, const float* sc, const float* sh, int mode, float eps,
                                   unsigned char* q, long ldq, unsigned char* mx, long mx_rows, int M, int D,
                                   const unsigned char* sel, long set_stride, int n_sets, void* s) {
  return (int)mc::launch_ln_modulate_mxfp4(x, ldx, sc, sh, mode, eps, q, ldq, mx, mx_rows, M, D, (hipStream_t)s, nullptr, nullptr,
                                           sel, set_stride, n_sets);
}

// the gated residual of launch_gemm_mxfp8 with per-row gates: mc_op_gemm_mxfp8 names neither gate2 / gate_sel nor a table.
// gate_stride == 0: the two-set form (gate, gate2, sel); != 0: the table form (gate = table, n_sets rows)
int mc_test_gemm_mxfp8_resid_rows(const void* A, long lda, const void* a_mx, long mx_rows_a, const void* W, long ldw,
                                  const void* w_mx, long mx_rows_w, const float* bias, int M, int N, int K, float* X, long ldx,
                                  const float* gate, const float* gate2, const unsigned char* sel, long gate_stride, int n_sets,
                                  void* s) {
  mc::GemmParams p = {};
  p.A = (const bf16_t*)A; p.lda = lda; p.W = (const bf16_t*)W; p.ldw = ldw; p.bias = bias;
  p.M = M; p.N = N; p.K = K;
  p.a_mx = (const uint8_t*)a_mx; p.mx_rows_a = mx_rows_a; p.w_mx = (const uint8_t*)w_mx; p.mx_rows_w = mx_rows_w;
  p.X = X; p.ldx = ldx; p.gate = gate; p.gate2 = gate2; p.gate_sel = sel; p.gate_stride = gate_stride; p.gate_sets = n_sets;
  if (gate_stride != 0 && !mc::gemm_gate_table_ok(p)) return (int)hipErrorInvalidValue;
  return (int)mc::launch_gemm_mxfp8(p, mc::EPI_RESID_GATE, (hipStream_t)s);
}

int mc_test_patchify(const float* lat, int C, int F, int H, int W, int tok0, int n_tok, int n_rows, void* out, long ldo,
                     void* s) {
  return (int)mc::launch_patchify(lat, C, F, H, W, tok0, n_tok, n_rows, (bf16_t*)out, ldo, (hipStream_t)s);
}

int mc_test_unpatchify(const float* tok, long ldt, int C, int F, int H, int W, int tok0, int n_tok, float* out, void* s) {
  return (int)mc::launch_unpatchify(tok, ldt, C, F, H, W, tok0, n_tok, out, (hipStream_t)s);
}

int mc_test_cast_pad_bf16(const float* src, long lds, int rows_valid, int rows, int cols, void* dst, long ldd, void* s) {
  return (int)mc::launch_cast_pad_bf16(src, lds, rows_valid, rows, cols, (bf16_t*)dst, ldd, (hipStream_t)s);
}

int mc_test_cast_bf16(const float* src, void* dst, size_t n, void* s) {
  return (int)mc::launch_cast_bf16(src, (bf16_t*)dst, n, (hipStream_t)s);
}

int mc_test_add_bf16(void* a, const void* b, size_t n, void* s) {
  return (int)mc::launch_add_bf16((bf16_t*)a, (const bf16_t*)b, n, (hipStream_t)s);
}

int mc_test_add_bcast(const float* a, int na, const float* b, float* out, int n, void* s) {
  return (int)mc::launch_add_bcast(a, na, b, out, n, (hipStream_t)s);
}

int mc_test_sinusoid(const float* t_dev, double t_host, int dim, float* out, void* s) {
  return (int)mc::launch_sinusoid(t_dev, t_host, dim, out, (hipStream_t)s);
}

int mc_test_colmean(const float* x, long ldx, int n_rows, int D, float* out, void* s) {
  return (int)mc::launch_colmean(x, ldx, n_rows, D, out, (hipStream_t)s);
}

int mc_test_rope_table_from_cos_sin(const float* cosv, const float* sinv, long ld, int n_rows, float* cs, void* s) {
  return (int)mc::launch_rope_table_from_cos_sin(cosv, sinv, ld, n_rows, cs, (hipStream_t)s);
}

int mc_test_cfg_euler(const float* cond, const float* uncond, float g, float dt, float* x, float* eps_out, size_t n, void* s) {
  return (int)mc::launch_cfg_euler(cond, uncond, g, dt, x, eps_out, n, (hipStream_t)s);
}

int mc_test_attn_merge(const void* const* o_parts, const float* const* lse_parts, int n, void* out, long ldo, int rows,
                       int rows_pad, int d, void* s) {
  return (int)mc::launch_attn_merge((const bf16_t* const*)o_parts, lse_parts, n, (bf16_t*)out, ldo, rows, rows_pad, d,
                                    (hipStream_t)s);
}

}  // extern "C"
