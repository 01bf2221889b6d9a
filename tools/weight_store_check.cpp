// The weight store's adapter bookkeeping (magcache_amd/csrc/host.cpp: base copies, replace, remove, apply, free) as a
// stand-alone host program for AddressSanitizer / UBSan: no GPU, no library.  "Device memory" is malloc, the copies are memcpy,
// and every launcher the store calls is a stub that touches exactly the bytes the kernel would read and write -- so a wrong
// size, a wrong offset, a freed base copy or a leaked operand is the sanitizer's to find.
//
//   hipcc -x hip --cuda-host-only -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -fno-omit-frame-pointer \
//         tools/weight_store_check.cpp -o weight_store_check && ./weight_store_check
//
// Exit status 0 and "weight store: N checks passed" when every return code is the expected one.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../magcache_amd/csrc/host.cpp"

// ---------------------------------------------------------------- the stub allocator and copies (these win over the runtime's)
static long g_live = 0;
extern "C" hipError_t hipMalloc(void** p, size_t n) {
  *p = malloc(n);
  if (*p) ++g_live;
  return *p ? hipSuccess : hipErrorOutOfMemory;
}
extern "C" hipError_t hipFree(void* p) {
  if (p) --g_live;
  free(p);
  return hipSuccess;
}
extern "C" hipError_t hipMemcpyAsync(void* dst, const void* src, size_t n, hipMemcpyKind, hipStream_t) {
  memmove(dst, src, n);
  return hipSuccess;
}
extern "C" hipError_t hipMemcpy2DAsync(void* dst, size_t dp, const void* src, size_t sp, size_t w, size_t h, hipMemcpyKind, hipStream_t) {
  for (size_t r = 0; r < h; ++r) memmove((char*)dst + r * dp, (const char*)src + r * sp, w);
  return hipSuccess;
}
extern "C" const char* hipGetErrorString(hipError_t) { return "stub"; }
extern "C" hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }

// ---------------------------------------------------------------- the launchers, as the bytes they touch
namespace mc {
static void touch(const void* p, size_t bytes) {   // read every byte
  volatile unsigned char acc = 0;
  for (size_t i = 0; i < bytes; ++i) acc = acc ^ ((const unsigned char*)p)[i];
}
hipError_t launch_cast_bf16(const float* src, bf16_t* dst, size_t n, hipStream_t) {
  touch(src, n * 4);
  memset(dst, 1, n * 2);
  return hipSuccess;
}
hipError_t launch_cast_pad_bf16(const float* src, long lds, int rows_valid, int rows, int cols, bf16_t* dst, long ldd, hipStream_t) {
  for (int r = 0; r < rows; ++r) {
    if (r < rows_valid) touch(src + (size_t)r * lds, (size_t)cols * 4);
    memset(dst + (size_t)r * ldd, 1, (size_t)cols * 2);
  }
  return hipSuccess;
}
hipError_t launch_quantize_rows_fp8(const bf16_t* x, const float*, long ldx, int M, int K, uint8_t* q, long ldq, float* scale, hipStream_t) {
  for (int r = 0; r < M; ++r) {
    touch(x + (size_t)r * ldx, (size_t)K * 2);
    memset(q + (size_t)r * ldq, 2, K);
    scale[r] = 1.f;
  }
  return hipSuccess;
}
// the three per-format launchers behind launch_quantize_rows_mx (ops.h): exactly M rows of mx_row_bytes and K / 32 scale bytes each
static long g_mx_q_bytes = 0, g_mx_scale_bytes = 0;   // written by the last call
static hipError_t quantize_mx_stub(MxFormat f, const bf16_t* x, long ldx, int M, int K, uint8_t* q, long ldq, uint8_t* s, long rows_pad) {
  g_mx_q_bytes = g_mx_scale_bytes = 0;
  for (int r = 0; r < M; ++r) {
    touch(x + (size_t)r * ldx, (size_t)K * 2);
    memset(q + (size_t)r * ldq, 2, mx_row_bytes(f, K));
    g_mx_q_bytes += mx_row_bytes(f, K);
    for (int kb = 0; kb < K / 32; ++kb, ++g_mx_scale_bytes) s[(size_t)kb * rows_pad + r] = 127;
  }
  return hipSuccess;
}
hipError_t launch_quantize_rows_mxfp8(const bf16_t* x, const float*, long ldx, int M, int K, uint8_t* q, long ldq, uint8_t* s, long rows_pad,
                                      hipStream_t) {
  return quantize_mx_stub(MX_E4M3, x, ldx, M, K, q, ldq, s, rows_pad);
}
hipError_t launch_quantize_rows_mxfp4(const bf16_t* x, const float*, long ldx, int M, int K, uint8_t* q, long ldq, uint8_t* s, long rows_pad,
                                      hipStream_t) {
  return quantize_mx_stub(MX_E2M1, x, ldx, M, K, q, ldq, s, rows_pad);
}
hipError_t launch_quantize_rows_mxfp6(const bf16_t* x, const float*, long ldx, int M, int K, uint8_t* q, long ldq, uint8_t* s, long rows_pad,
                                      hipStream_t) {
  return quantize_mx_stub(MX_E2M3, x, ldx, M, K, q, ldq, s, rows_pad);
}
hipError_t launch_lora_pack(const void* src, int src_f32, long rs, long cs, int n, int rank, int rank_pad, bf16_t* dst, hipStream_t) {
  for (int r = 0; r < n; ++r)
    for (int k = 0; k < rank; ++k) touch((const char*)src + ((size_t)r * rs + (size_t)k * cs) * (src_f32 ? 4 : 2), src_f32 ? 4 : 2);
  memset(dst, 3, lora_packed_elems(n, rank_pad) * 2);
  return hipSuccess;
}
template <class T>
static hipError_t merge_stub(const T* base, long ld_base, T* out, long ld_out, int rows, int K, const LoraTerm* t, int n) {
  if (n > kLoraMaxTerms) return hipErrorInvalidValue;
  for (int j = 0; j < n; ++j) {
    touch(t[j].up, lora_packed_elems(rows, t[j].rank_pad) * 2);
    touch(t[j].down, lora_packed_elems(K, t[j].rank_pad) * 2);
  }
  for (int r = 0; r < rows; ++r) memmove(out + (size_t)r * ld_out, base + (size_t)r * ld_base, (size_t)K * sizeof(T));
  return hipSuccess;
}
hipError_t launch_lora_merge(const bf16_t* base, long ld_base, bf16_t* out, long ld_out, int rows, int K, const LoraTerm* t, int n,
                             hipStream_t) {
  return merge_stub(base, ld_base, out, ld_out, rows, K, t, n);
}
hipError_t launch_lora_merge_f32(const float* base, long ld_base, float* out, long ld_out, int rows, int K, const LoraTerm* t, int n,
                                 hipStream_t) {
  return merge_stub(base, ld_base, out, ld_out, rows, K, t, n);
}
hipError_t launch_widen_f32(const void* src, int src_f32, float* dst, size_t n, hipStream_t) {
  touch(src, n * (src_f32 ? 4 : 2));
  for (size_t i = 0; i < n; ++i) dst[i] = 1.f;
  return hipSuccess;
}
static int g_adapter_merges = 0, g_adapter_magnitudes = 0;   // general merges launched; those that had a magnitude
hipError_t launch_adapter_merge(const bf16_t* base, long ld_base, bf16_t* out, long ld_out, int rows, int K, const LoraTerm* pairs,
                                int n_pairs, const KronTerm* krons, int n_kron, const HadaTerm* hadas, int n_hada,
                                const float* magnitude, float* scratch, hipStream_t) {
  if (n_pairs + n_kron + n_hada > kLoraMaxTerms) return hipErrorInvalidValue;
  for (int j = 0; j < n_kron; ++j) {
    if ((long)krons[j].r1 * krons[j].r2 != rows || (long)krons[j].c1 * krons[j].c2 != K) return hipErrorInvalidValue;
    touch(krons[j].w1, (size_t)krons[j].r1 * krons[j].c1 * 4);
    touch(krons[j].w2, (size_t)krons[j].r2 * krons[j].c2 * 4);
  }
  for (int j = 0; j < n_hada; ++j) {
    for (const float* u : {hadas[j].u1, hadas[j].u2}) touch(u, (size_t)rows * hadas[j].rank * 4);
    for (const float* dd : {hadas[j].d1, hadas[j].d2}) touch(dd, (size_t)hadas[j].rank * K * 4);
  }
  if (magnitude) touch(magnitude, (size_t)rows * 4);
  memset(scratch, 0, (size_t)rows * K * 4);
  ++g_adapter_merges;
  g_adapter_magnitudes += magnitude != nullptr;
  return merge_stub(base, ld_base, out, ld_out, rows, K, pairs, n_pairs);
}
hipError_t launch_param_delta(const float* base, float* out, size_t n, const float* const* deltas, const float* scales, int n_terms,
                              hipStream_t) {
  if (n_terms < 1 || n_terms > kLoraMaxTerms) return hipErrorInvalidValue;
  for (size_t i = 0; i < n; ++i) {
    float sum = 0.f;
    for (int j = 0; j < n_terms; ++j) sum += scales[j] * deltas[j][i];
    out[i] = base[i] + sum;
  }
  return hipSuccess;
}
hipError_t launch_gemm_bf16(const GemmParams&, int, hipStream_t) { return hipSuccess; }
int g_mx_fp4 = 0, g_mx_fp6 = 0;   // engine.cpp's, read by latch_mx_format
hipError_t launch_attention(const AttnParams&, hipStream_t) { return hipSuccess; }
}  // namespace mc

// ---------------------------------------------------------------- the scenario
static int g_checks = 0, g_failed = 0;
#define EXPECT(expr, want)                                                                             \
  do {                                                                                                 \
    const mc_status _got = (expr);                                                                     \
    ++g_checks;                                                                                        \
    if (_got != (want)) {                                                                              \
      ++g_failed;                                                                                      \
      printf("line %d: %s = %d, expected %d (%s)\n", __LINE__, #expr, (int)_got, (int)(want), mc::last_error()); \
    }                                                                                                  \
  } while (0)
#define EXPECT_TRUE(cond)                                        \
  do {                                                           \
    ++g_checks;                                                  \
    if (!(cond)) { ++g_failed; printf("line %d: %s is false\n", __LINE__, #cond); } \
  } while (0)

int main() {
  using namespace mc;
  constexpr size_t d = 64, kt = 12, rank = 5;
  {
    WeightStore W;
    W.allow_f32_targets = true;
    Linear qkv, patch;
    float *w_time = nullptr, *mod = nullptr;
    EXPECT(W.add_linear(qkv, "blk.", {{"q", d}, {"k", d}, {"v", d}}, d, QUANT_ROW), MC_OK);
    EXPECT(W.add_linear(patch, "", {{"patch", d}}, d), MC_OK);
    W.slots.at("patch.weight").fixed = true;
    EXPECT(W.add_f32(w_time, "time.weight", d * kt, kt), MC_OK);
    EXPECT(W.add_f32(mod, "mod", 6 * d), MC_OK);
    std::vector<float> src(6 * d * d, 0.5f);
    const int64_t mat[2] = {(int64_t)d, (int64_t)d}, vec[1] = {(int64_t)d}, tm[2] = {(int64_t)d, (int64_t)kt}, md[3] = {1, 6, (int64_t)d};
    for (const char* p : {"q", "k", "v"}) {
      EXPECT(W.set((std::string("blk.") + p + ".weight").c_str(), src.data(), MC_F32, mat, 2, nullptr), MC_OK);
      EXPECT(W.set((std::string("blk.") + p + ".bias").c_str(), src.data(), MC_F32, vec, 1, nullptr), MC_OK);
    }
    EXPECT(W.set("patch.weight", src.data(), MC_F32, mat, 2, nullptr), MC_OK);
    EXPECT(W.set("patch.bias", src.data(), MC_F32, vec, 1, nullptr), MC_OK);
    EXPECT(W.set("time.weight", src.data(), MC_F32, tm, 2, nullptr), MC_OK);
    EXPECT(W.set("mod", src.data(), MC_F32, md, 3, nullptr), MC_OK);
    EXPECT_TRUE(W.all_loaded(nullptr));

    std::vector<float> down(rank * d, 0.1f), up(d * rank, 0.2f), down_t(rank * kt, 0.1f), delta(d * kt, 0.01f);   // the largest delta: time.weight
    // apply with nothing live, on a store that never saw an adapter
    int merged = -1;
    EXPECT(W.lora_apply(nullptr, &merged), MC_OK);
    EXPECT_TRUE(merged == 0 && !W.dirty());
    // set: bf16 parts of one Linear (one base copy), an fp32 matrix, deltas on a fused bias, a table and the fp32 matrix
    EXPECT(W.lora_set("a", "blk.q.weight", down.data(), rank * d, up.data(), d * rank, MC_F32, rank, 2.f, nullptr), MC_OK);
    EXPECT(W.lora_set("a", "blk.v.weight", down.data(), rank * d, up.data(), d * rank, MC_F32, rank, 1.f, nullptr), MC_OK);
    EXPECT(W.lora_set("b", "blk.q.weight", down.data(), rank * d, up.data(), d * rank, MC_F32, rank, 1.f, nullptr), MC_OK);
    EXPECT(W.lora_set("a", "time.weight", down_t.data(), rank * kt, up.data(), d * rank, MC_F32, rank, 1.f, nullptr), MC_OK);
    EXPECT(W.lora_set_delta("a", "blk.k.bias", delta.data(), d, MC_F32, nullptr), MC_OK);
    EXPECT(W.lora_set_delta("b", "mod", delta.data(), 6 * d, MC_F32, nullptr), MC_OK);
    EXPECT(W.lora_set_delta("b", "time.weight", delta.data(), d * kt, MC_F32, nullptr), MC_OK);
    // replace: the same (adapter, name) again, another rank
    EXPECT(W.lora_set("a", "blk.q.weight", down.data(), 2 * d, up.data(), d * 2, MC_F32, 2, 1.f, nullptr), MC_OK);
    EXPECT(W.lora_set_delta("b", "mod", delta.data(), 6 * d, MC_F32, nullptr), MC_OK);
    // refusals: nothing may stay allocated behind them
    const long live = g_live;
    EXPECT(W.lora_set("a", "nope.weight", down.data(), rank * d, up.data(), d * rank, MC_F32, rank, 1.f, nullptr), MC_EINVAL);
    EXPECT(W.lora_set("a", "patch.weight", down.data(), rank * d, up.data(), d * rank, MC_F32, rank, 1.f, nullptr), MC_EINVAL);
    EXPECT(W.lora_set("a", "mod", down.data(), rank * d, up.data(), 6 * rank, MC_F32, rank, 1.f, nullptr), MC_EINVAL);
    EXPECT(W.lora_set("a", "time.weight", down_t.data(), rank * kt + 1, up.data(), d * rank, MC_F32, rank, 1.f, nullptr), MC_EINVAL);
    EXPECT(W.lora_set_delta("a", "blk.q.weight", delta.data(), d * d, MC_F32, nullptr), MC_EINVAL);
    EXPECT(W.lora_set_delta("a", "mod", delta.data(), 6 * d - 1, MC_F32, nullptr), MC_EINVAL);
    EXPECT(W.lora_set_delta("a", "mod", delta.data(), 6 * d, MC_BF16, nullptr), MC_EINVAL);
    EXPECT_TRUE(g_live == live);
    for (int i = 0; i < kLoraMaxTerms - 1; ++i)
      EXPECT(W.lora_set_delta(("n" + std::to_string(i)).c_str(), "mod", delta.data(), 6 * d, MC_F32, nullptr), MC_OK);
    EXPECT(W.lora_set_delta("ninth", "mod", delta.data(), 6 * d, MC_F32, nullptr), MC_EINVAL);
    for (int i = 0; i < kLoraMaxTerms - 1; ++i) EXPECT(W.lora_remove(("n" + std::to_string(i)).c_str()), MC_OK);
    EXPECT_TRUE(W.dirty());
    EXPECT(W.lora_apply(nullptr, &merged), MC_OK);
    EXPECT_TRUE(merged == 5 && !W.dirty());   // q, v, time, k.bias, mod
    int adapters = 0, params = 0;
    size_t bytes = 0;
    W.lora_info(&adapters, &params, &bytes);
    EXPECT_TRUE(adapters == 2 && params == 4 && bytes == 3 * d * d * 2 + (d * kt + d + 6 * d) * 4);
    // set on touched parameters goes to the base copies and waits for the apply
    EXPECT(W.set("time.weight", src.data(), MC_F32, tm, 2, nullptr), MC_OK);
    EXPECT(W.set("blk.k.bias", src.data(), MC_F32, vec, 1, nullptr), MC_OK);
    EXPECT(W.set("blk.q.weight", src.data(), MC_F32, mat, 2, nullptr), MC_OK);
    EXPECT_TRUE(W.dirty());
    EXPECT(W.lora_apply(nullptr, &merged), MC_OK);
    EXPECT_TRUE(merged == 3);
    // scale 0: every term of the adapter is left out, the base copies stay
    EXPECT(W.lora_scale("a", 0.f), MC_OK);
    EXPECT(W.lora_scale("zz", 1.f), MC_EINVAL);
    EXPECT(W.lora_apply(nullptr, nullptr), MC_OK);
    // remove one adapter, then all of them: the base copies go with the last term
    EXPECT(W.lora_remove("a"), MC_OK);
    EXPECT(W.lora_remove("a"), MC_EINVAL);
    EXPECT(W.lora_apply(nullptr, nullptr), MC_OK);
    W.lora_info(&adapters, &params, &bytes);
    EXPECT_TRUE(adapters == 1 && params == 3 && bytes == 3 * d * d * 2 + (d * kt + 6 * d) * 4);
    EXPECT(W.lora_remove(nullptr), MC_OK);
    EXPECT(W.lora_apply(nullptr, &merged), MC_OK);
    W.lora_info(&adapters, &params, &bytes);
    EXPECT_TRUE(adapters == 0 && params == 0 && bytes == 0 && qkv.w_base == nullptr);
    EXPECT(W.lora_apply(nullptr, &merged), MC_OK);
    EXPECT_TRUE(merged == 0);
    // adapters still set when the store goes: free_all takes everything
    EXPECT(W.lora_set("c", "blk.k.weight", down.data(), rank * d, up.data(), d * rank, MC_F32, rank, 1.f, nullptr), MC_OK);
    EXPECT(W.lora_set_delta("c", "mod", delta.data(), 6 * d, MC_F32, nullptr), MC_OK);
    W.free_all();
    EXPECT_TRUE(g_live == 0);
  }
  {  // a store whose engine did not opt in (the MM-DiT engine): fp32 targets and deltas are refused
    mc::WeightStore W;
    float* head = nullptr;
    std::vector<float> v(64 * 16, 0.f);
    EXPECT(W.add_f32(head, "head.weight", 64 * 16, 16), MC_OK);
    EXPECT(W.lora_set("a", "head.weight", v.data(), 4 * 16, v.data(), 64 * 4, MC_F32, 4, 1.f, nullptr), MC_EINVAL);
    EXPECT(W.lora_set_delta("a", "head.weight", v.data(), 64 * 16, MC_F32, nullptr), MC_EINVAL);
    W.free_all();
    EXPECT_TRUE(g_live == 0);
  }
  {  // Kronecker and Hadamard terms and DoRA magnitudes: fp32 copies, the general merge with its scratch, the shared limit
    WeightStore W;
    W.allow_f32_targets = true;
    Linear qkv;
    float* w_time = nullptr;
    EXPECT(W.add_linear(qkv, "blk.", {{"q", d}, {"k", d}, {"v", d}}, d, QUANT_ROW), MC_OK);
    EXPECT(W.add_f32(w_time, "time.weight", d * kt, kt), MC_OK);
    std::vector<float> src(d * d, 0.5f), w1(4 * 8, 0.1f), w2(16 * 8, 0.2f), g(d, 1.f), down(rank * d, 0.1f), up(d * rank, 0.2f);
    std::vector<uint16_t> ub(d * rank, 0x3c00), db(rank * d, 0x3c00);   // bf16 operands: widened on the way in
    const int64_t mat[2] = {(int64_t)d, (int64_t)d}, tm[2] = {(int64_t)d, (int64_t)kt};
    const int64_t s1[2] = {4, 8}, s2[2] = {16, 8}, bad[2] = {5, 8}, us[2] = {(int64_t)d, (int64_t)rank}, ds[2] = {(int64_t)rank, (int64_t)d},
                  ds_bad[2] = {(int64_t)rank + 1, (int64_t)d};
    for (const char* p : {"q", "k", "v"}) EXPECT(W.set((std::string("blk.") + p + ".weight").c_str(), src.data(), MC_F32, mat, 2, nullptr), MC_OK);
    EXPECT(W.set("time.weight", src.data(), MC_F32, tm, 2, nullptr), MC_OK);
    EXPECT(W.lora_set_kron("a", "blk.q.weight", w1.data(), s1, w2.data(), s2, MC_F32, 1.f, nullptr), MC_OK);
    EXPECT(W.lora_set_hada("a", "blk.q.weight", ub.data(), us, db.data(), ds, ub.data(), db.data(), MC_BF16, 0.5f, nullptr), MC_OK);
    EXPECT(W.lora_set_magnitude("a", "blk.q.weight", g.data(), d, MC_F32, nullptr), MC_OK);
    EXPECT(W.lora_set("a", "blk.q.weight", down.data(), rank * d, up.data(), d * rank, MC_F32, rank, 2.f, nullptr), MC_OK);
    long live = g_live;
    // replace: the same (adapter, weight) and kind again
    EXPECT(W.lora_set_kron("a", "blk.q.weight", w2.data(), s2, w1.data(), s1, MC_F32, 1.f, nullptr), MC_OK);
    EXPECT(W.lora_set_hada("a", "blk.q.weight", ub.data(), us, db.data(), ds, ub.data(), db.data(), MC_BF16, 1.f, nullptr), MC_OK);
    EXPECT(W.lora_set_magnitude("a", "blk.q.weight", g.data(), d, MC_F32, nullptr), MC_OK);
    EXPECT_TRUE(g_live == live);
    // refusals: nothing may stay allocated behind them
    EXPECT(W.lora_set_kron("a", "blk.q.weight", w1.data(), bad, w2.data(), s2, MC_F32, 1.f, nullptr), MC_EINVAL);
    EXPECT(W.lora_set_kron("a", "time.weight", w1.data(), s1, w2.data(), s2, MC_F32, 1.f, nullptr), MC_EINVAL);
    EXPECT(W.lora_set_kron("a", "nope.weight", w1.data(), s1, w2.data(), s2, MC_F32, 1.f, nullptr), MC_EINVAL);
    EXPECT(W.lora_set_kron("a", "blk.q.weight", nullptr, s1, w2.data(), s2, MC_F32, 1.f, nullptr), MC_EINVAL);
    EXPECT(W.lora_set_hada("a", "blk.q.weight", ub.data(), us, db.data(), ds_bad, ub.data(), db.data(), MC_BF16, 1.f, nullptr), MC_EINVAL);
    EXPECT(W.lora_set_hada("a", "time.weight", ub.data(), us, db.data(), ds, ub.data(), db.data(), MC_BF16, 1.f, nullptr), MC_EINVAL);
    EXPECT(W.lora_set_magnitude("a", "blk.q.weight", g.data(), d - 1, MC_F32, nullptr), MC_EINVAL);
    EXPECT(W.lora_set_magnitude("a", "time.weight", g.data(), d, MC_F32, nullptr), MC_EINVAL);
    EXPECT(W.lora_set_magnitude("b", "blk.q.weight", g.data(), d, MC_F32, nullptr), MC_EINVAL);   // a second adapter's magnitude
    EXPECT_TRUE(strstr(last_error(), "'a'") && strstr(last_error(), "'b'"));
    EXPECT_TRUE(g_live == live);
    // all kinds count towards the limit: q carries a pair, a Kronecker and a Hadamard term
    for (int i = 0; i < kLoraMaxTerms - 3; ++i)
      EXPECT(W.lora_set_kron(("n" + std::to_string(i)).c_str(), "blk.q.weight", w1.data(), s1, w2.data(), s2, MC_F32, 1.f, nullptr), MC_OK);
    EXPECT(W.lora_set_kron("ninth", "blk.q.weight", w1.data(), s1, w2.data(), s2, MC_F32, 1.f, nullptr), MC_EINVAL);
    EXPECT(W.lora_set("ninth", "blk.q.weight", down.data(), rank * d, up.data(), d * rank, MC_F32, rank, 1.f, nullptr), MC_EINVAL);
    EXPECT(W.lora_set_hada("ninth", "blk.q.weight", ub.data(), us, db.data(), ds, ub.data(), db.data(), MC_BF16, 1.f, nullptr), MC_EINVAL);
    // a pair alone on another part of the same Linear keeps the pair merge
    EXPECT(W.lora_set("a", "blk.k.weight", down.data(), rank * d, up.data(), d * rank, MC_F32, rank, 1.f, nullptr), MC_OK);
    int merged = -1;
    live = g_live;
    EXPECT(W.lora_apply(nullptr, &merged), MC_OK);
    EXPECT_TRUE(merged == 2 && g_adapter_merges == 1 && g_adapter_magnitudes == 1 && g_live == live);   // the scratch came and went
    // scale 0: the terms and the magnitude of "a" are left out, the others' Kronecker terms stay
    EXPECT(W.lora_scale("a", 0.f), MC_OK);
    EXPECT(W.lora_apply(nullptr, &merged), MC_OK);
    EXPECT_TRUE(merged == 2 && g_adapter_merges == 2 && g_adapter_magnitudes == 1);
    for (int i = 0; i < kLoraMaxTerms - 3; ++i) EXPECT(W.lora_remove(("n" + std::to_string(i)).c_str()), MC_OK);
    EXPECT(W.lora_apply(nullptr, &merged), MC_OK);
    EXPECT_TRUE(merged == 1 && g_adapter_merges == 2 && qkv.w_base != nullptr);   // nothing live on q: the base rows, copied back
    EXPECT(W.lora_scale("a", 1.f), MC_OK);
    EXPECT(W.lora_remove("a"), MC_OK);
    EXPECT(W.lora_apply(nullptr, &merged), MC_OK);
    int adapters = -1, params = -1;
    size_t bytes = 1;
    W.lora_info(&adapters, &params, &bytes);
    EXPECT_TRUE(adapters == 0 && params == 0 && bytes == 0 && qkv.w_base == nullptr && g_adapter_merges == 2);
    // entries still set when the store goes: free_all takes everything
    EXPECT(W.lora_set_hada("c", "blk.v.weight", ub.data(), us, db.data(), ds, ub.data(), db.data(), MC_BF16, 1.f, nullptr), MC_OK);
    EXPECT(W.lora_set_magnitude("c", "blk.v.weight", g.data(), d, MC_F32, nullptr), MC_OK);
    W.free_all();
    EXPECT_TRUE(g_live == 0);
  }
  {  // MX copies in every element format: setting the LAST part of a fused Linear writes the last rows of q and of every scale
     // block, so a row size or a row offset that is too large runs off the allocation
    constexpr size_t n = 64, k = 512;
    std::vector<float> w(n * k, 0.25f);
    const int64_t mat[2] = {(int64_t)n, (int64_t)k};
    for (MxFormat f : {MX_E4M3, MX_E2M1, MX_E2M3}) {
      WeightStore W;
      Linear kv;
      EXPECT(W.add_linear(kv, "", {{"k", n}, {"v", n}}, k, QUANT_MX, f), MC_OK);
      EXPECT_TRUE(kv.fmt == f && kv.q_row_bytes() == mx_row_bytes(f, k));
      for (const char* name : {"k.weight", "v.weight"}) {
        EXPECT(W.set(name, w.data(), MC_F32, mat, 2, nullptr), MC_OK);
        EXPECT_TRUE(g_mx_q_bytes == (long)n * mx_row_bytes(f, k) && g_mx_scale_bytes == (long)(k / 32 * n));
      }
      W.free_all();
      EXPECT_TRUE(g_live == 0);
    }
    EXPECT_TRUE(mx_row_bytes(MX_E4M3, k) == 512 && mx_row_bytes(MX_E2M1, k) == 256 && mx_row_bytes(MX_E2M3, k) == 384);
    // the create-time latch: one format, e4m3 without MX Linears, both options refused
    MxFormat f = MX_E2M1;
    EXPECT(latch_mx_format(true, &f), MC_OK);
    EXPECT_TRUE(f == MX_E4M3);
    g_mx_fp6 = 1;
    EXPECT(latch_mx_format(true, &f), MC_OK);
    EXPECT_TRUE(f == MX_E2M3);
    EXPECT(latch_mx_format(false, &f), MC_OK);
    EXPECT_TRUE(f == MX_E4M3);
    g_mx_fp4 = 1;
    EXPECT(latch_mx_format(true, &f), MC_EINVAL);
    g_mx_fp6 = 0;
    EXPECT(latch_mx_format(true, &f), MC_OK);
    EXPECT_TRUE(f == MX_E2M1);
    EXPECT(check_mx_k(f, "q", 768), MC_OK);
    EXPECT(check_mx_k(f, "q", 640), MC_EINVAL);
    EXPECT(check_mx_k(f, "q", 256), MC_EINVAL);
  }
  if (g_failed) {
    printf("weight store: %d of %d checks FAILED\n", g_failed, g_checks);
    return 1;
  }
  printf("weight store: %d checks passed\n", g_checks);
  return 0;
}
