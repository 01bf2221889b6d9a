// Torch-free kernel A/B harness for the two MFMA-bound kernels at the Wan2.1-1.3B 480p shapes, through the C ABI.
//
//   kbench.bin <what> <rounds> <launches> libA.so [libB.so ...]
//      what: gemm | attn | attn_mx8 | attn_band | attn_sparse | attn_sparse_sp | attn_band_sp | attn_joint | attn_predict | attn_predict_sparse | calib | all
//      (attn_joint: the MM-DiT joint shapes, HunyuanVideo 720p and FLUX 1024^2; KBENCH_JOINT picks another)
//
// Every library given on the command line is dlopen'ed privately (RTLD_LOCAL), so build variants of
// libmagcache_hip.so (tools/build_variants.py, tools/build_v5_variants.py, tools/build_gemm_v2_variants.py) are measured INTERLEAVED IN ONE PROCESS on the same
// buffers: per shape a 1 s warm-up (sustained-power regime), then <rounds> rounds of <launches> back-to-back launches
// per library, hipEvent-timed; median and minimum per library are printed (CDNA4 guide, methodology rules 24/25: a
// within-probe interleaved A/B on random data).  Results of libB.. are compared bit for bit with libA, and libA is
// spot-checked against an fp64 reference.  KBENCH_AMP=0 gives zero-filled operands (shows how much of a rate is DVFS;
// never a number to quote).
#include <dlfcn.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "magcache_hip.h"

#define CK(x)                                                                     \
  do {                                                                            \
    hipError_t e_ = (x);                                                          \
    if (e_ != hipSuccess) {                                                       \
      fprintf(stderr, "HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); \
      exit(2);                                                                    \
    }                                                                             \
  } while (0)

struct Lib {
  std::string path;
  void* h;
  decltype(&mc_op_gemm_bf16) gemm;
  decltype(&mc_op_attention) attn;
  decltype(&mc_op_calib_stats) calib;
  decltype(&mc_op_attn_quantize_mx8) quant_mx8;   // null in a library older than the MX fp8 attention (attn_mx8 only)
  decltype(&mc_op_attention_mx8) attn_mx8;
  decltype(&mc_op_attention_band) attn_band;      // null in a library older than the frame-block causal kernel (attn_band only)
  decltype(&mc_op_attention_sparse) attn_sparse;  // null in a library older than the tile-sparse kernel (attn_sparse only)
  decltype(&mc_op_attention_tile_predict) predict;  // null in a library older than the tile-mask predictor (attn_predict* only)
  decltype(&mc_op_attention_partial) attn_partial;                 // the dense chain of attn_sparse_sp
  decltype(&mc_op_attention_sparse_partial) attn_sparse_partial;   // null in a library older than the sharded tile-sparse kernel
  decltype(&mc_op_attention_band_partial) attn_band_partial;       // null in a library older than the sharded band kernel (attn_band_sp only)
  decltype(&mc_set_option) set_option;
  decltype(&mc_last_error) last_error;
};
static std::vector<Lib> g_libs;
static float g_amp = 1.0f;

#define MCL(lib, x)                                                                           \
  do {                                                                                        \
    if ((x) != MC_OK) {                                                                       \
      fprintf(stderr, "%s: mc error: %s at %s:%d\n", (lib).path.c_str(), (lib).last_error(), __FILE__, __LINE__); \
      exit(2);                                                                                \
    }                                                                                         \
  } while (0)

__device__ __forceinline__ uint32_t hash32(uint32_t i, uint32_t seed) {
  uint32_t h = i * 2654435761u + seed * 0x9e3779b9u;
  h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
  return h;
}
// standard normal (Box-Muller on two hashes): the bench's operands are randn, and the sustained clock depends on the
// operand distribution
__device__ __forceinline__ float randn(size_t i, uint32_t seed) {
  const float u1 = ((hash32((uint32_t)i, seed) >> 8) + 1) * (1.0f / 16777216.0f);
  const float u2 = (hash32((uint32_t)i, seed ^ 0x5bd1e995u) >> 8) * (1.0f / 16777216.0f);
  return sqrtf(-2.0f * __logf(u1)) * __cosf(6.28318530718f * u2);
}
__global__ void fill_bf16(uint16_t* p, size_t n, uint32_t seed, float amp) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    __bf16 b = (__bf16)(randn(i, seed) * amp);
    p[i] = __builtin_bit_cast(uint16_t, b);
  }
}
__global__ void fill_f32(float* p, size_t n, uint32_t seed, float amp, float bias) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    p[i] = randn(i, seed) * amp + bias;
}
__global__ void count_diff(const uint32_t* a, const uint32_t* b, size_t n, unsigned long long* out) {
  unsigned long long c = 0;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) c += a[i] != b[i];
  if (c) atomicAdd(out, c);
}

__device__ __forceinline__ float bf16_to_f32_dev(uint16_t v) { return __uint_as_float((uint32_t)v << 16); }
static float bf16_to_f(uint16_t v) {
  uint32_t u = (uint32_t)v << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
}

template <class F>
static void measure(const char* what, double flops_or_bytes, const char* unit, double unit_scale, int rounds, int launches,
                    F&& launch) {
  hipEvent_t a, b;
  CK(hipEventCreate(&a));
  CK(hipEventCreate(&b));
  // warm-up: ~1 s of the first library
  {
    CK(hipEventRecord(a, nullptr));
    float ms = 0;
    int n = 0;
    do {
      for (int i = 0; i < 20; ++i) launch(0);
      CK(hipEventRecord(b, nullptr));
      CK(hipEventSynchronize(b));
      CK(hipEventElapsedTime(&ms, a, b));
      n += 20;
    } while (ms < 1000.f && n < 20000);
  }
  std::vector<std::vector<double>> t(g_libs.size());
  for (int r = 0; r < rounds; ++r) {
    for (size_t l = 0; l < g_libs.size(); ++l) {
      launch((int)l);
      CK(hipEventRecord(a, nullptr));
      for (int i = 0; i < launches; ++i) launch((int)l);
      CK(hipEventRecord(b, nullptr));
      CK(hipEventSynchronize(b));
      float ms = 0;
      CK(hipEventElapsedTime(&ms, a, b));
      t[l].push_back(ms / launches);
    }
  }
  for (size_t l = 0; l < g_libs.size(); ++l) {
    std::sort(t[l].begin(), t[l].end());
    const double med = t[l][t[l].size() / 2], mn = t[l][0];
    printf("%-12s lib%zu  median %8.4f ms %8.1f %s | min %8.4f ms %8.1f %s | x%.3f vs lib0 (median)\n", what, l, med,
           flops_or_bytes / (med * 1e-3) * unit_scale, unit, mn, flops_or_bytes / (mn * 1e-3) * unit_scale, unit,
           t[0][t[0].size() / 2] / med);
  }
  fflush(stdout);
  CK(hipEventDestroy(a));
  CK(hipEventDestroy(b));
}

// ------------------------------------------------------------------------------------------ GEMM
static void bench_gemm(const char* name, int M, int N, int K, int epi, int rounds, int launches) {
  uint16_t *A, *W, *Cb, *Cref;
  float *bias, *gate, *X, *X0, *Xref;
  CK(hipMalloc(&A, (size_t)M * K * 2));
  CK(hipMalloc(&W, (size_t)N * K * 2));
  CK(hipMalloc(&bias, (size_t)N * 4));
  CK(hipMalloc(&gate, (size_t)N * 4));
  CK(hipMalloc(&Cb, (size_t)M * N * 2));
  CK(hipMalloc(&Cref, (size_t)M * N * 2));
  CK(hipMalloc(&X, (size_t)M * N * 4));
  CK(hipMalloc(&X0, (size_t)M * N * 4));
  CK(hipMalloc(&Xref, (size_t)M * N * 4));
  unsigned long long* dcount;
  CK(hipMalloc(&dcount, 8));
  fill_bf16<<<2048, 256>>>(A, (size_t)M * K, 1, 1.0f * g_amp);
  fill_bf16<<<2048, 256>>>(W, (size_t)N * K, 2, 0.02f * g_amp);
  fill_f32<<<64, 256>>>(bias, N, 3, 0.02f, 0.f);
  fill_f32<<<64, 256>>>(gate, N, 4, 0.3f, 0.f);
  fill_f32<<<2048, 256>>>(X0, (size_t)M * N, 5, 1.0f, 0.f);
  CK(hipMemcpy(X, X0, (size_t)M * N * 4, hipMemcpyDeviceToDevice));
  CK(hipDeviceSynchronize());
  auto launch = [&](int l) {
    MCL(g_libs[l], g_libs[l].gemm(A, K, W, K, bias, M, N, K, epi, Cb, N, X, N, gate, nullptr, 0, nullptr, 0, nullptr, 0, 0, nullptr));
  };
  char what[64];
  snprintf(what, sizeof(what), "gemm_%s", name);
  printf("# %s: M=%d N=%d K=%d epi=%d\n", what, M, N, K, epi);
  measure(what, 2.0 * M * N * K, "TF", 1e-12, rounds, launches, launch);
  // bitwise comparison with lib0 on pristine outputs
  for (size_t l = 0; l < g_libs.size(); ++l) {
    CK(hipMemcpy(X, X0, (size_t)M * N * 4, hipMemcpyDeviceToDevice));
    CK(hipMemset(Cb, 0, (size_t)M * N * 2));
    launch((int)l);
    CK(hipDeviceSynchronize());
    if (l == 0) {
      CK(hipMemcpy(Cref, Cb, (size_t)M * N * 2, hipMemcpyDeviceToDevice));
      CK(hipMemcpy(Xref, X, (size_t)M * N * 4, hipMemcpyDeviceToDevice));
      // fp64 spot check of 64 outputs
      std::vector<uint16_t> ha((size_t)M * K), hw((size_t)N * K);
      std::vector<float> hb(N), hg(N);
      CK(hipMemcpy(ha.data(), A, ha.size() * 2, hipMemcpyDeviceToHost));
      CK(hipMemcpy(hw.data(), W, hw.size() * 2, hipMemcpyDeviceToHost));
      CK(hipMemcpy(hb.data(), bias, N * 4, hipMemcpyDeviceToHost));
      CK(hipMemcpy(hg.data(), gate, N * 4, hipMemcpyDeviceToHost));
      double worst = 0;
      for (int s = 0; s < 64; ++s) {
        const int m = (int)(((uint64_t)s * 2654435761ull + 17) % (uint64_t)M), n = (int)(((uint64_t)s * 40503ull + 5) % (uint64_t)N);
        double acc = 0;
        for (int k = 0; k < K; ++k) acc += (double)bf16_to_f(ha[(size_t)m * K + k]) * bf16_to_f(hw[(size_t)n * K + k]);
        acc += hb[n];
        double got, want;
        if (epi <= 1) {
          uint16_t c;
          CK(hipMemcpy(&c, Cref + (size_t)m * N + n, 2, hipMemcpyDeviceToHost));
          got = bf16_to_f(c);
          want = epi == 0 ? acc : 0.5 * acc * (1.0 + std::tanh(0.7978845608028654 * (acc + 0.044715 * acc * acc * acc)));
        } else {
          float xv, x0v;
          CK(hipMemcpy(&xv, Xref + (size_t)m * N + n, 4, hipMemcpyDeviceToHost));
          CK(hipMemcpy(&x0v, X0 + (size_t)m * N + n, 4, hipMemcpyDeviceToHost));
          got = xv;
          want = x0v + hg[n] * acc;
        }
        worst = std::max(worst, std::fabs(got - want) / (std::fabs(want) + 1e-2));
      }
      printf("  %s lib0 vs fp64 (64 samples): worst rel err %.3e\n", what, worst);
    } else {
      CK(hipMemset(dcount, 0, 8));
      if (epi <= 1) count_diff<<<1024, 256>>>((const uint32_t*)Cb, (const uint32_t*)Cref, (size_t)M * N / 2, dcount);
      else count_diff<<<1024, 256>>>((const uint32_t*)X, (const uint32_t*)Xref, (size_t)M * N, dcount);
      unsigned long long c;
      CK(hipMemcpy(&c, dcount, 8, hipMemcpyDeviceToHost));
      printf("  %s lib%zu vs lib0: %llu differing dwords\n", what, l, c);
    }
  }
  fflush(stdout);
  CK(hipFree(A)); CK(hipFree(W)); CK(hipFree(bias)); CK(hipFree(gate)); CK(hipFree(Cb)); CK(hipFree(Cref));
  CK(hipFree(X)); CK(hipFree(X0)); CK(hipFree(Xref)); CK(hipFree(dcount));
}

// ------------------------------------------------------------------------------------- attention
// strided: q | k | v interleaved in one [Lq_pad, 3D] buffer (the engine's layout, row stride 3D) instead of three
// contiguous [Lq_pad, D] tensors
static void bench_attn(const char* name, int Lq_pad, int H, int valid, float q_amp, int rounds, int launches,
                       bool strided = false) {
  const int D = H * 128;
  const int LD = strided ? 3 * D : D;
  uint16_t *Q, *K, *V, *O, *Oref, *QKV = nullptr;
  if (strided) {
    CK(hipMalloc(&QKV, (size_t)Lq_pad * 3 * D * 2));
    fill_bf16<<<2048, 256>>>(QKV, (size_t)Lq_pad * 3 * D, 14, 1.0f * g_amp);
    Q = QKV; K = QKV + D; V = QKV + 2 * D;
  } else {
    CK(hipMalloc(&Q, (size_t)Lq_pad * D * 2));
    CK(hipMalloc(&K, (size_t)Lq_pad * D * 2));
    CK(hipMalloc(&V, (size_t)Lq_pad * D * 2));
  }
  CK(hipMalloc(&O, (size_t)Lq_pad * D * 2));
  CK(hipMalloc(&Oref, (size_t)Lq_pad * D * 2));
  unsigned long long* dcount;
  CK(hipMalloc(&dcount, 8));
  if (!strided) {
    fill_bf16<<<2048, 256>>>(Q, (size_t)Lq_pad * D, 11, q_amp * g_amp);   // post-RMSNorm q, k: unit variance
    fill_bf16<<<2048, 256>>>(K, (size_t)Lq_pad * D, 12, 1.0f * g_amp);
    fill_bf16<<<2048, 256>>>(V, (size_t)Lq_pad * D, 13, 1.0f * g_amp);
  }
  CK(hipDeviceSynchronize());
  const float scale = 1.0f / std::sqrt(128.0f);
  auto launch = [&](int l) {
    MCL(g_libs[l], g_libs[l].attn(Q, LD, K, LD, 0, V, LD, 0, O, D, Lq_pad, H, Lq_pad, valid, 1, scale, nullptr));
  };
  char what[64];
  snprintf(what, sizeof(what), "attn_%s", name);
  printf("# %s: Lq_pad=%d heads=%d valid keys=%d q_amp=%.1f\n", what, Lq_pad, H, valid, q_amp);
  measure(what, 4.0 * (double)valid * valid * D, "TF", 1e-12, rounds, launches, launch);
  std::vector<uint16_t> hq((size_t)Lq_pad * D), hk((size_t)Lq_pad * D), hv((size_t)Lq_pad * D), ho((size_t)Lq_pad * D);
  CK(hipMemcpy2D(hq.data(), (size_t)D * 2, Q, (size_t)LD * 2, (size_t)D * 2, Lq_pad, hipMemcpyDeviceToHost));
  CK(hipMemcpy2D(hk.data(), (size_t)D * 2, K, (size_t)LD * 2, (size_t)D * 2, Lq_pad, hipMemcpyDeviceToHost));
  CK(hipMemcpy2D(hv.data(), (size_t)D * 2, V, (size_t)LD * 2, (size_t)D * 2, Lq_pad, hipMemcpyDeviceToHost));
  for (size_t l = 0; l < g_libs.size(); ++l) {
    CK(hipMemset(O, 0xff, (size_t)Lq_pad * D * 2));
    launch((int)l);
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(ho.data(), O, ho.size() * 2, hipMemcpyDeviceToHost));
    // fp64 reference on 8 sampled (row, head) pairs
    double num = 0, den = 0;
    size_t nan = 0;
    for (int s = 0; s < 8; ++s) {
      const int row = (int)(((uint64_t)s * 2654435761ull + 12345) % (uint64_t)valid), head = s % H;
      std::vector<double> sc(valid);
      double mx = -1e300;
      for (int k = 0; k < valid; ++k) {
        double dot = 0;
        for (int d = 0; d < 128; ++d)
          dot += (double)bf16_to_f(hq[(size_t)row * D + head * 128 + d]) * bf16_to_f(hk[(size_t)k * D + head * 128 + d]);
        sc[k] = dot * scale;
        mx = std::max(mx, sc[k]);
      }
      double z = 0;
      std::vector<double> acc(128, 0.0);
      for (int k = 0; k < valid; ++k) {
        const double pw = std::exp(sc[k] - mx);
        z += pw;
        for (int d = 0; d < 128; ++d) acc[d] += pw * bf16_to_f(hv[(size_t)k * D + head * 128 + d]);
      }
      for (int d = 0; d < 128; ++d) {
        const double got = bf16_to_f(ho[(size_t)row * D + head * 128 + d]), want = acc[d] / z;
        if (got != got) ++nan;
        num += (got - want) * (got - want);
        den += want * want;
      }
    }
    printf("  %s lib%zu vs fp64 (8 rows): rel_l2 %.3e nan %zu", what, l, std::sqrt(num / den), nan);
    if (l == 0) {
      CK(hipMemcpy(Oref, O, (size_t)Lq_pad * D * 2, hipMemcpyDeviceToDevice));
      printf("\n");
    } else {
      CK(hipMemset(dcount, 0, 8));
      count_diff<<<1024, 256>>>((const uint32_t*)O, (const uint32_t*)Oref, (size_t)valid * D / 2, dcount);
      unsigned long long c;
      CK(hipMemcpy(&c, dcount, 8, hipMemcpyDeviceToHost));
      printf(" | vs lib0: %llu differing dwords\n", c);
    }
  }
  fflush(stdout);
  if (strided) { CK(hipFree(QKV)); } else { CK(hipFree(Q)); CK(hipFree(K)); CK(hipFree(V)); }
  CK(hipFree(O)); CK(hipFree(Oref)); CK(hipFree(dcount));
}

// Short-key sweep (cross-attention shapes): 32768 query rows against `keys` keys -- time per launch as a function of the
// key count separates the per-workgroup fixed cost (prologue, Q load, epilogue) from the per-tile cost.
static void bench_attn_keys(int Lq_pad, int H, int rounds, int launches) {
  const int D = H * 128;
  uint16_t *Q, *K, *V, *O;
  CK(hipMalloc(&Q, (size_t)Lq_pad * D * 2));
  CK(hipMalloc(&K, (size_t)4096 * D * 2));
  CK(hipMalloc(&V, (size_t)4096 * D * 2));
  CK(hipMalloc(&O, (size_t)Lq_pad * D * 2));
  fill_bf16<<<2048, 256>>>(Q, (size_t)Lq_pad * D, 11, 1.0f * g_amp);
  fill_bf16<<<2048, 256>>>(K, (size_t)4096 * D, 12, 1.0f * g_amp);
  fill_bf16<<<2048, 256>>>(V, (size_t)4096 * D, 13, 1.0f * g_amp);
  CK(hipDeviceSynchronize());
  const float scale = 1.0f / std::sqrt(128.0f);
  for (int keys : {64, 128, 256, 512, 1024, 2048, 4096}) {
    auto launch = [&](int l) {
      MCL(g_libs[l], g_libs[l].attn(Q, D, K, D, 0, V, D, 0, O, D, Lq_pad, H, keys, keys, 1, scale, nullptr));
    };
    char what[64];
    snprintf(what, sizeof(what), "attn_k%d", keys);
    measure(what, 4.0 * (double)Lq_pad * keys * D, "TF", 1e-12, rounds, launches, launch);
  }
  CK(hipFree(Q)); CK(hipFree(K)); CK(hipFree(V)); CK(hipFree(O));
}

// The opt-in MX fp8 self-attention beside the bf16 kernel on the same q, k, v -- library 0 only, the three launches interleaved
// round by round: attn (the bf16 line above), its pre-pass (quantise q, k, v: HBM-bound, GB/s of bf16 read + images written)
// and its kernel (TF over the same 4 L^2 D).  The outputs are two precisions of one result: their relative L2 distance is printed.
static void bench_attn_mx8(int Lq_pad, int H, int valid, int rounds, int launches) {
  const Lib& lib = g_libs[0];
  if (!lib.quant_mx8 || !lib.attn_mx8) {
    fprintf(stderr, "%s: no mc_op_attention_mx8\n", lib.path.c_str());
    exit(2);
  }
  const int D = H * 128;
  const size_t n = (size_t)Lq_pad * D;
  uint16_t *Q, *K, *V, *O, *O8;
  uint8_t* im[6];
  for (uint16_t** p : {&Q, &K, &V, &O, &O8}) CK(hipMalloc(p, n * 2));
  for (int i = 0; i < 6; ++i) CK(hipMalloc(&im[i], i % 2 ? n / 32 : n));   // q, qs, k, ks, vt, vs
  fill_bf16<<<2048, 256>>>(Q, n, 11, g_amp);
  fill_bf16<<<2048, 256>>>(K, n, 12, g_amp);
  fill_bf16<<<2048, 256>>>(V, n, 13, g_amp);
  CK(hipDeviceSynchronize());
  const float scale = 1.0f / std::sqrt(128.0f);
  auto launch = [&](int kind) {
    if (kind == 0) MCL(lib, lib.attn(Q, D, K, D, 0, V, D, 0, O, D, Lq_pad, H, Lq_pad, valid, 1, scale, nullptr));
    if (kind == 1) MCL(lib, lib.quant_mx8(Q, D, K, D, V, D, Lq_pad, H, Lq_pad, valid, scale, im[0], im[1], im[2], im[3], im[4], im[5], nullptr));
    if (kind == 2) MCL(lib, lib.attn_mx8(im[0], im[1], im[2], im[3], im[4], im[5], O8, D, Lq_pad, H, Lq_pad, valid, 1, nullptr, nullptr));
  };
  printf("# attn_mx8: Lq_pad=%d heads=%d valid keys=%d\n", Lq_pad, H, valid);
  hipEvent_t a, b;
  CK(hipEventCreate(&a));
  CK(hipEventCreate(&b));
  float ms = 0;
  CK(hipEventRecord(a, nullptr));
  do {   // ~1 s warm-up of all three
    for (int kind = 0; kind < 3; ++kind) launch(kind);
    CK(hipEventRecord(b, nullptr));
    CK(hipEventSynchronize(b));
    CK(hipEventElapsedTime(&ms, a, b));
  } while (ms < 1000.f);
  std::vector<double> t[3];
  for (int r = 0; r < rounds; ++r)
    for (int kind = 0; kind < 3; ++kind) {
      launch(kind);
      CK(hipEventRecord(a, nullptr));
      for (int i = 0; i < launches; ++i) launch(kind);
      CK(hipEventRecord(b, nullptr));
      CK(hipEventSynchronize(b));
      CK(hipEventElapsedTime(&ms, a, b));
      t[kind].push_back(ms / launches);
    }
  const char* names[3] = {"attn (bf16)", "mx8 pre-pass", "mx8 kernel"};
  const double work[3] = {4.0 * valid * (double)valid * D * 1e-12, (3.0 * n * 2 + 3.0 * n * 33 / 32) * 1e-9, 4.0 * valid * (double)valid * D * 1e-12};
  double med[3];
  for (int kind = 0; kind < 3; ++kind) {
    std::sort(t[kind].begin(), t[kind].end());
    med[kind] = t[kind][t[kind].size() / 2];
    printf("%-13s median %8.4f ms %8.1f %s | min %8.4f ms\n", names[kind], med[kind], work[kind] / (med[kind] * 1e-3), kind == 1 ? "GB/s" : "TF",
           t[kind][0]);
  }
  printf("mx8 kernel x%.3f, pre-pass + kernel x%.3f vs attn (bf16) (median)\n", med[0] / med[2], med[0] / (med[1] + med[2]));
  std::vector<uint16_t> h16(n), h8(n);
  CK(hipMemcpy(h16.data(), O, n * 2, hipMemcpyDeviceToHost));
  CK(hipMemcpy(h8.data(), O8, n * 2, hipMemcpyDeviceToHost));
  double num = 0, den = 0;
  for (size_t i = 0; i < (size_t)valid * D; ++i) {
    const double x = bf16_to_f(h16[i]), y = bf16_to_f(h8[i]);
    num += (x - y) * (x - y);
    den += x * x;
  }
  printf("  attn_mx8 vs attn (bf16): rel l2 %.3e over %d rows\n", std::sqrt(num / den), valid);
  fflush(stdout);
  for (void* p : {(void*)Q, (void*)K, (void*)V, (void*)O, (void*)O8}) CK(hipFree(p));
  for (int i = 0; i < 6; ++i) CK(hipFree(im[i]));
}

// The frame-block causal / windowed kernel beside the unmasked launch on the same q, k, v -- library 0 only, all launches
// interleaved round by round.  Per band: the time, its ratio to the unmasked launch, the fraction of (128-row item, 64-key
// tile) pairs the kernel visits, and the time against the ideal "fraction x unmasked time".  Eight rows of the first band are
// checked against an fp64 sum over their visible keys.
static void bench_attn_band(int Lq_pad, int H, int valid, int rounds, int launches) {
  const Lib& lib = g_libs[0];
  if (!lib.attn_band) {
    fprintf(stderr, "%s: no mc_op_attention_band\n", lib.path.c_str());
    exit(2);
  }
  struct BandCase { const char* name; int bt, win; };
  const int frame = valid / 21;   // 32760 = 21 latent frames of 1560 tokens
  const BandCase bands[] = {{"causal 21 blocks", frame, 0}, {"causal 7 blocks", 3 * frame, 0}, {"causal 3 blocks", 7 * frame, 0},
                            {"21 blocks, window 3", frame, 3}};
  constexpr int NB = 4;
  const int D = H * 128;
  const size_t n = (size_t)Lq_pad * D;
  uint16_t *Q, *K, *V, *O, *Ob;
  for (uint16_t** p : {&Q, &K, &V, &O, &Ob}) CK(hipMalloc(p, n * 2));
  fill_bf16<<<2048, 256>>>(Q, n, 11, g_amp);
  fill_bf16<<<2048, 256>>>(K, n, 12, g_amp);
  fill_bf16<<<2048, 256>>>(V, n, 13, g_amp);
  CK(hipDeviceSynchronize());
  const float scale = 1.0f / std::sqrt(128.0f);
  auto lo = [&](const BandCase& c, int b) { return c.win ? std::max(0, b - c.win + 1) * c.bt : 0; };
  auto hi = [&](const BandCase& c, int b) { return std::min((b + 1) * c.bt, valid); };
  auto blk = [&](const BandCase& c, int row) { return std::min(row, valid - 1) / c.bt; };
  auto launch = [&](int kind) {
    if (kind == 0) MCL(lib, lib.attn(Q, D, K, D, 0, V, D, 0, O, D, Lq_pad, H, Lq_pad, valid, 1, scale, nullptr));
    else MCL(lib, lib.attn_band(Q, D, K, D, V, D, Ob, D, Lq_pad, H, Lq_pad, valid, bands[kind - 1].bt, bands[kind - 1].win, scale, nullptr));
  };
  printf("# attn_band: Lq_pad=%d heads=%d valid keys=%d\n", Lq_pad, H, valid);
  hipEvent_t a, b;
  CK(hipEventCreate(&a));
  CK(hipEventCreate(&b));
  float ms = 0;
  CK(hipEventRecord(a, nullptr));
  do {   // ~1 s warm-up of all of them
    for (int kind = 0; kind <= NB; ++kind) launch(kind);
    CK(hipEventRecord(b, nullptr));
    CK(hipEventSynchronize(b));
    CK(hipEventElapsedTime(&ms, a, b));
  } while (ms < 1000.f);
  std::vector<double> t[NB + 1];
  for (int r = 0; r < rounds; ++r)
    for (int kind = 0; kind <= NB; ++kind) {
      launch(kind);
      CK(hipEventRecord(a, nullptr));
      for (int i = 0; i < launches; ++i) launch(kind);
      CK(hipEventRecord(b, nullptr));
      CK(hipEventSynchronize(b));
      CK(hipEventElapsedTime(&ms, a, b));
      t[kind].push_back(ms / launches);
    }
  double med[NB + 1];
  for (int kind = 0; kind <= NB; ++kind) {
    std::sort(t[kind].begin(), t[kind].end());
    med[kind] = t[kind][t[kind].size() / 2];
  }
  printf("%-20s median %8.4f ms %8.1f TF | min %8.4f ms\n", "attn (unmasked)", med[0], 4.0 * valid * (double)valid * D * 1e-12 / (med[0] * 1e-3), t[0][0]);
  for (int kind = 1; kind <= NB; ++kind) {
    const BandCase& c = bands[kind - 1];
    double visited = 0, all = 0;
    for (int q0 = 0; q0 < Lq_pad; q0 += 128) {
      visited += (hi(c, blk(c, q0 + 127)) - 1) / 64 - lo(c, blk(c, q0)) / 64 + 1;
      all += (valid + 63) / 64;
    }
    const double frac = visited / all;
    printf("%-20s median %8.4f ms | min %8.4f ms | x%.3f of unmasked | tiles visited %.4f, ideal %8.4f ms, measured / ideal %.3f\n", c.name,
           med[kind], t[kind][0], med[kind] / med[0], frac, frac * med[0], med[kind] / (frac * med[0]));
  }
  {   // spot check: the first band
    const BandCase& c = bands[0];
    launch(1);
    CK(hipDeviceSynchronize());
    std::vector<uint16_t> hq(n), hk(n), hv(n), ho(n);
    CK(hipMemcpy(hq.data(), Q, n * 2, hipMemcpyDeviceToHost));
    CK(hipMemcpy(hk.data(), K, n * 2, hipMemcpyDeviceToHost));
    CK(hipMemcpy(hv.data(), V, n * 2, hipMemcpyDeviceToHost));
    CK(hipMemcpy(ho.data(), Ob, n * 2, hipMemcpyDeviceToHost));
    double num = 0, den = 0;
    for (int i = 0; i < 8; ++i) {
      const int row = (int)(((long)i * 4099 + 17) % valid), head = i % H;
      const int k0 = lo(c, blk(c, row)), k1 = hi(c, blk(c, row));
      std::vector<double> s(k1 - k0);
      double mx = -1e300, z = 0, acc[128] = {0};
      for (int k = k0; k < k1; ++k) {
        double d = 0;
        for (int j = 0; j < 128; ++j) d += (double)bf16_to_f(hq[(size_t)row * D + head * 128 + j]) * bf16_to_f(hk[(size_t)k * D + head * 128 + j]);
        s[k - k0] = d * scale;
        mx = std::max(mx, s[k - k0]);
      }
      for (int k = k0; k < k1; ++k) {
        const double pw = std::exp(s[k - k0] - mx);
        z += pw;
        for (int j = 0; j < 128; ++j) acc[j] += pw * bf16_to_f(hv[(size_t)k * D + head * 128 + j]);
      }
      for (int j = 0; j < 128; ++j) {
        const double got = bf16_to_f(ho[(size_t)row * D + head * 128 + j]), want = acc[j] / z;
        num += (got - want) * (got - want);
        den += want * want;
      }
    }
    printf("  attn_band (%s) vs fp64 (8 rows): rel_l2 %.3e\n", c.name, std::sqrt(num / den));
  }
  fflush(stdout);
  for (void* p : {(void*)Q, (void*)K, (void*)V, (void*)O, (void*)Ob}) CK(hipFree(p));
}

// The tile-sparse kernel beside the unmasked launch (and, where a mask is a band rounded out to tiles, beside the band kernel)
// on the same q, k, v -- library 0 only, all launches interleaved round by round.  Every mask carries the heavy-first order
// table the engine would build for it.  Per mask: the time, its ratio to the unmasked launch, the density = visited (item,
// valid key tile) pairs over all of them, and the time against the ideal "density x unmasked time".  Eight rows of the
// temporal-decay mask are checked against an fp64 sum over their visible keys.
static void bench_attn_sparse(int Lq_pad, int H, int valid, int rounds, int launches) {
  const Lib& lib = g_libs[0];
  if (!lib.attn_sparse || !lib.attn_band) {
    fprintf(stderr, "%s: no mc_op_attention_sparse / mc_op_attention_band\n", lib.path.c_str());
    exit(2);
  }
  const int F = 21, tpf = valid / F;   // 32760 = 21 latent frames of 1560 tokens
  const int nqt = Lq_pad / 128, nkt = Lq_pad / 64, words = (nkt + 31) / 32, vk = (valid + 63) / 64;
  typedef std::vector<uint32_t> Bits;   // [nqt][words]
  auto span = [&](Bits& m, int qt, int k_lo, int k_hi) {   // keys k_lo .. k_hi (inclusive) -> their tiles
    for (int kt = k_lo / 64; kt <= k_hi / 64; ++kt) m[(size_t)qt * words + (kt >> 5)] |= 1u << (kt & 31);
  };
  auto band_cover = [&](int win) {   // the tile cover of 21 causal blocks, window `win` (0: all earlier blocks)
    Bits m((size_t)nqt * words, 0);
    for (int qt = 0; qt < nqt; ++qt) {
      const int b0 = std::min(qt * 128, valid - 1) / tpf, b1 = std::min(qt * 128 + 127, valid - 1) / tpf;
      span(m, qt, win ? std::max(0, b0 - win + 1) * tpf : 0, std::min((b1 + 1) * tpf, valid) - 1);
    }
    return m;
  };
  auto decay_cover = [&](int dense, int sink) {   // sparse_masks.temporal_decay_tile_mask, the same intervals
    Bits m((size_t)nqt * words, 0);
    for (int qt = 0; qt * 128 < valid; ++qt) {
      const int q0 = qt * 128, q1 = std::min(q0 + 127, valid - 1);
      for (int fi = q0 / tpf; fi <= q1 / tpf; ++fi) {
        const int a = std::max(q0, fi * tpf) - fi * tpf, b = std::min(q1, fi * tpf + tpf - 1) - fi * tpf;
        for (int fj = 0; fj < F; ++fj) {
          const int d = std::abs(fi - fj);
          if (d < dense || fj < sink) { span(m, qt, fj * tpf, fj * tpf + tpf - 1); continue; }
          int s = 1;
          while ((dense << s) <= d) ++s;
          const int w = (tpf + (1 << s) - 1) / (1 << s) - 1;
          span(m, qt, fj * tpf + std::max(a - w, 0), fj * tpf + std::min(b + w, tpf - 1));
        }
      }
    }
    return m;
  };
  struct MaskCase { const char* name; Bits even, odd; int band_win; };   // odd empty: one mask for every head; band_win < 0: no band twin
  const Bits ones((size_t)nqt * words, 0xffffffffu);
  std::vector<MaskCase> cases = {{"all bits set", ones, {}, -1}, {"21 causal blocks", band_cover(0), {}, 0},
                                 {"21 blocks, window 3", band_cover(3), {}, 3}, {"decay 1:1", decay_cover(1, 1), {}, -1},
                                 {"decay 2:1", decay_cover(2, 1), {}, -1}, {"decay 1:1 | window 3", decay_cover(1, 1), band_cover(3), -1}};
  const int NM = (int)cases.size();
  const int D = H * 128;
  const size_t n = (size_t)Lq_pad * D;
  uint16_t *Q, *K, *V, *O, *Ob;
  for (uint16_t** p : {&Q, &K, &V, &O, &Ob}) CK(hipMalloc(p, n * 2));
  fill_bf16<<<2048, 256>>>(Q, n, 11, g_amp);
  fill_bf16<<<2048, 256>>>(K, n, 12, g_amp);
  fill_bf16<<<2048, 256>>>(V, n, 13, g_amp);
  std::vector<uint32_t*> bits_dev(NM);
  std::vector<int32_t*> order_dev(NM);
  std::vector<double> density(NM);
  for (int c = 0; c < NM; ++c) {
    const int mh = cases[c].odd.empty() ? 1 : H;
    Bits all;
    for (int h = 0; h < mh; ++h) { const Bits& m = (h & 1) ? cases[c].odd : cases[c].even; all.insert(all.end(), m.begin(), m.end()); }
    std::vector<int> count((size_t)mh * nqt, 0);
    double visited = 0;
    for (int r = 0; r < mh * nqt; ++r) {
      for (int kt = 0; kt < vk; ++kt) count[r] += (all[(size_t)r * words + (kt >> 5)] >> (kt & 31)) & 1;
      visited += count[r];
    }
    density[c] = visited / ((double)mh * nqt * vk);
    std::vector<int32_t> order((size_t)nqt * H);
    for (size_t i = 0; i < order.size(); ++i) order[i] = (int32_t)i;
    auto cnt = [&](int32_t it) { return count[(size_t)(mh == 1 ? 0 : it % H) * nqt + it / H]; };
    std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) {
      return cnt(x) != cnt(y) ? cnt(x) > cnt(y) : x / H != y / H ? x / H > y / H : x < y;
    });
    CK(hipMalloc(&bits_dev[c], all.size() * 4));
    CK(hipMalloc(&order_dev[c], order.size() * 4));
    CK(hipMemcpy(bits_dev[c], all.data(), all.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(order_dev[c], order.data(), order.size() * 4, hipMemcpyHostToDevice));
  }
  CK(hipDeviceSynchronize());
  const float scale = 1.0f / std::sqrt(128.0f);
  // kinds: 0 unmasked, 1 .. NM the masks, NM + 1 / NM + 2 the band kernel at window 0 / 3
  const int NK = NM + 3;
  auto launch = [&](int kind) {
    if (kind == 0) MCL(lib, lib.attn(Q, D, K, D, 0, V, D, 0, O, D, Lq_pad, H, Lq_pad, valid, 1, scale, nullptr));
    else if (kind <= NM)
      MCL(lib, lib.attn_sparse(Q, D, K, D, V, D, Ob, D, Lq_pad, H, Lq_pad, valid, bits_dev[kind - 1], cases[kind - 1].odd.empty() ? 1 : H,
                               order_dev[kind - 1], scale, nullptr));
    else MCL(lib, lib.attn_band(Q, D, K, D, V, D, Ob, D, Lq_pad, H, Lq_pad, valid, tpf, kind == NM + 1 ? 0 : 3, scale, nullptr));
  };
  printf("# attn_sparse: Lq_pad=%d heads=%d valid keys=%d\n", Lq_pad, H, valid);
  hipEvent_t a, b;
  CK(hipEventCreate(&a));
  CK(hipEventCreate(&b));
  float ms = 0;
  CK(hipEventRecord(a, nullptr));
  do {   // ~1 s warm-up of all of them
    for (int kind = 0; kind < NK; ++kind) launch(kind);
    CK(hipEventRecord(b, nullptr));
    CK(hipEventSynchronize(b));
    CK(hipEventElapsedTime(&ms, a, b));
  } while (ms < 1000.f);
  std::vector<std::vector<double>> t(NK);
  for (int r = 0; r < rounds; ++r)
    for (int kind = 0; kind < NK; ++kind) {
      launch(kind);
      CK(hipEventRecord(a, nullptr));
      for (int i = 0; i < launches; ++i) launch(kind);
      CK(hipEventRecord(b, nullptr));
      CK(hipEventSynchronize(b));
      CK(hipEventElapsedTime(&ms, a, b));
      t[kind].push_back(ms / launches);
    }
  std::vector<double> med(NK);
  for (int kind = 0; kind < NK; ++kind) {
    std::sort(t[kind].begin(), t[kind].end());
    med[kind] = t[kind][t[kind].size() / 2];
  }
  printf("%-24s median %8.4f ms %8.1f TF | min %8.4f ms\n", "attn (unmasked)", med[0], 4.0 * valid * (double)valid * D * 1e-12 / (med[0] * 1e-3), t[0][0]);
  for (int kind = 1; kind <= NM; ++kind) {
    const MaskCase& c = cases[kind - 1];
    printf("%-24s median %8.4f ms | min %8.4f ms | x%.3f of unmasked | density %.4f, ideal %8.4f ms, measured / ideal %.3f", c.name, med[kind],
           t[kind][0], med[kind] / med[0], density[kind - 1], density[kind - 1] * med[0], med[kind] / (density[kind - 1] * med[0]));
    if (c.band_win >= 0) {
      const int bk = c.band_win == 0 ? NM + 1 : NM + 2;
      printf(" | band kernel %8.4f ms, sparse / band %.3f", med[bk], med[kind] / med[bk]);
    }
    printf("\n");
  }
  {   // spot check: the temporal-decay mask
    const Bits& m = cases[3].even;
    launch(4);
    CK(hipDeviceSynchronize());
    std::vector<uint16_t> hq(n), hk(n), hv(n), ho(n);
    CK(hipMemcpy(hq.data(), Q, n * 2, hipMemcpyDeviceToHost));
    CK(hipMemcpy(hk.data(), K, n * 2, hipMemcpyDeviceToHost));
    CK(hipMemcpy(hv.data(), V, n * 2, hipMemcpyDeviceToHost));
    CK(hipMemcpy(ho.data(), Ob, n * 2, hipMemcpyDeviceToHost));
    double num = 0, den = 0;
    for (int i = 0; i < 8; ++i) {
      const int row = (int)(((long)i * 4099 + 17) % valid), head = i % H;
      std::vector<int> keys;
      for (int k = 0; k < valid; ++k)
        if ((m[(size_t)(row / 128) * words + (k / 64 >> 5)] >> (k / 64 & 31)) & 1) keys.push_back(k);
      std::vector<double> s(keys.size());
      double mx = -1e300, z = 0, acc[128] = {0};
      for (size_t k = 0; k < keys.size(); ++k) {
        double d = 0;
        for (int j = 0; j < 128; ++j) d += (double)bf16_to_f(hq[(size_t)row * D + head * 128 + j]) * bf16_to_f(hk[(size_t)keys[k] * D + head * 128 + j]);
        s[k] = d * scale;
        mx = std::max(mx, s[k]);
      }
      for (size_t k = 0; k < keys.size(); ++k) {
        const double pw = std::exp(s[k] - mx);
        z += pw;
        for (int j = 0; j < 128; ++j) acc[j] += pw * bf16_to_f(hv[(size_t)keys[k] * D + head * 128 + j]);
      }
      for (int j = 0; j < 128; ++j) {
        const double got = bf16_to_f(ho[(size_t)row * D + head * 128 + j]), want = acc[j] / z;
        num += (got - want) * (got - want);
        den += want * want;
      }
    }
    printf("  attn_sparse (%s) vs fp64 (8 rows): rel_l2 %.3e\n", cases[3].name, std::sqrt(num / den));
  }
  fflush(stdout);
  for (void* p : {(void*)Q, (void*)K, (void*)V, (void*)O, (void*)Ob}) CK(hipFree(p));
  for (int c = 0; c < NM; ++c) { CK(hipFree(bits_dev[c])); CK(hipFree(order_dev[c])); }
}

// The self-attention chain of ONE rank of a sequence-parallel engine at the 1.3B 480p sp 4 geometry: 32760 tokens, 8190 per rank
// padded to 8192 query rows, 12 heads; the local shard ("kv_local" [8192][k | v]) with lse_out, then one gather round of 4 x 8192
// keys with this rank's shard skipped, merged in place through the lse.  The dense chain (mc_op_attention_partial of the LAST
// library given: the parent commit's build when one is named) and library 0's mc_op_attention_sparse_partial chain with all bits
// set and with the sharded cover of sparse_masks.temporal_decay_tile_mask's rule, interleaved round by round.
static void bench_attn_sparse_sp(int rounds, int launches) {
  const Lib &lib = g_libs[0], &base = g_libs.back();
  if (!lib.attn_sparse_partial || !base.attn_partial) {
    fprintf(stderr, "no mc_op_attention_sparse_partial (library 0) / mc_op_attention_partial (last library)\n");
    exit(2);
  }
  const int P = 4, rank = 1, H = 12, D = H * 128, L = 32760, Lr = L / P, Lp = 8192, F = 21, tpf = L / F;
  const int nqt = Lp / 128, tpr = Lp / 64, words = (P * tpr + 31) / 32, vk = (Lr + 63) / 64, vq = (Lr + 127) / 128;
  typedef std::vector<uint32_t> Bits;   // [nqt][words]
  auto span = [&](Bits& m, int qt, int k_lo, int k_hi) {   // global keys k_lo .. k_hi (inclusive) -> their tiles in every shard
    for (int p = 0; p < P; ++p) {
      const int lo = std::max(k_lo, p * Lr) - p * Lr, hi = std::min(k_hi, (p + 1) * Lr - 1) - p * Lr;
      for (int kt = lo / 64; lo <= hi && kt <= hi / 64; ++kt) m[(size_t)qt * words + ((p * tpr + kt) >> 5)] |= 1u << ((p * tpr + kt) & 31);
    }
  };
  auto decay_cover = [&](int dense, int sink) {   // sparse_masks.shard_tile_cover of temporal_decay_tile_mask's rule, by intervals
    Bits m((size_t)nqt * words, 0);
    for (int qt = 0; qt < vq; ++qt) {
      const int q0 = rank * Lr + qt * 128, q1 = rank * Lr + std::min(qt * 128 + 127, Lr - 1);
      for (int fi = q0 / tpf; fi <= q1 / tpf; ++fi) {
        const int a = std::max(q0, fi * tpf) - fi * tpf, b = std::min(q1, fi * tpf + tpf - 1) - fi * tpf;
        for (int fj = 0; fj < F; ++fj) {
          const int d = std::abs(fi - fj);
          if (d < dense || fj < sink) { span(m, qt, fj * tpf, fj * tpf + tpf - 1); continue; }
          int s = 1;
          while ((dense << s) <= d) ++s;
          const int w = (tpf + (1 << s) - 1) / (1 << s) - 1;
          span(m, qt, fj * tpf + std::max(a - w, 0), fj * tpf + std::min(b + w, tpf - 1));
        }
      }
    }
    return m;
  };
  struct MaskCase { const char* name; Bits bits; };
  const std::vector<MaskCase> cases = {{"all bits set", Bits((size_t)nqt * words, 0xffffffffu)}, {"decay 1:1", decay_cover(1, 1)},
                                       {"decay 2:1", decay_cover(2, 1)}};
  const int NM = (int)cases.size();
  std::vector<uint32_t*> bits_dev(NM);
  std::vector<double> density(NM);
  for (int c = 0; c < NM; ++c) {
    double visited = 0;
    for (int qt = 0; qt < vq; ++qt)
      for (int p = 0; p < P; ++p)
        for (int kt = 0; kt < vk; ++kt) visited += (cases[c].bits[(size_t)qt * words + ((p * tpr + kt) >> 5)] >> ((p * tpr + kt) & 31)) & 1;
    density[c] = visited / ((double)vq * P * vk);
    CK(hipMalloc(&bits_dev[c], cases[c].bits.size() * 4));
    CK(hipMemcpy(bits_dev[c], cases[c].bits.data(), cases[c].bits.size() * 4, hipMemcpyHostToDevice));
  }
  const size_t nq = (size_t)Lp * D, nkv = (size_t)Lp * 2 * D;
  uint16_t *Q, *KVl, *KVg, *O, *Ob;
  float *lse, *lse_b;
  CK(hipMalloc(&Q, nq * 2)); CK(hipMalloc(&O, nq * 2)); CK(hipMalloc(&Ob, nq * 2));
  CK(hipMalloc(&KVl, nkv * 2)); CK(hipMalloc(&KVg, P * nkv * 2));
  CK(hipMalloc(&lse, (size_t)H * Lp * 4)); CK(hipMalloc(&lse_b, (size_t)H * Lp * 4));
  fill_bf16<<<2048, 256>>>(Q, nq, 11, g_amp);
  fill_bf16<<<2048, 256>>>(KVg, P * nkv, 12, g_amp);
  CK(hipMemcpy(KVl, KVg + (size_t)rank * nkv, nkv * 2, hipMemcpyDeviceToDevice));
  CK(hipDeviceSynchronize());
  const float scale = 1.0f / std::sqrt(128.0f);
  const long ld = 2L * D, stride = (long)Lp * ld;
  auto launch = [&](int kind) {   // 0: the dense chain; 1 .. NM: the sparse chain under mask kind - 1
    if (kind == 0) {
      MCL(base, base.attn_partial(Q, D, KVl, ld, 0, KVl + D, ld, 0, O, D, Lp, H, Lp, Lr, 1, scale, -1, lse, nullptr, nullptr));
      MCL(base, base.attn_partial(Q, D, KVg, ld, stride, KVg + D, ld, stride, O, D, Lp, H, Lp, Lr, P, scale, rank, nullptr, lse, nullptr));
      return;
    }
    const uint32_t* bits = bits_dev[kind - 1];
    MCL(lib, lib.attn_sparse_partial(Q, D, KVl, ld, 0, KVl + D, ld, 0, Ob, D, Lp, H, Lp, Lr, 1, scale, -1, lse_b, nullptr, bits, 1, words,
                                     rank * tpr, 0, nullptr, nullptr));
    MCL(lib, lib.attn_sparse_partial(Q, D, KVg, ld, stride, KVg + D, ld, stride, Ob, D, Lp, H, Lp, Lr, P, scale, rank, nullptr, lse_b, bits, 1,
                                     words, 0, tpr, nullptr, nullptr));
  };
  const int NK = NM + 1;
  printf("# attn_sparse_sp: rank %d of %d, %d query rows (%d valid), %d heads, local shard + one round of %d x %d keys (own skipped)\n", rank, P,
         Lp, Lr, H, P, Lp);
  hipEvent_t a, b;
  CK(hipEventCreate(&a));
  CK(hipEventCreate(&b));
  float ms = 0;
  CK(hipEventRecord(a, nullptr));
  do {   // ~1 s warm-up of all of them
    for (int kind = 0; kind < NK; ++kind) launch(kind);
    CK(hipEventRecord(b, nullptr));
    CK(hipEventSynchronize(b));
    CK(hipEventElapsedTime(&ms, a, b));
  } while (ms < 1000.f);
  std::vector<std::vector<double>> t(NK);
  for (int r = 0; r < rounds; ++r)
    for (int kind = 0; kind < NK; ++kind) {
      launch(kind);
      CK(hipEventRecord(a, nullptr));
      for (int i = 0; i < launches; ++i) launch(kind);
      CK(hipEventRecord(b, nullptr));
      CK(hipEventSynchronize(b));
      CK(hipEventElapsedTime(&ms, a, b));
      t[kind].push_back(ms / launches);
    }
  std::vector<double> med(NK);
  for (int kind = 0; kind < NK; ++kind) {
    std::sort(t[kind].begin(), t[kind].end());
    med[kind] = t[kind][t[kind].size() / 2];
  }
  printf("%-22s median %8.4f ms %8.1f TF | min %8.4f ms\n", "dense chain", med[0], 4.0 * Lr * (double)L * D * 1e-12 / (med[0] * 1e-3), t[0][0]);
  for (int kind = 1; kind <= NM; ++kind)
    printf("%-22s median %8.4f ms | min %8.4f ms | x%.3f of dense | density %.4f, ideal %8.4f ms, measured / ideal %.3f\n", cases[kind - 1].name,
           med[kind], t[kind][0], med[kind] / med[0], density[kind - 1], density[kind - 1] * med[0], med[kind] / (density[kind - 1] * med[0]));
  printf("break-even density (dense / all bits set, time taken as linear in the density): %.3f\n", med[0] / med[1]);
  {   // all bits set against the dense chain: the largest element difference over the valid rows
    launch(0);
    launch(1);
    CK(hipDeviceSynchronize());
    std::vector<uint16_t> ho(nq), hb(nq);
    CK(hipMemcpy(ho.data(), O, nq * 2, hipMemcpyDeviceToHost));
    CK(hipMemcpy(hb.data(), Ob, nq * 2, hipMemcpyDeviceToHost));
    double worst = 0;
    for (size_t i = 0; i < (size_t)Lr * D; ++i) worst = std::max(worst, (double)std::fabs(bf16_to_f(ho[i]) - bf16_to_f(hb[i])));
    printf("  all bits set vs the dense chain: max |difference| %.3e\n", worst);
  }
  fflush(stdout);
  for (void* p : {(void*)Q, (void*)KVl, (void*)KVg, (void*)O, (void*)Ob, (void*)lse, (void*)lse_b}) CK(hipFree(p));
  for (int c = 0; c < NM; ++c) CK(hipFree(bits_dev[c]));
}

// The self-attention chain of EVERY rank of a sequence-parallel engine under sharded causal blocks, at the 1.3B 480p sp 4
// geometry with 4 gather rounds: 32760 tokens, 8190 per rank padded to 8192 query rows, 12 heads; the local shard with lse_out,
// then rounds c = 0 .. 3 of 4 x 2048 rows (2046 valid in the last) with this rank's shard skipped, merged in place through the
// lse -- the launches and arguments of sp_attn_launch.  The dense chain (mc_op_attention_partial of the LAST library given; it
// does not depend on the rank) and library 0's mc_op_attention_band_partial chain per (rank, band), interleaved round by round.
// The visited-tile fraction is the kernel's own walk (item's first row's lo .. last row's hi per shard) counted on the host.
static void bench_attn_band_sp(int rounds, int launches) {
  const Lib &lib = g_libs[0], &base = g_libs.back();
  if (!lib.attn_band_partial || !base.attn_partial) {
    fprintf(stderr, "no mc_op_attention_band_partial (library 0) / mc_op_attention_partial (last library)\n");
    exit(2);
  }
  const int P = 4, C = 4, H = 12, D = H * 128, L = 32760, Lr = L / P, Lp = 8192, Lc = Lp / C, F = 21, tpf = L / F, vq = (Lr + 127) / 128;
  struct BandCase { const char* name; int frames, window; };
  const std::vector<BandCase> cases = {{"causal 21 blocks", 1, 0}, {"causal 7 blocks", 3, 0}, {"causal 3 blocks", 7, 0}, {"21 blocks window 3", 1, 3}};
  const int NB = (int)cases.size();
  auto round_valid = [&](int c) { return std::max(0, std::min(Lc, Lr - c * Lc)); };
  auto tiles = [&](long glo, long ghi, long key0, int valid) {   // visited tiles of one shard: BandShards::tiles
    const long a = std::min<long>(std::max<long>(glo - key0, 0), valid), b = std::min<long>(std::max<long>(ghi - key0, 0), valid);
    return b > a ? (int)((b - 1) / 64 - a / 64 + 1) : 0;
  };
  auto fraction = [&](int rank, const BandCase& bc) {
    const long bt = (long)bc.frames * tpf;
    double visited = 0, dense = 0;
    for (int qt = 0; qt < vq; ++qt) {
      const long b0 = ((long)rank * Lr + std::min(qt * 128, Lr - 1)) / bt, b1 = ((long)rank * Lr + std::min(qt * 128 + 127, Lr - 1)) / bt;
      const long glo = bc.window ? std::max(0l, b0 - bc.window + 1) * bt : 0, ghi = (b1 + 1) * bt;
      visited += tiles(glo, ghi, (long)rank * Lr, Lr);
      dense += (Lr + 63) / 64;
      for (int c = 0; c < C; ++c)
        for (int p = 0; p < P; ++p)
          if (p != rank) {
            visited += tiles(glo, ghi, (long)c * Lc + (long)p * Lr, round_valid(c));
            dense += (round_valid(c) + 63) / 64;
          }
    }
    return visited / dense;
  };
  const size_t nq = (size_t)Lp * D, nkv = (size_t)Lp * 2 * D;
  uint16_t *Q, *KVl, *KVg, *O, *Ob;
  float *lse, *lse_b;
  CK(hipMalloc(&Q, nq * 2)); CK(hipMalloc(&O, nq * 2)); CK(hipMalloc(&Ob, nq * 2));
  CK(hipMalloc(&KVl, nkv * 2)); CK(hipMalloc(&KVg, P * nkv * 2));   // "kv_gather": [C][P][Lc][k | v]
  CK(hipMalloc(&lse, (size_t)H * Lp * 4)); CK(hipMalloc(&lse_b, (size_t)H * Lp * 4));
  fill_bf16<<<2048, 256>>>(Q, nq, 11, g_amp);
  fill_bf16<<<2048, 256>>>(KVg, P * nkv, 12, g_amp);
  fill_bf16<<<2048, 256>>>(KVl, nkv, 13, g_amp);
  CK(hipDeviceSynchronize());
  const float scale = 1.0f / std::sqrt(128.0f);
  const long ld = 2L * D, stride = (long)Lc * ld;
  auto launch = [&](int kind) {   // 0: the dense chain (as rank 1); 1 + rank * NB + band: the band chain
    if (kind == 0) {
      MCL(base, base.attn_partial(Q, D, KVl, ld, 0, KVl + D, ld, 0, O, D, Lp, H, Lp, Lr, 1, scale, -1, lse, nullptr, nullptr));
      for (int c = 0; c < C; ++c) {
        const uint16_t* kv = KVg + (size_t)c * P * Lc * ld;
        MCL(base, base.attn_partial(Q, D, kv, ld, stride, kv + D, ld, stride, O, D, Lp, H, Lc, round_valid(c), P, scale, 1,
                                    c + 1 < C ? lse : nullptr, lse, nullptr));
      }
      return;
    }
    const int rank = (kind - 1) / NB;
    const BandCase& bc = cases[(kind - 1) % NB];
    const int bt = bc.frames * tpf;
    MCL(lib, lib.attn_band_partial(Q, D, KVl, ld, 0, KVl + D, ld, 0, Ob, D, Lp, H, Lp, Lr, 1, scale, -1, lse_b, nullptr, bt, bc.window,
                                   rank * Lr, Lr, rank * Lr, 0, nullptr));
    for (int c = 0; c < C; ++c) {
      const uint16_t* kv = KVg + (size_t)c * P * Lc * ld;
      MCL(lib, lib.attn_band_partial(Q, D, kv, ld, stride, kv + D, ld, stride, Ob, D, Lp, H, Lc, round_valid(c), P, scale, rank,
                                     c + 1 < C ? lse_b : nullptr, lse_b, bt, bc.window, rank * Lr, Lr, c * Lc, Lr, nullptr));
    }
  };
  const int NK = 1 + P * NB;
  printf("# attn_band_sp: %d ranks, %d query rows (%d valid) each, %d heads, local shard + %d rounds of %d x %d rows (own skipped)\n", P, Lp,
         Lr, H, C, P, Lc);
  hipEvent_t a, b;
  CK(hipEventCreate(&a));
  CK(hipEventCreate(&b));
  float ms = 0;
  CK(hipEventRecord(a, nullptr));
  do {   // ~1 s warm-up of all of them
    for (int kind = 0; kind < NK; ++kind) launch(kind);
    CK(hipEventRecord(b, nullptr));
    CK(hipEventSynchronize(b));
    CK(hipEventElapsedTime(&ms, a, b));
  } while (ms < 1000.f);
  std::vector<std::vector<double>> t(NK);
  for (int r = 0; r < rounds; ++r)
    for (int kind = 0; kind < NK; ++kind) {
      launch(kind);
      CK(hipEventRecord(a, nullptr));
      for (int i = 0; i < launches; ++i) launch(kind);
      CK(hipEventRecord(b, nullptr));
      CK(hipEventSynchronize(b));
      CK(hipEventElapsedTime(&ms, a, b));
      t[kind].push_back(ms / launches);
    }
  std::vector<double> med(NK);
  for (int kind = 0; kind < NK; ++kind) {
    std::sort(t[kind].begin(), t[kind].end());
    med[kind] = t[kind][t[kind].size() / 2];
  }
  printf("%-22s median %8.4f ms %8.1f TF | min %8.4f ms\n", "dense chain", med[0], 4.0 * Lr * (double)L * D * 1e-12 / (med[0] * 1e-3), t[0][0]);
  for (int bi = 0; bi < NB; ++bi) {
    double worst = 0, sum = 0;
    for (int rank = 0; rank < P; ++rank) {
      const int kind = 1 + rank * NB + bi;
      const double f = fraction(rank, cases[bi]);
      printf("%-20s rank %d median %8.4f ms | min %8.4f ms | x%.3f of dense | visited %.4f, ideal %8.4f ms, measured / ideal %.3f\n",
             cases[bi].name, rank, med[kind], t[kind][0], med[kind] / med[0], f, f * med[0], med[kind] / (f * med[0]));
      worst = std::max(worst, med[kind]);
      sum += med[kind];
    }
    printf("%-20s slowest rank %8.4f ms = x%.3f of dense, x%.3f of the ranks' mean (the imbalance of the contiguous split)\n", cases[bi].name,
           worst, worst / med[0], worst * P / sum);
  }
  {   // one block of everything against the dense chain: the largest element difference over the valid rows
    const int bt = L;
    MCL(lib, lib.attn_band_partial(Q, D, KVl, ld, 0, KVl + D, ld, 0, Ob, D, Lp, H, Lp, Lr, 1, scale, -1, lse_b, nullptr, bt, 0, Lr, Lr, Lr, 0, nullptr));
    for (int c = 0; c < C; ++c) {
      const uint16_t* kv = KVg + (size_t)c * P * Lc * ld;
      MCL(lib, lib.attn_band_partial(Q, D, kv, ld, stride, kv + D, ld, stride, Ob, D, Lp, H, Lc, round_valid(c), P, scale, 1,
                                     c + 1 < C ? lse_b : nullptr, lse_b, bt, 0, Lr, Lr, c * Lc, Lr, nullptr));
    }
    launch(0);
    CK(hipDeviceSynchronize());
    std::vector<uint16_t> ho(nq), hb(nq);
    CK(hipMemcpy(ho.data(), O, nq * 2, hipMemcpyDeviceToHost));
    CK(hipMemcpy(hb.data(), Ob, nq * 2, hipMemcpyDeviceToHost));
    double worst = 0;
    for (size_t i = 0; i < (size_t)Lr * D; ++i) worst = std::max(worst, (double)std::fabs(bf16_to_f(ho[i]) - bf16_to_f(hb[i])));
    printf("  one block (rank 1) vs the dense chain: max |difference| %.3e\n", worst);
  }
  fflush(stdout);
  for (void* p : {(void*)Q, (void*)KVl, (void*)KVg, (void*)O, (void*)Ob, (void*)lse, (void*)lse_b}) CK(hipFree(p));
}

// The tile-mask predictor (library 0) beside the dense launch of the LAST library given (the parent commit's build, to compare
// with it in one process; library 0's own when it is the only one), all launches interleaved round by round.
//   with_sparse = false: the predictor alone at mass 0.9 on randn operands (its cost does not depend on the content).
//   with_sparse = true:  operands whose attention is concentrated -- q and k are randn plus 0.6 x a direction of the token's
//   latent frame (21 frames of 1560 tokens), q also 0.3 x the directions of the two neighbouring frames: the own frame scores
//   ~4 nats, its neighbours ~2 nats above the rest -- and per mass: predictor + sparse launch (order NULL, what the engine
//   runs), the sparse launch alone on the predicted bits, and the same with the heavy-first order table of the static path.
__global__ void add_frame_directions(uint16_t* p, int rows, int valid, int D, int tpf, float own, float side) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < (size_t)rows * D; i += (size_t)gridDim.x * blockDim.x) {
    const int row = (int)(i / D), col = (int)(i % D), f = min(row, valid - 1) / tpf;
    float v = bf16_to_f32_dev(p[i]) + own * randn((size_t)f * D + col, 77);
    if (side != 0.f) v += side * (randn((size_t)(f + 1) * D + col, 77) + (f ? randn((size_t)(f - 1) * D + col, 77) : 0.f));
    __bf16 b = (__bf16)v;
    p[i] = __builtin_bit_cast(uint16_t, b);
  }
}
static void bench_attn_predict(int Lq_pad, int H, int valid, int rounds, int launches, bool with_sparse) {
  const Lib& lib = g_libs[0];
  const Lib& dense = g_libs.back();
  if (!lib.predict || !lib.attn_sparse) {
    fprintf(stderr, "%s: no mc_op_attention_tile_predict / mc_op_attention_sparse\n", lib.path.c_str());
    exit(2);
  }
  auto scratch_bytes = (decltype(&mc_op_attention_tile_predict_scratch))dlsym(lib.h, "mc_op_attention_tile_predict_scratch");
  const int D = H * 128, nqt = Lq_pad / 128, nkt = Lq_pad / 64, words = (nkt + 31) / 32, vq = (valid + 127) / 128, vk = (valid + 63) / 64;
  const size_t n = (size_t)Lq_pad * D, nbits = (size_t)H * nqt * words;
  uint16_t *Q, *K, *V, *O, *Ob;
  for (uint16_t** p : {&Q, &K, &V, &O, &Ob}) CK(hipMalloc(p, n * 2));
  fill_bf16<<<2048, 256>>>(Q, n, 11, g_amp);
  fill_bf16<<<2048, 256>>>(K, n, 12, g_amp);
  fill_bf16<<<2048, 256>>>(V, n, 13, g_amp);
  if (with_sparse) {
    add_frame_directions<<<2048, 256>>>(Q, Lq_pad, valid, D, valid / 21, 0.6f, 0.3f);
    add_frame_directions<<<2048, 256>>>(K, Lq_pad, valid, D, valid / 21, 0.6f, 0.f);
  }
  const float masses[2] = {0.7f, 0.9f};
  const int NMASS = with_sparse ? 2 : 0;
  const float scale = 1.0f / std::sqrt(128.0f);
  void* scratch;
  uint32_t *bits_live, *bits[2];
  int32_t* order[2];
  double density[2] = {0, 0};
  CK(hipMalloc(&scratch, scratch_bytes(Lq_pad, H, Lq_pad)));
  CK(hipMalloc(&bits_live, nbits * 4));
  for (int m = 0; m < NMASS; ++m) {   // the bits of each mass, kept, and the order table the static path would build for them
    CK(hipMalloc(&bits[m], nbits * 4));
    CK(hipMalloc(&order[m], (size_t)nqt * H * 4));
    MCL(lib, lib.predict(Q, D, K, D, Lq_pad, H, Lq_pad, valid, scale, masses[m], bits[m], scratch, nullptr));
    std::vector<uint32_t> hb(nbits);
    CK(hipMemcpy(hb.data(), bits[m], nbits * 4, hipMemcpyDeviceToHost));
    std::vector<int> count((size_t)H * nqt, 0);
    for (int r = 0; r < H * nqt; ++r) {
      for (int kt = 0; kt < vk; ++kt) count[r] += (hb[(size_t)r * words + (kt >> 5)] >> (kt & 31)) & 1;
      if (r % nqt < vq) density[m] += count[r];
    }
    density[m] /= (double)H * vq * vk;
    std::vector<int32_t> ord((size_t)nqt * H);
    for (size_t i = 0; i < ord.size(); ++i) ord[i] = (int32_t)i;
    auto cnt = [&](int32_t it) { return count[(size_t)(it % H) * nqt + it / H]; };
    std::stable_sort(ord.begin(), ord.end(), [&](int32_t x, int32_t y) {
      return cnt(x) != cnt(y) ? cnt(x) > cnt(y) : x / H != y / H ? x / H > y / H : x < y;
    });
    CK(hipMemcpy(order[m], ord.data(), ord.size() * 4, hipMemcpyHostToDevice));
  }
  CK(hipDeviceSynchronize());
  // kinds: 0 dense, 1 predictor alone (mass 0.9); per mass m: 2 + 3 m predictor + sparse, 3 + 3 m sparse alone, 4 + 3 m sparse, heavy first
  const int NK = 2 + 3 * NMASS;
  auto launch = [&](int kind) {
    if (kind == 0) { MCL(dense, dense.attn(Q, D, K, D, 0, V, D, 0, O, D, Lq_pad, H, Lq_pad, valid, 1, scale, nullptr)); return; }
    if (kind == 1) { MCL(lib, lib.predict(Q, D, K, D, Lq_pad, H, Lq_pad, valid, scale, 0.9f, bits_live, scratch, nullptr)); return; }
    const int m = (kind - 2) / 3, sub = (kind - 2) % 3;
    if (sub == 0) MCL(lib, lib.predict(Q, D, K, D, Lq_pad, H, Lq_pad, valid, scale, masses[m], bits_live, scratch, nullptr));
    MCL(lib, lib.attn_sparse(Q, D, K, D, V, D, Ob, D, Lq_pad, H, Lq_pad, valid, sub == 0 ? bits_live : bits[m], H, sub == 2 ? order[m] : nullptr,
                             scale, nullptr));
  };
  printf("# attn_predict%s: Lq_pad=%d heads=%d valid keys=%d; dense launch of %s\n", with_sparse ? "_sparse" : "", Lq_pad, H, valid,
         dense.path.c_str());
  hipEvent_t a, b;
  CK(hipEventCreate(&a));
  CK(hipEventCreate(&b));
  float ms = 0;
  CK(hipEventRecord(a, nullptr));
  do {   // ~1 s warm-up of all of them
    for (int kind = 0; kind < NK; ++kind) launch(kind);
    CK(hipEventRecord(b, nullptr));
    CK(hipEventSynchronize(b));
    CK(hipEventElapsedTime(&ms, a, b));
  } while (ms < 1000.f);
  std::vector<std::vector<double>> t(NK);
  for (int r = 0; r < rounds; ++r)
    for (int kind = 0; kind < NK; ++kind) {
      launch(kind);
      CK(hipEventRecord(a, nullptr));
      for (int i = 0; i < launches; ++i) launch(kind);
      CK(hipEventRecord(b, nullptr));
      CK(hipEventSynchronize(b));
      CK(hipEventElapsedTime(&ms, a, b));
      t[kind].push_back(ms / launches);
    }
  std::vector<double> med(NK);
  for (int kind = 0; kind < NK; ++kind) {
    std::sort(t[kind].begin(), t[kind].end());
    med[kind] = t[kind][t[kind].size() / 2];
  }
  const double pool_bytes = 2.0 * valid * D * 2;
  printf("%-28s median %8.4f ms | min %8.4f ms\n", "attn (dense)", med[0], t[0][0]);
  printf("%-28s median %8.4f ms | min %8.4f ms | x%.4f of dense | one read of Q and K = %.1f MB: %.0f GB/s if it were all\n", "predict (mass 0.9)",
         med[1], t[1][0], med[1] / med[0], pool_bytes * 1e-6, pool_bytes * 1e-9 / (med[1] * 1e-3));
  for (int m = 0; m < NMASS; ++m) {
    const double* x = &med[2 + 3 * m];
    // t(density) ~ c density + predictor, c from this point: the density at which predictor + sparse would equal the dense launch
    const double breakeven = density[m] * (med[0] - (x[0] - x[1])) / x[1];
    printf("mass %.2f: density %.4f | predict + sparse %8.4f ms x%.3f of dense | sparse alone %8.4f ms | sparse, heavy first %8.4f ms "
           "(order NULL costs x%.3f) | break-even density %.3f\n", masses[m], density[m], x[0], x[0] / med[0], x[1], x[2], x[1] / x[2], breakeven);
  }
  fflush(stdout);
  for (void* p : {(void*)Q, (void*)K, (void*)V, (void*)O, (void*)Ob, (void*)scratch, (void*)bits_live}) CK(hipFree(p));
  for (int m = 0; m < NMASS; ++m) { CK(hipFree(bits[m])); CK(hipFree(order[m])); }
}

// The tile-sparse JOINT kernel (library 0) beside the dense launch of the LAST library given, on the MM-DiT engine's layout:
// q | k | v in one [Sp, 3d] buffer, O in [Sp, 5d].  The joint rows are [text ; image] (text_first) or [image ; text]; the ranges
// are the engine's (kalways = key tiles of the valid text rows, qdense = query tiles of the text rows).  Per density p: a random
// bitmap, one row per (head, query tile), each bit set with probability p; the launch with the kernel's own arithmetic item order
// (dense items first) and with the identity order passed as a table (memory order: in [image ; text] the dense tiles run last) --
// the difference is the tail the item order removes.  density = visited (item, valid key tile) pairs under the full rule over all
// pairs; ideal = density x dense time.  Last, the predictor (mass 0.9) on the same q and k as a share of the dense launch.
static void bench_attn_joint(const char* name, bool text_first, int Li, int Lt, const std::vector<double>& ps, int rounds, int launches) {
  const Lib& lib = g_libs[0];
  const Lib& dense = g_libs.back();
  auto joint = (mc_status (*)(const void*, long, const void*, long, const void*, long, void*, long, int, int, int, int, const uint32_t*, int,
                              int, int, int, int, const int32_t*, float, void*))dlsym(lib.h, "mc_op_attention_joint_sparse");
  auto scratch_bytes = (decltype(&mc_op_attention_tile_predict_scratch))dlsym(lib.h, "mc_op_attention_tile_predict_scratch");
  if (!joint || !lib.predict || !scratch_bytes) {
    fprintf(stderr, "%s: no mc_op_attention_joint_sparse / mc_op_attention_tile_predict\n", lib.path.c_str());
    exit(2);
  }
  const int H = 24, d = H * 128, S = Li + Lt, Sp = (S + 255) / 256 * 256, valid = S;
  const int nqt = Sp / 128, nkt = Sp / 64, words = (nkt + 31) / 32, vq = (S + 127) / 128, vk = (valid + 63) / 64;
  const int txt0 = text_first ? 0 : Li;
  const int q0 = txt0 / 128, q1 = (txt0 + Lt + 127) / 128, k0 = txt0 / 64, k1 = (txt0 + Lt + 63) / 64;
  const int NP = (int)ps.size();
  uint16_t *qkv, *am;
  CK(hipMalloc(&qkv, (size_t)Sp * 3 * d * 2));
  CK(hipMalloc(&am, (size_t)Sp * 5 * d * 2));
  fill_bf16<<<2048, 256>>>(qkv, (size_t)Sp * 3 * d, 31, g_amp);
  std::vector<uint32_t*> bits(NP);
  std::vector<double> density(NP);
  for (int c = 0; c < NP; ++c) {
    std::vector<uint32_t> m((size_t)H * nqt * words, 0);
    uint64_t lcg = 0x9e3779b97f4a7c15ull + (uint64_t)c;
    double visited = 0;
    for (int h = 0; h < H; ++h)
      for (int qt = 0; qt < nqt; ++qt)
        for (int kt = 0; kt < nkt; ++kt) {
          lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
          const bool bit = (double)(lcg >> 11) * (1.0 / 9007199254740992.0) < ps[c];
          if (bit) m[((size_t)h * nqt + qt) * words + (kt >> 5)] |= 1u << (kt & 31);
          if (qt < vq && kt < vk && (bit || (qt >= q0 && qt < q1) || (kt >= k0 && kt < k1))) visited += 1;
        }
    density[c] = visited / ((double)H * vq * vk);
    CK(hipMalloc(&bits[c], m.size() * 4));
    CK(hipMemcpy(bits[c], m.data(), m.size() * 4, hipMemcpyHostToDevice));
  }
  std::vector<int32_t> ident((size_t)nqt * H);
  for (size_t i = 0; i < ident.size(); ++i) ident[i] = (int32_t)i;
  int32_t* ident_dev;
  CK(hipMalloc(&ident_dev, ident.size() * 4));
  CK(hipMemcpy(ident_dev, ident.data(), ident.size() * 4, hipMemcpyHostToDevice));
  uint32_t* bits_live;
  void* scratch;
  CK(hipMalloc(&bits_live, (size_t)H * nqt * words * 4));
  CK(hipMalloc(&scratch, scratch_bytes(Sp, H, Sp)));
  CK(hipDeviceSynchronize());
  const float scale = 1.0f / std::sqrt(128.0f);
  const uint16_t *Q = qkv, *K = qkv + d, *V = qkv + 2 * d;
  // kinds: 0 dense (last library), 1 + 2c / 2 + 2c density c in arithmetic / identity order, 2 NP + 1 the predictor
  const int NK = 2 * NP + 2;
  auto launch = [&](int kind) {
    if (kind == 0) MCL(dense, dense.attn(Q, 3L * d, K, 3L * d, 0, V, 3L * d, 0, am, 5L * d, Sp, H, Sp, valid, 1, scale, nullptr));
    else if (kind <= 2 * NP)
      MCL(lib, joint(Q, 3L * d, K, 3L * d, V, 3L * d, am, 5L * d, Sp, H, Sp, valid, bits[(kind - 1) / 2], H, q0, q1, k0, k1,
                     (kind - 1) % 2 ? ident_dev : nullptr, scale, nullptr));
    else MCL(lib, lib.predict(Q, 3L * d, K, 3L * d, Sp, H, Sp, valid, scale, 0.9f, bits_live, scratch, nullptr));
  };
  printf("# attn_joint %s: %s, image %d + text %d rows padded to %d, %d heads, ld 3d / 5d; dense launch from %s\n", name,
         text_first ? "[text ; image]" : "[image ; text]", Li, Lt, Sp, H, dense.path.c_str());
  hipEvent_t a, b;
  CK(hipEventCreate(&a));
  CK(hipEventCreate(&b));
  float ms = 0;
  for (int kind = 0; kind < NK; ++kind) launch(kind);   // warm-up: every kind once, then the dense launch for ~0.5 s
  CK(hipEventRecord(a, nullptr));
  do {
    launch(0);
    CK(hipEventRecord(b, nullptr));
    CK(hipEventSynchronize(b));
    CK(hipEventElapsedTime(&ms, a, b));
  } while (ms < 500.f);
  std::vector<std::vector<double>> t(NK);
  for (int r = 0; r < rounds; ++r)
    for (int kind = 0; kind < NK; ++kind) {
      launch(kind);
      CK(hipEventRecord(a, nullptr));
      for (int i = 0; i < launches; ++i) launch(kind);
      CK(hipEventRecord(b, nullptr));
      CK(hipEventSynchronize(b));
      CK(hipEventElapsedTime(&ms, a, b));
      t[kind].push_back(ms / launches);
    }
  std::vector<double> med(NK);
  for (int kind = 0; kind < NK; ++kind) {
    std::sort(t[kind].begin(), t[kind].end());
    med[kind] = t[kind][t[kind].size() / 2];
  }
  printf("%-22s median %9.4f ms %7.1f TF | min %9.4f ms\n", "attn (dense)", med[0], 4.0 * valid * (double)valid * d * 1e-12 / (med[0] * 1e-3), t[0][0]);
  for (int c = 0; c < NP; ++c) {
    const double ar = med[1 + 2 * c], id = med[2 + 2 * c];
    printf("bitmap p %.2f: density %.4f | dense first %9.4f ms (min %9.4f) x%.3f of dense, measured / ideal %.3f | identity order %9.4f ms "
           "(min %9.4f) | identity / dense first %.3f\n", ps[c], density[c], ar, t[1 + 2 * c][0], ar / med[0], ar / (density[c] * med[0]), id,
           t[2 + 2 * c][0], id / ar);
  }
  printf("predictor (mass 0.9)   median %9.4f ms | min %9.4f ms | %.2f %% of the dense launch\n", med[NK - 1], t[NK - 1][0], 100.0 * med[NK - 1] / med[0]);
  fflush(stdout);
  for (void* p : {(void*)qkv, (void*)am, (void*)ident_dev, (void*)bits_live, scratch}) CK(hipFree(p));
  for (int c = 0; c < NP; ++c) CK(hipFree(bits[c]));
}

// ------------------------------------------------------------------------------------- calibration statistics
static void bench_calib(int M, int D, int rounds, int launches) {
  float *r, *rp, *stats;
  double *partial, *sums;
  CK(hipMalloc(&r, (size_t)M * D * 4));
  CK(hipMalloc(&rp, (size_t)M * D * 4));
  CK(hipMalloc(&partial, (2048 * 4 + 2) * 8));
  CK(hipMalloc(&sums, 32));
  CK(hipMalloc(&stats, 12));
  CK(hipMemset(partial, 0, (2048 * 4 + 2) * 8));
  fill_f32<<<2048, 256>>>(r, (size_t)M * D, 21, 1.0f, 0.f);
  fill_f32<<<2048, 256>>>(rp, (size_t)M * D, 22, 1.1f, 0.f);
  CK(hipDeviceSynchronize());
  auto launch = [&](int l) { MCL(g_libs[l], g_libs[l].calib(r, D, rp, D, M, D, partial, 2048, sums, stats, nullptr)); };
  printf("# calib_stats: 2 x [%d, %d] fp32\n", M, D);
  measure("calib_stats", 2.0 * M * D * 4, "GB/s", 1e-9, rounds, launches, launch);
  for (size_t l = 0; l < g_libs.size(); ++l) {
    launch((int)l);
    float hs[3];
    CK(hipMemcpy(hs, stats, 12, hipMemcpyDeviceToHost));
    printf("  calib_stats lib%zu: norm_ratio %.6f norm_std %.6f cos_dis %.6f\n", l, hs[0], hs[1], hs[2]);
  }
  CK(hipFree(r)); CK(hipFree(rp)); CK(hipFree(partial)); CK(hipFree(sums)); CK(hipFree(stats));
}

int main(int argc, char** argv) {
  if (argc < 5) {
    fprintf(stderr, "usage: kbench.bin <gemm|attn|attn_mx8|attn_band|attn_sparse|attn_sparse_sp|attn_band_sp|attn_joint|attn_predict|attn_predict_sparse|attn_keys|calib|all> <rounds> <launches> libA.so [libB.so ...]\n");
    return 2;
  }
  if (getenv("KBENCH_AMP")) g_amp = (float)atof(getenv("KBENCH_AMP"));
  const std::string what = argv[1];
  const int rounds = atoi(argv[2]), launches = atoi(argv[3]);
  for (int i = 4; i < argc; ++i) {
    Lib l;
    l.path = argv[i];
    l.h = dlopen(argv[i], RTLD_NOW | RTLD_LOCAL);
    if (!l.h) {
      fprintf(stderr, "dlopen %s: %s\n", argv[i], dlerror());
      return 2;
    }
    l.gemm = (decltype(l.gemm))dlsym(l.h, "mc_op_gemm_bf16");
    l.attn = (decltype(l.attn))dlsym(l.h, "mc_op_attention");
    l.calib = (decltype(l.calib))dlsym(l.h, "mc_op_calib_stats");
    l.quant_mx8 = (decltype(l.quant_mx8))dlsym(l.h, "mc_op_attn_quantize_mx8");
    l.attn_mx8 = (decltype(l.attn_mx8))dlsym(l.h, "mc_op_attention_mx8");
    l.attn_band = (decltype(l.attn_band))dlsym(l.h, "mc_op_attention_band");
    l.attn_sparse = (decltype(l.attn_sparse))dlsym(l.h, "mc_op_attention_sparse");
    l.predict = (decltype(l.predict))dlsym(l.h, "mc_op_attention_tile_predict");
    l.attn_partial = (decltype(l.attn_partial))dlsym(l.h, "mc_op_attention_partial");
    l.attn_sparse_partial = (decltype(l.attn_sparse_partial))dlsym(l.h, "mc_op_attention_sparse_partial");
    l.attn_band_partial = (decltype(l.attn_band_partial))dlsym(l.h, "mc_op_attention_band_partial");
    l.set_option = (decltype(l.set_option))dlsym(l.h, "mc_set_option");
    l.last_error = (decltype(l.last_error))dlsym(l.h, "mc_last_error");
    if (!l.gemm || !l.attn || !l.calib || !l.set_option || !l.last_error) {
      fprintf(stderr, "%s: missing symbols\n", argv[i]);
      return 2;
    }
    // KBENCH_OPT_<i>="key=value": a process-wide option of library i (e.g. gemm_kernel=1)
    char envn[32];
    snprintf(envn, sizeof(envn), "KBENCH_OPT_%d", i - 4);
    if (const char* o = getenv(envn)) {
      std::string s(o);
      const size_t eq = s.find('=');
      if (eq != std::string::npos) MCL(l, l.set_option(s.substr(0, eq).c_str(), atoi(s.c_str() + eq + 1)));
    }
    printf("lib%d = %s\n", i - 4, argv[i]);
    g_libs.push_back(l);
  }
  const int M = 32768;
  if (what == "gemm" || what == "all") {
    bench_gemm("qkv", M, 4608, 1536, 0, rounds, launches);
    bench_gemm("ffn1_gelu", M, 8960, 1536, 1, rounds, launches);
    bench_gemm("ffn2_resid", M, 1536, 8960, 2, rounds, launches);
    bench_gemm("o_resid", M, 1536, 1536, 2, rounds, launches);
    bench_gemm("o_bf16", M, 1536, 1536, 0, rounds, launches);
  }
  if (what == "attn" || what == "all") {
    bench_attn("self480p", 32768, 12, 32760, 1.0f, rounds, std::max(1, launches / 4));
    bench_attn("self480p_q6", 32768, 12, 32760, 6.0f, rounds, std::max(1, launches / 4));
  }
  if (what == "attn_mx8") bench_attn_mx8(32768, 12, 32760, rounds, std::max(1, launches / 4));
  if (what == "attn_band") bench_attn_band(32768, 12, 32760, rounds, std::max(1, launches / 4));
  if (what == "attn_sparse") bench_attn_sparse(32768, 12, 32760, rounds, std::max(1, launches / 4));
  if (what == "attn_sparse_sp") bench_attn_sparse_sp(rounds, std::max(1, launches / 4));
  if (what == "attn_band_sp") bench_attn_band_sp(rounds, std::max(1, launches / 4));
  if (what == "attn_predict") bench_attn_predict(32768, 12, 32760, rounds, std::max(1, launches / 4), false);
  if (what == "attn_predict_sparse") bench_attn_predict(32768, 12, 32760, rounds, std::max(1, launches / 4), true);
  if (what == "attn_joint") {
    // KBENCH_JOINT="first|last:image rows:text rows:p1,p2,..": one shape of the caller's; default: HunyuanVideo 720p 129 f and FLUX 1024^2
    if (const char* o = getenv("KBENCH_JOINT")) {
      char pos[8] = {0}, list[128] = {0};
      int li = 0, lt = 0;
      if (sscanf(o, "%7[a-z]:%d:%d:%127s", pos, &li, &lt, list) != 4 || li <= 0 || lt < 0) {
        fprintf(stderr, "KBENCH_JOINT=first|last:image rows:text rows:p1,p2,..\n");
        return 2;
      }
      std::vector<double> ps;
      for (char* tok = strtok(list, ","); tok; tok = strtok(nullptr, ",")) ps.push_back(atof(tok));
      bench_attn_joint("custom", std::string(pos) == "first", li, lt, ps, rounds, std::max(1, launches / 4));
    } else {
      bench_attn_joint("hunyuan720p", false, 118800, 256, {0.14, 0.45, 1.0}, rounds, std::max(1, launches / 16));
      bench_attn_joint("flux1024", true, 4096, 512, {0.14, 0.45, 1.0}, rounds, launches);
    }
  }
  if (what == "attn_strided" || what == "all") bench_attn("self480p_qkv", 32768, 12, 32760, 1.0f, rounds, std::max(1, launches / 4), true);
  if (what == "attn_keys") bench_attn_keys(32768, 12, rounds, launches);
  if (what == "attn1") bench_attn("self480p", 32768, 12, 32760, 1.0f, rounds, launches);          // one shape (PMC passes)
  if (what == "gemm1") bench_gemm("qkv", M, 4608, 1536, 0, rounds, launches);
  if (what == "calib" || what == "all") bench_calib(32760, 1536, rounds, launches * 2);
  return 0;
}
