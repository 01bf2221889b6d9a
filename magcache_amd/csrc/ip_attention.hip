// IP-Adapter cross-attention of the FLUX double block (diffusers FluxIPAdapterJointAttnProcessor2_0):
//   out[row, head] = sum_j scale_j * softmax(q_n[row, head] . K_j[head]^T / sqrt(128)) V_j[head]
// over up to kIpMaxAdapters image-prompt adapters with 1..kIpMaxKeys keys each; q_n is the image stream's q after norm_q and
// BEFORE RoPE.  The launch runs in front of launch_headnorm_rope, which rotates q in place, so the kernel reads the raw q
// columns of "qkv" and normalises them itself: the sums of headnorm_rope_kernel in that kernel's summation tree and its two
// roundings, so the value is that kernel's value without a table bit for bit, bf16(bf16(q rstd) w).
//
// One block = 4 waves = one head x 128 query rows; a wave owns 32 rows.
//   1. norm: the wave's 32 raw rows into its LDS image [32][128] bf16 (rows padded to 272 bytes); a lane (query row =
//      lane & 31, half = lane >> 5) sums the squares of its half of the row, joins lane ^ 32, and normalises the 8 B-operand
//      fragments of Q^T it takes from the image and keeps for good.
//   2. per adapter, per tile of 32 keys: the block stages K [32 keys][128] and V^T [128][32 keys] of the head in LDS (a key
//      row past `valid` re-reads row valid - 1 and its score is masked: pad rows of the cache are never read).
//      S^T = K Q^T on 8 MFMAs (32x32x16 bf16): key on the registers, query row on the lane, so the row maximum and sum are 16
//      registers and one exchange with lane ^ 32.  Online softmax in fp32 (log2 domain), then the accumulator is the B operand
//      of O^T += V^T P with no lane movement: registers 8s .. 8s + 7 converted pairwise are the fragment of k-step s, whose
//      element j of lane half h is key 16s + 8(j >> 2) + 4h + (j & 3) -- which is how the V^T fragments are read.
//   3. total += O^T scale_j / l per adapter in fp32; one bf16 rounding; through the wave's LDS image to 16-byte row stores.
// An adapter with scale 0 is left out by the launcher; with none left the rows are written as zeros.
#include "common.h"
#include "ops.h"

namespace mc {
namespace {

constexpr int IP_QROW = 272;   // bytes per row of a [32][128] bf16 LDS image: 256 + 16, so that 16-byte reads of 32 rows spread
constexpr int IP_VROW = 80;    // bytes per row of the V^T image [128][32 keys]: 64 + 16
constexpr int IP_IMG = 32 * IP_QROW;
constexpr int IP_LDS = 4 * IP_IMG;   // the four waves' images; K (IP_IMG) and V^T (128 * IP_VROW) tiles reuse the front
static_assert(IP_IMG + 128 * IP_VROW <= IP_LDS, "K and V^T tiles live in the query images' space");

struct IpArgs {
  const bf16_t* kv[kIpMaxAdapters];
  long ld[kIpMaxAdapters];
  int valid[kIpMaxAdapters];
  float scale[kIpMaxAdapters];
  int n;
};

// a thread's 16 bytes of K and of V of key rows key0 + (tid >> 4) and 16 further (a row past `valid`: row valid - 1 again)
__device__ __forceinline__ void ip_fetch(const bf16_t* kv, long ld, int valid, int d, int tid, int key0, u32x4 (&kk)[2], u32x4 (&vv)[2]) {
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const bf16_t* src = kv + (size_t)min(key0 + (tid >> 4) + 16 * u, valid - 1) * ld + (tid & 15) * 8;
    kk[u] = *(const u32x4*)src;
    vv[u] = *(const u32x4*)(src + d);
  }
}

// Step 2 for one adapter (kv: its rows at the head's columns; V is d columns behind K) over all its keys:
// o = sum_k 2^(s_k - m) V_k, unnormalised; returns sum_k 2^(s_k - m).  ks / vs: the block's K and V^T tiles.
MC_NO_PK_F32 __device__ __forceinline__ float ip_attend(const bf16_t* kv, long ld, int valid, int d, int tid, int r, int h,
                                                        const bf16x8 (&qf)[8], char* ks, char* vs, f32x16 (&o)[4]) {
  const float sl2 = 0.08838834764831845f * 1.4426950408889634f;   // 1 / sqrt(128) in the log2 domain
  float m = -INFINITY, l = 0.f;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int g = 0; g < 16; ++g) o[t][g] = 0.f;

  // a thread's share of a tile: 16 bytes of K and of V of key rows (tid >> 4) and 16 + (tid >> 4); the next tile's share is
  // on its way from memory while this tile's products run
  u32x4 kk[2], vv[2];
  ip_fetch(kv, ld, valid, d, tid, 0, kk, vv);
#pragma unroll 1
  for (int key0 = 0; key0 < valid; key0 += 32) {
    __syncthreads();   // the fragments of Q, or the previous tile, have been read
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int key = (tid >> 4) + 16 * u, c8 = (tid & 15) * 8;
      *(u32x4*)(ks + key * IP_QROW + c8 * 2) = kk[u];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        *(uint16_t*)(vs + (c8 + 2 * e) * IP_VROW + key * 2) = (uint16_t)(vv[u][e] & 0xffffu);
        *(uint16_t*)(vs + (c8 + 2 * e + 1) * IP_VROW + key * 2) = (uint16_t)(vv[u][e] >> 16);
      }
    }
    __syncthreads();
    if (key0 + 32 < valid) ip_fetch(kv, ld, valid, d, tid, key0 + 32, kk, vv);
    // S^T[key][query row]: register g is key (g & 3) + 8 (g >> 2) + 4 h of the tile, the lane's column is query row r
    f32x16 st;
#pragma unroll
    for (int g = 0; g < 16; ++g) st[g] = 0.f;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const bf16x8 kf = *(const bf16x8*)(ks + r * IP_QROW + (16 * s + 8 * h) * 2);
      st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[s], st, 0, 0, 0);
    }
    float mx = -INFINITY;
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const int key = key0 + (g & 3) + 8 * (g >> 2) + 4 * h;
      st[g] = key < valid ? st[g] * sl2 : -INFINITY;
      mx = fmaxf(mx, st[g]);
    }
    mx = half_swap_max(mx);               // key0 < valid: at least one key of the tile counts, mx is finite
    const float m_new = fmaxf(m, mx);
    const float alpha = __builtin_amdgcn_exp2f(m - m_new);   // first tile: 2^-inf = 0
    float sum = 0.f;
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      st[g] = __builtin_amdgcn_exp2f(st[g] - m_new);   // a masked key: 2^-inf = 0
      sum += st[g];
    }
    l = l * alpha + half_swap_sum(sum);
    m = m_new;
    bf16x8 pf[2];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int e = 0; e < 8; ++e) pf[s][e] = (__bf16)st[8 * s + e];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
      for (int g = 0; g < 16; ++g) o[t][g] *= alpha;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        // A operand V^T[channel 32 t + r][key]: elements 0..3 keys 16 s + 4 h + (0..3), elements 4..7 eight keys further
        const char* vr = vs + (32 * t + r) * IP_VROW + (16 * s + 4 * h) * 2;
        const bf16x4 lo = *(const bf16x4*)vr, hi = *(const bf16x4*)(vr + 16);
        const bf16x8 vf = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
        o[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf[s], o[t], 0, 0, 0);
      }
    }
  }
  return l;
}

// MODE 0: any number of adapters.  MODE 1: exactly one adapter (a.n == 1), the common case: no second set of 64
// accumulators.  MODE 2 (the test entry launch_ip_attention_qnorm): stop after step 1 and store q_n itself.
template <int MODE>
MC_NO_PK_F32 __global__ __launch_bounds__(256) void ip_attention_kernel(const bf16_t* __restrict__ q, long ldq,
                                                                       const float* __restrict__ wq, float eps, IpArgs a,
                                                                       bf16_t* __restrict__ out, long ldo, int rows, int d) {
  __shared__ __attribute__((aligned(16))) char lds[IP_LDS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  // heads run fastest over the grid: the blocks in flight together read and write whole rows, not one 256-byte column of all
  const int head = blockIdx.x;
  const int row0 = (blockIdx.y * 4 + wave) * 32;   // may lie past `rows`: such a wave computes on row rows - 1 and stores nothing
  char* img = lds + wave * IP_IMG;

  // ---- 1. q_n of the wave's 32 rows: headnorm_rope_kernel's arithmetic (no table), in this kernel's layout.  That kernel
  // holds pair i = (2i, 2i+1) of a row on lane i and sums the 64 squares with wave_sum, the xor butterfly 32, 16, .., 1: a
  // fixed tree over the pair index whatever lane evaluates it (a + b is b + a bit for bit).  Here a lane owns half a row: the
  // pairs i = 2k + h, k = 0..31, whose tree levels 32 .. 2 pair k with k ^ 16 .. k ^ 1 inside the lane; the last level (xor 1)
  // joins the two halves, lane ^ 32.  The same sums in the same tree, with one cross-lane step per row where the butterfly
  // has six, and all 32 rows of a wave at once.
  {
    uint32_t raw[32];   // all 32 row loads in flight together
#pragma unroll
    for (int i = 0; i < 32; ++i) raw[i] = ((const uint32_t*)(q + (size_t)min(row0 + i, rows - 1) * ldq + head * 128))[lane];
#pragma unroll
    for (int i = 0; i < 32; ++i) *(uint32_t*)(img + i * IP_QROW + lane * 4) = raw[i];
  }
  __syncthreads();
  float rstd;
  {
    float p[32];
#pragma unroll
    for (int k = 0; k < 32; ++k) {
      const uint32_t b = *(const uint32_t*)(img + r * IP_QROW + 8 * k + 4 * h);
      const float re = __uint_as_float(b << 16), im = __uint_as_float(b & 0xffff0000u);
      p[k] = re * re + im * im;
    }
#pragma unroll
    for (int n = 16; n >= 1; n >>= 1)
#pragma unroll
      for (int k = 0; k < n; ++k) p[k] = p[k] + p[k + n];
    rstd = rsqrtf(half_swap_sum(p[0]) * (1.0f / 128.0f) + eps);
  }
  bf16x8 qf[8];   // B operand of S^T = K Q^T: Q[row r][16 s + 8 h + j], normalised: bf16(bf16(q rstd) w)
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    const u32x4 b = *(const u32x4*)(img + r * IP_QROW + (16 * s + 8 * h) * 2);
    const f32x4 w0 = *(const f32x4*)(wq + 16 * s + 8 * h), w1 = *(const f32x4*)(wq + 16 * s + 8 * h + 4);
    const float w[8] = {w0[0], w0[1], w0[2], w0[3], w1[0], w1[1], w1[2], w1[3]};
    u32x4 y;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float re = __uint_as_float(b[j] << 16), im = __uint_as_float(b[j] & 0xffff0000u);
      re = bf16_round(re * rstd) * w[2 * j];
      im = bf16_round(im * rstd) * w[2 * j + 1];
      y[j] = pack_bf16x2(re, im);
    }
    qf[s] = __builtin_bit_cast(bf16x8, y);
  }
  if constexpr (MODE == 2) {
    __syncthreads();   // every lane has read the raw rows
#pragma unroll
    for (int s = 0; s < 8; ++s) *(bf16x8*)(img + r * IP_QROW + (16 * s + 8 * h) * 2) = qf[s];
    __syncthreads();
  } else {
    char* ks = lds;            // [32 keys][IP_QROW]
    char* vs = lds + IP_IMG;   // [128 channels][IP_VROW]
    f32x16 total[4];
    if constexpr (MODE == 1) {
      const float w = a.scale[0] / ip_attend(a.kv[0] + head * 128, a.ld[0], a.valid[0], d, tid, r, h, qf, ks, vs, total);
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int g = 0; g < 16; ++g) total[t][g] *= w;
    } else {
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int g = 0; g < 16; ++g) total[t][g] = 0.f;
#pragma unroll 1
      for (int j = 0; j < a.n; ++j) {
        f32x16 o[4];
        const float w = a.scale[j] / ip_attend(a.kv[j] + head * 128, a.ld[j], a.valid[j], d, tid, r, h, qf, ks, vs, o);
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int g = 0; g < 16; ++g) total[t][g] += o[t][g] * w;
      }
    }
    // ---- 3. O^T register g of tile t: channel 32 t + (g & 3) + 8 (g >> 2) + 4 h of query row r -> the wave's image
    __syncthreads();   // the last K / V^T tile has been read
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const u32x2 p = {pack_bf16x2(total[t][4 * g4], total[t][4 * g4 + 1]), pack_bf16x2(total[t][4 * g4 + 2], total[t][4 * g4 + 3])};
        *(u32x2*)(img + r * IP_QROW + (32 * t + 8 * g4 + 4 * h) * 2) = p;
      }
    __syncthreads();
  }
  // the wave's image (the result; MODE 2: q_n) -> its rows, 16 bytes per lane
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int i = lane + 64 * u, rr = i >> 4, c8 = (i & 15) * 8;
    if (row0 + rr < rows)
      *(u32x4*)(out + (size_t)(row0 + rr) * ldo + head * 128 + c8) = *(const u32x4*)(img + rr * IP_QROW + c8 * 2);
  }
}

bool ip_misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }
bool ip_rows_ok(const bf16_t* q, long ldq, const float* wq, const bf16_t* out, long ldo, int rows, int heads) {
  const long d = (long)heads * 128;
  return q && wq && out && rows >= 1 && rows <= 65535 * 128 && heads >= 1 && ldq >= d && (ldq % 8) == 0 && ldo >= d && (ldo % 8) == 0 &&
         !ip_misaligned(q) && !ip_misaligned(wq) && !ip_misaligned(out);
}

}  // namespace

hipError_t launch_ip_attention(const bf16_t* q, long ldq, const float* wq, float eps, const IpKeys* adapters, int n_adapters,
                               bf16_t* out, long ldo, int rows, int heads, hipStream_t stream) {
  if (!adapters || n_adapters < 1 || n_adapters > kIpMaxAdapters || !ip_rows_ok(q, ldq, wq, out, ldo, rows, heads)) return hipErrorInvalidValue;
  const long d = (long)heads * 128;
  IpArgs a = {};
  for (int j = 0; j < n_adapters; ++j) {
    const IpKeys& k = adapters[j];
    if (!k.kv || ip_misaligned(k.kv) || k.ld < 2 * d || (k.ld % 8) != 0 || k.valid < 1 || k.valid > kIpMaxKeys) return hipErrorInvalidValue;
    if (k.scale == 0.f) continue;   // left out here: the kernel sees the adapters that count
    a.kv[a.n] = k.kv; a.ld[a.n] = k.ld; a.valid[a.n] = k.valid; a.scale[a.n] = k.scale;
    ++a.n;
  }
  const dim3 grid((unsigned)heads, (unsigned)((rows + 127) / 128));
  if (a.n == 1) hipLaunchKernelGGL(ip_attention_kernel<1>, grid, dim3(256), 0, stream, q, ldq, wq, eps, a, out, ldo, rows, (int)d);
  else hipLaunchKernelGGL(ip_attention_kernel<0>, grid, dim3(256), 0, stream, q, ldq, wq, eps, a, out, ldo, rows, (int)d);
  return hipGetLastError();
}

hipError_t launch_ip_attention_qnorm(const bf16_t* q, long ldq, const float* wq, float eps, bf16_t* out, long ldo, int rows, int heads,
                                     hipStream_t stream) {
  if (!ip_rows_ok(q, ldq, wq, out, ldo, rows, heads)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ip_attention_kernel<2>, dim3((unsigned)heads, (unsigned)((rows + 127) / 128)), dim3(256), 0, stream, q, ldq, wq,
                     eps, IpArgs{}, out, ldo, rows, heads * 128);
  return hipGetLastError();
}

}  // namespace mc
