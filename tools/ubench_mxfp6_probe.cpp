// Probe of v_mfma_scale_f32_16x16x128_f8f6f4 (gfx950) with FP6 (OCP e2m3) operands, cbsz / blgp = 2, before gemm_mxfp6.hip
// was built on it (round 14; the FP4 and e4m3 probes are tools/ubench_mx_probe.cpp).  One wave, exact data.  It establishes
//   * the e2m3 code book (all 64 codes against e4m3 1.0);
//   * which bits of the 32-byte operand argument are read, and which (k, code bit) each is: every one of the 256 bits of a
//     lane is set alone (magnitude bits) or cleared alone from an all-ones operand (sign bits, unread bits), against an e4m3
//     operand with a distinct value at every k -- the known e4m3 map is the yardstick;
//   * that the scale byte of lane group g, picked by op_sel, multiplies exactly the 32 codes of lane group g;
//   * FP6 x FP6 on random codes and scales 2^-1 .. 2^1 against the sum computed on the host (exact: every product is a multiple
//     of 2^-8 and the sums stay below 2^15);
//   * where the 12 bytes of each lane of a global_load_lds_dwordx3 land in the LDS (the GEMM's LDS-DMA pieces).  Finding that
//     shaped the kernel: at M0 + 16 l, NOT M0 + 12 l -- the lane stride is 16 bytes as for _dwordx4 and bytes 12..15 of every
//     16 stay unwritten, so a 96-byte row of 128 codes still takes 128 bytes of LDS, in 16-byte slots of 12.
// Log: profiles/r14/mxfp6_probe.log.
//   hipcc --offload-arch=gfx950 -O2 tools/ubench_mxfp6_probe.cpp -o tools/ubench_mxfp6_probe.bin
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

#define CK(x)                                                                       \
  do {                                                                              \
    hipError_t e_ = (x);                                                            \
    if (e_ != hipSuccess) {                                                         \
      printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); \
      exit(2);                                                                      \
    }                                                                               \
  } while (0)

template <int FA, int FB, int OPA, int OPB>
__global__ void k_mx_fmt(const i32x8* a, const i32x8* b, const int* sa, const int* sb, f32x4* out) {
  const int l = threadIdx.x;
  f32x4 c = {0.f, 0.f, 0.f, 0.f};
  c = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a[l], b[l], c, FA, FB, OPA, sa[l], OPB, sb[l]);
  out[l] = c;
}

// 64 lanes x 12 bytes from src to the LDS at byte offset lds_off, then the first 1280 bytes of the LDS to out
__global__ void k_dma_x3(const unsigned char* src, unsigned char* out, int lds_off) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int l = threadIdx.x;
  for (int i = l; i < 1280; i += 64) smem[i] = 0xEE;
  __syncthreads();
  const uint32_t off = l * 12;
  const uint32_t lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem + lds_off;
  asm volatile(
      "s_mov_b32 m0, %1\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx3 %0, %2\n\t"
      "s_waitcnt vmcnt(0)"
      :
      : "v"(off), "s"(__builtin_amdgcn_readfirstlane(lds)), "s"(src)
      : "memory", "m0");
  __syncthreads();
  for (int i = l; i < 1280; i += 64) out[i] = smem[i];
}

struct Dev {
  unsigned char *a, *b;
  int *sa, *sb;
  f32x4* out;
};

typedef std::vector<unsigned char> Bytes;

template <int FA, int FB, int OPA, int OPB>
static void run_fmt(Dev& d, const Bytes& A, const Bytes& B, const std::vector<int>& SA, const std::vector<int>& SB, float D[16][16]) {
  CK(hipMemcpy(d.a, A.data(), 2048, hipMemcpyHostToDevice));
  CK(hipMemcpy(d.b, B.data(), 2048, hipMemcpyHostToDevice));
  CK(hipMemcpy(d.sa, SA.data(), 256, hipMemcpyHostToDevice));
  CK(hipMemcpy(d.sb, SB.data(), 256, hipMemcpyHostToDevice));
  k_mx_fmt<FA, FB, OPA, OPB><<<1, 64>>>((i32x8*)d.a, (i32x8*)d.b, d.sa, d.sb, d.out);
  CK(hipDeviceSynchronize());
  float o[64][4];
  CK(hipMemcpy(o, d.out, sizeof(o), hipMemcpyDeviceToHost));
  for (int l = 0; l < 64; ++l)
    for (int r = 0; r < 4; ++r) D[4 * (l >> 4) + r][l & 15] = o[l][r];   // C/D map: col = lane%16, row = 4*(lane/16)+reg
}

static const unsigned char ONE = 0x38;   // e4m3 1.0
// e4m3 byte of the k-th of 128 distinct values (codes 0x08 + k / 2, all normal), sign = k & 1; the e4m3 operand map
static unsigned char e4m3_tag(int k) { return (unsigned char)((0x08 + (k >> 1)) | ((k & 1) << 7)); }
static float e4m3_value(unsigned char c) {
  const int e = (c >> 3) & 15, m = c & 7;
  const float v = (e ? (1.f + m / 8.f) * ldexpf(1.f, e - 7) : (m / 8.f) * ldexpf(1.f, -6));
  return (c & 0x80) ? -v : v;
}
static int e4m3_k(int g, int p) { return p < 16 ? 16 * g + p : 64 + 16 * g + (p - 16); }
static Bytes tagged(int row) {
  Bytes E(2048, 0);
  for (int g = 0; g < 4; ++g)
    for (int p = 0; p < 32; ++p) E[(16 * g + row) * 32 + p] = e4m3_tag(e4m3_k(g, p));
  return E;
}
static int k_of_tag_value(float v) {
  for (int k = 0; k < 128; ++k)
    if (e4m3_value(e4m3_tag(k)) == v) return k;
  return -1;
}
// the e2m3 code book as OCP MX v1.0 words it: bias 1, exponent field 0 is subnormal
static float e2m3_value(int c) {
  const int e = (c >> 3) & 3, m = c & 7;
  const float v = e ? (1.f + m / 8.f) * ldexpf(1.f, e - 1) : m / 8.f;
  return (c & 32) ? -v : v;
}
static void set_code(Bytes& X, int lane, int i, int code) {   // the order under test: code i at bits 6 i .. 6 i + 5 of the lane's bytes
  for (int b = 0; b < 6; ++b) {
    const int bit = 6 * i + b;
    unsigned char& byte = X[lane * 32 + bit / 8];
    byte = (unsigned char)((byte & ~(1 << (bit % 8))) | (((code >> b) & 1) << (bit % 8)));
  }
}

int main() {
  Dev d;
  CK(hipMalloc(&d.a, 2048));
  CK(hipMalloc(&d.b, 2048));
  CK(hipMalloc(&d.sa, 256));
  CK(hipMalloc(&d.sb, 256));
  CK(hipMalloc(&d.out, 1024));
  float D[16][16];
  const std::vector<int> S1(64, 127);

  // ---- code book: code c in bits 0..5 of lane 3, against e4m3 ones
  {
    int bad = 0;
    printf("code book (code c in bits 0..5 of byte 0 of lane 3, first operand FP6, second e4m3 1.0):\n ");
    for (int c = 0; c < 64; ++c) {
      Bytes A(2048, 0), B(2048, ONE);
      A[3 * 32] = (unsigned char)c;
      run_fmt<2, 0, 0, 0>(d, A, B, S1, S1, D);
      printf(" %g", D[3][0]);
      if (c % 16 == 15) printf("\n ");
      if (D[3][0] != e2m3_value(c)) ++bad;
    }
    printf("e2m3 code book (0 .. 0.875 by 0.125, 1 .. 1.875 by 0.125, 2 .. 3.75 by 0.25, 4 .. 7.5 by 0.5, bit 5 the sign): %s\n",
           bad ? "NO" : "PASS");
  }
  // ---- every bit of the 32 bytes of a lane, both operand positions.  Magnitude bits: the bit alone against ones gives the
  // code bit's value (0.125 0.25 0.5 1 2), against the tagged operand value * tag(k).  A bit that gives 0 alone is a sign bit
  // or is not read: with it set in an operand whose magnitude-bit-3 positions are all set (every code 1.0; found in the first
  // pass) the sum against ones drops from 128 to 126 for a sign bit, and against the tags by 2 tag(k).
  for (int which = 0; which < 2; ++which) {
    const int frow = which == 0 ? 3 : 5, erow = which == 0 ? 5 : 3;
    const Bytes E = tagged(erow);
    Bytes ones(2048, 0);
    for (int g = 0; g < 4; ++g) memset(&ones[(16 * g + erow) * 32], ONE, 32);
    float tagsum = 0.f;
    for (int k = 0; k < 128; ++k) tagsum += e4m3_value(e4m3_tag(k));
    int kmap[4][256], bmap[4][256];   // k and code bit (5 = sign, -1 = not read) of every bit
    for (int g = 0; g < 4; ++g)
      for (int bit = 0; bit < 256; ++bit) {
        Bytes F(2048, 0);
        F[(16 * g + frow) * 32 + bit / 8] = (unsigned char)(1 << (bit % 8));
        if (which == 0) run_fmt<2, 0, 0, 0>(d, F, ones, S1, S1, D); else run_fmt<0, 2, 0, 0>(d, ones, F, S1, S1, D);
        const float v = D[3][5];
        kmap[g][bit] = -1;
        bmap[g][bit] = v == 0.125f ? 0 : v == 0.25f ? 1 : v == 0.5f ? 2 : v == 1.f ? 3 : v == 2.f ? 4 : -1;
        if (bmap[g][bit] < 0) continue;
        if (which == 0) run_fmt<2, 0, 0, 0>(d, F, E, S1, S1, D); else run_fmt<0, 2, 0, 0>(d, E, F, S1, S1, D);
        kmap[g][bit] = k_of_tag_value(D[3][5] / v);
      }
    for (int g = 0; g < 4; ++g) {
      Bytes allone(2048, 0);   // every code 1.0 in every lane group of the row
      for (int g2 = 0; g2 < 4; ++g2)
        for (int bit = 0; bit < 256; ++bit)
          if (bmap[g2][bit] == 3) allone[(16 * g2 + frow) * 32 + bit / 8] |= (unsigned char)(1 << (bit % 8));
      for (int bit = 0; bit < 256; ++bit) {
        if (bmap[g][bit] >= 0) continue;
        Bytes F = allone;
        F[(16 * g + frow) * 32 + bit / 8] |= (unsigned char)(1 << (bit % 8));
        if (which == 0) run_fmt<2, 0, 0, 0>(d, F, ones, S1, S1, D); else run_fmt<0, 2, 0, 0>(d, ones, F, S1, S1, D);
        if (D[3][5] == 128.f) continue;   // not read
        if (D[3][5] != 126.f) { printf("  bit %d of lane group %d: all ones + this bit gives %g\n", bit, g, D[3][5]); continue; }
        bmap[g][bit] = 5;
        if (which == 0) run_fmt<2, 0, 0, 0>(d, F, E, S1, S1, D); else run_fmt<0, 2, 0, 0>(d, E, F, S1, S1, D);
        kmap[g][bit] = k_of_tag_value((tagsum - D[3][5]) / 2.f);
      }
    }
    bool ok = true;
    for (int g = 0; g < 4; ++g)
      for (int bit = 0; bit < 256; ++bit)
        ok &= bit < 192 ? (kmap[g][bit] == 32 * g + bit / 6 && bmap[g][bit] == bit % 6) : (bmap[g][bit] == -1);
    printf("%s operand FP6: bit b < 192 of lane group g's 32 bytes is bit b %% 6 of the code of k = 32 g + b / 6 (little-endian bit "
           "stream over bytes 0..23), bits 192..255 are not read: %s\n", which == 0 ? "first" : "second", ok ? "PASS" : "NO");
    if (!ok)
      for (int g = 0; g < 4; ++g) {
        printf("  g %d (k:codebit per bit):", g);
        for (int bit = 0; bit < 256; ++bit) printf(" %d:%d", kmap[g][bit], bmap[g][bit]);
        printf("\n");
      }
  }
  // ---- whose scale multiplies code i of lane group g?  scale = 2^(lane group), the other operand all 1.0 with unit scales
  Bytes allone(2048, 0);
  for (int l = 0; l < 64; ++l)
    for (int i = 0; i < 32; ++i) set_code(allone, l, i, 8);
  for (int which = 0; which < 2; ++which) {
    std::vector<int> SG(64);
    for (int l = 0; l < 64; ++l) SG[l] = 127 + (l >> 4);
    int bad = 0;
    for (int g = 0; g < 4; ++g)
      for (int i = 0; i < 32; ++i) {
        Bytes F(2048, 0);
        set_code(F, 16 * g + (which == 0 ? 3 : 5), i, 8);
        if (which == 0) run_fmt<2, 2, 0, 0>(d, F, allone, SG, S1, D); else run_fmt<2, 2, 0, 0>(d, allone, F, S1, SG, D);
        if (D[3][5] != (float)(1 << g)) { ++bad; printf("  operand %d (g %d, i %d): D = %g, expected %d\n", which, g, i, D[3][5], 1 << g); }
      }
    printf("%s operand FP6: the scale byte of lane group g multiplies all 32 codes of lane group g: %s\n",
           which == 0 ? "first" : "second", bad ? "NO" : "PASS");
  }
  {
    std::vector<int> SR(64), S4(64, 127 | (128 << 8) | (129 << 16) | (130 << 24));
    for (int l = 0; l < 64; ++l) SR[l] = 127 + (l & 15) % 4;
    run_fmt<2, 2, 0, 0>(d, allone, allone, SR, S1, D);
    printf("FP6 all ones, scaleA = 2^((lane%%16)%%4): D[i][0] i = 0..4: %g %g %g %g %g (expect 128 256 512 1024 128)\n", D[0][0], D[1][0],
           D[2][0], D[3][0], D[4][0]);
    run_fmt<2, 2, 0, 0>(d, allone, allone, S1, SR, D);
    printf("FP6 all ones, scaleB = 2^((lane%%16)%%4): D[0][j] j = 0..4: %g %g %g %g %g\n", D[0][0], D[0][1], D[0][2], D[0][3], D[0][4]);
    run_fmt<2, 2, 3, 0>(d, allone, allone, S4, S1, D);
    printf("FP6 op_sel A = 3: D[0][0] = %g (expect 1024)\n", D[0][0]);
    run_fmt<2, 2, 1, 0>(d, allone, allone, S4, S1, D);
    printf("FP6 op_sel A = 1: D[0][0] = %g (expect 256)\n", D[0][0]);
    run_fmt<2, 2, 0, 2>(d, allone, allone, S1, S4, D);
    printf("FP6 op_sel B = 2: D[0][0] = %g (expect 512)\n", D[0][0]);
  }
  // ---- FP6 x FP6, random codes, random scales 2^-1 .. 2^1 per (row, lane group), bytes 24..31 of every lane garbage
  {
    srand(14);
    int bad = 0;
    for (int rep = 0; rep < 8; ++rep) {
      Bytes A(2048), B(2048);
      for (auto& x : A) x = (unsigned char)rand();
      for (auto& x : B) x = (unsigned char)rand();
      int ca[64][32], cb[64][32];
      std::vector<int> SA(64), SB(64);
      for (int l = 0; l < 64; ++l) {
        SA[l] = 127 + rand() % 3 - 1;
        SB[l] = 127 + rand() % 3 - 1;
        for (int i = 0; i < 32; ++i) {
          ca[l][i] = rand() & 63, cb[l][i] = rand() & 63;
          set_code(A, l, i, ca[l][i]);
          set_code(B, l, i, cb[l][i]);
        }
      }
      run_fmt<2, 2, 0, 0>(d, A, B, SA, SB, D);
      for (int r = 0; r < 16; ++r)
        for (int c = 0; c < 16; ++c) {
          double s = 0;
          for (int g = 0; g < 4; ++g) {
            double t = 0;
            for (int i = 0; i < 32; ++i) t += (double)e2m3_value(ca[16 * g + r][i]) * e2m3_value(cb[16 * g + c][i]);
            s += t * ldexp(1.0, SA[16 * g + r] - 127 + SB[16 * g + c] - 127);
          }
          if ((double)D[r][c] != s) { if (++bad < 5) printf("  rep %d D[%d][%d] = %.9g, host %.9g\n", rep, r, c, D[r][c], s); }
        }
    }
    printf("FP6 x FP6, random codes and scales, 8 x 256 outputs equal the host sums (garbage in bytes 24..31): %s\n", bad ? "NO" : "PASS");
  }
  // ---- global_load_lds_dwordx3: lane l's 12 bytes land at M0 + 16 l, the other 4 bytes of each 16 are not written
  {
    unsigned char *src, *out;
    CK(hipMalloc(&src, 768));
    CK(hipMalloc(&out, 1280));
    Bytes S(768), O(1280);
    for (int i = 0; i < 768; ++i) S[i] = (unsigned char)(i * 7 + 1);
    CK(hipMemcpy(src, S.data(), 768, hipMemcpyHostToDevice));
    for (int lds_off : {0, 16, 208}) {
      k_dma_x3<<<1, 64, 1280>>>(src, out, lds_off);
      CK(hipDeviceSynchronize());
      CK(hipMemcpy(O.data(), out, 1280, hipMemcpyDeviceToHost));
      int bad = 0;
      for (int i = 0; i < 1280; ++i) {
        const int r = i - lds_off;   // lane r / 16, byte r % 16 of its slot
        const unsigned char want = (r >= 0 && r < 1024 && r % 16 < 12) ? S[r / 16 * 12 + r % 16] : 0xEE;
        if (O[i] != want) ++bad;
      }
      printf("global_load_lds_dwordx3, M0 = LDS base + %d: lane l's 12 bytes at M0 + 16 l, bytes 12..15 of every 16 and everything else unwritten: %s\n",
             lds_off, bad ? "NO" : "PASS");
      if (bad) {
        printf("  first 64 bytes:");
        for (int i = 0; i < 64; ++i) printf(" %02x", O[i]);
        printf("\n");
      }
    }
  }
  return 0;
}
