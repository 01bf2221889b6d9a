// Probe of v_mfma_scale_f32_16x16x128_f8f6f4 (gfx950) before building the MX fp8 GEMM on it: which k a lane's 32 bytes
// carry, which rows / k blocks a lane's scale byte applies to, what op_sel selects.  One wave; prints PASS / the values.
// Finding that mattered (last block of the output): the scale of lane group g multiplies k = 32 g .. 32 g + 31, but a
// lane's 32 bytes are k = 16 g + 0..15 and 64 + 16 g + 0..15 -- the all-ones tests above cannot see that.
// Second part (probe_fp4, round 12, before gemm_mxfp4.hip): the same instruction with FP4 (e2m1) operands -- the code book, which
// k nibble i of lane group g carries (against an e4m3 operand with a distinct value at every k: k = 32 g + i, the even i in the
// low nibble), which lane group's scale byte multiplies it, op_sel, and that only 16 bytes per lane are read
// (profiles/r12/mx_probe_fp4.log).
//   hipcc --offload-arch=gfx950 -O2 tools/ubench_mx_probe.cpp -o tools/ubench_mx_probe.bin
#include <hip/hip_runtime.h>

#include <cmath>
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

// a, b: [64 lanes][32 bytes]; sa, sb: [64] dwords; out: [64][4]
template <int OPA, int OPB>
__global__ void k_mx(const i32x8* a, const i32x8* b, const int* sa, const int* sb, f32x4* out) {
  const int l = threadIdx.x;
  f32x4 c = {0.f, 0.f, 0.f, 0.f};
  c = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a[l], b[l], c, 0, 0, OPA, sa[l], OPB, sb[l]);
  out[l] = c;
}

static const unsigned char ONE = 0x38;   // e4m3 1.0
static const unsigned char TWO = 0x40;   // e4m3 2.0

struct Dev {
  unsigned char *a, *b;
  int *sa, *sb;
  f32x4* out;
};

static void run(Dev& d, const std::vector<unsigned char>& A, const std::vector<unsigned char>& B, const std::vector<int>& SA,
                const std::vector<int>& SB, float D[16][16], int opa = 0, int opb = 0) {
  CK(hipMemcpy(d.a, A.data(), 2048, hipMemcpyHostToDevice));
  CK(hipMemcpy(d.b, B.data(), 2048, hipMemcpyHostToDevice));
  CK(hipMemcpy(d.sa, SA.data(), 256, hipMemcpyHostToDevice));
  CK(hipMemcpy(d.sb, SB.data(), 256, hipMemcpyHostToDevice));
  if (opa == 0 && opb == 0) k_mx<0, 0><<<1, 64>>>((i32x8*)d.a, (i32x8*)d.b, d.sa, d.sb, d.out);
  else if (opa == 1) k_mx<1, 0><<<1, 64>>>((i32x8*)d.a, (i32x8*)d.b, d.sa, d.sb, d.out);
  else if (opa == 2) k_mx<2, 0><<<1, 64>>>((i32x8*)d.a, (i32x8*)d.b, d.sa, d.sb, d.out);
  else if (opa == 3) k_mx<3, 0><<<1, 64>>>((i32x8*)d.a, (i32x8*)d.b, d.sa, d.sb, d.out);
  else k_mx<0, 2><<<1, 64>>>((i32x8*)d.a, (i32x8*)d.b, d.sa, d.sb, d.out);
  CK(hipDeviceSynchronize());
  float o[64][4];
  CK(hipMemcpy(o, d.out, sizeof(o), hipMemcpyDeviceToHost));
  for (int l = 0; l < 64; ++l)
    for (int r = 0; r < 4; ++r) D[4 * (l >> 4) + r][l & 15] = o[l][r];   // C/D map: col = lane%16, row = 4*(lane/16)+reg
}

// ---- FP4 (e2m1) operands on the same instruction: cbsz / blgp = 4 declare the first / second operand FP4; such an operand
// is 16 bytes per lane (the low four dwords of the register argument), two codes per byte.
template <int FA, int FB, int OPA, int OPB>
__global__ void k_mx_fmt(const i32x8* a, const i32x8* b, const int* sa, const int* sb, f32x4* out) {
  const int l = threadIdx.x;
  f32x4 c = {0.f, 0.f, 0.f, 0.f};
  c = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a[l], b[l], c, FA, FB, OPA, sa[l], OPB, sb[l]);
  out[l] = c;
}

template <int FA, int FB, int OPA, int OPB>
static void run_fmt(Dev& d, const std::vector<unsigned char>& A, const std::vector<unsigned char>& B, const std::vector<int>& SA,
                    const std::vector<int>& SB, float D[16][16]) {
  CK(hipMemcpy(d.a, A.data(), 2048, hipMemcpyHostToDevice));
  CK(hipMemcpy(d.b, B.data(), 2048, hipMemcpyHostToDevice));
  CK(hipMemcpy(d.sa, SA.data(), 256, hipMemcpyHostToDevice));
  CK(hipMemcpy(d.sb, SB.data(), 256, hipMemcpyHostToDevice));
  k_mx_fmt<FA, FB, OPA, OPB><<<1, 64>>>((i32x8*)d.a, (i32x8*)d.b, d.sa, d.sb, d.out);
  CK(hipDeviceSynchronize());
  float o[64][4];
  CK(hipMemcpy(o, d.out, sizeof(o), hipMemcpyDeviceToHost));
  for (int l = 0; l < 64; ++l)
    for (int r = 0; r < 4; ++r) D[4 * (l >> 4) + r][l & 15] = o[l][r];
}

// e4m3 byte of the k-th of 128 distinct values: magnitudes 2^-6 .. (codes 0x08 + k / 2, all normal), sign = k & 1
static unsigned char e4m3_tag(int k) { return (unsigned char)((0x08 + (k >> 1)) | ((k & 1) << 7)); }
static float e4m3_value(unsigned char c) {
  const int e = (c >> 3) & 15, m = c & 7;
  const float v = (e ? (1.f + m / 8.f) * ldexpf(1.f, e - 7) : (m / 8.f) * ldexpf(1.f, -6));
  return (c & 0x80) ? -v : v;
}
// the k (in the order the e4m3 probe above established: lane group g, byte p -> k = 16 g + p, 64 + 16 g + p - 16) of an
// e4m3 operand's (lane group, byte)
static int e4m3_k(int g, int p) { return p < 16 ? 16 * g + p : 64 + 16 * g + (p - 16); }

static void probe_fp4(Dev& d) {
  float D[16][16];
  std::vector<int> S1(64, 127);
  printf("---- FP4 (e2m1) operands\n");
  // every code of the code book against e4m3 1.0: first operand FP4 (cbsz = 4), second e4m3
  {
    std::vector<unsigned char> B(2048, ONE);
    printf("code book (one code in lane 3, low nibble of byte 0): ");
    for (int c = 0; c < 16; ++c) {
      std::vector<unsigned char> A(2048, 0);
      A[3 * 32] = (unsigned char)c;
      run_fmt<4, 0, 0, 0>(d, A, B, S1, S1, D);
      printf("%g ", D[3][0]);
    }
    printf("\n");
  }
  // which k does nibble i of lane group g carry?  FP4 one-hot (code 2 = 1.0) in the first operand, row 3; the second
  // operand is e4m3 with a distinct value at every k of column 5
  int map_a[4][32], map_b[4][32];
  for (int which = 0; which < 2; ++which)
    for (int g = 0; g < 4; ++g)
      for (int i = 0; i < 32; ++i) {
        std::vector<unsigned char> F(2048, 0), E(2048, 0);
        const int frow = which == 0 ? 3 : 5, erow = which == 0 ? 5 : 3;
        F[(16 * g + frow) * 32 + i / 2] = (unsigned char)(2 << (4 * (i & 1)));
        for (int g2 = 0; g2 < 4; ++g2)
          for (int p = 0; p < 32; ++p) E[(16 * g2 + erow) * 32 + p] = e4m3_tag(e4m3_k(g2, p));
        if (which == 0) run_fmt<4, 0, 0, 0>(d, F, E, S1, S1, D);
        else run_fmt<0, 4, 0, 0>(d, E, F, S1, S1, D);
        int k = -1;
        for (int kk = 0; kk < 128; ++kk)
          if (e4m3_value(e4m3_tag(kk)) == D[3][5]) k = kk;
        (which == 0 ? map_a : map_b)[g][i] = k;
      }
  for (int which = 0; which < 2; ++which) {
    bool consecutive = true;
    for (int g = 0; g < 4; ++g)
      for (int i = 0; i < 32; ++i) consecutive &= (which == 0 ? map_a : map_b)[g][i] == 32 * g + i;
    printf("%s operand FP4: k of nibble i (even i = low nibble of byte i / 2) of lane group g = 32 g + i: %s\n",
           which == 0 ? "first" : "second", consecutive ? "PASS" : "NO");
    if (!consecutive)
      for (int g = 0; g < 4; ++g) {
        printf("  g %d:", g);
        for (int i = 0; i < 32; ++i) printf(" %d", (which == 0 ? map_a : map_b)[g][i]);
        printf("\n");
      }
  }
  // both operands FP4: one-hot against one-hot, same (g, i) must meet and no other
  {
    int bad = 0;
    for (int g = 0; g < 4; ++g)
      for (int i : {0, 1, 2, 15, 16, 30, 31}) {
        std::vector<unsigned char> A(2048, 0), B(2048, 0);
        A[(16 * g + 3) * 32 + i / 2] = (unsigned char)(4 << (4 * (i & 1)));   // 2.0
        for (int g2 = 0; g2 < 4; ++g2)
          for (int b = 0; b < 16; ++b) B[(16 * g2 + 5) * 32 + b] = 0x22;      // 1.0 at every k
        run_fmt<4, 4, 0, 0>(d, A, B, S1, S1, D);
        if (D[3][5] != 2.f) ++bad;
        std::fill(B.begin(), B.end(), 0);
        B[(16 * g + 5) * 32 + i / 2] = (unsigned char)(6 << (4 * (i & 1)));   // 4.0 (code 6)
        run_fmt<4, 4, 0, 0>(d, A, B, S1, S1, D);
        if (D[3][5] != 8.f) { ++bad; printf("  FP4 x FP4 (g %d, i %d): D = %g, expected 8\n", g, i, D[3][5]); }
      }
    printf("FP4 x FP4: the same (lane group, nibble) of both operands meet: %s\n", bad ? "NO" : "PASS");
  }
  // whose scale multiplies nibble i of lane group g?  scale = 2^(lane group), the other operand all ones with unit scales
  for (int which = 0; which < 2; ++which) {
    std::vector<int> SG(64);
    for (int l = 0; l < 64; ++l) SG[l] = 127 + (l >> 4);
    int bad = 0;
    for (int g = 0; g < 4; ++g)
      for (int i = 0; i < 32; ++i) {
        std::vector<unsigned char> F(2048, 0), O(2048, 0x22);
        F[(16 * g + (which == 0 ? 3 : 5)) * 32 + i / 2] = (unsigned char)(2 << (4 * (i & 1)));
        if (which == 0) run_fmt<4, 4, 0, 0>(d, F, O, SG, S1, D);
        else run_fmt<4, 4, 0, 0>(d, O, F, S1, SG, D);
        if (D[3][5] != (float)(1 << g)) { ++bad; printf("  operand %d (g %d, i %d): D = %g, expected %d\n", which, g, i, D[3][5], 1 << g); }
      }
    printf("%s operand FP4: the scale byte of lane group g multiplies all 32 codes of lane group g: %s\n",
           which == 0 ? "first" : "second", bad ? "NO" : "PASS");
  }
  // the scale follows the lane's row, op_sel picks the byte
  {
    std::vector<unsigned char> A(2048, 0x22), B(2048, 0x22);
    std::vector<int> SR(64), S4(64, 127 | (128 << 8) | (129 << 16) | (130 << 24));
    for (int l = 0; l < 64; ++l) SR[l] = 127 + (l & 15) % 4;
    run_fmt<4, 4, 0, 0>(d, A, B, SR, S1, D);
    printf("FP4 all ones, scaleA = 2^((lane%%16)%%4): D[i][0] i = 0..4: %g %g %g %g %g (expect 128 256 512 1024 128)\n", D[0][0], D[1][0],
           D[2][0], D[3][0], D[4][0]);
    run_fmt<4, 4, 0, 0>(d, A, B, S1, SR, D);
    printf("FP4 all ones, scaleB = 2^((lane%%16)%%4): D[0][j] j = 0..4: %g %g %g %g %g\n", D[0][0], D[0][1], D[0][2], D[0][3], D[0][4]);
    run_fmt<4, 4, 3, 0>(d, A, B, S4, S1, D);
    printf("FP4 op_sel A = 3: D[0][0] = %g (expect 1024)\n", D[0][0]);
    run_fmt<4, 4, 0, 2>(d, A, B, S1, S4, D);
    printf("FP4 op_sel B = 2: D[0][0] = %g (expect 512)\n", D[0][0]);
    // the high four dwords of an FP4 operand register are ignored
    for (int l = 0; l < 64; ++l)
      for (int b = 16; b < 32; ++b) A[l * 32 + b] = 0x77, B[l * 32 + b] = 0x77;
    run_fmt<4, 4, 0, 0>(d, A, B, S1, S1, D);
    printf("FP4 all ones, bytes 16..31 of every lane = 0x77: D[0][0] = %g (expect 128: only 16 bytes per lane are read)\n", D[0][0]);
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
  std::vector<unsigned char> A(2048, ONE), B(2048, ONE);
  std::vector<int> SA(64, 127), SB(64, 127);

  run(d, A, B, SA, SB, D);
  printf("all ones, unit scales: D[0][0] = %g D[15][15] = %g (expect 128)\n", D[0][0], D[15][15]);

  // scale of the first operand follows the lane's row (lane % 16)
  for (int l = 0; l < 64; ++l) SA[l] = 127 + (l & 15) % 4;
  run(d, A, B, SA, SB, D);
  printf("scaleA = 2^((lane%%16)%%4): D[i][0] for i = 0..7: ");
  for (int i = 0; i < 8; ++i) printf("%g ", D[i][0]);
  printf("| D[0][j] j = 0..3: %g %g %g %g   (rows scale if the first operand indexes D rows)\n", D[0][0], D[0][1], D[0][2], D[0][3]);

  // scale follows the lane's k block (lane / 16)
  for (int l = 0; l < 64; ++l) SA[l] = 127 + (l >> 4);
  run(d, A, B, SA, SB, D);
  printf("scaleA = 2^(lane/16): D[0][0] = %g D[5][9] = %g (expect 32*(1+2+4+8) = 480 if a lane's byte scales its own 32 k)\n", D[0][0], D[5][9]);
  for (int l = 0; l < 64; ++l) SA[l] = 127;
  for (int l = 0; l < 64; ++l) SB[l] = 127 + (l >> 4);
  run(d, A, B, SA, SB, D);
  printf("scaleB = 2^(lane/16): D[0][0] = %g D[5][9] = %g (expect 480)\n", D[0][0], D[5][9]);
  for (int l = 0; l < 64; ++l) SB[l] = 127 + (l & 15) % 4;
  run(d, A, B, SA, SB, D);
  printf("scaleB = 2^((lane%%16)%%4): D[0][j] j = 0..7: ");
  for (int j = 0; j < 8; ++j) printf("%g ", D[0][j]);
  printf("\n");
  for (int l = 0; l < 64; ++l) SB[l] = 127;

  // op_sel: byte of the scale dword
  for (int l = 0; l < 64; ++l) SA[l] = 127 | (128 << 8) | (129 << 16) | (130 << 24);
  for (int op = 0; op < 4; ++op) {
    run(d, A, B, SA, SB, D, op, 0);
    printf("op_sel A = %d: D[0][0] = %g (expect %d)\n", op, D[0][0], 128 << op);
  }
  for (int l = 0; l < 64; ++l) SA[l] = 127;
  for (int l = 0; l < 64; ++l) SB[l] = 127 | (128 << 8) | (129 << 16) | (130 << 24);
  run(d, A, B, SA, SB, D, 0, 2);
  printf("op_sel B = 2: D[0][0] = %g (expect 512)\n", D[0][0]);
  for (int l = 0; l < 64; ++l) SB[l] = 127;

  // which k does byte p of lane (row, kb) carry?  one-hot A at (row 3, lane block kb, byte p) against one-hot B at
  // (col 5, lane block kb2, byte p2): non-zero iff they name the same k
  int bad = 0;
  for (int kb = 0; kb < 4; ++kb)
    for (int p : {0, 1, 7, 8, 15, 16, 17, 31}) {
      std::vector<unsigned char> A1(2048, 0), B1(2048, 0);
      A1[(16 * kb + 3) * 32 + p] = TWO;
      int hits = 0, hit_kb = -1, hit_p = -1;
      for (int kb2 = 0; kb2 < 4; ++kb2)
        for (int p2 = 0; p2 < 32; ++p2) {
          std::fill(B1.begin(), B1.end(), 0);
          B1[(16 * kb2 + 5) * 32 + p2] = ONE;
          run(d, A1, B1, SA, SB, D);
          if (D[3][5] != 0.f) {
            ++hits;
            hit_kb = kb2;
            hit_p = p2;
          }
        }
      const bool ok = hits == 1 && hit_kb == kb && hit_p == p;
      if (!ok) {
        ++bad;
        printf("A one-hot (kb %d, byte %d) meets B at (kb %d, byte %d), %d hits\n", kb, p, hit_kb, hit_p, hits);
      }
    }
  printf("k of byte p in lane block kb = 32 kb + p for both operands: %s\n", bad ? "NO (see above)" : "PASS");

  // whose scale multiplies the products of lane group kb?  A one-hot (row 3, lane group kb), B all ones, scaleA = 2^(lane/16)
  for (int l = 0; l < 64; ++l) SA[l] = 127 + (l >> 4);
  for (int l = 0; l < 64; ++l) SB[l] = 127;
  for (int kb = 0; kb < 4; ++kb) {
    std::vector<unsigned char> A1(2048, 0), B1(2048, ONE);
    A1[(16 * kb + 3) * 32 + 5] = TWO;
    run(d, A1, B1, SA, SB, D);
    printf("A one-hot in lane group %d, scaleA = 2^(lane group): D[3][0] = %g (2 * 2^g: the scale of lane group g was applied)\n", kb, D[3][0]);
  }
  for (int l = 0; l < 64; ++l) SA[l] = 127;
  for (int l = 0; l < 64; ++l) SB[l] = 127 + (l >> 4);
  for (int kb = 0; kb < 4; ++kb) {
    std::vector<unsigned char> A1(2048, ONE), B1(2048, 0);
    B1[(16 * kb + 5) * 32 + 9] = TWO;
    run(d, A1, B1, SA, SB, D);
    printf("B one-hot in lane group %d, scaleB = 2^(lane group): D[0][5] = %g\n", kb, D[0][5]);
  }
  probe_fp4(d);
  return 0;
}
