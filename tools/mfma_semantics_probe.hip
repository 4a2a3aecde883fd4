// Probe of MFMA arithmetic semantics the NCF certified pre-filter relies on:
//  (a) v_mfma_f32_32x32x2_f32: is D = fma(a1, b1, fma(a0, b0, c)) bitwise (k = lane half)?
//  (b) v_mfma_f32_32x32x16_f16: are f16 denormal inputs kept (not flushed)?
//  (c) v_mfma_f32_32x32x16_f16: is the accumulation exact-product + fp32 rounding no worse
//      than a sequential fp32 sum (max |err| vs a double reference, in fp32 ulps)?
//  (d) v_smfmac_f32_16x16x64_f16 (A with 2:4 structured sparsity): which stored A value (lane,
//      element, position bits) meets which B half (lane, element), found by one-hot operands; how
//      the index VGPR and abid select positions; D's layout; then, on the map found, random
//      operands against a host loop, denormals and exact products.
// Build: hipcc --offload-arch=gfx950 -O3 tools/mfma_semantics_probe.hip -o build/mfma_sem
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// (a) one 32x32x2 step per launch slot: A[i][k], B[k][j], C[i][j] random
__global__ void f32_step(const float* A, const float* B, const float* C, float* D) {
  const int l = threadIdx.x, r = l & 31, h = l >> 5;
  f32x16 c;
  for (int q = 0; q < 16; ++q) c[q] = C[((q & 3) + 8 * (q >> 2) + 4 * h) * 32 + r];
  c = __builtin_amdgcn_mfma_f32_32x32x2f32(A[r * 2 + h], B[h * 32 + r], c, 0, 0, 0);
  for (int q = 0; q < 16; ++q) D[((q & 3) + 8 * (q >> 2) + 4 * h) * 32 + r] = c[q];
}

// (b)/(c) one 32x32x16 f16 MFMA: A[i][k] (32x16), B[k][j] (16x32), C = 0
__global__ void f16_step(const _Float16* A, const _Float16* B, float* D) {
  const int l = threadIdx.x, r = l & 31, h = l >> 5;
  h8 a, b;
  for (int e = 0; e < 8; ++e) {
    a[e] = A[r * 16 + 8 * h + e];
    b[e] = B[(8 * h + e) * 32 + r];
  }
  f32x16 c = {};
  c = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
  for (int q = 0; q < 16; ++q) D[((q & 3) + 8 * (q >> 2) + 4 * h) * 32 + r] = c[q];
}

// (d) discovery: block (a, f, v) puts a 1 into stored A value f of lane a, with every group's index
// nibble = nib[v], and walks a 1 through the 1,024 B halves (lane L, element e).  hit[block][L * 16
// + e] = 4 * lane + register of the one D value that became 1, -1 for none, -2 for anything else.
template <int ABID>
__global__ void sp_pairs(const int* nib, int* hit) {
  const int lane = threadIdx.x, a = blockIdx.x >> 3, f = blockIdx.x & 7, v = blockIdx.y;
  h8 av;
  for (int e = 0; e < 8; ++e) av[e] = (lane == a && e == f) ? (_Float16)1.f : (_Float16)0.f;
  // the 16 index bits of the selected half; the other half holds the complementary positions
  const int lo = nib[v] * 0x1111, other = (nib[v] ^ 0xA) * 0x1111;
  const int idx = ABID ? (lo << 16) | other : (other << 16) | lo;
  for (int s = 0; s < 1024; ++s) {
    h16 bv;
    for (int e = 0; e < 16; ++e) bv[e] = (lane == (s >> 4) && e == (s & 15)) ? (_Float16)1.f : (_Float16)0.f;
    f32x4 c = {};
    c = __builtin_amdgcn_smfmac_f32_16x16x64_f16(av, bv, c, idx, 0, ABID);
    int mine = -1, n = 0;
    for (int r = 0; r < 4; ++r)
      if (c[r] != 0.f) {
        mine = c[r] == 1.f ? 4 * lane + r : -2;
        ++n;
      }
    if (n > 1) mine = -2;
    const unsigned long long any = __ballot(n > 0);
    int res = -1;
    if (any) {
      const int src = __builtin_ctzll(any);
      res = (any & (any - 1)) ? -2 : __shfl(mine, src);
    }
    if (lane == 0) hit[((size_t)v * 512 + blockIdx.x) * 1024 + s] = res;
  }
}

// (d) one instruction on given operands: lane l's 8 stored A values, its index bits, 16 B halves
// and 4 accumulator values in, 4 D values out
__global__ void sp_step(const _Float16* A, const int* idx, const _Float16* B, const float* C, float* D) {
  const int l = threadIdx.x;
  h8 a;
  h16 b;
  f32x4 c;
  for (int e = 0; e < 8; ++e) a[e] = A[l * 8 + e];
  for (int e = 0; e < 16; ++e) b[e] = B[l * 16 + e];
  for (int r = 0; r < 4; ++r) c[r] = C[l * 4 + r];
  c = __builtin_amdgcn_smfmac_f32_16x16x64_f16(a, b, c, idx[l], 0, 0);
  for (int r = 0; r < 4; ++r) D[l * 4 + r] = c[r];
}

static float frand() { return (float)rand() / RAND_MAX * 2.f - 1.f; }

// (d): see the header.  slot[ga][f][p] = 16 g + e: stored value f of a lane in A k-group ga, at
// position p of its group of four, meets element e of the B lanes of k-group g.
static void sparse_probe() {
  static const int nibs[6] = {0x4, 0xE, 0x8, 0xD, 0xC, 0x9};  // (p0, p1) = 01 23 02 13 03 12
  static const int pos[6][2] = {{0, 1}, {2, 3}, {0, 2}, {1, 3}, {0, 3}, {1, 2}};
  int *nib, *hit;
  hipMallocManaged(&nib, sizeof(nibs));
  hipMallocManaged(&hit, (size_t)6 * 512 * 1024 * 4);
  for (int v = 0; v < 6; ++v) nib[v] = nibs[v];
  int slot[4][8][4];
  bool have = false;
  for (int abid = 0; abid < 2; ++abid) {
    if (abid) hipLaunchKernelGGL(sp_pairs<1>, dim3(512, 6), dim3(64), 0, 0, nib, hit);
    else hipLaunchKernelGGL(sp_pairs<0>, dim3(512, 6), dim3(64), 0, 0, nib, hit);
    if (hipDeviceSynchronize() != hipSuccess) { printf("(d) launch failed\n"); return; }
    int s2[4][8][4], bad = 0, badd = 0, incons = 0;
    for (int ga = 0; ga < 4; ++ga) for (int f = 0; f < 8; ++f) for (int p = 0; p < 4; ++p) s2[ga][f][p] = -1;
    for (int v = 0; v < 6; ++v)
      for (int a = 0; a < 64; ++a)
        for (int f = 0; f < 8; ++f) {
          const int* hrow = hit + ((size_t)v * 512 + a * 8 + f) * 1024;
          int n = 0, sl = -1;
          unsigned cols = 0;
          for (int s = 0; s < 1024; ++s) {
            if (hrow[s] == -1) continue;
            const int L = s >> 4, e = s & 15, j = L & 15, row = a & 15;
            const int here = 16 * (L >> 4) + e;
            if (sl < 0) sl = here;
            if (here != sl) ++bad;
            cols |= 1u << j;
            ++n;
            // the dense 16x16 D layout: row 4 (lane >> 4) + register, column lane & 15
            if (hrow[s] != 4 * (16 * (row >> 2) + j) + (row & 3)) ++badd;
          }
          if (n != 16 || cols != 0xffffu) ++bad;
          int& ref = s2[a >> 4][f][pos[v][f & 1]];
          if (ref < 0) ref = sl;
          else if (ref != sl) ++incons;
        }
    printf("(d) smfmac 16x16x64 f16, abid %d (index bits [%d:%d]): one-hot pairs not one B slot x 16 columns "
           "%d, D not at row 4 (lane >> 4) + r / column lane & 15: %d, slots at odds with nibble = p0 | p1 << 2 "
           "(value f -> position p[f & 1]): %d\n", abid, abid ? 31 : 15, abid ? 16 : 0, bad, badd, incons);
    if (!abid) {
      for (int ga = 0; ga < 4; ++ga)
        for (int f = 0; f < 8; f += 2) {
          printf("    A lanes %2d-%2d, stored values %d,%d: positions 0..3 meet B (k-group, element)", 16 * ga,
                 16 * ga + 15, f, f + 1);
          for (int p = 0; p < 4; ++p) {
            const int x = s2[ga][f][p] >= 0 ? s2[ga][f][p] : s2[ga][f + 1][p];
            printf(" (%d,%2d)", x >> 4, x & 15);
            // one group's two values see the same four B halves
            if (s2[ga][f][p] >= 0 && s2[ga][f + 1][p] >= 0 && s2[ga][f][p] != s2[ga][f + 1][p]) printf("!");
          }
          printf("\n");
        }
      for (int ga = 0; ga < 4; ++ga) for (int f = 0; f < 8; ++f) for (int p = 0; p < 4; ++p)
        slot[ga][f][p] = s2[ga][f][p] >= 0 ? s2[ga][f][p] : s2[ga][f ^ 1][p];
      have = bad == 0 && badd == 0 && incons == 0;
    } else {
      int diff = 0;
      for (int ga = 0; ga < 4; ++ga) for (int f = 0; f < 8; ++f) for (int p = 0; p < 4; ++p)
        diff += s2[ga][f][p] >= 0 && s2[ga][f][p] != slot[ga][f][p];
      printf("    abid 1 against abid 0: %d slots differ\n", diff);
    }
  }
  if (!have) { printf("(d) no consistent map: the checks on it are skipped\n"); return; }
  _Float16 *As, *Bs;
  int* ix;
  float *Cs, *Ds;
  hipMallocManaged(&As, 512 * 2);
  hipMallocManaged(&Bs, 1024 * 2);
  hipMallocManaged(&ix, 64 * 4);
  hipMallocManaged(&Cs, 256 * 4);
  hipMallocManaged(&Ds, 256 * 4);
  // host loop over the map: D[row][col] = C + sum over lanes a of the row, stored values f
  auto host = [&](double* ref, double* mag) {
    for (int i = 0; i < 256; ++i) { ref[i] = Cs[i]; mag[i] = fabs(Cs[i]); }
    for (int a = 0; a < 64; ++a)
      for (int f = 0; f < 8; ++f) {
        const int p = (ix[a] >> (4 * (f >> 1) + 2 * (f & 1))) & 3, sl = slot[a >> 4][f][p];
        const int row = a & 15;
        for (int j = 0; j < 16; ++j) {
          const double pr = (double)(float)As[a * 8 + f] * (double)(float)Bs[(16 * (sl >> 4) + j) * 16 + (sl & 15)];
          const int o = (16 * (row >> 2) + j) * 4 + (row & 3);
          ref[o] += pr;
          mag[o] += fabs(pr);
        }
      }
  };
  double ref[256], mag[256], worst = 0;
  for (int trial = 0; trial < 200; ++trial) {
    for (int i = 0; i < 512; ++i) As[i] = (_Float16)(frand() * powf(2.f, (float)(rand() % 8)));
    for (int i = 0; i < 1024; ++i) Bs[i] = (_Float16)(frand() * powf(2.f, (float)(rand() % 8)));
    for (int i = 0; i < 256; ++i) Cs[i] = frand();
    for (int l = 0; l < 64; ++l) {  // every lane its own positions, any of the six pairs a group
      ix[l] = (int)((unsigned)rand() << 16);  // (the unselected half: noise)
      for (int g = 0; g < 4; ++g) ix[l] |= nibs[rand() % 6] << (4 * g);
    }
    hipLaunchKernelGGL(sp_step, dim3(1), dim3(64), 0, 0, As, ix, Bs, Cs, Ds);
    hipDeviceSynchronize();
    host(ref, mag);
    for (int i = 0; i < 256; ++i) {
      const double err = fabs(Ds[i] - ref[i]) / (mag[i] * ldexp(1.0, -24));
      if (err > worst) worst = err;
    }
  }
  printf("(d) random operands, per-lane random positions, 200 trials: max |err| / ((|c| + sum|a b|) * 2^-24) = "
         "%.3f\n", worst);
  // the scan's two patterns: rows of positions {0, 1} and of {2, 3}; denormals; exact products
  for (int l = 0; l < 64; ++l) ix[l] = (l & 1) ? 0xEEEE : 0x4444;
  for (int i = 0; i < 512; ++i) As[i] = (_Float16)0.f;
  for (int i = 0; i < 1024; ++i) Bs[i] = (_Float16)1.f;
  for (int i = 0; i < 256; ++i) Cs[i] = 0.f;
  As[0] = (_Float16)ldexpf(1.f, -20);      // row 0, positions {0, 1}
  As[8 + 1] = (_Float16)ldexpf(1.f, -20);  // row 1, positions {2, 3}
  hipLaunchKernelGGL(sp_step, dim3(1), dim3(64), 0, 0, As, ix, Bs, Cs, Ds);
  hipDeviceSynchronize();
  printf("(d) f16 denormal 2^-20 * 1, rows of positions {0,1} / {2,3} -> %g / %g (expect %g)\n", Ds[0], Ds[1],
         ldexpf(1.f, -20));
  As[0] = As[9] = (_Float16)ldexpf(1.f, -12);
  for (int i = 0; i < 1024; ++i) Bs[i] = (_Float16)ldexpf(1.f, -12);
  hipLaunchKernelGGL(sp_step, dim3(1), dim3(64), 0, 0, As, ix, Bs, Cs, Ds);
  hipDeviceSynchronize();
  printf("(d) product 2^-12 * 2^-12 -> %g / %g (expect %g)\n", Ds[0], Ds[1], ldexpf(1.f, -24));
  const _Float16 big = (_Float16)(1.f + ldexpf(1.f, -10));
  As[0] = As[9] = big;
  for (int i = 0; i < 1024; ++i) Bs[i] = big;
  hipLaunchKernelGGL(sp_step, dim3(1), dim3(64), 0, 0, As, ix, Bs, Cs, Ds);
  hipDeviceSynchronize();
  const float exact = (1.f + ldexpf(1.f, -10)) * (1.f + ldexpf(1.f, -10));  // 21 bits: exact in fp32
  printf("(d) product (1 + 2^-10)^2 -> %.9g / %.9g (expect %.9g: %s)\n", Ds[0], Ds[1], exact,
         Ds[0] == exact && Ds[1] == exact ? "exact" : "NOT exact");
}

int main() {
  srand(1);
  float *A, *B, *C, *D;
  hipMallocManaged(&A, 4096 * 4);
  hipMallocManaged(&B, 4096 * 4);
  hipMallocManaged(&C, 4096 * 4);
  hipMallocManaged(&D, 4096 * 4);
  long m01 = 0, m10 = 0, msum = 0, n = 0;
  for (int trial = 0; trial < 200; ++trial) {
    for (int i = 0; i < 64; ++i) A[i] = frand() * powf(2.f, (float)(rand() % 20 - 10));
    for (int i = 0; i < 64; ++i) B[i] = frand() * powf(2.f, (float)(rand() % 20 - 10));
    for (int i = 0; i < 1024; ++i) C[i] = frand() * powf(2.f, (float)(rand() % 20 - 10));
    hipLaunchKernelGGL(f32_step, dim3(1), dim3(64), 0, 0, A, B, C, D);
    hipDeviceSynchronize();
    for (int i = 0; i < 32; ++i)
      for (int j = 0; j < 32; ++j) {
        const float a0 = A[i * 2], a1 = A[i * 2 + 1], b0 = B[j], b1 = B[32 + j], c = C[i * 32 + j];
        const float d = D[i * 32 + j];
        m01 += d != fmaf(a1, b1, fmaf(a0, b0, c));
        m10 += d != fmaf(a0, b0, fmaf(a1, b1, c));
        msum += d != (float)((double)a0 * b0 + (double)a1 * b1 + (double)c);
        ++n;
      }
  }
  printf("(a) f32 32x32x2: mismatches vs fma(a1,b1,fma(a0,b0,c)) %ld, vs fma(a0,b0,fma(a1,b1,c)) %ld, "
         "vs double-rounded-once %ld, of %ld\n", m01, m10, msum, n);

  _Float16 *Ah, *Bh;
  hipMallocManaged(&Ah, 512 * 2);
  hipMallocManaged(&Bh, 512 * 2);
  // (b) denormals: A = 2^-20 (f16 subnormal), B = 1 on the k=0 row only
  for (int i = 0; i < 512; ++i) { Ah[i] = (_Float16)0.f; Bh[i] = (_Float16)0.f; }
  for (int i = 0; i < 32; ++i) Ah[i * 16] = (_Float16)ldexpf(1.f, -20);
  for (int j = 0; j < 32; ++j) Bh[j] = (_Float16)1.f;
  hipLaunchKernelGGL(f16_step, dim3(1), dim3(64), 0, 0, Ah, Bh, D);
  hipDeviceSynchronize();
  printf("(b) f16 denormal input 2^-20 * 1 -> %g (expect %g)\n", D[0], ldexpf(1.f, -20));
  for (int i = 0; i < 32; ++i) Ah[i * 16] = (_Float16)ldexpf(1.f, -12);
  for (int j = 0; j < 32; ++j) Bh[j] = (_Float16)ldexpf(1.f, -12);
  hipLaunchKernelGGL(f16_step, dim3(1), dim3(64), 0, 0, Ah, Bh, D);
  hipDeviceSynchronize();
  printf("(b) f16 product 2^-12*2^-12 -> %g (expect %g)\n", D[0], ldexpf(1.f, -24));

  // (c) accumulation error vs double
  double worst = 0;
  for (int trial = 0; trial < 200; ++trial) {
    for (int i = 0; i < 512; ++i) {
      Ah[i] = (_Float16)(frand() * powf(2.f, (float)(rand() % 8)));
      Bh[i] = (_Float16)(frand() * powf(2.f, (float)(rand() % 8)));
    }
    hipLaunchKernelGGL(f16_step, dim3(1), dim3(64), 0, 0, Ah, Bh, D);
    hipDeviceSynchronize();
    for (int i = 0; i < 32; ++i)
      for (int j = 0; j < 32; ++j) {
        double ref = 0, mag = 0;
        for (int k = 0; k < 16; ++k) {
          const double p = (double)(float)Ah[i * 16 + k] * (double)(float)Bh[k * 32 + j];
          ref += p;
          mag += fabs(p);
        }
        const double err = fabs(D[i * 32 + j] - ref) / (mag * ldexp(1.0, -24));
        if (err > worst) worst = err;
      }
  }
  printf("(c) f16 MFMA K=16: max |err| / (sum|a b| * 2^-24) = %.3f\n", worst);
  sparse_probe();
  return 0;
}
