// Timing harness of ncf16_scan_kernel (THRESH mode, no appends) at the bench shape
// (B = 4096 users x 105,542 items, 24 partitions): kernel-only time, best of 7 after a
// clock warm-up, so scan variants can be compared without the rest of the step.  Both layouts
// of the two-layer scan are timed, alternating (SHAPE 0: 32x32x16, 1: 16x16x32;
// HNM_OPT_SCAN_SHAPE), layout 1 with its pair loop pipelined by hand (HNM_OPT_SCAN_PIPE), and that
// loop with the epilogue on the sparse instruction (HNM_OPT_SCAN_SPARSE) beside it, and the sparse
// epilogue with the test values in rows 0-3 and in rows 0, 4, 8, 12 (HNM_OPT_SCAN_ROW0), alternating.
// Diagnostic build only (the scan unit is included as text: the kernel is private to it;
// cert_shape comes from ncf_cert.o through ncf_cert_internal.h):
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -c tools/scan_ablation.hip -o build/scan_ablation.o
//   hipcc --offload-arch=gfx950 build/scan_ablation.o <every build/obj/*.o but ncf_cert_scan.o> \
//         -L/opt/rocm/lib -lrccl -o tools/bin/scan_ablation
#include "../hnm_recommendation_amd/csrc/ncf_cert_scan.hip"

#include <vector>

template <typename T>
static T* dev_fill(size_t n, float lo, float hi, unsigned seed) {
  std::vector<T> h(n);
  unsigned x = seed * 2654435761u + 1;
  for (size_t i = 0; i < n; ++i) {
    x = x * 1664525u + 1013904223u;
    h[i] = (T)(lo + (hi - lo) * ((x >> 8) * (1.0f / 16777216.0f)));
  }
  T* d;
  (void)hipMalloc(&d, n * sizeof(T));
  (void)hipMemcpy(d, h.data(), n * sizeof(T), hipMemcpyHostToDevice);
  return d;
}

template <int SHAPE, bool PIPE = false, bool SPARSE = false, bool ROW0 = false>
static float time_scan(dim3 grid, const ScanArgs& a) {
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0);
  (void)hipEventCreate(&e1);
  float best = 1e30f;
  for (int rep = 0; rep < 8; ++rep) {
    (void)hipEventRecord(e0);
    hipLaunchKernelGGL((ncf16_scan_kernel<SCAN_THRESH, false, SHAPE, PIPE, SPARSE, ROW0>), grid, dim3(256), 0, 0, a);
    (void)hipEventRecord(e1);
    (void)hipEventSynchronize(e1);
    if (hipGetLastError() != hipSuccess) printf("launch error\n");
    float ms;
    (void)hipEventElapsedTime(&ms, e0, e1);
    if (rep > 0 && ms < best) best = ms;
  }
  return best;
}

int main() {
  const int64_t B = 4096, I = 105542;
  const CertShape sh = cert_shape(B, I, 12, 256);
  ScanArgs a{};
  a.P16 = dev_fill<_Float16>(B * 64, -0.25f, 0.25f, 1);
  a.WG16 = dev_fill<_Float16>(B * 64, -0.5f, 0.5f, 2);
  a.Q16 = dev_fill<_Float16>(I * 64, -0.25f, 0.25f, 3);
  a.G16 = dev_fill<_Float16>(I * 64, -0.5f, 0.5f, 4);
  a.W2h = dev_fill<_Float16>(32 * 64, -0.1f, 0.1f, 5);
  a.wmh = dev_fill<_Float16>(32, -0.5f, 0.5f, 6);
  a.b2s = dev_fill<float>(32, -0.01f, 0.01f, 7);
  a.Bi = dev_fill<float>(I, 0.f, 1.f, 8);
  a.Di = dev_fill<float>(I, 0.f, 1.f, 9);
  a.Cu = dev_fill<float>(B, 0.f, 1.f, 10);
  a.tau = dev_fill<float>(B, 1e30f, 1e30f, 11);  // no appends
  CertParams hp{};
  hp.unit = 1.f;
  hp.cg = 1.f;
  CertParams* prm;
  (void)hipMalloc(&prm, sizeof(CertParams));
  (void)hipMemcpy(prm, &hp, sizeof(hp), hipMemcpyHostToDevice);
  a.prm = prm;
  a.B = B;
  a.I = I;
  a.upw = 32;

  a.ipp = sh.part.ipp;
  a.NP = sh.part.np;
  a.capp = sh.capp;
  (void)hipMalloc(&a.cnt, B * sh.part.np * 4);
  (void)hipMalloc(&a.buf, (size_t)B * sh.part.np * sh.capp * 4);
  dim3 grid((unsigned)sh.part.np, (unsigned)hnm_cdiv(B, 128));
  const double pairs = (double)B * I, useful = 4352.0 * pairs;
  printf("grid %u x %u, ipp %ld\n", grid.x, grid.y, (long)sh.part.ipp);
  for (int w = 0; w < 100; ++w)  // clock warm-up (~0.2 s of scan work)
    hipLaunchKernelGGL((ncf16_scan_kernel<SCAN_THRESH>), grid, dim3(256), 0, 0, a);
  (void)hipDeviceSynchronize();
  for (int rep = 0; rep < 9; ++rep) {
    const int shape = rep % 3 != 0, pipe = rep % 3 == 2;
    const float ms = pipe ? time_scan<1, true>(grid, a)
                          : shape ? time_scan<1>(grid, a) : time_scan<0>(grid, a);
    printf("ncf16_scan shape %d pipe %d  %7.3f ms  %6.1f TF useful  %5.2f cyc/user-tile/SIMD @2.2GHz\n",
           shape, pipe, ms, useful / (ms * 1e-3) / 1e12, ms * 1e-3 * 2.2e9 / (pairs / 32 / 1024));
  }
  // the dense and the sparse epilogue alternating, each figure the best of 7: the pipelined
  // threshold pass, then the plain loop
  for (int rep = 0; rep < 12; ++rep) {
    const int sparse = rep & 1, pipe = rep < 8;
    const float ms = pipe ? (sparse ? time_scan<1, true, true>(grid, a) : time_scan<1, true>(grid, a))
                          : (sparse ? time_scan<1, false, true>(grid, a) : time_scan<1>(grid, a));
    printf("ncf16_scan shape 1 pipe %d sparse %d  %7.3f ms\n", pipe, sparse, ms);
  }
  // the sparse epilogue's test values in four registers of lanes 0-15 and in one register of all 64
  // lanes, alternating: the pipelined threshold pass (seven rounds), then the plain loop
  for (int rep = 0; rep < 20; ++rep) {
    const int row0 = rep & 1, pipe = rep < 14;
    const float ms = pipe ? (row0 ? time_scan<1, true, true, true>(grid, a) : time_scan<1, true, true>(grid, a))
                          : (row0 ? time_scan<1, false, true, true>(grid, a) : time_scan<1, false, true>(grid, a));
    printf("ncf16_scan shape 1 pipe %d sparse 1 row0 %d  %7.3f ms\n", pipe, row0, ms);
  }
  return 0;
}
