// The k-loop of the fp32-MFMA projection (api.hip linear_rows_mfma_kernel), shared with the
// NeuralCF table kernel (ncf_cert_params.hip ncf_tables_kernel): one definition, so the rows either
// kernel writes are bitwise the same.
#pragma once
#include "hnm_device.h"

#define LIN_TN 64
#define LIN_TK 32
#define LIN_RS (LIN_TK + 1)  // LDS row stride (floats): rows spread over the banks

// acc[r] = sum_k X[x(m0 + wr + mfma32_row(r, h)), k] W[n0 + wc + i, k] for the calling wave's
// 32 x 32 tile of a 64-row x 64-output block (waves 2 r + c: wr = 32 r, wc = 32 c; i = lane & 31,
// h = lane >> 5): a chain of v_mfma_f32_32x32x2_f32 from C = 0 over k = 0, 1, .., K - 1 (an exact
// fp32 fma chain in k order), K in chunks of 32 staged through xs / ws (64 * LIN_RS floats each,
// the next chunk prefetched into registers;
// 16-B global loads: K, ldx, ldw multiples of 4 -- K of 32 -- and 16-B aligned X and W).  Rows
// m >= M read as zero, rows whose id is out of range as NaN (flagged through err).  Called by
// the whole 256-thread workgroup; ends with a barrier, so xs / ws are free on return.
__device__ __forceinline__ f32x16 linear_mfma_tile(
    const float* __restrict__ X, int64_t ldx, const int64_t* __restrict__ ids, int64_t x_rows,
    int64_t M, int K, const float* __restrict__ W, int64_t ldw, int N, int64_t m0, int n0,
    float* xs, float* ws, unsigned* err) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int i = lane & 31, h = lane >> 5;
  const int wr = 32 * (wave >> 1), wc = 32 * (wave & 1);
  f32x16 acc = {};
  // chunk k0 + 32 is fetched into registers while chunk k0's MFMAs run (two 16-B loads of X and
  // of W a thread and chunk), so one load latency a chunk is hidden behind the matrix pipe
  float4 xv[2], wv[2];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int e = t + 256 * q;
      const int rr = e / (LIN_TK / 4), kq = 4 * (e % (LIN_TK / 4));
      const int64_t m = m0 + rr;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (m < M) {
        const int64_t src = ids ? ids[m] : m;
        if (src < 0 || src >= x_rows) {
          if (kq == 0) hnm_flag(err, HNM_ERR_OOB);
          v = make_float4(__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""),
                          __builtin_nanf(""));
        } else {
          v = *reinterpret_cast<const float4*>(X + src * ldx + k0 + kq);
        }
      }
      xv[q] = v;
      float4 u = make_float4(0.f, 0.f, 0.f, 0.f);
      if (n0 + rr < N) u = *reinterpret_cast<const float4*>(W + (int64_t)(n0 + rr) * ldw + k0 + kq);
      wv[q] = u;
    }
  };
  fetch(0);
  for (int k0 = 0; k0 < K; k0 += LIN_TK) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int e = t + 256 * q;
      const int rr = e / (LIN_TK / 4), kq = 4 * (e % (LIN_TK / 4));
      float* xr = xs + rr * LIN_RS + kq;
      xr[0] = xv[q].x; xr[1] = xv[q].y; xr[2] = xv[q].z; xr[3] = xv[q].w;
      float* wr4 = ws + rr * LIN_RS + kq;
      wr4[0] = wv[q].x; wr4[1] = wv[q].y; wr4[2] = wv[q].z; wr4[3] = wv[q].w;
    }
    __syncthreads();
    if (k0 + LIN_TK < K) fetch(k0 + LIN_TK);
    const float* xa = xs + (wr + i) * LIN_RS + h;  // A[i][h] of step s: row wr + i, k = 2 s + h
    const float* wb = ws + (wc + i) * LIN_RS + h;  // B[h][j = i]: output wc + i, k = 2 s + h
#pragma unroll
    for (int st = 0; st < LIN_TK / 2; ++st) acc = mfma32x32x2(xa[2 * st], wb[2 * st], acc);
    __syncthreads();
  }
  return acc;
}
