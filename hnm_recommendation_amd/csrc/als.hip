// ImplicitALS (Hu, Koren & Volinsky 2008): the Gram matrix of a factor table and the per-row
// regularised least-squares solve of one alternating half-step.  No reference counterpart: the
// contract is stated in include/hnm.h and restated in float64 numpy by tests/als_oracle.py.
//
// Half-step for row r of a CSR (ptr, idx) against a table T [tab_rows, d], G = T^T T:
//   S   = sum_{j in row r} t_j t_j^T        b0 = sum_{j in row r} t_j          (stored order)
//   A   = fma(alpha, S, G) + reg * I        b  = (1 + alpha) * b0
//   out = A^-1 b   by Cholesky A = L L^T, L y = b, L^T x = y
// all in fp32.  S runs on the exact fp32 MFMA (v_mfma_f32_32x32x2_f32: a k-ordered fmaf chain,
// so "stored order" is literal); b0 is a plain add chain.
//
// Files.  als_internal.h holds what every half-step shares: the image + MFMA loop and the kernel
// template als_solve_kernel<NT, WEIGHTED, SOLVER>, whose stages 1 and 2 below leave A and b in
// LDS.  This file holds the Gram kernels and SOLVER = AlsCholesky (stages 3 and 4 below);
// als_cg.hip holds SOLVER = AlsCg, a few conjugate-gradient steps from a start vector in place of
// stages 3 and 4 (hnm_als_cg_rows_f32, an option of the fit).  The Cholesky instantiations
// compile to the registers, LDS and occupancy they had as one kernel in this file
// (profiles/als_cg_resources.txt).
//
// Shape.  One 256-thread workgroup per output row; d is padded to NT = ceil(d / 32) tiles of 32
// (the padding columns are zero and never leave the tile registers).
//   1. the row's table rows are gathered 32 at a time into an LDS image (coalesced along d,
//      zero-filled past the row's end; the next image is loaded into registers under the
//      current one's MFMAs); the lower-triangle 32 x 32 tiles of S are dealt round
//      robin to the four waves (<= 3 tiles a wave at NT = 4), each wave feeding its MFMAs from
//      the image; threads c < d add column c into b0.  A long row (a popular item's tens of
//      thousands of users) is this same loop run longer: one route, no length threshold, and the
//      result is a function of the inputs and of ALS_CHUNK alone.
//   2. the tiles become the lower triangle of A in an LDS matrix with an odd row stride (column
//      walks are conflict-free), b becomes row d of it: factoring the augmented matrix carries
//      the forward solve L y = b along for free (row d of L is y^T).
//   3. right-looking Cholesky, two barriers a column: scale column k by 1 / sqrt(a_kk); then wave w
//      takes rows k + 1 + w, + 4, ... of the trailing matrix, a lane per column.
//   4. wave 0 solves L^T x = y with x in registers (lane i holds x_i and x_{i + 64}); one
//      broadcast and one LDS row read a step, no barrier.
// The LDS matrix is (32 NT + 1)^2 floats: 66.6 KB at d = 128 (two workgroups a CU), 16.9 KB at
// d = 64 (the 2,048-thread limit, eight workgroups, binds first).  The gather image shares it.
// Measured at the H&M shape (tools/als_bench.py): user step 84.6 ms at d = 64, 904 ms at d = 128
// (the CG half-step at 3 steps: 13.2 and 93.0 ms, profiles/als_cg_bench.txt).
// A one-barrier-a-column variant (column k scaled as it is read and kept in the upper triangle,
// four rows a wave in flight, indices prefetched two images ahead) took 116.7 / 1,144 ms: 73
// instead of 56 VGPR at d = 64 cost more occupancy than the barriers it saved.
//
// Weighted half-step (hnm_als_solve_rows_weighted_f32; als_solve_kernel<NT, true, .>): a weight w_j
// per stored entry, c = 1 + alpha w, p = 1:
//   S  = sum w_j t_j t_j^T  (fl(w_j t_j[i]) * t_j[c] in the chain: the weight scales the MFMA's A
//        operand, the one indexed by the output row)
//   b0 = sum t_j (as above)    bw = fmaf chain of w_j t_j    b = fma(alpha, bw, b0)
// and everything from A on is the code above.  With every weight 1 (or 2^e) the result is
// bitwise the unweighted one at alpha (or 2^e alpha) when 1 + alpha is exact in fp32.  The
// unweighted instantiation is unchanged: the same registers and LDS as before the template
// parameter (56 VGPR at d = 64); the weighted one takes 64 there (six instead of seven waves a
// SIMD), which is its measured cost at d = 64.
//
// Gram.  Workgroup c sums rows [c * ALS_GRAM_ROWS, (c + 1) * ALS_GRAM_ROWS) through the same
// image + MFMA loop and writes its lower triangle to the ctx workspace; a second kernel adds
// the chunk partials in ascending chunk order and mirrors the result.  Chunk size and order are
// compile-time, so the bits do not depend on the grid or the CU count.  No float atomics.
#include "als_internal.h"

namespace {

// ------------------------------------------------------------------ solve
// Stages 3 and 4 behind als_solve_kernel's stages 1 and 2 (als_internal.h).
struct AlsCholesky {
  template <int NT>
  static __device__ __forceinline__ void run(float* As, int d, float* __restrict__ orow, int) {
    constexpr int DP = 32 * NT, LD = DP + 1;
    __shared__ float piv[DP];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    // right-looking Cholesky of rows 0 .. d (row d = b^T becomes y^T)
    for (int k = 0; k < d; ++k) {
      const float p = sqrtf(As[k * LD + k]);
      for (int i = k + 1 + t; i <= d; i += 256) As[i * LD + k] = As[i * LD + k] / p;
      if (t == 0) piv[k] = p;
      __syncthreads();
      for (int i = k + 1 + wave; i <= d; i += 4) {
        const float lik = As[i * LD + k];
        const int jhi = i < d ? i : d - 1;
        for (int j = k + 1 + lane; j <= jhi; j += 64)
          As[i * LD + j] = fmaf(-lik, As[j * LD + k], As[i * LD + j]);
      }
      __syncthreads();
    }
    // L^T x = y on wave 0: lane i holds entries i and i + 64
    if (wave == 0) {
      float y0 = lane < d ? As[d * LD + lane] : 0.f;
      float y1 = lane + 64 < d ? As[d * LD + lane + 64] : 0.f;
      for (int k = d - 1; k >= 0; --k) {
        const float yk = __shfl(k >= 64 ? y1 : y0, k & 63);
        const float xk = yk / piv[k];
        if (lane == (k & 63)) {
          if (k >= 64) y1 = xk;
          else y0 = xk;
        }
        if (lane < k) y0 = fmaf(-As[k * LD + lane], xk, y0);
        if (lane + 64 < k) y1 = fmaf(-As[k * LD + lane + 64], xk, y1);
      }
      if (lane < d) orow[lane] = y0;
      if (lane + 64 < d) orow[lane + 64] = y1;
    }
  }
};

// ------------------------------------------------------------------ Gram
// Workgroup c: part[c] (lower triangle of a [d, d] block) = the chunk's T^T T.
template <int NT>
__global__ __launch_bounds__(256) void als_gram_kernel(const float* __restrict__ tab, int64_t rows,
                                                       int64_t ld, int d, float* __restrict__ part) {
  constexpr int DP = 32 * NT, NTILES = NT * (NT + 1) / 2;
  __shared__ float img[ALS_CHUNK * DP];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * ALS_GRAM_ROWS;
  const int64_t r1 = std::min<int64_t>(rows, r0 + ALS_GRAM_ROWS);
  f32x16 acc[ALS_MAX_TILES];
#pragma unroll
  for (int s = 0; s < ALS_MAX_TILES; ++s)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[s][q] = 0.f;
  for (int64_t c0 = r0; c0 < r1; c0 += ALS_CHUNK) {
    const int n = (int)std::min<int64_t>(ALS_CHUNK, r1 - c0);
    __syncthreads();
    for (int e = t; e < ALS_CHUNK * DP; e += 256) {
      const int k = e / DP, c = e % DP;
      img[e] = (k < n && c < d) ? tab[(c0 + k) * ld + c] : 0.f;
    }
    __syncthreads();
    als_mfma_chunk<NT>(img, n, acc);
  }
  float* o = part + (int64_t)blockIdx.x * d * d;
#pragma unroll
  for (int s = 0; s < ALS_MAX_TILES; ++s) {
    const int q = wave + 4 * s;
    if (q < NTILES) {
      int ti, tj;
      als_tile(q, ti, tj);
      const int j = 32 * tj + (lane & 31);
#pragma unroll
      for (int x = 0; x < 16; ++x) {
        const int i = 32 * ti + mfma32_row(x, lane >> 5);
        if (i < d && j <= i) o[i * d + j] = acc[s][x];
      }
    }
  }
}

// out[i, j] = out[j, i] = part[0][i, j] + part[1][i, j] + ... in ascending chunk order (j <= i).
__global__ __launch_bounds__(256) void als_gram_reduce_kernel(const float* __restrict__ part,
                                                              int64_t nchunks, int d,
                                                              float* __restrict__ out) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= d * d) return;
  const int i = e / d, j = e % d;
  if (j > i) return;
  float s = part[e];
  for (int64_t c = 1; c < nchunks; ++c) s += part[c * d * d + e];
  out[i * d + j] = s;
  out[j * d + i] = s;
}

}  // namespace

extern "C" hnm_status hnm_als_gram_f32(hnm_ctx* ctx, const float* tab, int64_t rows, int64_t ld,
                                       int64_t d, float* out) {
  HNM_CTX_DEVICE(ctx);
  HNM_REQUIRE(ctx, HNM_EINVAL, "als_gram: ctx is NULL");
  HNM_REQUIRE(als_dim_ok(d), HNM_EUNSUPPORTED,
              "als_gram: d = %lld (multiples of 16 in [16, 128] supported)", (long long)d);
  HNM_REQUIRE(rows >= 0 && ld >= d, HNM_EINVAL, "als_gram: rows < 0 or ld < d");
  HNM_REQUIRE(out && (tab || rows == 0), HNM_EINVAL, "als_gram: NULL table or output");
  if (rows == 0) {
    HNM_HIP_CHECK(hipMemsetAsync(out, 0, (size_t)d * d * 4, ctx->stream));
    return HNM_OK;
  }
  const int64_t nchunks = hnm_cdiv(rows, ALS_GRAM_ROWS);
  HNM_REQUIRE(nchunks <= INT32_MAX, HNM_EUNSUPPORTED, "als_gram: too many rows");
  float* part = nullptr;
  hnm_status st = hnm_workspace(ctx, (size_t)nchunks * d * d * 4, (void**)&part);
  if (st != HNM_OK) return st;
  const int nt = (int)hnm_cdiv(d, 32);
  const dim3 grid((unsigned)nchunks), block(256);
  switch (nt) {
    case 1: hipLaunchKernelGGL(als_gram_kernel<1>, grid, block, 0, ctx->stream, tab, rows, ld, (int)d, part); break;
    case 2: hipLaunchKernelGGL(als_gram_kernel<2>, grid, block, 0, ctx->stream, tab, rows, ld, (int)d, part); break;
    case 3: hipLaunchKernelGGL(als_gram_kernel<3>, grid, block, 0, ctx->stream, tab, rows, ld, (int)d, part); break;
    default: hipLaunchKernelGGL(als_gram_kernel<4>, grid, block, 0, ctx->stream, tab, rows, ld, (int)d, part); break;
  }
  HNM_LAUNCH_CHECK();
  hipLaunchKernelGGL(als_gram_reduce_kernel, dim3((unsigned)hnm_cdiv(d * d, 256)), block, 0,
                     ctx->stream, part, nchunks, (int)d, out);
  HNM_LAUNCH_CHECK();
  return HNM_OK;
}

namespace {

// The two solve entries: w == NULL and weighted == false is hnm_als_solve_rows_f32.
hnm_status als_solve_rows(hnm_ctx* ctx, const int64_t* ptr, const int32_t* idx, const float* w,
                          bool weighted, int64_t n_rows, const float* tab, int64_t tab_rows,
                          int64_t ld, int64_t d, const float* gram, float alpha, float reg,
                          const int64_t* row_ids, int64_t B, float* out, int64_t ldo) {
  HNM_CTX_DEVICE(ctx);
  HNM_REQUIRE(ctx, HNM_EINVAL, "als_solve_rows: ctx is NULL");
  HNM_REQUIRE(als_dim_ok(d), HNM_EUNSUPPORTED,
              "als_solve_rows: d = %lld (multiples of 16 in [16, 128] supported)", (long long)d);
  HNM_REQUIRE(std::isfinite(reg) && reg > 0.f, HNM_EINVAL,
              "als_solve_rows: reg must be finite and > 0");
  HNM_REQUIRE(std::isfinite(alpha) && alpha >= 0.f, HNM_EINVAL,
              "als_solve_rows: alpha must be finite and >= 0");
  HNM_REQUIRE(B >= 0 && n_rows >= 0 && tab_rows >= 0, HNM_EINVAL, "als_solve_rows: bad size");
  HNM_REQUIRE(B <= INT32_MAX && tab_rows < INT_BIG, HNM_EUNSUPPORTED,
              "als_solve_rows: B or tab_rows exceeds 2^31 - 1");
  if (B == 0 || n_rows == 0) return HNM_OK;
  HNM_REQUIRE(ld >= d && ldo >= d, HNM_EINVAL, "als_solve_rows: ld or ldo < d");
  HNM_REQUIRE(ptr && idx && gram && out && (tab || tab_rows == 0), HNM_EINVAL,
              "als_solve_rows: NULL argument");
  HNM_REQUIRE(w || !weighted, HNM_EINVAL, "als_solve_rows_weighted: w is NULL");
  HNM_REQUIRE(row_ids || B <= n_rows, HNM_EINVAL,
              "als_solve_rows: B > n_rows without row_ids");
  const int nt = (int)hnm_cdiv(d, 32);
  const dim3 grid((unsigned)B), block(256);
  const float one_alpha = 1.0f + alpha;
#define ALS_SOLVE(NT, W)                                                                       \
  hipLaunchKernelGGL((als_solve_kernel<NT, W, AlsCholesky>), grid, block, 0, ctx->stream, ptr, \
                     idx, w, n_rows, tab, tab_rows, ld, (int)d, gram, alpha, one_alpha, reg,    \
                     row_ids, out, ldo, ctx->err_dev, 0)
  hnm_timer_begin(ctx, HNM_TIME_SCORE);
  if (weighted) {
    switch (nt) {
      case 1: ALS_SOLVE(1, true); break;
      case 2: ALS_SOLVE(2, true); break;
      case 3: ALS_SOLVE(3, true); break;
      default: ALS_SOLVE(4, true); break;
    }
  } else {
    switch (nt) {
      case 1: ALS_SOLVE(1, false); break;
      case 2: ALS_SOLVE(2, false); break;
      case 3: ALS_SOLVE(3, false); break;
      default: ALS_SOLVE(4, false); break;
    }
  }
  hnm_timer_end(ctx, HNM_TIME_SCORE);
#undef ALS_SOLVE
  HNM_LAUNCH_CHECK();
  return HNM_OK;
}

}  // namespace

extern "C" hnm_status hnm_als_solve_rows_f32(hnm_ctx* ctx, const int64_t* ptr, const int32_t* idx,
                                             int64_t n_rows, const float* tab, int64_t tab_rows,
                                             int64_t ld, int64_t d, const float* gram, float alpha,
                                             float reg, const int64_t* row_ids, int64_t B,
                                             float* out, int64_t ldo) {
  return als_solve_rows(ctx, ptr, idx, nullptr, false, n_rows, tab, tab_rows, ld, d, gram, alpha,
                        reg, row_ids, B, out, ldo);
}

extern "C" hnm_status hnm_als_solve_rows_weighted_f32(hnm_ctx* ctx, const int64_t* ptr,
                                                      const int32_t* idx, const float* w,
                                                      int64_t n_rows, const float* tab,
                                                      int64_t tab_rows, int64_t ld, int64_t d,
                                                      const float* gram, float alpha, float reg,
                                                      const int64_t* row_ids, int64_t B,
                                                      float* out, int64_t ldo) {
  return als_solve_rows(ctx, ptr, idx, w, true, n_rows, tab, tab_rows, ld, d, gram, alpha, reg,
                        row_ids, B, out, ldo);
}
