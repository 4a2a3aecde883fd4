// Shared between als.hip (Gram, Cholesky half-step) and als_cg.hip (conjugate-gradient
// half-step): the gather image + fp32-MFMA loop that sums t t^T over a CSR row, and the code that
// turns it into the row's system (A's lower triangle and b) in LDS.  Both solvers start from the
// same A and b, bit for bit; what differs is what they do with them.
#pragma once
#include "hnm_device.h"
#include "hnm_internal.h"

#include <cmath>

namespace {

constexpr int ALS_CHUNK = 32;          // table rows per LDS image
constexpr int ALS_GRAM_ROWS = 2048;    // table rows per Gram partial (a multiple of ALS_CHUNK)
constexpr int ALS_MAX_TILES = 3;       // lower-triangle tiles per wave: ceil(10 / 4) at NT = 4

// lower-triangle tile number q -> (ti, tj), tj <= ti, rows first: (0,0) (1,0) (1,1) (2,0) ...
__device__ __forceinline__ void als_tile(int q, int& ti, int& tj) {
  ti = 0;
  while ((ti + 1) * (ti + 2) / 2 <= q) ++ti;
  tj = q - ti * (ti + 1) / 2;
}

// acc[s] += image^T image restricted to this wave's tiles, rows [0, n) of the image in order.
// WEIGHTED: image^T diag(ws) image, the weight of image row k applied to the operand indexed by
// the output row (the MFMA's A operand) as it is read: fl(ws[k] * t_k[i]) * t_k[c].
template <int NT, bool WEIGHTED = false>
__device__ __forceinline__ void als_mfma_chunk(const float* img, int n, f32x16 (&acc)[ALS_MAX_TILES],
                                               const float* ws = nullptr) {
  constexpr int DP = 32 * NT, NTILES = NT * (NT + 1) / 2;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int kh = lane >> 5, c = lane & 31;
#pragma unroll
  for (int s = 0; s < ALS_MAX_TILES; ++s) {
    const int q = wave + 4 * s;
    if (q < NTILES) {  // uniform over the wave
      int ti, tj;
      als_tile(q, ti, tj);
      const float* pa = img + kh * DP + 32 * ti + c;
      const float* pb = img + kh * DP + 32 * tj + c;
      if constexpr (WEIGHTED) {
        const float* pw = ws + kh;
        for (int k = 0; k < n; k += 2)  // rows past n are zero, and so are their weights
          acc[s] = mfma32x32x2(pw[k] * pa[k * DP], pb[k * DP], acc[s]);
      } else {
        for (int k = 0; k < n; k += 2)  // rows past n are zero: fma(0, 0, x) = x
          acc[s] = mfma32x32x2(pa[k * DP], pb[k * DP], acc[s]);
      }
    }
  }
}

// ------------------------------------------------------------------ half-step
// One 256-thread workgroup per output row.  Stages 1 and 2 -- the gather images, the MFMA tile
// loop, the b0 / bw chains, A and b into LDS -- are this kernel whatever the solver; SOLVER::run
// takes over once A's lower triangle stands in As[i * LD + j] (j <= i < d, LD = 32 NT + 1) and b
// in row d of it, behind a barrier: AlsCholesky (als.hip) or AlsCg (als_cg.hip).  `out` is the
// solver's output, and for AlsCg also its start vector; `steps` is AlsCg's.
// WEIGHTED (the ..._weighted_f32 entries): wgt holds one weight per idx entry; an image's 32
// weights travel with its 32 indices (prefetched the same way) into `ws`, the MFMA loop scales
// its row-side operand by them, and the b0 chain and bw = sum w t run side by side on the last
// wave (d <= 64) or the last two.  The unweighted
// instantiation is the code it was: `ws`, `badw` and every weighted statement compile away.
template <int NT, bool WEIGHTED, class SOLVER>
__global__ __launch_bounds__(256) void als_solve_kernel(
    const int64_t* __restrict__ ptr, const int32_t* __restrict__ idx,
    const float* __restrict__ wgt, int64_t n_rows,
    const float* __restrict__ tab, int64_t tab_rows, int64_t ld, int d,
    const float* __restrict__ gram, float alpha, float one_alpha, float reg,
    const int64_t* __restrict__ row_ids, float* __restrict__ out, int64_t ldo, unsigned* err,
    int steps) {
  constexpr int DP = 32 * NT, LD = DP + 1, NTILES = NT * (NT + 1) / 2;
  static_assert(ALS_CHUNK * DP <= LD * LD, "the gather image fits in the matrix");
  __shared__ float As[LD * LD];  // rows 0 .. d of the augmented matrix; first the gather image
  __shared__ int bad;
  __shared__ float ws[ALS_CHUNK];  // WEIGHTED: the image rows' weights, zero past the row's end
  __shared__ int badw;             // WEIGHTED: a negative or non-finite weight was loaded
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t b = blockIdx.x;
  float* orow = out + b * ldo;
  const int64_t r = row_ids ? row_ids[b] : b;
  if (r < 0 || r >= n_rows) {  // uniform over the workgroup
    if (t == 0) hnm_flag(err, HNM_ERR_OOB);
    if (t < d) orow[t] = __builtin_nanf("");
    return;
  }
  const int64_t p0 = ptr[r];
  const int64_t h = ptr[r + 1] - p0;
  if (h <= 0) {
    if (t < d) orow[t] = 0.f;
    return;
  }
  if (t == 0) bad = 0;
  if constexpr (WEIGHTED) {
    if (t == 0) badw = 0;
  }
  f32x16 acc[ALS_MAX_TILES];
#pragma unroll
  for (int s = 0; s < ALS_MAX_TILES; ++s)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[s][q] = 0.f;
  float bsum = 0.f;
  float bw = 0.f;  // WEIGHTED: the fmaf chain of w t
  // WEIGHTED: column bc of b0 and bw belongs to thread BT0 + bc -- the last wave at d <= 64, the
  // last two above: the waves with the fewest MFMA tiles (none at d <= 64), where the unweighted
  // kernel's threads c < d sit on the waves with the most.  Which thread runs a chain does not
  // show in its bits.
  constexpr int BT0 = 256 - 64 * ((NT + 1) / 2);
  const int bc = t - BT0;
  // this thread's EPT elements of the image of rows [c0, c0 + ALS_CHUNK) of the CSR row, held in
  // registers: the next image is in flight under this one's MFMAs
  constexpr int EPT = ALS_CHUNK * DP / 256;
  float v[EPT];
  bool mybad = false;
  float wv = 0.f;  // WEIGHTED: thread k < ALS_CHUNK holds the weight of image row k (checked when
                   // it goes to LDS)
  bool mybadw = false;
  auto gather = [&](int64_t c0) {
    const int n = (int)std::min<int64_t>(ALS_CHUNK, h - c0);
    if constexpr (WEIGHTED) {
      // issued with the image's first index load and not looked at here: a test of the value
      // would wait out a whole memory latency of its own (the weights stream, one new line an
      // image), which the long rows of the item step pay once per image
      if (t < ALS_CHUNK) wv = t < n ? wgt[p0 + c0 + t] : 0.f;
    }
#pragma unroll
    for (int q = 0; q < EPT; ++q) {
      const int e = t + 256 * q, k = e / DP, c = e % DP;
      float x = 0.f;
      if (k < n && c < d) {
        const int32_t j = idx[p0 + c0 + k];
        if (j < 0 || j >= tab_rows) mybad = true;
        else x = tab[(int64_t)j * ld + c];
      }
      v[q] = x;
    }
  };
  gather(0);
  for (int64_t c0 = 0; c0 < h; c0 += ALS_CHUNK) {
    const int n = (int)std::min<int64_t>(ALS_CHUNK, h - c0);
    __syncthreads();  // the previous image has been read (and `bad` is initialised)
#pragma unroll
    for (int q = 0; q < EPT; ++q) As[t + 256 * q] = v[q];
    if constexpr (WEIGHTED) {
      if (t < ALS_CHUNK) {
        if (!(wv >= 0.f && wv < __builtin_inff())) mybadw = true;  // negative, inf or NaN
        ws[t] = wv;
      }
    }
    __syncthreads();
    if (c0 + ALS_CHUNK < h) gather(c0 + ALS_CHUNK);
    als_mfma_chunk<NT, WEIGHTED>(As, n, acc, ws);
    if constexpr (WEIGHTED) {
      if (bc >= 0 && bc < d) {
#pragma unroll 4  // deeper unrolls cost VGPRs: at d = 64 this one stays at 64 (6 waves a SIMD)
        for (int k = 0; k < n; ++k) {
          const float x = As[k * DP + bc];
          bsum += x;
          bw = fmaf(ws[k], x, bw);
        }
      }
    } else {
      if (t < d)
        for (int k = 0; k < n; ++k) bsum += As[k * DP + t];
    }
  }
  if (mybad) bad = 1;
  if constexpr (WEIGHTED) {
    if (mybadw) badw = 1;
  }
  __syncthreads();  // the last image has been read: the matrix takes its place
  if constexpr (WEIGHTED) {
    if (bad || badw) {  // uniform
      if (t == 0) hnm_flag(err, (bad ? HNM_ERR_OOB : 0u) | (badw ? HNM_ERR_WEIGHT : 0u));
      if (t < d) orow[t] = __builtin_nanf("");
      return;
    }
  } else {
    if (bad) {  // uniform
      if (t == 0) hnm_flag(err, HNM_ERR_OOB);
      if (t < d) orow[t] = __builtin_nanf("");
      return;
    }
  }
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
        if (i < d && j <= i) {
          float a = fmaf(alpha, acc[s][x], gram[(int64_t)i * d + j]);
          if (i == j) a += reg;
          As[i * LD + j] = a;
        }
      }
    }
  }
  if constexpr (WEIGHTED) {
    if (bc >= 0 && bc < d) As[d * LD + bc] = fmaf(alpha, bw, bsum);
  } else {
    if (t < d) As[d * LD + t] = one_alpha * bsum;
  }
  __syncthreads();
  SOLVER::template run<NT>(As, d, orow, steps);
}

inline bool als_dim_ok(int64_t d) { return d >= 16 && d <= 128 && d % 16 == 0; }

}  // namespace
