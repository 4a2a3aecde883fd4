// LightGCN graph path, CSR build (a5): the normalized adjacency D^-1/2 (A + I) D^-1/2 as CSR.
//
// lightgcn.py:81-134: edges are radix-sorted by row (stable, so within a row the reference's
// edge order is kept) and each row gets its self-loop appended last, the same summation order
// as the reference's `cat([edges, loops])` (lightgcn.py:128-131).  deg = row sum of the weights
// (exact integer counts for unweighted graphs), dinv = deg^-1/2 with inf -> 0,
// val = (dinv[row] * w) * dinv[col] (lightgcn.py:104-106).
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "hnm_device.h"
#include "hnm_internal.h"

__global__ void csr_prep_kernel(const int64_t* __restrict__ ei, int64_t E, int64_t N,
                                int32_t* __restrict__ keys, int32_t* __restrict__ vals,
                                unsigned* err) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < E;
       e += (int64_t)gridDim.x * 256) {
    int64_t r = ei[e], c = ei[E + e];
    if (r < 0 || r >= N || c < 0 || c >= N) {
      hnm_flag(err, HNM_ERR_OOB);
      r = 0;
    }
    keys[e] = (int32_t)r;
    vals[e] = (int32_t)e;
  }
}

// Row extents from the sorted keys (no atomics: power-law rows would serialize them):
// first[r] / last[r] = first and one-past-last sorted position of row r (0 / 0 if empty).
__global__ void csr_extent_kernel(const int32_t* __restrict__ skeys, int64_t E,
                                  int32_t* __restrict__ first, int32_t* __restrict__ last) {
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < E;
       p += (int64_t)gridDim.x * 256) {
    const int32_t r = skeys[p];
    if (p == 0 || skeys[p - 1] != r) first[r] = (int32_t)p;
    if (p == E - 1 || skeys[p + 1] != r) last[r] = (int32_t)(p + 1);
  }
}

__global__ void csr_counts_kernel(const int32_t* __restrict__ first,
                                  const int32_t* __restrict__ last, int64_t N,
                                  int64_t* __restrict__ counts) {
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r <= N;
       r += (int64_t)gridDim.x * 256)
    counts[r] = r < N ? (int64_t)(last[r] - first[r]) + 1 : 0;
}

__global__ void csr_place_kernel(const int64_t* __restrict__ ei, const float* __restrict__ w,
                                 int64_t E, int64_t N, const int32_t* __restrict__ skeys,
                                 const int32_t* __restrict__ svals,
                                 const int64_t* __restrict__ rowptr, int32_t* __restrict__ col,
                                 float* __restrict__ wt) {
  const int64_t total = E + N;
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < total;
       p += (int64_t)gridDim.x * 256) {
    if (p < E) {
      const int64_t r = skeys[p];
      const int64_t e = svals[p];
      const int64_t dst = p + r;  // rows < r each hold one extra (self-loop) entry
      int64_t c = ei[E + e];
      if (c < 0 || c >= N) c = 0;
      col[dst] = (int32_t)c;
      wt[dst] = w ? w[e] : 1.f;
    } else {
      const int64_t r = p - E;
      const int64_t dst = rowptr[r + 1] - 1;
      col[dst] = (int32_t)r;
      wt[dst] = 1.f;
    }
  }
}

// dinv[r] = deg^-1/2 (inf -> 0); one wave per row, fixed-order reduction when weighted
__global__ __launch_bounds__(256) void csr_degree_kernel(const int64_t* __restrict__ rowptr,
                                                         const float* __restrict__ wt, int64_t N,
                                                         bool weighted,
                                                         float* __restrict__ dinv) {
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= N) return;
  const int lane = threadIdx.x & 63;
  const int64_t s = rowptr[r], e = rowptr[r + 1];
  float deg;
  if (!weighted) {
    deg = (float)(e - s);
  } else {
    float acc = 0.f;
    for (int64_t p = s + lane; p < e; p += 64) acc += wt[p];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o);
    deg = acc;
  }
  if (lane == 0) {
    float di = 1.0f / sqrtf(deg);
    if (isinf(di)) di = 0.f;
    dinv[r] = di;
  }
}

// val = (dinv[row] * w) * dinv[col]: one thread per entry (edges via the sorted keys,
// then the self-loops), so power-law rows cost nothing extra.
__global__ void csr_norm_kernel(const int32_t* __restrict__ skeys, int64_t E, int64_t N,
                                const int64_t* __restrict__ rowptr,
                                const int32_t* __restrict__ col, const float* __restrict__ dinv,
                                float* __restrict__ val) {
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < E + N;
       p += (int64_t)gridDim.x * 256) {
    int64_t r, dst;
    if (p < E) {
      r = skeys[p];
      dst = p + r;
    } else {
      r = p - E;
      dst = rowptr[r + 1] - 1;
    }
    val[dst] = (dinv[r] * val[dst]) * dinv[col[dst]];
  }
}

extern "C" hnm_status hnm_csr_build_norm(hnm_ctx* ctx, const int64_t* edge_index,
                                         const float* edge_weight, int64_t E, int64_t N,
                                         int64_t* rowptr, int32_t* col, float* val) {
  HNM_CTX_DEVICE(ctx);
  HNM_REQUIRE(ctx && rowptr && col && val && (edge_index || E == 0), HNM_EINVAL,
              "csr_build: NULL argument");
  HNM_REQUIRE(N > 0 && N < 0x7fffffff && E >= 0 && E < 0x7fffffff, HNM_EUNSUPPORTED,
              "csr_build: N and E must fit int32 (N=%lld, E=%lld)", (long long)N, (long long)E);
  hipStream_t st = ctx->stream;
  const int64_t En = std::max<int64_t>(E, 1);
  int bits = 1;
  while (bits < 31 && ((int64_t)1 << bits) < N) ++bits;
  size_t sort_tmp = 0, scan_tmp = 0;
  HNM_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_tmp, (int32_t*)nullptr,
                                                   (int32_t*)nullptr, (int32_t*)nullptr,
                                                   (int32_t*)nullptr, (int)En, 0, bits, st));
  HNM_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_tmp, (int64_t*)nullptr,
                                                 (int64_t*)nullptr, (int)(N + 1), st));
  const size_t s4 = hnm_align((size_t)En * 4);
  const size_t sc = hnm_align((size_t)(N + 1) * 4), sc8 = hnm_align((size_t)(N + 1) * 8);
  const size_t sd = hnm_align((size_t)N * 4);
  const size_t tmp = hnm_align(std::max(sort_tmp, scan_tmp));
  void* wsp;
  hnm_status s = hnm_workspace(ctx, 4 * s4 + 2 * sc + sc8 + sd + tmp, &wsp);
  if (s) return s;
  char* p = (char*)wsp;
  int32_t* kin = (int32_t*)p; p += s4;
  int32_t* kout = (int32_t*)p; p += s4;
  int32_t* vin = (int32_t*)p; p += s4;
  int32_t* vout = (int32_t*)p; p += s4;
  int32_t* first = (int32_t*)p; p += sc;
  int32_t* last = (int32_t*)p; p += sc;
  int64_t* counts = (int64_t*)p; p += sc8;
  float* dinv = (float*)p; p += sd;
  void* t = p;

  HNM_HIP_CHECK(hipMemsetAsync(first, 0, (size_t)(N + 1) * 4, st));
  HNM_HIP_CHECK(hipMemsetAsync(last, 0, (size_t)(N + 1) * 4, st));
  const unsigned g = 8 * 1024;
  if (E > 0) {
    hipLaunchKernelGGL(csr_prep_kernel, dim3(g), dim3(256), 0, st, edge_index, E, N, kin, vin,
                       ctx->err_dev);
    HNM_LAUNCH_CHECK();
    size_t tb = sort_tmp;
    HNM_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(t, tb, kin, kout, vin, vout, (int)E, 0, bits, st));
    hipLaunchKernelGGL(csr_extent_kernel, dim3(g), dim3(256), 0, st, kout, E, first, last);
    HNM_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(csr_counts_kernel, dim3(g), dim3(256), 0, st, first, last, N, counts);
  HNM_LAUNCH_CHECK();
  size_t tb = scan_tmp;
  HNM_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(t, tb, counts, rowptr, (int)(N + 1), st));
  hipLaunchKernelGGL(csr_place_kernel, dim3(g), dim3(256), 0, st, edge_index, edge_weight, E, N,
                     kout, vout, rowptr, col, val);
  HNM_LAUNCH_CHECK();
  const dim3 rg((unsigned)hnm_cdiv(N, 4));
  hipLaunchKernelGGL(csr_degree_kernel, rg, dim3(256), 0, st, rowptr, val, N,
                     edge_weight != nullptr, dinv);
  HNM_LAUNCH_CHECK();
  hipLaunchKernelGGL(csr_norm_kernel, dim3(g), dim3(256), 0, st, kout, E, N, rowptr, col, dinv,
                     val);
  HNM_LAUNCH_CHECK();
  return HNM_OK;
}
