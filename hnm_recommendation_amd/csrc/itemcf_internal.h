// The wave-resident top-N list of the neighbour-table fits (itemcf.hip, content.hip, seqcf.hip): slot s of a
// row's list lives in lane s of one register pair, (value descending, index ascending) order.  And
// the scan of the item -> row transpose that itemcf.hip and seqcf.hip build.
#pragma once
#include "hnm_device.h"
#include "hnm_internal.h"

namespace {

// Offer one candidate per lane to a single-register wave list (slot s in lane s, K <= 64).
__device__ __forceinline__ void icf_offer(float& lv, int& li, float sv, int si, bool valid, int K) {
  const float tv = hnm_readlane_f(lv, K - 1);
  const int ti = hnm_readlane_i(li, K - 1);
  uint64_t m = __ballot(valid && hnm_better(sv, si, tv, ti));
  while (m) {
    const int l = __builtin_ctzll(m);
    m &= m - 1;
    list1_insert(lv, li, hnm_readlane_f(sv, l), hnm_readlane_i(si, l), K);
  }
}

// Fold the lists of waves 1..3 of a 256-thread workgroup into wave 0's (mv / mi: 256 slots of
// LDS).  Every thread calls it; the result is valid in wave 0.
__device__ __forceinline__ void icf_merge4(float& lv, int& li, float* mv, int* mi, int K) {
  const int t = threadIdx.x;
  mv[t] = lv;
  mi[t] = li;
  __syncthreads();
  if (t < 64) {
    for (int w = 1; w < 4; ++w) {
      const float cv = mv[w * 64 + t];
      const int ci = mi[w * 64 + t];
      icf_offer(lv, li, cv, ci, ci != HNM_SENTINEL_IDX, K);
    }
  }
}

// One workgroup: tptr = exclusive scan of cnt (tptr[I] = total), cursor = tptr[0, I),
// item_count = cnt as int64.
__global__ __launch_bounds__(1024) void icf_scan_kernel(const int* __restrict__ cnt, int64_t I,
                                                        int* __restrict__ tptr,
                                                        int* __restrict__ cursor,
                                                        int64_t* __restrict__ item_count) {
  __shared__ int part[1024];
  const int t = threadIdx.x;
  const int64_t per = hnm_cdiv(I, 1024);
  const int64_t b = std::min<int64_t>(I, t * per), e = std::min<int64_t>(I, b + per);
  int s = 0;
  for (int64_t x = b; x < e; ++x) s += cnt[x];
  part[t] = s;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const int v = t >= o ? part[t - o] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int base = part[t] - s;
  for (int64_t x = b; x < e; ++x) {
    const int c = cnt[x];
    tptr[x] = base;
    cursor[x] = base;
    item_count[x] = c;
    base += c;
  }
  if (t == 1023) tptr[I] = part[1023];
}

}  // namespace
