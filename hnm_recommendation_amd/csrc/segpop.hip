// SegmentPopularity (no reference module; `scripts/analyze_recommendation_challenges.py` names
// the strategy: "Demographics -> popular items in age/gender group", fallback global
// popularity): popularity.hip's fit with one count table per user segment, and a per-row top-K
// that continues a short segment list from the global one.
//
// Fit: S segments, row S = every transaction (the global row, hnm_popularity_fit_f64's result).
//   cnt[d, s, i] = rows with day d, item i and a user of segment s   (int32, integer atomics)
//   count[s, i]  = sum_d cnt[d, s, i]
//   pop[s, i]    = ((0 + cnt[0,s,i] w[0]) + cnt[1,s,i] w[1]) + ...  ascending d, float64, one
//                  rounded product and one rounded add per day (no fma)
// The table lives in the ctx workspace as [slab days, S + 1, num_items]; a thread per (s, i)
// cell folds it, so the fold is pop_fold_kernel over (S + 1) * num_items cells and row S has
// the baseline's bits.  The day range is walked in ascending slabs of at most POP_TABLE_CAP.
//
// Top-K: one wave per request row, two phases of pop_topk_kernel's pass (an LDS bitmap over a
// window of an order, clear positions emitted by ballot + popcount prefix):
//   1. order s (the row's segment) over min(R_s, k + h), marking the h history items;
//   2. the global order over min(R_g, k + h), marking the history AND the e items phase 1
//      emitted (read back from the row's own output), continuing at slot e.
// h + e marks remove at most h + e of the first (k - e) + h + e ranks, so the window suffices.
#include "hnm_device.h"
#include "hnm_internal.h"
#include "popularity_internal.h"

namespace {

// cnt[((d - d0) * (S + 1) + row) * I + item] += 1 for row = S and row = the user's segment.
__global__ __launch_bounds__(256) void segpop_fill_kernel(
    const int64_t* __restrict__ item_ids, const int64_t* __restrict__ user_ids,
    const int32_t* __restrict__ user_segment, int64_t num_users,
    const int32_t* __restrict__ days_ago, int64_t n, int64_t num_items, int S, int d0, int d1,
    int* __restrict__ cnt, unsigned* err) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += stride) {
    // The first slab checks the ids of every row, whatever its day; the later ones read the
    // day alone (4 of a row's 20 bytes, and no segment gather) for the rows outside the slab.
    const int d = days_ago ? days_ago[r] : 0;
    const bool inside = d >= d0 && d < d1;  // false outside [0, num_days)
    if (!inside && d0 != 0) continue;
    const int64_t it = item_ids[r];
    const int64_t u = user_ids[r];
    if (it < 0 || it >= num_items || u < 0 || u >= num_users) {
      hnm_flag(err, HNM_ERR_OOB);
      continue;
    }
    const int s = user_segment[u];
    if (s >= S) {
      hnm_flag(err, HNM_ERR_OOB);
      continue;
    }
    if (!inside) continue;
    int* day = cnt + (int64_t)(d - d0) * (S + 1) * num_items;
    atomicAdd(&day[(int64_t)S * num_items + it], 1);
    if (s >= 0) atomicAdd(&day[(int64_t)s * num_items + it], 1);  // s < 0: segment unknown
  }
}

// One thread per (segment, item) cell: pop_fold_kernel's chain over the slab's days.
__global__ __launch_bounds__(256) void segpop_fold_kernel(const int* __restrict__ cnt,
                                                          int64_t cells, int d0, int d1,
                                                          const double* __restrict__ w, bool first,
                                                          int64_t* __restrict__ count,
                                                          double* __restrict__ pop) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= cells) return;
  int64_t c64 = first ? 0 : count[c];
  double acc = first ? 0.0 : pop[c];
  {
#pragma clang fp contract(off)
    for (int d = d0; d < d1; ++d) {
      const int x = cnt[(int64_t)(d - d0) * cells + c];
      c64 += x;
      const double prod = (double)x * (w ? w[d] : 1.0);
      acc = acc + prod;
    }
  }
  count[c] = c64;
  pop[c] = acc;
}

// One phase of a row: continue it at slot `emitted` with the first clear positions of
// order[0, W), in passes of `chunk` ascending ranks (pop_topk_kernel's pass).  Marked: the h
// history items, and the first `prior` entries of the row's own output `oi` (what the phase
// before emitted; the caller has put a barrier between those stores and these loads).
// `flag`: this pass reports out-of-range history ids; the first pass of a row clears it, so an
// id is reported once whichever phase meets it first.  Returns the new emitted count.
__device__ __forceinline__ int segpop_phase(const int64_t* __restrict__ order,
                                            const float* __restrict__ order_val, int64_t W,
                                            const int32_t* __restrict__ rank, int64_t num_items,
                                            const int32_t* __restrict__ midx, int64_t m0, int64_t h,
                                            int prior, int k, int chunk, float* ov, int64_t* oi,
                                            unsigned* bits, bool& flag, unsigned* err,
                                            int emitted) {
  const int lane = threadIdx.x;
  for (int64_t c0 = 0; c0 < W && emitted < k; c0 += chunk) {
    const int len = (int)(W - c0 < chunk ? W - c0 : chunk);
    const int nw = (len + 31) >> 5;
    for (int x = lane; x < nw; x += 64) bits[x] = 0u;
    __syncthreads();
    for (int64_t j = lane; j < h; j += 64) {
      const int32_t it = midx[m0 + j];
      if (it < 0 || it >= num_items) {
        if (flag) hnm_flag(err, HNM_ERR_OOB);
        continue;
      }
      const int64_t r = (int64_t)rank[it] - c0;
      if (r >= 0 && r < len) atomicOr(&bits[r >> 5], 1u << (r & 31));
    }
    for (int j = lane; j < prior; j += 64) {
      const int64_t it = oi[j];
      if (it < 0 || it >= num_items) continue;  // an installed order with a foreign id
      const int64_t r = (int64_t)rank[it] - c0;
      if (r >= 0 && r < len) atomicOr(&bits[r >> 5], 1u << (r & 31));
    }
    flag = false;
    __syncthreads();
    for (int g = 0; g < len && emitted < k; g += 64) {
      const int p = g + lane;
      const bool clear = p < len && !((bits[p >> 5] >> (p & 31)) & 1u);
      const uint64_t m = __ballot(clear);
      const int slot = emitted + __popcll(m & ((1ull << lane) - 1ull));
      if (clear && slot < k) {
        ov[slot] = order_val[c0 + p];
        oi[slot] = order[c0 + p];
      }
      emitted += __popcll(m);
    }
    __syncthreads();  // the next pass clears the bitmap these reads used
  }
  return emitted < k ? emitted : k;
}

// One wave (one 64-thread workgroup) per request row.
__global__ __launch_bounds__(64) void segpop_topk_kernel(
    const int64_t* __restrict__ order, const float* __restrict__ order_val,
    const int64_t* __restrict__ order_ptr, const int32_t* __restrict__ rank, int64_t num_items,
    int S, const int32_t* __restrict__ seg, const int64_t* __restrict__ mptr,
    const int32_t* __restrict__ midx, int k, int chunk, float* out_val, int64_t* out_idx,
    int32_t* __restrict__ out_nseg, unsigned* err) {
  __shared__ unsigned bits[POP_CHUNK_MAX / 32];
  const int64_t b = blockIdx.x;
  const int lane = threadIdx.x;
  float* ov = out_val + b * k;
  int64_t* oi = out_idx + b * k;
  int64_t m0 = 0, h = 0;
  if (mptr) {
    m0 = mptr[b];
    h = mptr[b + 1] - m0;
    if (h < 0) h = 0;
  }
  int s = seg ? seg[b] : -1;
  if (s >= S) {
    if (lane == 0) hnm_flag(err, HNM_ERR_OOB);
    s = -1;  // answered as a row without a segment
  }
  bool flag = true;
  int emitted = 0;
  if (s >= 0) {
    const int64_t o0 = order_ptr[s];
    const int64_t R = order ? order_ptr[s + 1] - o0 : 0;
    const int64_t W = R < (int64_t)k + h ? R : (int64_t)k + h;
    emitted = segpop_phase(order + o0, order_val + o0, W, rank + (int64_t)s * num_items,
                           num_items, midx, m0, h, 0, k, chunk, ov, oi, bits, flag, err, 0);
  }
  if (out_nseg && lane == 0) out_nseg[b] = emitted;
  if (emitted < k) {
    // phase 2 reads oi[0, emitted) back: the barrier (and the workgroup fence it carries)
    // orders phase 1's stores before those loads
    __syncthreads();
    const int64_t o0 = order_ptr[S];
    const int64_t R = order ? order_ptr[S + 1] - o0 : 0;
    const int64_t W = R < (int64_t)k + h ? R : (int64_t)k + h;
    emitted = segpop_phase(order + o0, order_val + o0, W, rank + (int64_t)S * num_items,
                           num_items, midx, m0, h, emitted, k, chunk, ov, oi, bits, flag, err,
                           emitted);
  }
  for (int x = emitted + lane; x < k; x += 64) {
    ov[x] = -__builtin_inff();
    oi[x] = -1;
  }
}

}  // namespace

extern "C" hnm_status hnm_segpop_fit_f64(hnm_ctx* ctx, const int64_t* item_ids,
                                         const int64_t* user_ids, int64_t n,
                                         const int32_t* user_segment, int64_t num_users,
                                         const int32_t* days_ago, const double* day_weight,
                                         int64_t num_items, int64_t num_segments,
                                         int64_t num_days, int64_t slab, int64_t* count,
                                         double* pop) {
  HNM_CTX_DEVICE(ctx);
  HNM_REQUIRE(ctx && ((item_ids && user_ids) || n == 0) && (user_segment || num_users == 0) &&
                  (count || num_items == 0) && (pop || num_items == 0),
              HNM_EINVAL, "segpop_fit: NULL argument");
  HNM_REQUIRE(n >= 0 && num_items >= 0 && num_users >= 0 && slab >= 0, HNM_EINVAL,
              "segpop_fit: bad size");
  HNM_REQUIRE(num_segments >= 1, HNM_EINVAL, "segpop_fit: num_segments must be >= 1");
  const double* w = day_weight;
  if (!days_ago) {  // plain counts: one day of weight 1.0
    num_days = 1;
    w = nullptr;
  }
  HNM_REQUIRE(num_days >= 1, HNM_EINVAL, "segpop_fit: num_days must be >= 1");
  HNM_REQUIRE(num_days <= POP_MAX_DAYS, HNM_EUNSUPPORTED, "segpop_fit: num_days = %lld exceeds %d",
              (long long)num_days, POP_MAX_DAYS);
  HNM_REQUIRE(num_items <= INT32_MAX && num_segments < INT32_MAX, HNM_EUNSUPPORTED,
              "segpop_fit: num_items or num_segments exceeds 2^31");
  if (num_items == 0) return HNM_OK;
  const size_t rows = (size_t)num_segments + 1;
  HNM_REQUIRE(rows <= POP_TABLE_CAP / ((size_t)num_items * sizeof(int)), HNM_EUNSUPPORTED,
              "segpop_fit: one day's [%lld + 1, %lld] count table exceeds %zu bytes",
              (long long)num_segments, (long long)num_items, POP_TABLE_CAP);
  const int64_t cells = (int64_t)rows * num_items;
  const int D = (int)num_days;
  int64_t L = slab;
  if (L == 0) L = std::max<int64_t>(1, (int64_t)(POP_TABLE_CAP / ((size_t)cells * sizeof(int))));
  if (L > D) L = D;
  int* cnt = nullptr;
  hnm_status st = hnm_workspace(ctx, (size_t)L * (size_t)cells * sizeof(int), (void**)&cnt);
  if (st != HNM_OK) return st;
  const unsigned fill_grid = (unsigned)std::min<int64_t>(POP_FILL_BLOCKS, hnm_cdiv(n, 256));
  const unsigned fold_grid = (unsigned)hnm_cdiv(cells, 256);
  for (int d0 = 0; d0 < D; d0 += (int)L) {
    const int d1 = (int)std::min<int64_t>(D, d0 + L);
    HNM_HIP_CHECK(
        hipMemsetAsync(cnt, 0, (size_t)(d1 - d0) * (size_t)cells * sizeof(int), ctx->stream));
    if (n > 0) {
      hipLaunchKernelGGL(segpop_fill_kernel, dim3(fill_grid), dim3(256), 0, ctx->stream, item_ids,
                         user_ids, user_segment, num_users, days_ago, n, num_items,
                         (int)num_segments, d0, d1, cnt, ctx->err_dev);
      HNM_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(segpop_fold_kernel, dim3(fold_grid), dim3(256), 0, ctx->stream, cnt, cells,
                       d0, d1, w, d0 == 0, count, pop);
    HNM_LAUNCH_CHECK();
  }
  return HNM_OK;
}

extern "C" hnm_status hnm_segpop_topk_f32(hnm_ctx* ctx, const int64_t* order,
                                          const float* order_val, const int64_t* order_ptr,
                                          const int32_t* rank, int64_t num_items,
                                          int64_t num_segments, const int32_t* seg,
                                          const int64_t* mask_ptr, const int32_t* mask_idx,
                                          int64_t B, int k, int chunk, float* out_val,
                                          int64_t* out_idx, int32_t* out_nseg) {
  HNM_CTX_DEVICE(ctx);
  HNM_REQUIRE(ctx, HNM_EINVAL, "segpop_topk: ctx is NULL");
  HNM_REQUIRE(B >= 0 && k >= 0 && num_items >= 0, HNM_EINVAL, "segpop_topk: bad size");
  HNM_REQUIRE(num_segments >= 1 && num_segments < INT32_MAX, HNM_EINVAL,
              "segpop_topk: num_segments must be in [1, 2^31 - 1)");
  HNM_REQUIRE(chunk == 0 || (chunk >= 64 && chunk <= POP_CHUNK_MAX && chunk % 64 == 0), HNM_EINVAL,
              "segpop_topk: chunk must be 0 or a multiple of 64 in [64, %d]", POP_CHUNK_MAX);
  HNM_REQUIRE(B <= INT32_MAX, HNM_EUNSUPPORTED, "segpop_topk: B exceeds 2^31 - 1");
  if (B == 0) return HNM_OK;
  if (k == 0) {  // no list: every row's segment part is empty
    if (out_nseg)
      HNM_HIP_CHECK(hipMemsetAsync(out_nseg, 0, (size_t)B * sizeof(int32_t), ctx->stream));
    return HNM_OK;
  }
  // order == NULL: every order is empty (a fit that saw no transaction)
  HNM_REQUIRE(out_val && out_idx && order_ptr && (order != nullptr) == (order_val != nullptr),
              HNM_EINVAL, "segpop_topk: NULL argument");
  HNM_REQUIRE(!mask_ptr || (mask_idx && rank), HNM_EINVAL,
              "segpop_topk: a mask needs mask_idx and the rank table");
  HNM_REQUIRE(rank || !seg, HNM_EINVAL, "segpop_topk: segments need the rank table");
  hipLaunchKernelGGL(segpop_topk_kernel, dim3((unsigned)B), dim3(64), 0, ctx->stream, order,
                     order_val, order_ptr, rank, num_items, (int)num_segments, seg, mask_ptr,
                     mask_idx, k, chunk ? chunk : POP_CHUNK_MAX, out_val, out_idx, out_nseg,
                     ctx->err_dev);
  HNM_LAUNCH_CHECK();
  return HNM_OK;
}
