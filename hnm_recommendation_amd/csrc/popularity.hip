// PopularityBaseline (reference: `src/models/baseline.py`): the fit and the per-user top-K.
//
// Fit (`baseline.py:137-165`: value_counts / groupby('article_idx')['weight'].sum()):
//   cnt[i, d]  = rows with item i and day d        (int32, integer atomics: order-independent)
//   count[i]   = sum_d cnt[i, d]
//   pop[i]     = ((0 + cnt[i,0] w[0]) + cnt[i,1] w[1]) + ...   ascending d, float64, one
//                rounded product and one rounded add per day (no fma)
// so the result is the same bits on every run and equals a host loop over an [I, D] count
// table.  The table lives in the ctx workspace as [slab days, num_items] (day-major: a
// thread per item reads it coalesced, and transactions sorted by date hit one 4*I-byte row);
// when D * I * 4 B exceeds POP_TABLE_CAP the day range is walked in ascending slabs, each
// continuing the chain from pop[i] -- the same additions in the same order.
//
// Top-K (`baseline.py:78-85, 183-187`: [x for x in item_popularity if x not in hist][:k]):
// a user with h history items needs at most the first k + h entries of the popularity order,
// so one wave marks rank[item] of its history in an LDS bitmap of that window and emits the
// first k clear positions by ballot + popcount prefix: O(k + h) per user instead of O(I).
#include "hnm_device.h"
#include "hnm_internal.h"
#include "popularity_internal.h"

namespace {

// cnt[(d - d0) * I + item] += 1 for the rows whose day falls in the slab [d0, d1).
__global__ __launch_bounds__(256) void pop_fill_kernel(const int64_t* __restrict__ item_ids,
                                                       const int32_t* __restrict__ days_ago,
                                                       int64_t n, int64_t num_items, int d0,
                                                       int d1, int* __restrict__ cnt,
                                                       unsigned* err) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += stride) {
    const int64_t it = item_ids[r];
    if (it < 0 || it >= num_items) {
      hnm_flag(err, HNM_ERR_OOB);
      continue;
    }
    const int d = days_ago ? days_ago[r] : 0;
    if (d < d0 || d >= d1) continue;  // outside the slab, or outside [0, num_days)
    atomicAdd(&cnt[(int64_t)(d - d0) * num_items + it], 1);
  }
}

// One thread per item: continue count[i] / pop[i] over the slab's days in ascending order.
__global__ __launch_bounds__(256) void pop_fold_kernel(const int* __restrict__ cnt,
                                                       int64_t num_items, int d0, int d1,
                                                       const double* __restrict__ w, bool first,
                                                       int64_t* __restrict__ count,
                                                       double* __restrict__ pop) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= num_items) return;
  int64_t c64 = first ? 0 : count[i];
  double acc = first ? 0.0 : pop[i];
  {
#pragma clang fp contract(off)
    for (int d = d0; d < d1; ++d) {
      const int c = cnt[(int64_t)(d - d0) * num_items + i];
      c64 += c;
      const double prod = (double)c * (w ? w[d] : 1.0);
      acc = acc + prod;
    }
  }
  count[i] = c64;
  pop[i] = acc;
}

// One wave (one 64-thread workgroup) per user.  Window W = min(R, k + h): h masked items can
// remove at most h of the first k + h ranks.  The window is processed in passes of `chunk`
// ascending ranks: clear the bitmap, set bit rank[item] - c0 for every history item whose rank
// falls in the pass (atomic OR: several lanes may share a word; duplicates and rank -1 do
// nothing), then emit the clear positions in rank order, carrying the emitted count.
__global__ __launch_bounds__(64) void pop_topk_kernel(
    const int64_t* __restrict__ order, const float* __restrict__ order_val, int64_t R,
    const int32_t* __restrict__ rank, int64_t num_items, const int64_t* __restrict__ mptr,
    const int32_t* __restrict__ midx, int k, int chunk, float* __restrict__ out_val,
    int64_t* __restrict__ out_idx, unsigned* err) {
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
  const int64_t W = R < (int64_t)k + h ? R : (int64_t)k + h;
  int emitted = 0;
  for (int64_t c0 = 0; c0 < W && emitted < k; c0 += chunk) {
    const int len = (int)(W - c0 < chunk ? W - c0 : chunk);
    const int nw = (len + 31) >> 5;
    for (int x = lane; x < nw; x += 64) bits[x] = 0u;
    __syncthreads();
    for (int64_t j = lane; j < h; j += 64) {
      const int32_t it = midx[m0 + j];
      if (it < 0 || it >= num_items) {
        if (c0 == 0) hnm_flag(err, HNM_ERR_OOB);
        continue;
      }
      const int64_t r = (int64_t)rank[it] - c0;
      if (r >= 0 && r < len) atomicOr(&bits[r >> 5], 1u << (r & 31));
    }
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
  if (emitted > k) emitted = k;
  for (int s = emitted + lane; s < k; s += 64) {
    ov[s] = -__builtin_inff();
    oi[s] = -1;
  }
}

}  // namespace

extern "C" hnm_status hnm_popularity_fit_f64(hnm_ctx* ctx, const int64_t* item_ids, int64_t n,
                                             const int32_t* days_ago, const double* day_weight,
                                             int64_t num_items, int64_t num_days, int64_t slab,
                                             int64_t* count, double* pop) {
  HNM_CTX_DEVICE(ctx);
  HNM_REQUIRE(ctx && (item_ids || n == 0) && (count || num_items == 0) && (pop || num_items == 0),
              HNM_EINVAL, "popularity_fit: NULL argument");
  HNM_REQUIRE(n >= 0 && num_items >= 0 && slab >= 0, HNM_EINVAL, "popularity_fit: bad size");
  const double* w = day_weight;
  if (!days_ago) {  // plain counts: one day of weight 1.0
    num_days = 1;
    w = nullptr;
  }
  HNM_REQUIRE(num_days >= 1, HNM_EINVAL, "popularity_fit: num_days must be >= 1");
  HNM_REQUIRE(num_days <= POP_MAX_DAYS, HNM_EUNSUPPORTED,
              "popularity_fit: num_days = %lld exceeds %d", (long long)num_days, POP_MAX_DAYS);
  HNM_REQUIRE(num_items <= INT32_MAX, HNM_EUNSUPPORTED, "popularity_fit: num_items exceeds 2^31");
  if (num_items == 0) return HNM_OK;
  const int D = (int)num_days;
  int64_t S = slab;
  if (S == 0) S = std::max<int64_t>(1, (int64_t)(POP_TABLE_CAP / ((size_t)num_items * 4)));
  if (S > D) S = D;
  const size_t table = (size_t)S * (size_t)num_items * sizeof(int);
  int* cnt = nullptr;
  hnm_status st = hnm_workspace(ctx, table, (void**)&cnt);
  if (st != HNM_OK) return st;
  const unsigned fill_grid = (unsigned)std::min<int64_t>(POP_FILL_BLOCKS, hnm_cdiv(n, 256));
  const unsigned fold_grid = (unsigned)hnm_cdiv(num_items, 256);
  for (int d0 = 0; d0 < D; d0 += (int)S) {
    const int d1 = (int)std::min<int64_t>(D, d0 + S);
    HNM_HIP_CHECK(hipMemsetAsync(cnt, 0, (size_t)(d1 - d0) * (size_t)num_items * sizeof(int),
                                 ctx->stream));
    if (n > 0) {
      hipLaunchKernelGGL(pop_fill_kernel, dim3(fill_grid), dim3(256), 0, ctx->stream, item_ids,
                         days_ago, n, num_items, d0, d1, cnt, ctx->err_dev);
      HNM_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(pop_fold_kernel, dim3(fold_grid), dim3(256), 0, ctx->stream, cnt, num_items,
                       d0, d1, w, d0 == 0, count, pop);
    HNM_LAUNCH_CHECK();
  }
  return HNM_OK;
}

extern "C" hnm_status hnm_popularity_topk_f32(hnm_ctx* ctx, const int64_t* order,
                                              const float* order_val, int64_t R,
                                              const int32_t* rank, int64_t num_items,
                                              const int64_t* mask_ptr, const int32_t* mask_idx,
                                              int64_t B, int k, int chunk, float* out_val,
                                              int64_t* out_idx) {
  HNM_CTX_DEVICE(ctx);
  HNM_REQUIRE(ctx, HNM_EINVAL, "popularity_topk: ctx is NULL");
  HNM_REQUIRE(B >= 0 && k >= 0 && R >= 0 && num_items >= 0, HNM_EINVAL,
              "popularity_topk: bad size");
  HNM_REQUIRE(chunk == 0 || (chunk >= 64 && chunk <= POP_CHUNK_MAX && chunk % 64 == 0), HNM_EINVAL,
              "popularity_topk: chunk must be 0 or a multiple of 64 in [64, %d]", POP_CHUNK_MAX);
  HNM_REQUIRE(B <= INT32_MAX, HNM_EUNSUPPORTED, "popularity_topk: B exceeds 2^31 - 1");
  if (B == 0 || k == 0) return HNM_OK;
  HNM_REQUIRE(out_val && out_idx && ((order && order_val) || R == 0), HNM_EINVAL,
              "popularity_topk: NULL argument");
  HNM_REQUIRE(!mask_ptr || ((mask_idx && rank) || R == 0), HNM_EINVAL,
              "popularity_topk: a mask needs mask_idx and the rank table");
  if (R == 0) mask_ptr = nullptr;  // nothing to filter: every slot is (-inf, -1)
  hipLaunchKernelGGL(pop_topk_kernel, dim3((unsigned)B), dim3(64), 0, ctx->stream, order, order_val,
                     R, rank, num_items, mask_ptr, mask_idx, k, chunk ? chunk : POP_CHUNK_MAX,
                     out_val, out_idx, ctx->err_dev);
  HNM_LAUNCH_CHECK();
  return HNM_OK;
}
