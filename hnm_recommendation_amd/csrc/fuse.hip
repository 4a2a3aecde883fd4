// Fusion of several models' top-K lists (GEMINI.md stage 5, "CF score ensemble"; no reference
// counterpart).  The contract is stated in include/hnm.h and restated in numpy by
// tests/fuse_oracle.py.
//
// hnm_topk_merge_f32 merges lists whose items are disjoint (item partitions, shards).  Here the
// lists overlap -- the same item may stand in the popularity list, the co-bought list and the
// factorisation's list of one user -- and an item's fused score depends on every list that holds
// it, so the merge needs a sum per item before it can select.
//
// Shape: one wave per row over an LDS open-addressing table keyed by item id (icf_topk_kernel's
// table), 2 * G * kc slots rounded up to a power of two, so every distinct item finds a slot.
// The lists are added one after the other, 64 entries a step: a lane claims its item's slot by
// compare-and-swap (two new items of one step may hash alike) and then owns it for that list,
// because the items of one list are distinct -- the add itself is a plain read-modify-write, no
// float atomic.  The lane that claims a slot stores its contribution, every later one adds to
// it: an item's sum starts from its first contribution and runs in ascending g whatever the
// lanes' timing, so the result is the same bits on every run.  Then the table's entries that
// are not in the row's mask go through the wave-resident list (WaveTopK<1> up to k = 64,
// WaveTopK<2> above); (score desc, item asc) is a total order over distinct items, so the order
// in which the table is walked is free.
//
// CASCADE rides the same table: the value of a slot is the code g * kc + j of the item's first
// occurrence (only the claiming lane stores), selection takes -code as the score (< 2,048: exact
// in fp32, all distinct), and the output value is read back from the list at the code.
#include "hnm_device.h"
#include "hnm_internal.h"

#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int FUSE_MAX_G = 16;
constexpr int FUSE_MAX_KC = 512;
constexpr int FUSE_MAX_ENTRIES = 2048;  // G * kc: a table of at most 4,096 slots (32 KiB)
constexpr int FUSE_MAX_K = 128;

__device__ __forceinline__ bool fuse_masked(const int32_t* midx, int64_t m0, int64_t m1, int item) {
  const int64_t p = mask_lower_bound(midx, m0, m1, item);
  return p < m1 && midx[p] == item;
}

// coef * val rounded to fp32; the add that follows must stay an add (no fma).
__device__ __forceinline__ float fuse_wmul(float w, float val) {
#pragma clang fp contract(off)
  const float prod = w * val;
  return prod;
}

// Entry t of the row's G * nch steps (step t = list t / nch, positions (t % nch) * 64 + lane):
// the item (-1: nothing to add) and what it adds -- RANK: coef[g * kc + j]; SCORE:
// fl(coef[g] * val); CASCADE: the code g * kc + j as a float.
template <int MODE>
__device__ __forceinline__ void fuse_step_load(const float* __restrict__ lv,
                                               const int64_t* __restrict__ li, int64_t gstride,
                                               int64_t row, int kc, int nch, int steps, int t,
                                               const float* __restrict__ coef, int64_t I,
                                               unsigned* err, int& idx, float& add) {
  idx = -1;
  add = 0.f;
  if (t >= steps) return;
  const int g = t / nch;
  const int j = (t - g * nch) * 64 + (int)threadIdx.x;
  if (j >= kc) return;
  const int64_t at = (int64_t)g * gstride + row + j;
  const int64_t it = li[at];
  const float v = lv[at];
  if (it < 0 || !(fabsf(v) <= 3.402823466e+38f)) return;  // empty: idx < 0, val inf or nan
  if (it >= I) {
    hnm_flag(err, HNM_ERR_OOB);
    return;
  }
  idx = (int)it;
  if constexpr (MODE == HNM_FUSE_RANK) add = coef[g * kc + j];
  else if constexpr (MODE == HNM_FUSE_SCORE) add = fuse_wmul(coef[g], v);
  else add = (float)(g * kc + j);
}

// One wave per row; dynamic LDS: cap keys, then cap values (cap = 1 << bits, >= 2 * G * kc).
template <int MODE, int NS>
__global__ __launch_bounds__(64) void fuse_topk_kernel(
    const float* __restrict__ list_val, const int64_t* __restrict__ list_idx, int G,
    int64_t gstride, int64_t bstride, int kc, const float* __restrict__ coef, int64_t I,
    const int64_t* __restrict__ mptr, const int32_t* __restrict__ midx, int k, int bits,
    float* __restrict__ out_val, int64_t* __restrict__ out_idx, unsigned* err) {
  extern __shared__ int fuse_lds[];
  const int cap = 1 << bits;
  int* key = fuse_lds;
  float* val = reinterpret_cast<float*>(fuse_lds + cap);
  const int64_t b = blockIdx.x;
  const int lane = threadIdx.x;
  for (int x = lane; x < cap; x += 64) {
    key[x] = -1;
    val[x] = 0.f;
  }
  __syncthreads();
  const int nch = (kc + 63) >> 6;
  const int steps = G * nch;
  const int64_t row = b * bstride;
  int nidx;
  float nadd;
  fuse_step_load<MODE>(list_val, list_idx, gstride, row, kc, nch, steps, 0, coef, I, err, nidx,
                       nadd);
  for (int t = 0; t < steps; ++t) {
    const int cidx = nidx;
    const float cadd = nadd;
    fuse_step_load<MODE>(list_val, list_idx, gstride, row, kc, nch, steps, t + 1, coef, I, err,
                         nidx, nadd);
    if (cidx >= 0) {
      unsigned slot = ((unsigned)cidx * 2654435761u) >> (32 - bits);
      int prev;
      for (;;) {  // at most G * kc <= cap / 2 slots are ever taken: the probe ends
        prev = atomicCAS(&key[slot], -1, cidx);
        if (prev == -1 || prev == cidx) break;
        slot = (slot + 1) & (cap - 1);
      }
      // this list's items are distinct: the slot is this lane's until the next list
      if (prev == -1) val[slot] = cadd;
      else if constexpr (MODE != HNM_FUSE_CASCADE) val[slot] = val[slot] + cadd;
    }
    __syncthreads();  // the next list reads what this one wrote (another lane's item)
  }
  int64_t m0 = 0, m1 = 0;
  if (mptr) {
    m0 = mptr[b];
    m1 = mptr[b + 1];
  }
  WaveTopK<NS> top;
  top.init();
  for (int g = 0; g < cap; g += 64) {
    const int kx = key[g + lane];
    float vx = val[g + lane];
    if constexpr (MODE == HNM_FUSE_CASCADE) vx = -vx;  // ascending code = descending -code
    bool ok = kx >= 0 && hnm_better(vx, kx, top.thr_v, top.thr_i);
    if (ok && m1 > m0) ok = !fuse_masked(midx, m0, m1, kx);
    top.offer(vx, kx, ok, k);
  }
  if constexpr (MODE == HNM_FUSE_CASCADE) {
#pragma unroll
    for (int r = 0; r < NS; ++r) {  // the value of the first occurrence, from the list itself
      if (top.i[r] != HNM_SENTINEL_IDX) {
        const int code = (int)(-top.v[r]);
        const int g = code / kc;
        top.v[r] = list_val[(int64_t)g * gstride + row + (code - g * kc)];
      }
    }
  }
  top.store(out_val + b * k, out_idx + b * k, k);
}

template <int MODE>
void fuse_launch(hnm_ctx* ctx, const float* list_val, const int64_t* list_idx, int64_t B, int G,
                 int64_t gstride, int64_t bstride, int kc, const float* coef, int64_t num_items,
                 const int64_t* mask_ptr, const int32_t* mask_idx, int k, float* out_val,
                 int64_t* out_idx) {
  int bits = 6;  // the selection walks the table 64 slots a step
  while ((1 << bits) < 2 * G * kc) ++bits;
  const size_t lds = (size_t)(1 << bits) * 8;
  if (k <= 64)
    hipLaunchKernelGGL((fuse_topk_kernel<MODE, 1>), dim3((unsigned)B), dim3(64), lds, ctx->stream,
                       list_val, list_idx, G, gstride, bstride, kc, coef, num_items, mask_ptr,
                       mask_idx, k, bits, out_val, out_idx, ctx->err_dev);
  else
    hipLaunchKernelGGL((fuse_topk_kernel<MODE, 2>), dim3((unsigned)B), dim3(64), lds, ctx->stream,
                       list_val, list_idx, G, gstride, bstride, kc, coef, num_items, mask_ptr,
                       mask_idx, k, bits, out_val, out_idx, ctx->err_dev);
}

}  // namespace

extern "C" hnm_status hnm_fuse_topk_f32(hnm_ctx* ctx, const float* list_val,
                                        const int64_t* list_idx, int64_t B, int64_t G,
                                        int64_t gstride, int64_t bstride, int kc, int mode,
                                        const float* coef, int64_t num_items,
                                        const int64_t* mask_ptr, const int32_t* mask_idx, int k,
                                        float* out_val, int64_t* out_idx) {
  HNM_CTX_DEVICE(ctx);
  HNM_REQUIRE(ctx, HNM_EINVAL, "fuse_topk: ctx is NULL");
  HNM_REQUIRE(mode == HNM_FUSE_RANK || mode == HNM_FUSE_SCORE || mode == HNM_FUSE_CASCADE,
              HNM_EINVAL, "fuse_topk: mode must be HNM_FUSE_RANK, _SCORE or _CASCADE");
  HNM_REQUIRE(coef || mode == HNM_FUSE_CASCADE, HNM_EINVAL,
              "fuse_topk: coef is NULL (only the cascade mode takes none)");
  HNM_REQUIRE(B >= 0 && num_items >= 0, HNM_EINVAL, "fuse_topk: bad size");
  HNM_REQUIRE(G >= 1 && G <= FUSE_MAX_G && kc >= 1 && kc <= FUSE_MAX_KC &&
                  G * kc <= FUSE_MAX_ENTRIES && k >= 0 && k <= FUSE_MAX_K,
              HNM_EUNSUPPORTED,
              "fuse_topk: 1 <= G <= %d, 1 <= kc <= %d, G * kc <= %d, 0 <= k <= %d", FUSE_MAX_G,
              FUSE_MAX_KC, FUSE_MAX_ENTRIES, FUSE_MAX_K);
  HNM_REQUIRE(B <= INT32_MAX && num_items < INT_BIG, HNM_EUNSUPPORTED,
              "fuse_topk: B or num_items exceeds 2^31 - 1");
  if (B == 0 || k == 0) return HNM_OK;
  HNM_REQUIRE(list_val && list_idx && out_val && out_idx, HNM_EINVAL,
              "fuse_topk: NULL list or output");
  HNM_REQUIRE(!mask_ptr || mask_idx, HNM_EINVAL, "fuse_topk: mask_ptr without mask_idx");
  if (mode == HNM_FUSE_RANK)
    fuse_launch<HNM_FUSE_RANK>(ctx, list_val, list_idx, B, (int)G, gstride, bstride, kc, coef,
                               num_items, mask_ptr, mask_idx, k, out_val, out_idx);
  else if (mode == HNM_FUSE_SCORE)
    fuse_launch<HNM_FUSE_SCORE>(ctx, list_val, list_idx, B, (int)G, gstride, bstride, kc, coef,
                                num_items, mask_ptr, mask_idx, k, out_val, out_idx);
  else
    fuse_launch<HNM_FUSE_CASCADE>(ctx, list_val, list_idx, B, (int)G, gstride, bstride, kc, coef,
                                  num_items, mask_ptr, mask_idx, k, out_val, out_idx);
  HNM_LAUNCH_CHECK();
  return HNM_OK;
}
