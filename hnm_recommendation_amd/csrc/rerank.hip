// Two-stage serving, the list kernels around the ranker (no reference counterpart; its design
// note asks for "Stage 1: candidate generation, Stage 2: ranking").  The contracts are stated in
// include/hnm.h and restated in numpy by tests/rerank_oracle.py.
//
// hnm_cand_union_i32: the G recall lists of a row -> one duplicate-free candidate row, ascending.
// One wave per row, four rows a workgroup.  The row's G * kc ids go into the wave's own LDS
// segment (the power of two >= G * kc ints, at most 8 KiB; empty entries and the padding hold
// INT_MAX, which no item id reaches), are sorted ascending by a bitonic network over the segment
// (64 compare-exchanges a step, only wave-level barriers: no other wave touches the segment), and
// the sorted row is compacted with ballot + popcount: an entry is kept when it differs from its
// left neighbour.  No atomics, no hashing: the output depends on the set of ids only, so it is the
// same bits on every run.
//
// hnm_cand_topk_f32: scored candidate rows -> the best k in (score desc, item asc) order.  One
// wave per row on WaveTopK (one register up to k = 64, two above).
#include "hnm_device.h"
#include "hnm_internal.h"

namespace {

constexpr int CAND_MAX_G = 16;         // the fuse kernel's limits (fuse.hip)
constexpr int CAND_MAX_KC = 512;
constexpr int CAND_MAX_ENTRIES = 2048;
constexpr int CAND_MAX_K = 128;
constexpr int CAND_EMPTY = INT_BIG;

// the wave's LDS segment is its own: order its accesses, wait for nobody else
__device__ __forceinline__ void cand_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// dynamic LDS: 4 segments of np = 1 << bits ints
__global__ __launch_bounds__(256) void cand_union_kernel(
    const float* __restrict__ list_val, const int64_t* __restrict__ list_idx, int64_t B, int G,
    int64_t gstride, int64_t bstride, int kc, int64_t I, int bits, int32_t* __restrict__ out_cand,
    int64_t ldc, int32_t* __restrict__ out_n, unsigned* err) {
  extern __shared__ int cand_lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t b = (int64_t)blockIdx.x * 4 + wave;
  if (b >= B) return;  // no block-level barriers below
  const int np = 1 << bits;
  int* const s = cand_lds + wave * np;
  const int n = G * kc;
  const int64_t row = b * bstride;
  for (int e = lane; e < np; e += 64) {
    int key = CAND_EMPTY;
    if (e < n) {
      const int g = e / kc, j = e - g * kc;
      const int64_t at = (int64_t)g * gstride + row + j;
      const int64_t it = list_idx[at];
      // empty: idx < 0, or a value given and not finite (hnm_fuse_topk_f32's rule)
      const bool live = it >= 0 && (!list_val || fabsf(list_val[at]) <= 3.402823466e+38f);
      if (live) {
        if (it >= I) hnm_flag(err, HNM_ERR_OOB);
        else key = (int)it;
      }
    }
    s[e] = key;
  }
  cand_wave_sync();
  // bitonic sort, ascending: step (k, j) pairs position i (bit j clear) with i | j
  for (int k = 2; k <= np; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = lane; t < (np >> 1); t += 64) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        const int a = s[i], c = s[i | j];
        const bool up = (i & k) == 0;  // this block ends ascending
        if ((a > c) == up) {
          s[i] = c;
          s[i | j] = a;
        }
      }
      cand_wave_sync();
    }
  }
  // compact: an id is kept where it differs from its left neighbour
  int32_t* const out = out_cand + b * ldc;
  int no = 0;
  for (int c0 = 0; c0 < np; c0 += 64) {
    const int e = c0 + lane;
    const int v = s[e];
    const int prev = e > 0 ? s[e - 1] : -1;
    const bool keep = v != CAND_EMPTY && v != prev;
    const uint64_t m = __ballot(keep);
    if (keep) out[no + __popcll(m & ((1ull << lane) - 1))] = v;  // no < n <= ldc
    no += __popcll(m);
  }
  for (int64_t e = no + lane; e < ldc; e += 64) out[e] = -1;
  if (lane == 0) out_n[b] = no;
}

template <int NS>
__global__ __launch_bounds__(256) void cand_topk_kernel(const float* __restrict__ scores,
                                                        const int32_t* __restrict__ cand,
                                                        int64_t ldc,
                                                        const int32_t* __restrict__ cand_n,
                                                        int64_t B, int k,
                                                        float* __restrict__ out_val,
                                                        int64_t* __restrict__ out_idx) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const int64_t n = std::min<int64_t>(std::max<int64_t>(cand_n[b], 0), ldc);
  WaveTopK<NS> top;
  top.init();
  for (int64_t c0 = 0; c0 < n; c0 += 64) {
    const int64_t e = c0 + lane;
    const bool in = e < n;
    const float v = in ? scores[b * ldc + e] : 0.f;
    const int it = in ? cand[b * ldc + e] : -1;
    // NaN fails the compare; +inf stays
    top.offer(v, it, in && it >= 0 && v > -__builtin_inff(), k);
  }
  top.store(out_val + b * k, out_idx + b * k, k);
}

}  // namespace

extern "C" hnm_status hnm_cand_union_i32(hnm_ctx* ctx, const float* list_val,
                                         const int64_t* list_idx, int64_t B, int64_t G,
                                         int64_t gstride, int64_t bstride, int kc,
                                         int64_t num_items, int32_t* out_cand, int64_t ldc,
                                         int32_t* out_n) {
  HNM_CTX_DEVICE(ctx);
  HNM_REQUIRE(ctx, HNM_EINVAL, "cand_union: ctx is NULL");
  HNM_REQUIRE(B >= 0 && num_items >= 0, HNM_EINVAL, "cand_union: bad size");
  HNM_REQUIRE(G >= 1 && G <= CAND_MAX_G && kc >= 1 && kc <= CAND_MAX_KC &&
                  G * kc <= CAND_MAX_ENTRIES,
              HNM_EUNSUPPORTED, "cand_union: 1 <= G <= %d, 1 <= kc <= %d, G * kc <= %d",
              CAND_MAX_G, CAND_MAX_KC, CAND_MAX_ENTRIES);
  HNM_REQUIRE(B <= INT32_MAX && num_items < INT_BIG, HNM_EUNSUPPORTED,
              "cand_union: B or num_items exceeds 2^31 - 1");
  HNM_REQUIRE(ldc >= G * kc, HNM_EINVAL, "cand_union: ldc %lld < G * kc = %lld", (long long)ldc,
              (long long)(G * kc));
  if (B == 0) return HNM_OK;
  HNM_REQUIRE(list_idx && out_cand && out_n, HNM_EINVAL, "cand_union: NULL list or output");
  int bits = 6;  // the compaction walks the segment 64 entries a step
  while ((1 << bits) < G * kc) ++bits;
  const size_t lds = (size_t)4 * (1 << bits) * sizeof(int);
  hipLaunchKernelGGL(cand_union_kernel, dim3((unsigned)hnm_cdiv(B, 4)), dim3(256), lds,
                     ctx->stream, list_val, list_idx, B, (int)G, gstride, bstride, kc, num_items,
                     bits, out_cand, ldc, out_n, ctx->err_dev);
  HNM_LAUNCH_CHECK();
  return HNM_OK;
}

extern "C" hnm_status hnm_cand_topk_f32(hnm_ctx* ctx, const float* scores, const int32_t* cand,
                                        int64_t ldc, const int32_t* cand_n, int64_t B, int k,
                                        float* out_val, int64_t* out_idx) {
  HNM_CTX_DEVICE(ctx);
  HNM_REQUIRE(ctx, HNM_EINVAL, "cand_topk: ctx is NULL");
  HNM_REQUIRE(B >= 0 && ldc >= 0, HNM_EINVAL, "cand_topk: bad size");
  HNM_REQUIRE(k >= 1 && k <= CAND_MAX_K, HNM_EUNSUPPORTED, "cand_topk: 1 <= k <= %d",
              CAND_MAX_K);
  HNM_REQUIRE(B <= INT32_MAX, HNM_EUNSUPPORTED, "cand_topk: B exceeds 2^31 - 1");
  if (B == 0) return HNM_OK;
  HNM_REQUIRE(cand_n && out_val && out_idx && ((scores && cand) || ldc == 0), HNM_EINVAL,
              "cand_topk: NULL input or output");
  const dim3 grid((unsigned)hnm_cdiv(B, 4));
  if (k <= 64)
    hipLaunchKernelGGL(cand_topk_kernel<1>, grid, dim3(256), 0, ctx->stream, scores, cand, ldc,
                       cand_n, B, k, out_val, out_idx);
  else
    hipLaunchKernelGGL(cand_topk_kernel<2>, grid, dim3(256), 0, ctx->stream, scores, cand, ldc,
                       cand_n, B, k, out_val, out_idx);
  HNM_LAUNCH_CHECK();
  return HNM_OK;
}
