// Wide&Deep over candidate lists (two-stage serving, stage 2): every user's listed items scored
// with wd_tile_fp32 -- the exact kernel's arithmetic on the same per-call tables (wd_setup), so a
// score is bitwise the dense entry's -- and selected in the same launch.  The contract is stated
// in include/hnm.h.
//
// Shape: wdc_rescore_kernel's (widedeep_rescore.hip), which does the same work on the certified
// cascade's survivor lists: a wave is one user, four waves a workgroup at (256, 1), the user's
// layer-1 row and the folded biases read from global memory (L2 hits after the first tile), the
// candidates' Qi rows gathered straight from global memory by lane (j, h).  The list is walked
// in tiles of 32; a lane past the list's end, or on a skipped candidate, reads item 0's row and
// stays out of the outputs.
#include <algorithm>

#include "widedeep_internal.h"

namespace {

constexpr int WDK_MAX_K = 64;      // WaveTopK<1>
constexpr int WDK_MAX_LDC = 2048;  // hnm_cand_union_i32's widest row

struct WdCandArgs {
  const float* Pu;
  const float* Qi;
  int K1P;
  const float4* W2f;
  const float4* W3f;
  const float* b2p;
  const float* b3p;
  const float* wdp;
  const float* cu;
  const float* wI;
  int64_t B, I;
  const int32_t* cand;  // [B, ldc]
  int64_t ldc;
  const int32_t* cand_n;  // [B]
  int K;                  // 0: scores only
  float* ov;              // [B, K]
  int64_t* oi;
  float* os;  // [B, ldc] or nullptr
  unsigned* err;
};

template <int RB2, int OB>
__global__ __launch_bounds__(256, 1) void widedeep_cand_kernel(WdCandArgs R) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, j = lane & 31;
  const int64_t b = (int64_t)blockIdx.x * 4 + wave;
  if (b >= R.B) return;  // no block-level barriers below
  const int K = R.K;
  const int n = (int)std::min<int64_t>(std::max<int64_t>(R.cand_n[b], 0), R.ldc);
  const int KS1 = R.K1P / 2, S4 = R.K1P / 8;
  const float cub = R.cu[b];
  const float* prow = R.Pu + b * R.K1P + h * KS1;
  const int32_t* crow = R.cand + b * R.ldc;
  float* const srow = R.os ? R.os + b * R.ldc : nullptr;
  WaveTopK<1> T;
  T.init();
  for (int t0 = 0; t0 < n; t0 += TILE) {
    const int nv = std::min(TILE, n - t0);
    const bool in = j < nv;
    const int c = crow[t0 + (in ? j : 0)];
    if (in && h == 0 && c >= R.I) hnm_flag(R.err, HNM_ERR_OOB);
    const bool ok = in && c >= 0 && c < R.I;
    const int it = ok ? c : 0;  // a valid row for every lane
    const float* qrow = R.Qi + (int64_t)it * R.K1P + h * KS1;
    float fin = wd_tile_fp32<RB2, OB>(prow, qrow, S4, R.W2f, R.W3f, R.b2p, R.b3p, R.wdp, lane, h);
    fin += __shfl_xor(fin, 32);
    const bool ivalid = lane < 32 && ok;
    const float score = fin + cub + (ivalid ? R.wI[it] : 0.f);
    if (srow && lane < 32 && in) srow[t0 + j] = ok ? score : -__builtin_inff();
    // NaN and -inf stay out, as in hnm_cand_topk_f32
    if (K > 0) T.offer(score, it, ivalid && score > -__builtin_inff(), K);
  }
  if (srow)
    for (int64_t e = n + lane; e < R.ldc; e += 64) srow[e] = -__builtin_inff();
  if (K > 0) T.store(R.ov + b * K, R.oi + b * K, K);
}

}  // namespace

extern "C" hnm_status hnm_widedeep_cand_topk_ex_f32(
    hnm_ctx* ctx, const hnm_widedeep_weights* w, const int64_t* user_ids, int64_t B,
    const float* user_features, const int32_t* cand, int64_t ldc, const int32_t* cand_n, int k,
    float* out_val, int64_t* out_idx, float* out_scores, const hnm_widedeep_item_features* itf,
    const float* item_features, int64_t ldf) {
  HNM_CTX_DEVICE(ctx);
  WdItemFeat F;
  F.itf = itf;
  F.f = item_features;
  F.ldf = ldf;
  HNM_REQUIRE(ctx && (user_ids || B == 0), HNM_EINVAL, "widedeep_cand: NULL argument");
  HNM_REQUIRE(k >= 0 && k <= WDK_MAX_K && ldc >= 0 && ldc <= WDK_MAX_LDC, HNM_EUNSUPPORTED,
              "widedeep_cand: 0 <= k <= %d (0: scores only), ldc <= %d", WDK_MAX_K, WDK_MAX_LDC);
  HNM_REQUIRE(k > 0 || out_scores || B == 0, HNM_EINVAL,
              "widedeep_cand: k = 0 needs out_scores");
  HNM_REQUIRE(k == 0 || (out_val && out_idx) || B == 0, HNM_EINVAL,
              "widedeep_cand: NULL output");
  WdSetup S;
  hnm_status st = wd_shape(w, &S.pr, F);
  if (st) return st;
  if (B <= 0) return HNM_OK;
  HNM_REQUIRE(B <= INT32_MAX, HNM_EUNSUPPORTED, "widedeep_cand: B exceeds 2^31 - 1");
  HNM_REQUIRE(cand_n && (cand || ldc == 0), HNM_EINVAL, "widedeep_cand: NULL candidate list");
  st = wd_setup(ctx, w, user_ids, B, user_features, 0, &S, F);
  if (st) return st;
  const WdPrep& pr = S.pr;
  WdCandArgs r{};
  r.Pu = S.Pu;
  r.Qi = S.Qi;
  r.K1P = S.K1P;
  r.W2f = pr.W2f;
  r.W3f = pr.W3f;
  r.b2p = pr.b2p;
  r.b3p = pr.b3p;
  r.wdp = pr.wdp;
  r.cu = S.cu;
  r.wI = S.wI;
  r.B = B;
  r.I = w->num_items;
  r.cand = cand;
  r.ldc = ldc;
  r.cand_n = cand_n;
  r.K = k;
  r.ov = out_val;
  r.oi = out_idx;
  r.os = out_scores;
  r.err = ctx->err_dev;
  const dim3 grid((unsigned)hnm_cdiv(B, 4));
  hnm_timer_begin(ctx, HNM_TIME_SCORE);
  const bool found = wd_dispatch<false>(pr.RB2, pr.OB, [&](auto R, auto O) {
    hipLaunchKernelGGL((widedeep_cand_kernel<R(), O()>), grid, dim3(256), 0, ctx->stream, r);
  });
  hnm_timer_end(ctx, HNM_TIME_SCORE);
  if (!found) return wd_not_instantiated(pr);
  HNM_LAUNCH_CHECK();
  return HNM_OK;
}
