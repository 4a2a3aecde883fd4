// Wide&Deep all-items scoring for gfx950 (wide_deep.py:157-285, recommend :405-435).
//
// Reference per pair: deep = BN3(relu(L3(BN2(relu(L2(BN1(relu(L1([e_u; e_i]))))))))),
// score = final_layer([onehot(u); onehot(i); deep]) = w[u] + w[U + i] + w_d . deep + b.
// The one-hot wide part (a 2.7 GB scatter per user per chunk in the reference) is two
// weight lookups; eval-mode BatchNorm is an affine map folded into the next layer:
//   L2(BN1(x)) = (W2 diag a1) x + (W2 c1 + b2),  a = g / sqrt(var + eps), c = beta - mean a
// and BN3 into w_d.  Layer 1 is decomposed (P_u + Q_i, computed once per call).
//
// Per (user, 32-item tile) a wave runs, with v_mfma_f32_32x32x2_f32 (exact fp32):
//   layer 2: D2 = W2' . relu(P_u + Q_i)^T   (rows = layer-2 units, cols = items); the A
//            fragments are pre-permuted in HBM so each lane streams them with 16-B loads
//            (weights are L2-resident: 640 KB)
//   layer 3: D3 = W3' . relu(D2 + b2')^T   -- D2's accumulator registers ARE the B
//            operand: k-step (rb, r) pairs row (r&3)+8(r>>2) of half 0 with +4 of half 1,
//            and W3' is pre-permuted to the same k order, so no LDS round trip.
//   final:   relu(D3 + b3') . w_d' (16-register epilogue + one cross-half shuffle)
// Item features (the _ex entries) are per item: their layer-1 part is added to Q_i and their wide
// cross to the per-item wide term before any of this runs (widedeep_features.hip).
// Layer-2 row blocks are processed 4 at a time (64 accumulator registers) and fed into
// the layer-3 accumulators (64 registers) as they complete.
// (The certified split-f16 scan: widedeep_cert.hip; its re-scoring cascade: widedeep_rescore.hip.)
#include <algorithm>

#include "widedeep_internal.h"

// ------------------------------------------------------------------ weight preparation
// W2f[rb][s4][lane].e = W2[o][k] * a1[k], o = rb*32 + (lane&31), k = 2(4 s4 + e) + (lane>>5)
__global__ void wd_prep_w2(hnm_widedeep_weights w, WdPrep p) {
  const int64_t n = (int64_t)p.RB2 * (p.K1P / 8) * 64 * 4;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n; t += (int64_t)gridDim.x * 256) {
    const int e = t & 3, lane = (t >> 2) & 63;
    const int64_t rest = t >> 8;
    const int s4 = (int)(rest % (p.K1P / 8)), rb = (int)(rest / (p.K1P / 8));
    const int o = rb * 32 + (lane & 31), k = 2 * (4 * s4 + e) + (lane >> 5);
    float v = 0.f;
    if (o < w.l2 && k < w.l1) v = w.w2[(int64_t)o * w.l1 + k] * bn_a(w.bn1_w, w.bn1_var, k, w.eps);
    reinterpret_cast<float*>(p.W2f)[t] = v;
  }
}

// W3f[ob][rb][r4][lane].e = W3[o][i] * a2[i], o = ob*32 + (lane&31),
// i = rb*32 + row(4 r4 + e, lane>>5)
__global__ void wd_prep_w3(hnm_widedeep_weights w, WdPrep p) {
  const int64_t n = (int64_t)p.OB * p.RB2 * 4 * 64 * 4;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n; t += (int64_t)gridDim.x * 256) {
    const int e = t & 3, lane = (t >> 2) & 63;
    int64_t rest = t >> 8;
    const int r4 = (int)(rest & 3);
    rest >>= 2;
    const int rb = (int)(rest % p.RB2), ob = (int)(rest / p.RB2);
    const int o = ob * 32 + (lane & 31);
    const int i = rb * 32 + mfma32_row(4 * r4 + e, lane >> 5);
    float v = 0.f;
    if (o < w.l3 && i < w.l2) v = w.w3[(int64_t)o * w.l2 + i] * bn_a(w.bn2_w, w.bn2_var, i, w.eps);
    reinterpret_cast<float*>(p.W3f)[t] = v;
  }
}

// b2' = b2 + W2 c1 [RB2*32], b3' = b3 + W3 c2 [OB*32], w_d' = w_d * a_last and the folded
// bias (zero padded); one thread per output.
__global__ void wd_prep_bias(hnm_widedeep_weights w, WdPrep p) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int last = p.OB > 0 ? w.l3 : w.l2;  // width of the last hidden layer
  const float* lg = p.OB > 0 ? w.bn3_w : w.bn2_w;
  const float* lb = p.OB > 0 ? w.bn3_b : w.bn2_b;
  const float* lm = p.OB > 0 ? w.bn3_mean : w.bn2_mean;
  const float* lv = p.OB > 0 ? w.bn3_var : w.bn2_var;
  const float* wd = w.final_deep;
  for (int o = t; o < p.RB2 * 32; o += gridDim.x * 256) {
    float v = 0.f;
    if (o < w.l2) {
      float s = 0.f;
      for (int i = 0; i < w.l1; ++i)
        s = fmaf(w.w2[(int64_t)o * w.l1 + i],
                 bn_c(w.bn1_w, w.bn1_b, w.bn1_mean, w.bn1_var, i, w.eps), s);
      v = w.b2[o] + s;
    }
    p.b2p[o] = v;
  }
  for (int o = t; o < p.OB * 32; o += gridDim.x * 256) {
    float v = 0.f;
    if (o < w.l3) {
      float s = 0.f;
      for (int i = 0; i < w.l2; ++i)
        s = fmaf(w.w3[(int64_t)o * w.l2 + i],
                 bn_c(w.bn2_w, w.bn2_b, w.bn2_mean, w.bn2_var, i, w.eps), s);
      v = w.b3[o] + s;
    }
    p.b3p[o] = v;
  }
  const int nlast = (p.OB > 0 ? p.OB : p.RB2) * 32;
  for (int o = t; o < nlast; o += gridDim.x * 256)
    p.wdp[o] = o < last ? wd[o] * bn_a(lg, lv, o, w.eps) : 0.f;
  if (t == 0) {
    float s = w.final_b[0];
    for (int o = 0; o < last; ++o) s = fmaf(wd[o], bn_c(lg, lb, lm, lv, o, w.eps), s);
    p.bias[0] = s;
  }
}

// per-user constant: folded bias + wide user weight (+ wide user-feature term)
__global__ void wd_user_const(hnm_widedeep_weights w, const int64_t* __restrict__ ids, int64_t B,
                              const float* __restrict__ wuf, const float* __restrict__ bias,
                              float* __restrict__ cu) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const int64_t u = ids[b];
  float v = bias[0];
  if (u >= 0 && u < w.num_users) v += w.wide_user[u];
  if (wuf) {
    const float* wf = w.wide_feat;
    for (int f = 0; f < w.num_user_features; ++f) v = fmaf(wuf[b * w.num_user_features + f], wf[f], v);
  }
  cu[b] = v;
}

// ------------------------------------------------------------------ main kernel
template <int RB2, int OB, bool DENSE>
__global__ __launch_bounds__(256, (RB2 >= 8 || OB >= 4) ? 1 : 2) void widedeep_score_kernel(
    const float* __restrict__ Pu, const float* __restrict__ Qi, int K1P,
    const float4* __restrict__ W2f, const float4* __restrict__ W3f,
    const float* __restrict__ b2p, const float* __restrict__ b3p,
    const float* __restrict__ wdp, const float* __restrict__ cu, const float* __restrict__ wI,
    int64_t B, int64_t I, int64_t ipp, const int64_t* __restrict__ mptr,
    const int32_t* __restrict__ midx, int K, float* __restrict__ cand_v,
    int32_t* __restrict__ cand_i, int NP, float* __restrict__ dense, int64_t ldo,
    const int32_t* __restrict__ rows) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int KS1 = K1P / 2, S4 = K1P / 8, QRS = K1P + 4;
  float* qs = smem;                    // [32][QRS]
  float* ps = smem + TILE * QRS;       // [4][K1P]
  float* cb2 = ps + 4 * K1P;           // [RB2*32] b2'
  float* cb3 = cb2 + RB2 * 32;         // [OB*32]  b3'
  float* cwd = cb3 + OB * 32;          // [32*max(OB,RB2)] w_d'

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, j = lane & 31;
  // rows (the certified path's fallback): slot -> batch row; outputs stay at the slot
  const int64_t slot = (int64_t)blockIdx.x * 4 + wave;
  const int64_t b = rows ? (slot < B ? (int64_t)rows[slot] : 0) : slot;
  const int p = blockIdx.y;
  const int64_t part_start = (int64_t)p * ipp;
  const int64_t part_end = std::min<int64_t>(I, part_start + ipp);

  for (int e = tid; e < 4 * K1P / 4; e += 256) {
    const int r = e / (K1P / 4), c = e % (K1P / 4);
    const int64_t bb = (int64_t)blockIdx.x * 4 + r;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (bb < B) v = *reinterpret_cast<const float4*>(Pu + (rows ? (int64_t)rows[bb] : bb) * K1P + 4 * c);
    *reinterpret_cast<float4*>(&ps[r * K1P + 4 * c]) = v;
  }
  for (int e = tid; e < RB2 * 32; e += 256) cb2[e] = b2p[e];
  for (int e = tid; e < OB * 32; e += 256) cb3[e] = b3p[e];
  for (int e = tid; e < (OB > 0 ? OB : RB2) * 32; e += 256) cwd[e] = wdp[e];
  const bool active = slot < B;
  const float cub = active ? cu[b] : 0.f;
  WaveTopK<1> L;
  L.init();
  int nm = INT_BIG, mpos = 0, mend = 0;
  if (!DENSE && mptr && active) {
    int64_t lo = mptr[b], hi = mptr[b + 1];
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (midx[mid] < part_start) lo = mid + 1;
      else hi = mid;
    }
    mpos = (int)lo;
    mend = (int)mptr[b + 1];
    nm = mpos < mend ? midx[mpos] : INT_BIG;
  }

  const int64_t ntiles = part_end > part_start ? hnm_cdiv(part_end - part_start, TILE) : 0;
  for (int64_t t = 0; t < ntiles; ++t) {
    const int64_t base = part_start + t * TILE;
    __syncthreads();  // previous tile's reads of qs are done
    for (int e = tid; e < TILE * K1P / 4; e += 256) {
      const int r = e / (K1P / 4), c = e % (K1P / 4);
      const int64_t item = base + r;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (item < part_end) v = *reinterpret_cast<const float4*>(Qi + item * K1P + 4 * c);
      *reinterpret_cast<float4*>(&qs[r * QRS + 4 * c]) = v;
    }
    __syncthreads();
    if (!active) continue;

    const float* prow = &ps[wave * K1P + h * KS1];
    const float* qrow = &qs[j * QRS + h * KS1];
    float fin = wd_tile_fp32<RB2, OB>(prow, qrow, S4, W2f, W3f, cb2, cb3, cwd, lane, h);
    fin += __shfl_xor(fin, 32);
    const int64_t item = base + j;
    const bool ivalid = lane < 32 && item < part_end;
    float score = fin + cub + (ivalid ? wI[item] : 0.f);
    if (DENSE) {
      if (ivalid) dense[b * ldo + item] = score;
    } else {
      const int64_t tile_end = std::min<int64_t>(base + TILE, part_end);
      while (nm < tile_end) {
        if (item == nm) score = -__builtin_inff();
        ++mpos;
        nm = mpos < mend ? midx[mpos] : INT_BIG;
      }
      L.offer(score, (int)item, ivalid, K);
    }
  }
  if (!DENSE && active) L.store(cand_v + (slot * NP + p) * K, cand_i + (slot * NP + p) * K, K);
}

// ------------------------------------------------------------------ pairwise forward
// WideDeep.forward(user_ids, item_ids[, features]) (wide_deep.py:157-230): one workgroup per
// pair, the unfolded reference op order (Linear -> ReLU -> BatchNorm per layer).
__global__ __launch_bounds__(256) void widedeep_pair_kernel(
    hnm_widedeep_weights w, const int64_t* __restrict__ uids, const int64_t* __restrict__ iids,
    int64_t n, const float* __restrict__ xu, int ldxu, const float* __restrict__ wide_extra,
    const float* __restrict__ wide_extra2, float* __restrict__ out, unsigned* err) {
  __shared__ float x0[512], x1[512];
  __shared__ float red[256];
  const int64_t e = blockIdx.x;
  const int t = threadIdx.x;
  const int64_t u = uids[e], i = iids[e];
  if (u < 0 || u >= w.num_users || i < 0 || i >= w.num_items) {
    if (t == 0) {
      hnm_flag(err, HNM_ERR_OOB);
      out[e] = __builtin_nanf("");
    }
    return;
  }
  const int din = w.l1_in;
  for (int c = t; c < din; c += 256) {
    float v;
    if (c < w.d) v = w.deep_user[u * w.d + c];
    else if (c < 2 * w.d) v = w.deep_item[i * w.d + c - w.d];
    else v = xu[e * ldxu + c - 2 * w.d];  // [deep user-feature | deep item-feature] chunks
    x0[c] = v;
  }
  __syncthreads();
  const int widths[3] = {w.l1, w.l2, w.l3};
  const float* W[3] = {w.w1, w.w2, w.w3};
  const float* Bs[3] = {w.b1, w.b2, w.b3};
  const float* G[3] = {w.bn1_w, w.bn2_w, w.bn3_w};
  const float* Be[3] = {w.bn1_b, w.bn2_b, w.bn3_b};
  const float* M[3] = {w.bn1_mean, w.bn2_mean, w.bn3_mean};
  const float* V[3] = {w.bn1_var, w.bn2_var, w.bn3_var};
  const int depth = w.l3 > 0 ? 3 : 2;
  float* cur = x0;
  float* nxt = x1;
  int in = din;
  for (int l = 0; l < depth; ++l) {
    for (int o = t; o < widths[l]; o += 256) {
      float s = 0.f;
      for (int k = 0; k < in; ++k) s = fmaf(W[l][(int64_t)o * in + k], cur[k], s);
      s = fmaxf(s + Bs[l][o], 0.f);
      s = (s - M[l][o]) / sqrtf(V[l][o] + w.eps) * G[l][o] + Be[l][o];
      nxt[o] = s;
    }
    __syncthreads();
    float* tmp = cur;
    cur = nxt;
    nxt = tmp;
    in = widths[l];
    __syncthreads();
  }
  const float* wd = w.final_deep;
  float s = 0.f;
  for (int o = t; o < in; o += 256) s = fmaf(wd[o], cur[o], s);
  red[t] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) red[t] += red[t + o];
    __syncthreads();
  }
  if (t == 0) {
    // wide part in the reference's concat order: user one-hot, item one-hot (both absent
    // when use_wide_user_item=False), user-feature cross, item-feature cross
    float v = red[0];
    if (w.wide_user) v += w.wide_user[u];
    if (w.wide_item) v += w.wide_item[i];
    v += w.final_b[0];
    if (wide_extra) v += wide_extra[e];
    if (wide_extra2) v += wide_extra2[e];
    out[e] = v;
  }
}

// ------------------------------------------------------------------ host side
static hnm_status wd_check(const hnm_widedeep_weights* w, const WdItemFeat& F) {
  HNM_REQUIRE(w && w->deep_user && w->deep_item && w->w1 && w->b1 && w->w2 && w->b2 &&
                  w->wide_user && w->wide_item && w->final_deep && w->final_b && w->bn1_w &&
                  w->bn2_w,
              HNM_EINVAL, "widedeep: NULL weight pointer");
  HNM_REQUIRE(w->num_users > 0 && w->num_items > 0 && w->num_items < INT_BIG, HNM_EINVAL,
              "widedeep: bad table sizes");
  HNM_REQUIRE(w->d >= 1 && w->l1 >= 1 && w->l1 <= 512 && w->l2 >= 1 && w->l2 <= 256 &&
                  w->l3 >= 0 && w->l3 <= 128 && (w->l3 == 0 || w->w3),
              HNM_EUNSUPPORTED,
              "widedeep: the fused kernel covers 2- or 3-layer towers with widths <= "
              "512/256/128 (got %d/%d/%d)", w->l1, w->l2, w->l3);
  if (F.on()) {
    const hnm_widedeep_item_features* itf = F.itf;
    HNM_REQUIRE(w->l1_in == (2 + (w->num_user_features > 0 ? 1 : 0) + 1) * w->d, HNM_EUNSUPPORTED,
                "widedeep: deep input must be [e_u; e_i(; user features); item features] "
                "(layer-1 input %d, embedding_dim %d)", w->l1_in, w->d);
    HNM_REQUIRE(F.f && itf->dif_w && itf->dif_b, HNM_EINVAL,
                "widedeep: item_features required (num_item_features > 0)");
    HNM_REQUIRE(F.ldf >= itf->num_item_features, HNM_EINVAL,
                "widedeep: item_features leading dimension %lld < %d", (long long)F.ldf,
                itf->num_item_features);
    HNM_REQUIRE(w->d <= WDF_MAX_D && itf->num_item_features <= WDF_MAX_F, HNM_EUNSUPPORTED,
                "widedeep: the item-feature fold covers embedding_dim <= %d and <= %d item "
                "features (got %d, %d)", WDF_MAX_D, WDF_MAX_F, w->d, itf->num_item_features);
    return HNM_OK;
  }
  HNM_REQUIRE(w->l1_in == 2 * w->d + (w->num_user_features > 0 ? w->d : 0), HNM_EUNSUPPORTED,
              "widedeep: deep input must be [e_u; e_i(; user features)] (item features are "
              "not available to predict_all_items, wide_deep.py:275)");
  return HNM_OK;
}

static int pow2_blocks(int width) {
  const int nb = (width + 31) / 32;
  int p = 1;
  while (p < nb) p <<= 1;
  return p;
}

hnm_status wd_shape(const hnm_widedeep_weights* w, WdPrep* pr, const WdItemFeat& F) {
  hnm_status st = wd_check(w, F);
  if (st) return st;
  pr->K1P = (w->l1 + 7) / 8 * 8;
  pr->RB2 = pow2_blocks(w->l2);
  pr->OB = w->l3 > 0 ? pow2_blocks(w->l3) : 0;
  if (!wd_dispatch<false>(pr->RB2, pr->OB, [](auto, auto) {})) {
    hnm_set_error("widedeep: layer widths %d/%d not instantiated", w->l2, w->l3);
    return HNM_EUNSUPPORTED;
  }
  return HNM_OK;
}

void wd_partition(const hnm_ctx* ctx, int64_t B, int64_t I, int64_t* np, int64_t* ipp, int upb) {
  const int64_t ublocks = hnm_cdiv(B, upb);
  const int64_t want = std::max<int64_t>(1, hnm_cdiv(2 * (int64_t)ctx->num_cus, ublocks));
  int64_t n = std::min<int64_t>(want, std::max<int64_t>(1, hnm_cdiv(I, 4 * TILE)));
  *ipp = hnm_cdiv(hnm_cdiv(I, n), TILE) * TILE;
  *np = hnm_cdiv(I, *ipp);
}

// candidate-list scratch (values + int32 items) of the exact list pass over n rows
static size_t wd_list_bytes(const hnm_ctx* ctx, int64_t n, int64_t I, int K) {
  int64_t np, ipp;
  wd_partition(ctx, n, I, &np, &ipp);
  return 2 * hnm_align((size_t)n * np * K * 4);
}

hnm_status wd_setup(hnm_ctx* ctx, const hnm_widedeep_weights* w, const int64_t* ids, int64_t B,
                    const float* ufeat, size_t extra, WdSetup* S, const WdItemFeat& F) {
  const int64_t I = w->num_items;
  WdPrep& pr = S->pr;
  const int K1P = pr.K1P;
  S->K1P = K1P;
  const int nlast = pr.OB > 0 ? pr.OB : pr.RB2;
  const size_t szW2 = hnm_align((size_t)pr.RB2 * (K1P / 8) * 64 * 16);
  const size_t szW3 = hnm_align((size_t)std::max(pr.OB, 1) * pr.RB2 * 4 * 64 * 16);
  const size_t szb2 = hnm_align((size_t)pr.RB2 * 32 * 4);
  const size_t szb3 = hnm_align((size_t)std::max(pr.OB, 1) * 32 * 4);
  const size_t szwd = hnm_align((size_t)nlast * 32 * 4);
  const size_t szP = hnm_align((size_t)B * K1P * 4), szQ = hnm_align((size_t)I * K1P * 4);
  const size_t szX = w->num_user_features > 0 ? hnm_align((size_t)B * w->d * 4) : 0;
  const size_t szF = ufeat ? hnm_align((size_t)B * w->num_user_features * 4) : 0;
  const size_t szU = hnm_align((size_t)B * 4);
  const size_t szT = w->num_user_features > 0 ? hnm_align((size_t)B * K1P * 4) : 0;
  // the folded wide item term (item features with a wide cross); else w->wide_item as it is
  const bool fold_wide = F.on() && F.itf->wif_w && F.itf->wide_feat;
  const size_t szI = fold_wide ? hnm_align((size_t)I * 4) : 0;
  void* wsp;
  hnm_status st = hnm_workspace(ctx, szW2 + szW3 + szb2 + szb3 + szwd + 256 + szP + szQ + szX +
                                         szF + szU + szT + szI + hnm_align(extra), &wsp);
  if (st) return st;
  char* q = (char*)wsp;
  pr.W2f = (float4*)q; q += szW2;
  pr.W3f = (float4*)q; q += szW3;
  pr.b2p = (float*)q; q += szb2;
  pr.b3p = (float*)q; q += szb3;
  pr.wdp = (float*)q; q += szwd;
  pr.bias = (float*)q; q += 256;
  float* Pu = (float*)q; q += szP;
  float* Qi = (float*)q; q += szQ;
  float* Xf = (float*)q; q += szX;
  float* WFu = (float*)q; q += szF;
  float* cu = (float*)q; q += szU;
  float* Tf = (float*)q; q += szT;
  float* wIf = (float*)q; q += szI;
  S->wI = fold_wide ? wIf : w->wide_item;
  S->Pu = Pu;
  S->Qi = Qi;
  S->cu = cu;
  S->extra = q;

  hipStream_t s = ctx->stream;
  hipLaunchKernelGGL(wd_prep_w2, dim3(256), dim3(256), 0, s, *w, pr);
  if (pr.OB > 0) hipLaunchKernelGGL(wd_prep_w3, dim3(128), dim3(256), 0, s, *w, pr);
  hipLaunchKernelGGL(wd_prep_bias, dim3(64), dim3(256), 0, s, *w, pr);
  HNM_LAUNCH_CHECK();
  // layer-1 decomposition: P_u = W1[:, :d] e_u + b1 (+ W1[:, 2d:3d] (Wf f_u + bf)),
  // Q_i = W1[:, d:2d] e_i, both pair-permuted with row stride K1P
  if (K1P != w->l1) {
    HNM_HIP_CHECK(hipMemsetAsync(Pu, 0, szP, s));
    HNM_HIP_CHECK(hipMemsetAsync(Qi, 0, szQ, s));
  }
  st = hnm_linear_rows_f32(ctx, w->deep_user, w->d, ids, w->num_users, B, w->d, w->w1, w->l1_in,
                           w->b1, w->l1, Pu, K1P, 1);
  if (st) return st;
  st = hnm_linear_rows_f32(ctx, w->deep_item, w->d, nullptr, I, I, w->d, w->w1 + w->d, w->l1_in,
                           nullptr, w->l1, Qi, K1P, 1);
  if (st) return st;
  if (F.on()) {
    st = wd_fold_item_features(ctx, w, F, K1P, Qi, fold_wide ? wIf : nullptr);
    if (st) return st;
  }
  const float* wuf = nullptr;
  if (w->num_user_features > 0) {
    HNM_REQUIRE(ufeat && w->duf_w && w->duf_b, HNM_EINVAL,
                "widedeep: user_features required (num_user_features > 0)");
    // deep user features -> Xf [B, d] (deep_user_features Linear(F, d), wide_deep.py:113)
    st = hnm_linear_rows_f32(ctx, ufeat, w->num_user_features, nullptr, B, B,
                             w->num_user_features, w->duf_w, w->num_user_features, w->duf_b,
                             w->d, Xf, w->d, 0);
    if (st) return st;
    // wide user features Linear(F, F)
    if (w->wuf_w && w->wide_feat) {
      st = hnm_linear_rows_f32(ctx, ufeat, w->num_user_features, nullptr, B, B,
                               w->num_user_features, w->wuf_w, w->num_user_features, w->wuf_b,
                               w->num_user_features, WFu, w->num_user_features, 0);
      if (st) return st;
      wuf = WFu;
    }
  }
  hipLaunchKernelGGL(wd_user_const, dim3((unsigned)hnm_cdiv(B, 256)), dim3(256), 0, s, *w, ids, B,
                     wuf, pr.bias, cu);
  HNM_LAUNCH_CHECK();
  if (w->num_user_features > 0) {
    // P_u += W1[:, 2d:3d] (deep user-feature projection), pair-permuted like P_u
    HNM_HIP_CHECK(hipMemsetAsync(Tf, 0, szT, s));
    st = hnm_linear_rows_f32(ctx, Xf, w->d, nullptr, B, B, w->d, w->w1 + 2 * w->d, w->l1_in,
                             nullptr, w->l1, Tf, K1P, 1);
    if (st) return st;
    st = hnm_axpby_f32(ctx, (int64_t)B * K1P, 1.f, Pu, 1.f, Tf, Pu);
    if (st) return st;
  }
  return HNM_OK;
}

hnm_status wd_exact(hnm_ctx* ctx, const hnm_widedeep_weights* w, const WdSetup& S, int64_t n,
                    const int64_t* mptr, const int32_t* midx, int K, const int32_t* rows,
                    float* cv, int32_t* ci, float* ov, int64_t* oi, float* dense, int64_t ldo,
                    bool timed) {
  const WdPrep& pr = S.pr;
  const int64_t I = w->num_items;
  int64_t np, ipp;
  wd_partition(ctx, n, I, &np, &ipp);
  const int K1P = S.K1P;
  const int nlast = pr.OB > 0 ? pr.OB : pr.RB2;
  const size_t lds = (size_t)(TILE * (K1P + 4) + 4 * K1P + (pr.RB2 + pr.OB + nlast) * 32) * 4;
  dim3 grid((unsigned)hnm_cdiv(n, 4), (unsigned)np);
  if (timed) hnm_timer_begin(ctx, HNM_TIME_SCORE);
  auto launch = [&](auto kern) {
    hipLaunchKernelGGL(kern, grid, dim3(256), lds, ctx->stream, S.Pu, S.Qi, K1P, pr.W2f, pr.W3f,
                       pr.b2p, pr.b3p, pr.wdp, S.cu, S.wI, n, I, ipp, mptr, midx, K, cv, ci,
                       (int)np, dense, ldo, rows);
  };
  const bool found = wd_dispatch<false>(pr.RB2, pr.OB, [&](auto R, auto O) {
    if (dense) launch(widedeep_score_kernel<R(), O(), true>);
    else launch(widedeep_score_kernel<R(), O(), false>);
  });
  if (timed) hnm_timer_end(ctx, HNM_TIME_SCORE);
  if (!found) return wd_not_instantiated(pr);
  HNM_LAUNCH_CHECK();
  if (dense) return HNM_OK;
  return hnm_topk_merge_i32(ctx, cv, ci, n, 1, 0, np * K, (int)(np * K), K, ov, oi);
}

extern "C" hnm_status hnm_widedeep_topk_ex_f32(hnm_ctx* ctx, const hnm_widedeep_weights* w,
                                               const int64_t* user_ids, int64_t B,
                                               const float* user_features,
                                               const int64_t* mask_ptr, const int32_t* mask_idx,
                                               int k, float* out_val, int64_t* out_idx,
                                               const hnm_widedeep_item_features* itf,
                                               const float* item_features, int64_t ldf) {
  HNM_CTX_DEVICE(ctx);
  WdItemFeat F;
  F.itf = itf;
  F.f = item_features;
  F.ldf = ldf;
  HNM_REQUIRE(k >= 1 && k <= 64 && (out_idx || B == 0), HNM_EINVAL, "widedeep_topk: fused path needs 1 <= k <= 64");
  HNM_REQUIRE(ctx && (user_ids || B == 0), HNM_EINVAL, "widedeep: NULL argument");
  WdSetup S;
  hnm_status st = wd_shape(w, &S.pr, F);
  if (st) return st;
  if (B <= 0) return HNM_OK;
  const int64_t I = w->num_items;
  if (wdc_eligible(ctx, S.pr, I, k, false)) {
    const size_t extra = wdc_carve(ctx, S.pr, B, I, k, nullptr, nullptr);
    st = wd_setup(ctx, w, user_ids, B, user_features, extra, &S, F);
    if (st) return st;
    WdcWs c;
    wdc_carve(ctx, S.pr, B, I, k, S.extra, &c);
    return wdc_topk(ctx, w, S, B, mask_ptr, mask_idx, k, c, out_val, out_idx);
  }
  const size_t lb = wd_list_bytes(ctx, B, I, k);
  st = wd_setup(ctx, w, user_ids, B, user_features, lb, &S, F);
  if (st) return st;
  int64_t np, ipp;
  wd_partition(ctx, B, I, &np, &ipp);
  float* cv = (float*)S.extra;
  int32_t* ci = (int32_t*)(S.extra + hnm_align((size_t)B * np * k * 4));
  return wd_exact(ctx, w, S, B, mask_ptr, mask_idx, k, nullptr, cv, ci, out_val, out_idx,
                  nullptr, 0, true);
}

extern "C" hnm_status hnm_widedeep_topk_f32(hnm_ctx* ctx, const hnm_widedeep_weights* w,
                                            const int64_t* user_ids, int64_t B,
                                            const float* user_features, const int64_t* mask_ptr,
                                            const int32_t* mask_idx, int k, float* out_val,
                                            int64_t* out_idx) {
  return hnm_widedeep_topk_ex_f32(ctx, w, user_ids, B, user_features, mask_ptr, mask_idx, k,
                                  out_val, out_idx, nullptr, nullptr, 0);
}

extern "C" hnm_status hnm_widedeep_scores_ex_f32(hnm_ctx* ctx, const hnm_widedeep_weights* w,
                                                 const int64_t* user_ids, int64_t B,
                                                 const float* user_features, float* out,
                                                 int64_t ldo,
                                                 const hnm_widedeep_item_features* itf,
                                                 const float* item_features, int64_t ldf) {
  HNM_CTX_DEVICE(ctx);
  WdItemFeat F;
  F.itf = itf;
  F.f = item_features;
  F.ldf = ldf;
  HNM_REQUIRE((out || B == 0) && w && ldo >= w->num_items, HNM_EINVAL, "widedeep_scores: bad output");
  HNM_REQUIRE(ctx && (user_ids || B == 0), HNM_EINVAL, "widedeep: NULL argument");
  WdSetup S;
  hnm_status st = wd_shape(w, &S.pr, F);
  if (st) return st;
  if (B <= 0) return HNM_OK;
  st = wd_setup(ctx, w, user_ids, B, user_features, 0, &S, F);
  if (st) return st;
  return wd_exact(ctx, w, S, B, nullptr, nullptr, 1, nullptr, nullptr, nullptr, nullptr,
                  nullptr, out, ldo, true);
}

extern "C" hnm_status hnm_widedeep_scores_f32(hnm_ctx* ctx, const hnm_widedeep_weights* w,
                                              const int64_t* user_ids, int64_t B,
                                              const float* user_features, float* out,
                                              int64_t ldo) {
  return hnm_widedeep_scores_ex_f32(ctx, w, user_ids, B, user_features, out, ldo, nullptr,
                                    nullptr, 0);
}

extern "C" hnm_status hnm_widedeep_pair_scores_ex_f32(hnm_ctx* ctx, const hnm_widedeep_weights* w,
                                                      const hnm_widedeep_item_features* itf,
                                                      const int64_t* user_ids,
                                                      const int64_t* item_ids,
                                                      const float* user_features,
                                                      const float* item_features, int64_t n,
                                                      float* out) {
  HNM_CTX_DEVICE(ctx);
  HNM_REQUIRE(ctx && w && ((user_ids && item_ids && out) || n == 0), HNM_EINVAL, "widedeep_pair: NULL argument");
  HNM_REQUIRE(w->l1 <= 512 && w->l2 <= 512 && w->l3 <= 512 && w->l1_in <= 512, HNM_EUNSUPPORTED,
              "widedeep_pair: widths must be <= 512");
  const int Fu = w->num_user_features, Fi = itf ? itf->num_item_features : 0;
  const int nch = (Fu > 0) + (Fi > 0);  // deep feature chunks after [e_u; e_i]
  HNM_REQUIRE(w->l1_in == (2 + nch) * w->d, HNM_EINVAL,
              "widedeep_pair: layer-1 input %d != %d x embedding_dim (features given)", w->l1_in,
              2 + nch);
  if (n <= 0) return HNM_OK;
  float* xf = nullptr;
  float* wide = nullptr;
  float* wide2 = nullptr;
  const int ldx = nch * w->d;
  if (nch > 0) {
    HNM_REQUIRE(Fu == 0 || (user_features && w->duf_w), HNM_EINVAL,
                "widedeep_pair: user_features required");
    HNM_REQUIRE(Fi == 0 || (item_features && itf->dif_w), HNM_EINVAL,
                "widedeep_pair: item_features required");
    const int Fm = std::max(Fu, Fi);
    const size_t szx = hnm_align((size_t)n * ldx * 4), szf = hnm_align((size_t)n * Fm * 4);
    const size_t szw = hnm_align((size_t)n * 4);
    void* wsp;
    hnm_status st = hnm_workspace(ctx, szx + szf + 2 * szw, &wsp);
    if (st) return st;
    xf = (float*)wsp;
    float* wf = (float*)((char*)wsp + szx);
    float* w1 = (float*)((char*)wsp + szx + szf);
    float* w2 = (float*)((char*)wsp + szx + szf + szw);
    if (Fu > 0) {  // deep_user_features (wide_deep.py:214-215) + its wide cross (:190-192)
      st = hnm_linear_rows_f32(ctx, user_features, Fu, nullptr, n, n, Fu, w->duf_w, Fu, w->duf_b,
                               w->d, xf, ldx, 0);
      if (st) return st;
      if (w->wuf_w && w->wide_feat) {
        st = hnm_linear_rows_f32(ctx, user_features, Fu, nullptr, n, n, Fu, w->wuf_w, Fu,
                                 w->wuf_b, Fu, wf, Fu, 0);
        if (st) return st;
        // wide feature term = wf . final_w[U + I : U + I + Fu]
        st = hnm_linear_rows_f32(ctx, wf, Fu, nullptr, n, n, Fu, w->wide_feat, Fu, nullptr, 1, w1,
                                 1, 0);
        if (st) return st;
        wide = w1;
      }
    }
    if (Fi > 0) {  // deep_item_features (:216-217) + its wide cross (:193-195)
      st = hnm_linear_rows_f32(ctx, item_features, Fi, nullptr, n, n, Fi, itf->dif_w, Fi,
                               itf->dif_b, w->d, xf + (Fu > 0 ? w->d : 0), ldx, 0);
      if (st) return st;
      if (itf->wif_w && itf->wide_feat) {
        st = hnm_linear_rows_f32(ctx, item_features, Fi, nullptr, n, n, Fi, itf->wif_w, Fi,
                                 itf->wif_b, Fi, wf, Fi, 0);
        if (st) return st;
        st = hnm_linear_rows_f32(ctx, wf, Fi, nullptr, n, n, Fi, itf->wide_feat, Fi, nullptr, 1,
                                 w2, 1, 0);
        if (st) return st;
        wide2 = w2;
      }
    }
  }
  hipLaunchKernelGGL(widedeep_pair_kernel, dim3((unsigned)n), dim3(256), 0, ctx->stream, *w,
                     user_ids, item_ids, n, xf, ldx, wide, wide2, out, ctx->err_dev);
  HNM_LAUNCH_CHECK();
  return HNM_OK;
}

extern "C" hnm_status hnm_widedeep_pair_scores_f32(hnm_ctx* ctx, const hnm_widedeep_weights* w,
                                                   const int64_t* user_ids,
                                                   const int64_t* item_ids,
                                                   const float* user_features, int64_t n,
                                                   float* out) {
  HNM_CTX_DEVICE(ctx);
  return hnm_widedeep_pair_scores_ex_f32(ctx, w, nullptr, user_ids, item_ids, user_features,
                                         nullptr, n, out);
}
