// NeuralCF top-K with a CERTIFIED f16 pre-filter and exact fp32 re-scoring
// (neural_cf.py:300-326 recommend over :143-208 predict_all_items).
//
// The fp32 MFMA rate is 1/16 of the f16 rate on gfx950, and the NCF pair MLP is MFMA-bound.
// So the all-items scan runs in f16 (v_mfma_f32_32x32x16_f16, fp32 accumulate) and only
// PRUNES; every returned score is recomputed in exact fp32 by the same arithmetic as the
// fp32 kernel (ncf32_kernel), so outputs are bit-identical to the fp32 path.  Pruning is
// safe because of a rigorous per-user error bound E_u:
//
//   |approx(u, i) - (exact(u, i) - bp)| <= E_u   for every item i            (*)
//
// Let T = the K-th best exact score of user u (bp excluded) and e(u, i) the bound of (*) for
// pair (u, i).  A strided item sample scored by the f16 kernel gives L_u = K-th best of
// (approx - e) over the sample <= T.  Every item of the exact top-K has approx + e >= exact
// >= T >= L_u, so the main f16 pass appends every item with approx + e(u, i) >= L_u, and
// the exact top-K of the appended candidates IS the exact top-K.  Rows whose candidate
// segments overflow (or whose bound is not usable) are recomputed by the exact fp32 kernel
// over all items (on-device fallback).  No atomics in the scan: a wave owns its 32 users
// within its item partition, so per-(user, partition) counters live in registers.
//
// Bound (*).  Let z_k = |P_k| + |Q_k| (the fp32 layer-1 values both paths read), v_k =
// sum_j |wm_j||W2_jk|, A_u = sum_k v_k |P_uk|, B_i = sum_k v_k |Q_ik|, c0 = sum_j |wm_j b2_j|,
// C_u = ||wp_gmf * g_u||_2, D_i = ||g_i||_2.  With f16 unit roundoff u = 2^-11, RNE
// conversions (denormals kept: tools/mfma_semantics_probe.hip) and products exact in the
// fp32 accumulator: the layer-1 sum and its operands contribute <= 2.01u z_k, W2 rounding
// u|W2|, so |dH_j| <= 3.02u sum_k |W2_jk| z_k; relu is 1-Lipschitz; rounding relu(H) and wm
// adds 2u |wm_j| R_j with R_j = |b2_j| + sum_k |W2_jk| z_k; the GMF dot adds 2.01u C_u D_i;
// fp32 accumulation of both paths (<= 110 * 2^-24 relative) and the final adds are far
// below u.  Hence |err| <= 5.1u (c0 + A_u + B_i) + 2.1u C_u D_i + (subnormal terms) and
// we use e(u, i) = 6u (c0 + A_u + B_i + C_u D_i) + abs_slack.
// tests/test_gpu_prefilter.py checks (*) pair by pair on the full catalogue.
// The accumulation slack holds for any summation order: the f16 x f16 products are exact in the
// fp32 accumulator and a score is at most 96 fp32 additions (64 layer-2 terms or 64 GMF terms,
// then 32 units) however the matrix instructions group them.  So both layouts of the scan
// (HNM_OPT_SCAN_SHAPE: 1 = layer 2 and the GMF on v_mfma_f32_16x16x32_f16, the default; 0 = on
// v_mfma_f32_32x32x16_f16; the A/B and parity switch) satisfy (*) with the same e(u, i); their
// approximate scores may differ in the last bits, the returned top-K never does
// (tests/test_gpu_ncf_scan_shape.py).  Layout 1 has a third summation order: its epilogue's 32
// unit terms summed by 2 v_smfmac_f32_16x16x64_f16 (HNM_OPT_SCAN_SPARSE 1, the default) in place
// of 4 dense instructions (0).  The sparse instruction keeps f16 denormals and accumulates exact
// products in fp32 as the dense ones do (tools/mfma_semantics_probe.hip (d)), so it satisfies (*)
// with the same e(u, i) (tests/test_gpu_ncf_scan_sparse.py checks it pair by pair).
//
// Scaling: every f16 operand is scaled by a power of two so its magnitude is <= 1 (layer-1
// inputs <= 0.5, which also makes the packed add's [0,1] CLAMP an exact ReLU:
// v_pk_add_f16 ... clamp).  Scores are compared in the scaled unit s1*sw*sm.
//
// Per-call kernels before the first sample pass (two-layer tower, HNM_OPT_NCF_TABLES = 1):
//   ncf_tables_kernel    P_u, wp * g_u, Q_i (fp32) and A_u, C_u, B_i, D_i + the maxima's partials
//   cert_scales_kernel   one workgroup: partials and weight statistics -> CertParams
//   cert_convert_kernel  f16 copies P16 / WG16 / Q16 / G16 / weights, Bs / Cs in test units
// HNM_OPT_NCF_TABLES = 0, deep towers, padded GMF copies, h0 % 32 != 0 or unaligned tables: the
// tables by hnm_linear_rows_f32 (users, items) and gather_scale_kernel (ncf.hip ncf_tables), then
// cert_stats_kernel, cert_scales_kernel, cert_convert_kernel (deep towers: cert_deep_u_kernel
// first).  Both routes leave bitwise the same tables, bound terms and CertParams.
//
// Source layout.  This unit: the derivation above, the sampling side (champions, gate, the bounds
// and thresholds from the samples' K-th), the plan of a call (shape and scratch carve) and the
// functions of ncf_internal.h.  The kernels listed above: ncf_cert_params.hip; ncf16_scan_kernel:
// ncf_cert_scan.hip; ncf_rescore_kernel: ncf_cert_rescore.hip; what they share:
// ncf_cert_internal.h.
#include <algorithm>

#include "ncf_cert_internal.h"
#include "sample_kth.h"

namespace {

// Per row: Eu = user-constant part of the bound (scaled): 6u unit (c0 + A_u) + unit abs.
// Exact scores and the scan's values satisfy |approx - (exact - bp) unit| <= Eu + e_i, so
// the sample's K-th best of (approx - e_i), kv, certifies a lower bound of the row's exact
// K-th best score in real units: L = (kv - Eu) / unit + bp (unit is a power of two; the
// relative 2^-21 covers the fp32 rounding of the subtraction and of + bp).  Rows with an
// unusable bound get L = -inf.  Any lower bound works downstream -- e.g. the max of the
// item shards' L over the ranks of a node (hnm_ncf_topk_begin_f32 / _finish_f32).
__device__ __forceinline__ float cert_row_bound(const CertParams* prm, float unit,
                                                const float* Au, int64_t b) {
  return unit * (prm->rho * (prm->c0 + Au[b]) + prm->absb);
}
__device__ __forceinline__ float cert_lower_bound(const CertParams* prm, float unit, float kv,
                                                  float e, const float* bp) {
  float l = (kv - e) / unit + bp[0];
  l -= fabsf(l) * 4.76837158203125e-07f;  // 2^-21
  return (!prm->bad && __builtin_isfinite(l) && __builtin_isfinite(e)) ? l : -__builtin_inff();
}

// The scan threshold of a row in this call's scaled units from a lower bound l of the exact
// K-th (real units): an item can be in the top-K only if exact >= l, i.e. approx + e_i >=
// (l - bp) unit - Eu; minus a guard for the fp32 rounding of the test quantities (2^-18 of
// the row's absolute score scale, 2^-20 relative).  Unusable rows: tau = +inf, flag = 1
// (the exact fallback scan).
__device__ __forceinline__ void cert_threshold(const CertParams* prm, float unit, const float* Au,
                                               const float* Cu, int64_t b, float l, float e,
                                               const float* bp, float* tau, int* flag) {
  const float scale = unit * (prm->c0 + Au[b] + prm->Bmax + Cu[b] * prm->Dmax);
  float tv = (l - bp[0]) * unit - e - 3.814697265625e-06f * scale;  // 2^-18
  tv -= fabsf(tv) * 9.5367431640625e-07f;                           // 2^-20
  const bool ok = !prm->bad && __builtin_isfinite(tv) && __builtin_isfinite(scale);
  tau[b] = ok ? tv : __builtin_inff();
  flag[b] = ok ? 0 : 1;
}

// The larger of two samples' lower bounds (kth2 used when *gate: the strided sample ran); a NaN
// in either (a row with a NaN score) stays NaN.
__device__ __forceinline__ float kth_pick(const float* kth, const float* kth2, const int* gate,
                                          int64_t x) {
  const float a = kth[x];
  if (!gate || *gate == 0) return a;
  const float c = kth2[x];
  return (a != a || c != c) ? __builtin_nanf("") : fmaxf(a, c);
}

__global__ __launch_bounds__(256) void cert_bound_kernel(const float* __restrict__ kth,
                                                         const float* __restrict__ kth2,
                                                         const int* __restrict__ gate, int K,
                                                         const float* __restrict__ Au,
                                                         const CertParams* __restrict__ prm,
                                                         const float* __restrict__ bp, int64_t B,
                                                         float* __restrict__ lb,
                                                         float* __restrict__ Eu) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const float unit = prm->unit;
  const float e = cert_row_bound(prm, unit, Au, b);
  if (Eu) Eu[b] = e;
  if (!kth) return;
  lb[b] = cert_lower_bound(prm, unit, kth_pick(kth, kth2, gate, b * K + (K - 1)), e, bp);
}

// Per (row, r < K): the certified lower bound of the exact score of the sample's r-th best
// item (real units, as cert_bound_kernel for the K-th), for an exchange of whole lists across
// item shards: the K-th best of the union of every shard's lists bounds the global K-th.
__global__ __launch_bounds__(256) void cert_bound_lists_kernel(const float* __restrict__ kth,
                                                               const float* __restrict__ kth2,
                                                               const int* __restrict__ gate,
                                                               int K,
                                                               const float* __restrict__ Eu,
                                                               const CertParams* __restrict__ prm,
                                                               const float* __restrict__ bp,
                                                               int64_t B, float* __restrict__ lists) {
  const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (x >= B * K) return;
  const float unit = prm->unit, e = Eu[x / K];
  // slot r of either sample's list lower-bounds the row's (r+1)-th best item of this shard,
  // so the larger of the two does too (the lists exchange needs exactly that per slot)
  lists[x] = cert_lower_bound(prm, unit, kth_pick(kth, kth2, gate, x), e, bp);
}

// Per row: cert_threshold of the lower bounds lb.
__global__ __launch_bounds__(256) void cert_tau_kernel(const float* __restrict__ lb,
                                                       const float* __restrict__ Au,
                                                       const float* __restrict__ Cu,
                                                       const float* __restrict__ Eu,
                                                       const CertParams* __restrict__ prm,
                                                       const float* __restrict__ bp, int64_t B,
                                                       float* __restrict__ tau,
                                                       int* __restrict__ flag) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  cert_threshold(prm, prm->unit, Au, Cu, b, lb[b], Eu[b], bp, tau, flag);
}

// One-shot calls (ncf_cert_topk, the deep towers' certified call): cert_bound_kernel's lower
// bound and cert_tau_kernel's threshold per row in the epilogue of the champion sample's K-th
// launch (round 6) -- the same three functions (L stored and reused as a register),
// two launches and kernel boundaries less on the per-call latency chain.  Not with the gated
// strided sample (its K-th comes from a second launch).
struct NcfBoundTauEpi {
  const CertParams* prm;
  const float* Au;
  const float* Cu;
  const float* bp;
  float* Eu;
  float* lb;
  float* tau;
  int* flag;
  __device__ void operator()(int64_t b, float kv) const {
    const float unit = prm->unit;
    const float e = cert_row_bound(prm, unit, Au, b);
    Eu[b] = e;
    const float l = cert_lower_bound(prm, unit, kv, e, bp);
    lb[b] = l;
    cert_threshold(prm, unit, Au, Cu, b, l, e, bp, tau, flag);
  }
};

// Champion sample: items split into nch contiguous groups of gsz; each group's item with the
// best mean (approx - e_i) over the proxy rows (the first users of the batch) -- a
// popularity-like sample in increasing item order.  Any item subset gives a valid lower
// bound of a row's K-th; this one tends to hold the rows' best items.  One wave per group.
// sloo (optional): also each proxy row r's leave-one-out champions, by the mean over the OTHER
// rows, at sloo[r * nch + g] (cert_gate_kernel's quality check).
__global__ __launch_bounds__(256) void cert_champion_kernel(const float* __restrict__ pd,
                                                            int64_t ld, int np_rows, int64_t I,
                                                            int64_t gsz, int64_t nch,
                                                            int32_t* __restrict__ sidx,
                                                            int32_t* __restrict__ sloo,
                                                            int64_t ns, int32_t* __restrict__ sidx2,
                                                            unsigned long long* __restrict__ gcnt) {
  // the gate's inputs: its counters zeroed, the strided sample's item map (tiles 0, S, 2S, ...
  // of 32 items: sidx2[0, ns)) -- both read only by later launches
  if (gcnt && blockIdx.x == 0 && threadIdx.x < 4) gcnt[threadIdx.x] = 0;
  if (sidx2)
    for (int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x; n < ns; n += (int64_t)gridDim.x * 256)
      sidx2[n] = (int32_t)((n >> 5) * (32 * CERT_STRIDE) + (n & 31));
  const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= nch) return;
  const int lane = threadIdx.x & 63;
  const int64_t i0 = g * gsz, i1 = std::min<int64_t>(I, i0 + gsz);
  float best = -__builtin_inff();
  int64_t bi = i0;
  float lbest[CERT_PROXY_USERS];
  int64_t lbi[CERT_PROXY_USERS];
#pragma unroll
  for (int r = 0; r < CERT_PROXY_USERS; ++r) {
    lbest[r] = -__builtin_inff();
    lbi[r] = i0;
  }
  for (int64_t i = i0 + lane; i < i1; i += 64) {
    float v[CERT_PROXY_USERS];
    float m = 0.f;
#pragma unroll
    for (int r = 0; r < CERT_PROXY_USERS; ++r) {
      v[r] = r < np_rows ? pd[r * ld + i] : 0.f;
      if (r < np_rows) m += v[r];
    }
    if (m > best) {  // NaN never wins; the lane's items are visited in increasing order
      best = m;
      bi = i;
    }
    if (sloo) {
#pragma unroll
      for (int r = 0; r < CERT_PROXY_USERS; ++r) {
        const float mr = m - v[r];
        if (mr > lbest[r]) {
          lbest[r] = mr;
          lbi[r] = i;
        }
      }
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {  // wave argmax, ties -> smaller item
    const float ob = __shfl_xor(best, o);
    const int64_t oi = __shfl_xor(bi, o);
    if (ob > best || (ob == best && oi < bi)) {
      best = ob;
      bi = oi;
    }
  }
  if (lane == 0) sidx[g] = (int32_t)bi;
  if (!sloo) return;
#pragma unroll
  for (int r = 0; r < CERT_PROXY_USERS; ++r) {
    float b = lbest[r];
    int64_t x = lbi[r];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const float ob = __shfl_xor(b, o);
      const int64_t oi = __shfl_xor(x, o);
      if (ob > b || (ob == b && oi < x)) {
        b = ob;
        x = oi;
      }
    }
    if (lane == 0 && r < np_rows) sloo[r * nch + g] = (int32_t)x;
  }
}

// Lane top-4 insert and the K-th of a wave's lists by K pops (sample_kth_kernel's scheme: a
// lower bound of the K-th best of the values offered; -inf when fewer).
struct Top4 {
  float t0 = -__builtin_inff(), t1 = -__builtin_inff(), t2 = -__builtin_inff(),
        t3 = -__builtin_inff();
  __device__ void offer(float x) {
    if (x > t3) {
      const float a = fminf(x, t2), c2 = fmaxf(x, t2);
      t3 = a;
      t2 = fminf(c2, t1);
      const float c1 = fmaxf(c2, t1);
      t1 = fminf(c1, t0);
      t0 = fmaxf(c1, t0);
    }
  }
  __device__ float kth(int K, int lane) {
    float kv = -__builtin_inff();
    for (int r = 0; r < K; ++r) {
      const float m = hnm_wave_max(t0);
      kv = m;
      if (m == -__builtin_inff()) break;  // wave-uniform
      const int wl = __builtin_ctzll(__ballot(t0 == m));
      if (lane == wl) {
        t0 = t1;
        t1 = t2;
        t2 = t3;
        t3 = -__builtin_inff();
      }
    }
    return kv;
  }
};

// The gate (one 1,024-thread workgroup per proxy row r).  Two lower bounds of the row's K-th best
// (approx - e_i): kc over its leave-one-out champions, ks over the strided sample's items (lane
// top-4 lists, each wave's K pops, the K-th of the 16 waves' lists); then, over the strided items
// -- a uniform 1/CERT_STRIDE sample of the catalogue, already in registers -- the count of those
// the main scan would append with the champion bound alone (approx + e_i >= kc - 2 Eu) and with
// the strided sample's bound too, times CERT_STRIDE.  The last workgroup writes *gate = 1 when
// the pass is predicted to save more than CERT_GATE_GAIN candidates a row.  Every load is issued
// in one of three batches (the proxy rows were just written: each dependent round trip costs
// microseconds).  Round 5, earlier forms: a kth kernel + a full-catalogue count kernel 25 + 24
// us, one fused kernel counting the whole catalogue 32 us a call.
constexpr int GATE_SPT = 16;  // strided items per thread (16,384 per row: I <= 524,288 fully)
__global__ __launch_bounds__(1024) void cert_gate_kernel(
    const float* __restrict__ pd, int64_t ld, int np_rows, const int32_t* __restrict__ sloo,
    int64_t nch, int K, int64_t ns, const float* __restrict__ Bs, const float* __restrict__ Di,
    const float* __restrict__ Cs, const float* __restrict__ Au, const CertParams* __restrict__ prm,
    unsigned long long* __restrict__ cnt, int* __restrict__ gate, int64_t B,
    unsigned long long* __restrict__ stats) {
  constexpr int NW = 16;
  __shared__ float wl[2][NW][64];
  __shared__ float kvs[2];
  __shared__ int part[2][NW];
  const int r = blockIdx.x, tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const float* row = pd + r * ld;
  const int32_t* sl = sloo + r * nch;
  // the strided sample: thread tid takes its items n = tid + 1024 u (u < GATE_SPT); with more
  // than 16,384 sampled items the rest are left out (a lower bound / a sample of the count)
  const int64_t nsg = std::min<int64_t>(ns, 1024 * GATE_SPT);
  int32_t ix[4];
  float v[GATE_SPT], bsv[GATE_SPT], dv[GATE_SPT];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int64_t q = u * 1024 + tid;
    ix[u] = q < nch ? sl[q] : -1;  // nch <= CERT_CHAMPIONS (<= 4,096 loaded)
  }
#pragma unroll
  for (int u = 0; u < GATE_SPT; ++u) {
    const int64_t n = u * 1024 + tid;
    const int64_t it = (n >> 5) * (32 * CERT_STRIDE) + (n & 31);
    const bool ok = n < nsg;
    v[u] = ok ? row[it] : -__builtin_inff();
    bsv[u] = ok ? Bs[it] : 0.f;
    dv[u] = ok ? Di[it] : 0.f;
  }
  Top4 c, t;
#pragma unroll
  for (int u = 0; u < 4; ++u) c.offer(ix[u] >= 0 ? row[ix[u]] : -__builtin_inff());
#pragma unroll
  for (int u = 0; u < GATE_SPT; ++u) t.offer(v[u]);
  for (int i = 0; i < 2; ++i) {  // each wave's K best survivors, descending
    Top4& L = i ? t : c;
    for (int q = 0; q < K; ++q) {
      const float m = hnm_wave_max(L.t0);
      if (lane == 0) wl[i][w][q] = m;
      if (m == -__builtin_inff()) {
        for (int z = q + 1 + lane; z < K; z += 64) wl[i][w][z] = -__builtin_inff();
        break;  // wave-uniform
      }
      const int wk = __builtin_ctzll(__ballot(L.t0 == m));
      if (lane == wk) {
        L.t0 = L.t1;
        L.t1 = L.t2;
        L.t2 = L.t3;
        L.t3 = -__builtin_inff();
      }
    }
  }
  __syncthreads();
  if (w < 2) {  // wave i: the K-th of the 16 waves' lists (exact for K <= 16: at most 4 values a
                // lane; a lower bound of it beyond, as good for a prediction)
    Top4 M;
    for (int z = lane; z < NW * K; z += 64) M.offer(wl[w][z / K][z % K]);
    const float kv = M.kth(K, lane);
    if (lane == 0) kvs[w] = kv;
  }
  __syncthreads();
  const float eu2 = 2.f * prm->unit * (prm->rho * (prm->c0 + Au[r]) + prm->absb);
  const float tc = kvs[0] - eu2, ts = fmaxf(kvs[0], kvs[1]) - eu2, cr = Cs[r];
  int nc = 0, nsv = 0;
#pragma unroll
  for (int u = 0; u < GATE_SPT; ++u) {
    const float ub = v[u] + 2.f * fmaf(cr, dv[u], bsv[u]);  // approx + e_i
    nc += ub >= tc;
    nsv += ub >= ts;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    nc += __shfl_xor(nc, o);
    nsv += __shfl_xor(nsv, o);
  }
  if (lane == 0) {
    part[0][w] = nc;
    part[1][w] = nsv;
  }
  __syncthreads();
  if (tid == 0) {
    unsigned long long s0 = 0, s1 = 0;
    for (int q = 0; q < NW; ++q) {
      s0 += (unsigned)part[0][q];
      s1 += (unsigned)part[1][q];
    }
    // scaled to the catalogue: the sampled share of the items
    const double scale = (double)ns / (double)std::max<int64_t>(nsg, 1) * CERT_STRIDE;
    atomicAdd(&cnt[0], (unsigned long long)(s0 * scale));
    atomicAdd(&cnt[1], (unsigned long long)(s1 * scale));
    __threadfence();
    const unsigned long long ticket = atomicAdd(&cnt[2], 1ull);
    if (ticket == (unsigned long long)gridDim.x - 1) {  // every count is in
      __threadfence();
      const unsigned long long c0 = atomicAdd(&cnt[0], 0ull), c1 = atomicAdd(&cnt[1], 0ull);
      const int on = (np_rows >= 4 && !prm->bad &&
                      c0 > c1 + (unsigned long long)(CERT_GATE_GAIN * np_rows)) ? 1 : 0;
      *gate = on;
      if (stats) {
        if (on) atomicAdd(&stats[3], (unsigned long long)B);
        // diagnostics (last call): the proxies' predicted candidates under each bound
        stats[4] = c0;
        stats[5] = c1;
      }
    }
  }
}

// Deep towers: the candidates the main scan would append for the proxy rows (whose every item the
// proxy pass scored: pd = approx - e_i), approx + e_i >= tau with tau ~ kv - 2 Eu (cert_tau_kernel)
// -- where the worst-case bound through two absolute-value layers is wider than the rows' score
// spread (init-like weights) the certified scan cannot prune and the call takes the exact kernels
// instead.  An unusable bound counts every item.
__global__ __launch_bounds__(256) void cert_predict_kernel(const float* __restrict__ pd, int64_t I,
                                                           int K, const float* __restrict__ kthv,
                                                           const float* __restrict__ Eu,
                                                           const float* __restrict__ Bs,
                                                           const float* __restrict__ Cs,
                                                           const float* __restrict__ Di,
                                                           const CertParams* __restrict__ prm,
                                                           unsigned long long* __restrict__ cnt) {
  const int r = blockIdx.y;
  const float thr = kthv[(int64_t)r * K + K - 1] - 2.f * Eu[r], cs = Cs[r];
  const bool bad = prm->bad || !__builtin_isfinite(thr);
  unsigned n = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < I; i += (int64_t)gridDim.x * 256)
    n += bad || !(pd[(int64_t)r * I + i] + 2.f * fmaf(cs, Di[i], Bs[i]) < thr);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) n += __shfl_xor(n, o);
  if ((threadIdx.x & 63) == 0 && n) atomicAdd(cnt, (unsigned long long)n);
}

// scaled -> real units, for the diagnostics entry point
__global__ void cert_unscale_kernel(float* __restrict__ a, float* __restrict__ e, int64_t lda,
                                    int64_t B, int64_t I, const CertParams* __restrict__ prm) {
  const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (x >= B * I) return;
  const int64_t o = (x / I) * lda + x % I;
  a[o] /= prm->unit;
  e[o] /= prm->unit;
}

// ~CERT_WG_PER_CU workgroups per CU (the scan's occupancy), NP a multiple of 8 (XCD-aware),
// <= CERT_MAX_NP
Partition scan_partition(int64_t I, int64_t ublocks, int num_cus) {
  int64_t np = std::max<int64_t>(
      1, (int64_t)CERT_WG_PER_CU * num_cus / std::max<int64_t>(ublocks, 1));
  np = std::min<int64_t>(np, std::max<int64_t>(1, hnm_cdiv(I, 4 * TILE)));
  np = std::min<int64_t>(np, CERT_MAX_NP);
  if (np >= 8) np = np / 8 * 8;
  const int64_t ipp = hnm_cdiv(hnm_cdiv(I, np), TILE) * TILE;
  return {(int)hnm_cdiv(I, ipp), ipp};
}

}  // namespace

CertShape cert_shape(int64_t B, int64_t I, int K, int num_cus) {
  CertShape sh;
  sh.gsz = std::max<int64_t>(CERT_GROUP_MIN, hnm_cdiv(I, CERT_CHAMPIONS));
  sh.nch = hnm_cdiv(I, sh.gsz);
  const int64_t nst = hnm_cdiv(hnm_cdiv(I, TILE), CERT_STRIDE);  // sampled tiles
  sh.ns = (nst - 1) * TILE + std::min<int64_t>(TILE, I - (nst - 1) * CERT_STRIDE * TILE);
  sh.part = scan_partition(I, hnm_cdiv(B, 128), num_cus);
  // a row's candidates: items within the bound's margin of the champion sample's K-th --
  // at worst (no shared best items) the K-th of a 1/gsz sample, ~K * gsz items; each
  // partition gets 4x its even share of 8x that, >= 64 slots (overflow: fallback row).
  // Round 5: 8x (was 2x) -- with the best-first re-scoring a long candidate list costs the
  // scan's appends and one sort, while an overflowing row costs an exact scan of the whole
  // catalogue ("norms" trained-like weights: 44 fallback rows -> 0, 3.50 -> 3.24 ms a step;
  // init weights unchanged: profiles/r6k_ncf_capp_ab.txt)
  const int64_t total = std::min<int64_t>(8192, std::max<int64_t>(512, 8 * (int64_t)K * sh.gsz));
  sh.capp = (int)std::max<int64_t>(64, std::min<int64_t>(total, hnm_cdiv(4 * total, sh.part.np)));
  return sh;
}

namespace {

// carve (or size, when base == nullptr) the scratch region of a call of shape sh
// strided: carve the gated strided sample's scratch (sloo, sidx2, sdense [B, ns], kth2) -- only
// for calls that may run it (HNM_OPT_STRIDED; ADVICE r5: ~0.2 GB a B = 4,096 call otherwise)
size_t cert_carve(char* base, const CertShape& sh, int64_t B, int64_t I, int K, int num_cus,
                  bool strided, CertWs* w) {
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* p = base ? base + off : nullptr;
    off += hnm_align(bytes);
    return p;
  };
  CertWs x;
  x.prm = (CertParams*)take(sizeof(CertParams));
  x.Au = (float*)take(B * 4);
  x.Cu = (float*)take(B * 4);
  x.Cs = (float*)take(B * 4);
  x.Bs = (float*)take(I * 4);
  x.part = (float*)take(4 * 4 * (1024 + 256));
  x.Bi = (float*)take(I * 4);
  x.Di = (float*)take(I * 4);
  x.tau = (float*)take(B * 4);
  x.Eu = (float*)take(B * 4);
  x.b2s = (float*)take(32 * 4);
  x.kthv = (float*)take((size_t)B * K * 4);
  x.lb = (float*)take((size_t)B * 4);
  x.pdense = (float*)take((size_t)CERT_PROXY_USERS * I * 4);
  x.cdense = (float*)take((size_t)B * sh.nch * 4);
  x.sidx = (int32_t*)take((size_t)sh.nch * 4);
  x.sloo = strided ? (int32_t*)take((size_t)CERT_PROXY_USERS * sh.nch * 4) : nullptr;
  x.sidx2 = strided ? (int32_t*)take((size_t)sh.ns * 4) : nullptr;
  x.sdense = strided ? (float*)take((size_t)B * sh.ns * 4) : nullptr;
  x.kth2 = strided ? (float*)take((size_t)B * K * 4) : nullptr;
  x.gate = (int*)take(4);
  x.gcnt = (unsigned long long*)take(4 * 8);
  x.kthi = (int64_t*)take((size_t)B * K * 8);
  x.cnt = (int*)take((size_t)B * sh.part.np * 4);
  x.flag = (int*)take(B * 4);
  x.ovf_cnt = (int32_t*)take(256);
  x.ovf_rows = (int32_t*)take(B * 4);
  x.buf = (int32_t*)take((size_t)B * sh.part.np * sh.capp * 4);
  x.bufd = (float*)take((size_t)B * sh.part.np * sh.capp * 4);
  x.P16 = (_Float16*)take((size_t)B * 64 * 2);
  x.WG16 = (_Float16*)take((size_t)B * 64 * 2);
  x.Q16 = (_Float16*)take((size_t)I * 64 * 2);
  x.G16 = (_Float16*)take((size_t)I * 64 * 2);
  x.W2h = (_Float16*)take(32 * 64 * 2);
  x.wmh = (_Float16*)take(32 * 2);
  x.W3h = (_Float16*)take(16 * 32 * 2);
  x.wph = (_Float16*)take(16 * 2);
  x.b3s = (float*)take(16 * 4);
  x.u = (float*)take(32 * 4);
  const size_t lb = ncf_list_bytes(B, I, K, num_cus);
  x.cv = (float*)take(lb);
  x.ci = (int32_t*)take(lb);
  if (w) *w = x;
  return off;
}

ScanArgs scan_args(const CertWs& x, int64_t B, bool deep) {
  ScanArgs a{};
  a.W3h = deep ? x.W3h : nullptr;  // selects the deep scan (cert_launch_scan)
  a.wph = x.wph;
  a.b3s = x.b3s;
  a.P16 = x.P16;
  a.WG16 = x.WG16;
  a.Q16 = x.Q16;
  a.G16 = x.G16;
  a.W2h = x.W2h;
  a.wmh = x.wmh;
  a.b2s = x.b2s;
  a.Bi = x.Bs;
  a.Di = x.Di;
  a.Cu = x.Cs;
  a.Eu = x.Eu;
  a.prm = x.prm;
  a.B = B;
  a.sidx = nullptr;
  a.upw = 32;
  return a;
}

}  // namespace

bool ncf_cert_eligible(const hnm_ncf_weights* w, int K) {
  // the scan addresses Q16 / G16 by 32-bit element offsets (item * 64 < 2^31: 33.5M items)
  return w->h1 <= 64 && w->mf <= 64 && w->h2 <= 32 && K <= 64 &&
         w->num_items >= CERT_MIN_ITEMS && w->num_items >= 64 * (int64_t)K &&
         w->num_items * 64 < ((int64_t)1 << 31);
}

size_t ncf_cert_bytes(const hnm_ctx* ctx, int64_t B, int64_t I, int K, bool strided) {
  return cert_carve(nullptr, cert_shape(B, I, K, ctx->num_cus), B, I, K, ctx->num_cus, strided,
                    nullptr);
}

CertPlan cert_plan(const hnm_ctx* ctx, int64_t B, int64_t I, int K, void* scratch, bool strided) {
  CertPlan pl;
  pl.sh = cert_shape(B, I, K, ctx->num_cus);
  cert_carve((char*)scratch, pl.sh, B, I, K, ctx->num_cus, strided, &pl.ws);
  return pl;
}

// Phase 1: per-call bound statistics and f16 copies, the champion sample, and every row's
// certified lower bound of the exact K-th best score (real units) into lb[B].
hnm_status ncf_cert_begin(hnm_ctx* ctx, const hnm_ncf_weights* w, const NcfTabs& t, int64_t B,
                          const int64_t* mptr, const int32_t* midx, int K, void* scratch,
                          bool strided, float* lb, float* lists, const CertDeep* dp) {
  const int64_t I = w->num_items;
  const CertPlan pl = cert_plan(ctx, B, I, K, scratch, strided);
  const CertShape& sh = pl.sh;
  const CertWs& x = pl.ws;
  hnm_status st = cert_prepare(ctx, w, t, B, x, dp);
  if (st) return st;
  const int64_t ublocks = hnm_cdiv(B, 128);
  const bool deep = dp != nullptr;
  // champion sample: the first rows' approx - e over all items -> the best item of each of
  // nch groups -> every row's K-th best approx - e over those items -> L (a lower bound of
  // the exact K-th for any item subset; this one tends to hold the rows' best items)
  const int64_t bp = std::min<int64_t>(CERT_PROXY_USERS, B);
  ScanArgs a = scan_args(x, bp, deep);
  a.I = I;
  a.dense = x.pdense;
  a.ldo = I;
  const int64_t np = std::min<int64_t>(3 * (int64_t)ctx->num_cus, hnm_cdiv(I, 4 * TILE));
  a.ipp = hnm_cdiv(hnm_cdiv(I, np), TILE) * TILE;
  a.NP = (int)hnm_cdiv(I, a.ipp);
  a.upw = 2;  // the <= 8 proxy rows as one user pair per wave (4x shorter per tile than one wave)
  cert_launch_scan(ctx, SCAN_SAMPLE, dim3((unsigned)a.NP, 1), a);
  HNM_LAUNCH_CHECK();
  hipLaunchKernelGGL(cert_champion_kernel, dim3((unsigned)hnm_cdiv(sh.nch, 4)), dim3(256), 0,
                     ctx->stream, x.pdense, I, (int)bp, I, sh.gsz, sh.nch, x.sidx,
                     strided ? x.sloo : nullptr, sh.ns, strided ? x.sidx2 : nullptr,
                     strided ? x.gcnt : nullptr);
  HNM_LAUNCH_CHECK();
  // the gate (8 workgroups, latency-bound: ~22 us) runs on the ctx's side stream beside the
  // champion pass of every row below (independent: both read the proxy rows and the champions);
  // the ctx stream joins before the strided pass reads the gate
  const bool gated = strided && bp >= 4;
  if (gated) {
    HNM_HIP_CHECK(hipEventRecord(ctx->side_in, ctx->stream));
    HNM_HIP_CHECK(hipStreamWaitEvent(ctx->side, ctx->side_in, 0));
    hipLaunchKernelGGL(cert_gate_kernel, dim3((unsigned)bp), dim3(1024), 0, ctx->side,
                       x.pdense, I, (int)bp, x.sloo, sh.nch, K, sh.ns, x.Bs, x.Di, x.Cs, x.Au,
                       x.prm, x.gcnt, x.gate, B, ctx->stats_on ? ctx->stats_dev : nullptr);
    HNM_LAUNCH_CHECK();
    HNM_HIP_CHECK(hipEventRecord(ctx->side_out, ctx->side));
  } else if (strided) {
    HNM_HIP_CHECK(hipMemsetAsync(x.gate, 0, 4, ctx->stream));
  }
  ScanArgs c = scan_args(x, B, deep);
  c.I = sh.nch;
  c.sidx = x.sidx;
  c.dense = x.cdense;
  c.ldo = sh.nch;
  // as many partitions as one round of workgroups holds (the main scan's >= 4-tile,
  // multiple-of-8 partitions would leave a third of the slots idle on 2,048 champions)
  const int64_t npc = std::max<int64_t>(1, (int64_t)CERT_WG_PER_CU * ctx->num_cus / ublocks);
  c.ipp = hnm_cdiv(hnm_cdiv(sh.nch, npc), TILE) * TILE;
  c.NP = (int)hnm_cdiv(sh.nch, c.ipp);
  cert_launch_scan(ctx, SCAN_SAMPLE, dim3((unsigned)c.NP, (unsigned)ublocks), c);
  if (gated) HNM_HIP_CHECK(hipStreamWaitEvent(ctx->stream, ctx->side_out, 0));  // join
  HNM_LAUNCH_CHECK();
  // one-shot call (no bound out, no lists, no strided sample): bound + threshold fused into the
  // K-th launch; ncf_cert_finish then skips cert_tau_kernel (same condition there)
  const bool fuse = lb == nullptr && lists == nullptr && !strided;
  if (fuse)
    return sample_kth_launch(ctx, x.cdense, sh.nch, B, sh.nch, mptr, midx, K, 1, 1, x.sidx, x.kthv,
                             nullptr, NcfBoundTauEpi{x.prm, x.Au, x.Cu, w->bp, x.Eu, x.lb, x.tau,
                                                     x.flag});
  st = hnm_sample_kth(ctx, x.cdense, sh.nch, B, sh.nch, mptr, midx, K, 1, 1, x.sidx, x.kthv);
  if (st) return st;
  // gated strided sample: every row against one tile in CERT_STRIDE (exits when gated off)
  ScanArgs g2 = scan_args(x, B, deep);
  g2.I = sh.ns;
  g2.sidx = x.sidx2;
  g2.dense = x.sdense;
  g2.ldo = sh.ns;
  g2.gate = x.gate;
  const Partition p2 = scan_partition(sh.ns, ublocks, ctx->num_cus);
  g2.ipp = p2.ipp;
  g2.NP = p2.np;
  if (strided) {
    cert_launch_scan(ctx, SCAN_SAMPLE, dim3((unsigned)p2.np, (unsigned)ublocks), g2);
    HNM_LAUNCH_CHECK();
    st = hnm_sample_kth(ctx, x.sdense, sh.ns, B, sh.ns, mptr, midx, K, 1, 1, x.sidx2, x.kth2, x.gate);
    if (st) return st;
  }
  const int* gp = strided ? x.gate : nullptr;
  hipLaunchKernelGGL(cert_bound_kernel, dim3((unsigned)hnm_cdiv(B, 256)), dim3(256), 0,
                     ctx->stream, x.kthv, x.kth2, gp, K, x.Au, x.prm, w->bp, B, lb ? lb : x.lb,
                     x.Eu);
  HNM_LAUNCH_CHECK();
  if (lists) {
    hipLaunchKernelGGL(cert_bound_lists_kernel, dim3((unsigned)hnm_cdiv(B * K, 256)), dim3(256), 0,
                       ctx->stream, x.kthv, x.kth2, gp, K, x.Eu, x.prm, w->bp, B, lists);
    HNM_LAUNCH_CHECK();
  }
  return HNM_OK;
}

// Phase 2: thresholds from the lower bounds lb (this call's, or the max over item shards),
// the main f16 scan, exact fp32 re-scoring + top-K, the exact fallback for unusable rows.
// short_ok: a row may keep fewer than K candidates (its bound came from another shard).
hnm_status ncf_cert_finish(hnm_ctx* ctx, const hnm_ncf_weights* w, const NcfTabs& t, int64_t B,
                           const int64_t* mptr, const int32_t* midx, int K, void* scratch,
                           bool strided, const float* lb, int short_ok, float* ov, int64_t* oi,
                           const CertDeep* dp, int32_t** ovf_rows, int32_t** ovf_cnt) {
  const int64_t I = w->num_items;
  const CertPlan pl = cert_plan(ctx, B, I, K, scratch, strided);
  const CertShape& sh = pl.sh;
  const CertWs& x = pl.ws;
  const int64_t ublocks = hnm_cdiv(B, 128);
  if (lb != nullptr || strided) {  // else tau / flag came with the begin phase's K-th
    hipLaunchKernelGGL(cert_tau_kernel, dim3((unsigned)hnm_cdiv(B, 256)), dim3(256), 0,
                       ctx->stream, lb ? lb : x.lb, x.Au, x.Cu, x.Eu, x.prm, w->bp, B, x.tau,
                       x.flag);
    HNM_LAUNCH_CHECK();
  }
  // main f16 scan: append items with approx + e >= tau_u to per-partition segments
  ScanArgs a = scan_args(x, B, dp != nullptr);
  a.I = I;
  a.mptr = mptr;
  a.midx = midx;
  a.tau = x.tau;
  a.cnt = x.cnt;
  a.buf = x.buf;
  a.segd = x.bufd;
  a.capp = sh.capp;
  a.ipp = sh.part.ipp;
  a.NP = sh.part.np;
  hnm_timer_begin(ctx, HNM_TIME_SCORE);
  cert_launch_scan(ctx, SCAN_THRESH, dim3((unsigned)sh.part.np, (unsigned)ublocks), a);
  hnm_timer_end(ctx, HNM_TIME_SCORE);
  HNM_LAUNCH_CHECK();
  // exact fp32 re-scoring + top-K of the candidates; unusable rows -> queue
  cert_launch_rescore(ctx, w, t, B, pl, K, short_ok, ov, oi, dp);
  HNM_LAUNCH_CHECK();
  if (dp) {  // the deep tower's exact scan of the queued rows is the caller's (ncf_deep.hip)
    *ovf_rows = x.ovf_rows;
    *ovf_cnt = x.ovf_cnt;
    return HNM_OK;
  }
  // exact fp32 scan over all items for the queued rows (device-side row list)
  hnm_status st =
      ncf_list_rows(ctx, w, t, B, mptr, midx, K, x.ovf_rows, x.ovf_cnt, x.cv, x.ci, ov, oi);
  if (st || !short_ok) return st;
  // short rows: what the scan appended below the caller's bound depends on f16 rounding
  return hnm_topk_trim_below(ctx, ov, oi, B, K, lb);
}

hnm_status ncf_cert_topk(hnm_ctx* ctx, const hnm_ncf_weights* w, const NcfTabs& t, int64_t B,
                         const int64_t* mptr, const int32_t* midx, int K, void* scratch,
                         bool strided, float* ov, int64_t* oi) {
  hnm_status st = ncf_cert_begin(ctx, w, t, B, mptr, midx, K, scratch, strided, nullptr);
  if (st) return st;
  return ncf_cert_finish(ctx, w, t, B, mptr, midx, K, scratch, strided, nullptr, 0, ov, oi);
}

hnm_status ncf_deep_cert_topk(hnm_ctx* ctx, const hnm_ncf_weights* w, const CertDeep& dp,
                              const NcfTabs& t, int64_t B, const int64_t* mptr,
                              const int32_t* midx, int K, void* scratch, float* ov, int64_t* oi,
                              int32_t** ovf_rows, int32_t** ovf_cnt, bool* pruned) {
  hnm_status st = ncf_cert_begin(ctx, w, t, B, mptr, midx, K, scratch, false, nullptr, nullptr, &dp);
  if (st) return st;
  // can the bound prune?  the proxy rows' predicted candidates (one read-back)
  const int64_t I = w->num_items;
  const CertPlan pl = cert_plan(ctx, B, I, K, scratch, false);
  const CertShape& sh = pl.sh;
  const CertWs& x = pl.ws;
  const int np_rows = (int)std::min<int64_t>(CERT_PROXY_USERS, B);
  HNM_HIP_CHECK(hipMemsetAsync(x.gcnt, 0, 8, ctx->stream));
  hipLaunchKernelGGL(cert_predict_kernel,
                     dim3((unsigned)std::min<int64_t>(64, hnm_cdiv(I, 256)), (unsigned)np_rows),
                     dim3(256), 0, ctx->stream, x.pdense, I, K, x.kthv, x.Eu, x.Bs, x.Cs, x.Di,
                     x.prm, x.gcnt);
  HNM_LAUNCH_CHECK();
  unsigned long long pc = 0;
  HNM_HIP_CHECK(hipMemcpyAsync(&pc, x.gcnt, 8, hipMemcpyDeviceToHost, ctx->stream));
  HNM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  // prune when a row would re-score at most 1/16 of the catalogue (re-scoring a candidate costs
  // several pairs of the exact tiled scan) and half its segments' capacity
  const int64_t limit = std::min<int64_t>(I / 16, (int64_t)sh.part.np * sh.capp / 2);
  *pruned = (int64_t)(pc / (unsigned long long)np_rows) <= limit;
  if (!*pruned) return HNM_OK;
  return ncf_cert_finish(ctx, w, t, B, mptr, midx, K, scratch, false, nullptr, 0, ov, oi, &dp,
                         ovf_rows, ovf_cnt);
}

hnm_status ncf_cert_debug(hnm_ctx* ctx, const hnm_ncf_weights* w, const NcfTabs& t, int64_t B,
                          void* scratch, float* approx, int64_t lda, float* bound,
                          const CertDeep* dp) {
  const int64_t I = w->num_items;
  const CertWs x = cert_plan(ctx, B, I, 1, scratch, false).ws;
  hnm_status st = cert_prepare(ctx, w, t, B, x, dp);
  if (st) return st;
  hipLaunchKernelGGL(cert_bound_kernel, dim3((unsigned)hnm_cdiv(B, 256)), dim3(256), 0, ctx->stream,
                     nullptr, nullptr, nullptr, 1, x.Au, x.prm, w->bp, B, nullptr, x.Eu);
  HNM_LAUNCH_CHECK();
  ScanArgs a = scan_args(x, B, dp != nullptr);
  a.I = I;
  a.dense = approx;
  a.dense2 = bound;
  a.ldo = lda;
  const int64_t ublocks = hnm_cdiv(B, 128);
  Partition part = choose_partition(I, ublocks, ctx->num_cus);
  a.ipp = part.ipp;
  a.NP = part.np;
  cert_launch_scan(ctx, SCAN_DEBUG, dim3((unsigned)part.np, (unsigned)ublocks), a);
  HNM_LAUNCH_CHECK();
  hipLaunchKernelGGL(cert_unscale_kernel, dim3((unsigned)hnm_cdiv(B * I, 256)), dim3(256), 0,
                     ctx->stream, approx, bound, lda, B, I, x.prm);
  HNM_LAUNCH_CHECK();
  return HNM_OK;
}
