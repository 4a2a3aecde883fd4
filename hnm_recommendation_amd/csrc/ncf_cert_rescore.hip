// Certified NeuralCF path, exact re-scoring: ncf_rescore_kernel (two-layer and deep chain) and
// its launcher.  Why the exact top-K of the scan's candidates is the exact top-K: the header of
// ncf_cert.hip.
#include <algorithm>

#include "ncf_cert_internal.h"

namespace {

// One wave per user: the exact fp32 score of each appended candidate, computed with the
// arithmetic of ncf32_kernel (same MFMA chain for layer 2, the GMF dot as the fma chain
// the f32 MFMA is bitwise equal to: tools/mfma_semantics_probe.hip (a)), then the exact
// (score desc, item asc) top-K.  Candidates sit in NP per-partition segments; a row with a
// flagged bound, an overflowing segment or fewer than K candidates is queued for the
// fallback.
// Four k steps' LDS operands per round trip in the layer-2 chain (round 4, under rocprofv3:
// 1 step 67.3 us, 2 steps 65.8-66.3, 4 steps 64.8 -- the operand waits are not what bounds it;
// the candidates' G / Q row gathers are).  RESCORE_PERSIST persistent workgroups per CU loop
// over rows (round 4, per-rank step of the sharded NCF, tools/rank_shape_probe.py: W = 1 2.172
// -> 2.147 ms, W = 8 (32,768 rows of ~1/8 the candidates) 2.381 -> 2.284 ms at 3 per CU, 6 per
// CU 2.151 / 2.315, against one workgroup per 4 rows): the W2 fragments are staged into LDS once
// per workgroup instead of once per 4 rows.
// DEEP (round 6): the candidates' exact scores by the deep tower's chain in ncf_deep_kernel's
// order (bitwise the exact deep kernels): layer 2 as an f32-MFMA chain FROM ZERO over k = 0..63
// (the staged A rows permuted so that accumulator register r of lane half h holds unit 2r + h),
// relu(acc + b2); layer 3 the same way over l = 2s + h with W3 row m on A row mfma32_row(m, 0)
// (so lane half 0 holds every unit of a candidate), relu(acc + b3); then in lane half 0 ONE fmaf
// chain over the GMF terms wp_j (g_u,j g_i,j) and the units' wp3_m z_m, + bp.
#ifndef RESCORE_PERSIST  // A/B builds only (tools/build_variant.sh)
#define RESCORE_PERSIST 3
#endif
#ifndef RESCORE_BEST_FIRST_AB
#define RESCORE_BEST_FIRST_AB 96
#endif
constexpr int RESCORE_BEST_FIRST = RESCORE_BEST_FIRST_AB;  // rows with more candidates score the best 64 first
template <bool DEEP>
__global__ __launch_bounds__(256, DEEP ? 2 : 3) void ncf_rescore_kernel(
    NcfTabs t, int mf, const float* __restrict__ W2, int h1, int h2, const float* __restrict__ b2,
    const float* __restrict__ wm, const float* __restrict__ bp, int64_t B,
    const int* __restrict__ flag, const int* __restrict__ cnt, const int32_t* __restrict__ buf,
    const float* __restrict__ bufd, const float* __restrict__ tau, const float* __restrict__ Eu,
    const float* __restrict__ Au, const float* __restrict__ Cu, const CertParams* __restrict__ prm,
    int NP, int capp, int K, int short_ok, float* __restrict__ ov, int64_t* __restrict__ oi,
    int32_t* __restrict__ ovf_rows, int32_t* __restrict__ ovf_cnt,
    unsigned long long* __restrict__ stats, CertDeep dp, int64_t num_users) {
  constexpr int KS = 32;
  __shared__ int stg[4][96];  // best-first: staged candidate ordinals
  // DEEP: layer-3 A fragments (16 k steps), b3, the prediction weights, each wave's user GMF row
  __shared__ float w3l[DEEP ? 16 * 64 : 1];
  __shared__ float b3l[16], wpl[DEEP ? 128 + 16 : 1];
  __shared__ float g0l[DEEP ? 4 : 1][64];
  __shared__ __attribute__((aligned(16))) float wgs[4][64];
  __shared__ __attribute__((aligned(16))) float b2l[32], wml[32];  // 0 beyond h2
  __shared__ int pref[4][CERT_MAX_NP + 1];
  // the layer-2 MFMA operands that do not change along a row -- W2 fragments (k step s, lane)
  // and the user's P row -- come from LDS (a broadcast read per MFMA) instead of 64 VGPRs, so
  // three waves per SIMD fit without spills
  __shared__ float w2l[KS * 64];
  __shared__ __attribute__((aligned(16))) float pl[4][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, j = lane & 31;
  if (tid < 32) {
    b2l[tid] = tid < h2 ? b2[tid] : 0.f;
    wml[tid] = !DEEP && tid < h2 ? wm[tid] : 0.f;  // (deep towers: wp holds mf + h3 only)
  }
  for (int e = tid; e < KS * 64; e += 256) {
    const int s = e >> 6, jj = e & 31, k = 2 * s + ((e >> 5) & 1);
    // DEEP: A row jj = mfma32_row(r, h) carries unit 2r + h
    const int row = DEEP ? 2 * ((jj & 3) + 4 * (jj >> 3)) + ((jj >> 2) & 1) : jj;
    w2l[e] = (row < h2 && k < h1) ? W2[row * h1 + k] : 0.f;
  }
  if constexpr (DEEP) {
    for (int e = tid; e < 16 * 64; e += 256) {
      const int s = e >> 6, jj = e & 31, k = 2 * s + ((e >> 5) & 1);
      const int m = (jj & 3) + 4 * (jj >> 3);  // rows mfma32_row(m, 0): lane half 0
      w3l[e] = (((jj >> 2) & 1) == 0 && m < dp.h3 && k < h2) ? dp.W3[m * h2 + k] : 0.f;
    }
    if (tid < 16) b3l[tid] = tid < dp.h3 ? dp.b3[tid] : 0.f;
    for (int e = tid; e < mf + dp.h3; e += 256) wpl[e] = dp.wp[e];
  }
  // persistent: the workgroup's shared operands loaded once, then each wave takes rows
  // b, b + 4 * gridDim.x, ... (its per-row LDS arrays are its own: no workgroup barrier inside)
  __syncthreads();
  for (int64_t b = (int64_t)blockIdx.x * 4 + wave; b < B; b += (int64_t)gridDim.x * 4) {
    wgs[wave][lane] = t.WGu[b * 64 + lane];  // pair-permuted wp*g_u
    pl[wave][lane] = t.Pu[b * 64 + lane];
    const int c = lane < NP ? cnt[b * NP + lane] : 0;
    if constexpr (DEEP) {
      const int64_t uid = dp.ids[b];  // out of range: flagged by the tables' gather
      g0l[wave][lane] =
          (lane < mf && uid >= 0 && uid < num_users) ? dp.gmf_user[uid * mf + lane] : 0.f;
    }
    // inclusive scan of the segment counts over the lanes
    int incl = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int v = __shfl_up(incl, o);
      if (lane >= o) incl += v;
    }
    if (lane == 0) pref[wave][0] = 0;
    if (lane < NP) pref[wave][lane + 1] = incl;
    // this wave's LDS writes, then its reads
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const int n = hnm_readlane_i(incl, 63);
    const bool over = __ballot(c > capp) != 0;
    // fewer than K candidates: the row's bound came from another item shard (short_ok: the
    // merge across shards completes the list) or the threshold is unusable -> fallback
    if (flag[b] || over || (n < K && !short_ok)) {
      if (lane == 0) {
        ovf_rows[atomicAdd(ovf_cnt, 1)] = (int32_t)b;
        if (stats) {
          atomicAdd(&stats[2], 1ull);
          if (b == 0) atomicAdd(&stats[0], (unsigned long long)B);
        }
      }
      continue;
    }
    const float bpv = bp[0];
    WaveTopK<1> L;
    L.init();
    const int32_t* rowbuf = buf + b * (int64_t)NP * capp;
    const float* rowd = bufd + b * (int64_t)NP * capp;
    // candidate g's slot in the row's segments (g < n): segment = last p with pref[p] <= g
    auto slot = [&](int g) {
      int lo = 0, hi = NP;
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (pref[wave][mid] <= g) lo = mid;
        else hi = mid;
      }
      return (int64_t)lo * capp + (g - pref[wave][lo]);
    };
    auto cand = [&](int g) { return g < n ? rowbuf[slot(g)] : 0; };
    // exact fp32 score of lane j's candidate (both halves of the wave), offered to the top-K
    auto score_deep = [&](int item, bool ok) {
      float q[KS];
      const float* qrow = t.Qi + (int64_t)item * 64 + h * KS;
#pragma unroll
      for (int s4 = 0; s4 < KS / 4; ++s4) {
        const float4 v = *reinterpret_cast<const float4*>(qrow + 4 * s4);
        q[4 * s4] = v.x; q[4 * s4 + 1] = v.y; q[4 * s4 + 2] = v.z; q[4 * s4 + 3] = v.w;
      }
      f32x16 acc = {};
      typedef __attribute__((address_space(3))) const float* lds_ptr;
#pragma unroll
      for (int s = 0; s < KS; s += 4) {
        float w[4], pv[4];
        asm volatile("ds_read_b32 %0, %8\n\tds_read_b32 %1, %9\n\tds_read_b32 %2, %10\n\t"
                     "ds_read_b32 %3, %11\n\tds_read_b32 %4, %12\n\tds_read_b32 %5, %13\n\t"
                     "ds_read_b32 %6, %14\n\tds_read_b32 %7, %15\n\ts_waitcnt lgkmcnt(0)"
                     : "=&v"(w[0]), "=&v"(w[1]), "=&v"(w[2]), "=&v"(w[3]),
                       "=&v"(pv[0]), "=&v"(pv[1]), "=&v"(pv[2]), "=&v"(pv[3])
                     : "v"((unsigned)(uintptr_t)(lds_ptr)&w2l[s * 64 + lane]),
                       "v"((unsigned)(uintptr_t)(lds_ptr)&w2l[(s + 1) * 64 + lane]),
                       "v"((unsigned)(uintptr_t)(lds_ptr)&w2l[(s + 2) * 64 + lane]),
                       "v"((unsigned)(uintptr_t)(lds_ptr)&w2l[(s + 3) * 64 + lane]),
                       "v"((unsigned)(uintptr_t)(lds_ptr)&pl[wave][h * KS + s]),
                       "v"((unsigned)(uintptr_t)(lds_ptr)&pl[wave][h * KS + s + 1]),
                       "v"((unsigned)(uintptr_t)(lds_ptr)&pl[wave][h * KS + s + 2]),
                       "v"((unsigned)(uintptr_t)(lds_ptr)&pl[wave][h * KS + s + 3]));
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = mfma32x32x2(w[e], fmaxf(pv[e] + q[s + e], 0.f), acc);
      }
      // layer 3: register s of half h is unit 2s + h, its relu(acc + b2) the k = 2s + h operand
      f32x16 a3 = {};
#pragma unroll
      for (int s = 0; s < 16; ++s)
        a3 = mfma32x32x2(w3l[s * 64 + lane], fmaxf(acc[s] + b2l[2 * s + h], 0.f), a3);
      float sc = 0.f;
      if (h == 0 && ok) {
        const float* grow = dp.gmf_item + (int64_t)item * mf;
        for (int j4 = 0; j4 < mf; j4 += 4) {
          const float4 gv = *reinterpret_cast<const float4*>(grow + j4);
          sc = fmaf(wpl[j4], g0l[wave][j4] * gv.x, sc);
          sc = fmaf(wpl[j4 + 1], g0l[wave][j4 + 1] * gv.y, sc);
          sc = fmaf(wpl[j4 + 2], g0l[wave][j4 + 2] * gv.z, sc);
          sc = fmaf(wpl[j4 + 3], g0l[wave][j4 + 3] * gv.w, sc);
        }
#pragma unroll
        for (int m = 0; m < 16; ++m)
          if (m < dp.h3) sc = fmaf(wpl[mf + m], fmaxf(a3[m] + b3l[m], 0.f), sc);
      }
      L.offer(sc + bp[0], item, ok && h == 0, K);
    };
    auto score_item = [&](int item, bool ok) {
      if constexpr (DEEP) {
        score_deep(item, ok);
        return;
      }
      // GMF: fma chain in the f32 MFMA's order (k = 2s, then 2s + 1) over all 64 k (zero
      // beyond mf, as the fp32 kernel's padded operands); loads in two batches of 8 float4
      // issued together (a runtime-bounded loop would wait on each load)
      float gm = 0.f;
      const float* grow = t.G + (int64_t)item * t.ldg;
      const int glast = (int)t.ldg - 4;
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        float4 gv[8];
#pragma unroll
        for (int q4 = 0; q4 < 8; ++q4)
          gv[q4] = *reinterpret_cast<const float4*>(grow + std::min(4 * (8 * half + q4), glast));
#pragma unroll
        for (int q4 = 0; q4 < 8; ++q4) {
          const int c4 = 8 * half + q4;
          const bool in = 4 * c4 < mf;
          // pair-permuted: wgs[2c4], wgs[2c4+1] = k 4c4, 4c4+2; wgs[32+2c4], [32+2c4+1] = 4c4+1, 4c4+3
          const float2 wv = *reinterpret_cast<const float2*>(&wgs[wave][2 * c4]);
          const float2 wv1 = *reinterpret_cast<const float2*>(&wgs[wave][KS + 2 * c4]);
          gm = fmaf(wv1.x, in ? gv[q4].y : 0.f, fmaf(wv.x, in ? gv[q4].x : 0.f, gm));
          gm = fmaf(wv1.y, in ? gv[q4].w : 0.f, fmaf(wv.y, in ? gv[q4].z : 0.f, gm));
        }
      }
      float q[KS];
      const float* qrow = t.Qi + (int64_t)item * 64 + h * KS;
#pragma unroll
      for (int s4 = 0; s4 < KS / 4; ++s4) {
        const float4 v = *reinterpret_cast<const float4*>(qrow + 4 * s4);
        q[4 * s4] = v.x; q[4 * s4 + 1] = v.y; q[4 * s4 + 2] = v.z; q[4 * s4 + 3] = v.w;
      }
      f32x16 acc;
      float wmr[16];
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {  // rows mfma32_row(4 r4 + e, h) = 8 r4 + 4 h + e
        const float4 bb = *reinterpret_cast<const float4*>(&b2l[8 * r4 + 4 * h]);
        const float4 ww = *reinterpret_cast<const float4*>(&wml[8 * r4 + 4 * h]);
        acc[4 * r4] = bb.x; acc[4 * r4 + 1] = bb.y; acc[4 * r4 + 2] = bb.z; acc[4 * r4 + 3] = bb.w;
        wmr[4 * r4] = ww.x; wmr[4 * r4 + 1] = ww.y; wmr[4 * r4 + 2] = ww.z; wmr[4 * r4 + 3] = ww.w;
      }
      typedef __attribute__((address_space(3))) const float* lds_ptr;
      // four k steps' operands per LDS round trip
#pragma unroll
      for (int s = 0; s < KS; s += 4) {
        float w[4], pv[4];
        asm volatile("ds_read_b32 %0, %8\n\tds_read_b32 %1, %9\n\tds_read_b32 %2, %10\n\t"
                     "ds_read_b32 %3, %11\n\tds_read_b32 %4, %12\n\tds_read_b32 %5, %13\n\t"
                     "ds_read_b32 %6, %14\n\tds_read_b32 %7, %15\n\ts_waitcnt lgkmcnt(0)"
                     : "=&v"(w[0]), "=&v"(w[1]), "=&v"(w[2]), "=&v"(w[3]),
                       "=&v"(pv[0]), "=&v"(pv[1]), "=&v"(pv[2]), "=&v"(pv[3])
                     : "v"((unsigned)(uintptr_t)(lds_ptr)&w2l[s * 64 + lane]),
                       "v"((unsigned)(uintptr_t)(lds_ptr)&w2l[(s + 1) * 64 + lane]),
                       "v"((unsigned)(uintptr_t)(lds_ptr)&w2l[(s + 2) * 64 + lane]),
                       "v"((unsigned)(uintptr_t)(lds_ptr)&w2l[(s + 3) * 64 + lane]),
                       "v"((unsigned)(uintptr_t)(lds_ptr)&pl[wave][h * KS + s]),
                       "v"((unsigned)(uintptr_t)(lds_ptr)&pl[wave][h * KS + s + 1]),
                       "v"((unsigned)(uintptr_t)(lds_ptr)&pl[wave][h * KS + s + 2]),
                       "v"((unsigned)(uintptr_t)(lds_ptr)&pl[wave][h * KS + s + 3]));
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = mfma32x32x2(w[e], fmaxf(pv[e] + q[s + e], 0.f), acc);
      }
      float m4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int r = 0; r < 16; ++r) m4[r & 3] = fmaf(fmaxf(acc[r], 0.f), wmr[r], m4[r & 3]);
      const float mlp = (m4[0] + m4[1]) + (m4[2] + m4[3]);
      const float tot = hnm_sum_halves(mlp + (h == 0 ? gm : 0.f));
      const float score = tot + bpv;
      L.offer(score, item, ok && h == 0, K);
    };
    // Best first (round 5), rows of more than RESCORE_BEST_FIRST candidates: the 64 with the best
    // scan test values are scored first; their K-th exact score thr lower-bounds the row's K-th,
    // so a remaining candidate is scored only if it would have passed the scan against thr -- its
    // test value against the threshold tau2 that cert_tau_kernel derives from thr, with twice that
    // kernel's guard (the extra rounding of d + tau).  Rows whose scan bound came from a poor
    // sample (user-specific best items: ~300 candidates a row) drop to about what a perfect
    // sample would leave (tools/ncf_bound_limit_probe.py).  Shorter rows: every candidate, in
    // order.  Candidates are staged 32 at a time (one scoring site: the kernel stays at 168 VGPRs).
    int* st = stg[wave];
    int ns = 0, nscored = 0;
    float v63 = 0.f, t2 = 0.f;
    int i63 = 0;
    bool usable = false;
    const float tb = tau[b];
    const bool bf = n > RESCORE_BEST_FIRST;
    int ti = HNM_SENTINEL_IDX;
    if (bf) {
      float tv = -__builtin_inff();
      for (int c0 = 0; c0 < n; c0 += 64) {  // the 64 best (test value desc, ordinal asc)
        const int g = c0 + lane;
        const float d = g < n ? rowd[slot(g)] : -__builtin_inff();
        float v1 = d != d ? __builtin_inff() : d;  // a NaN test value is scored first
        int i1 = g < n ? g : HNM_SENTINEL_IDX;
        // only a chunk holding an entry above the current 64th can change the 64 best
        const float c63 = hnm_readlane_f(tv, 63);
        const int c63i = hnm_readlane_i(ti, 63);
        if (__ballot(hnm_better(v1, i1, c63, c63i))) hnm_sort128(tv, ti, v1, i1);
      }
      v63 = hnm_readlane_f(tv, 63);
      i63 = hnm_readlane_i(ti, 63);
    }
    for (int phase = bf ? 0 : 2; phase < (bf ? 2 : 3); ++phase) {  // bf: 0, 1; else 2
      if (phase == 0) {  // the 64 best, already in ti (lane = rank)
        st[lane] = ti;
        ns = 64;
      }
      if (phase == 1) {
        const float thr = L.thr_v;  // 64 >= K items scored: a valid K-th
        const float unit = prm->unit;
        const float scale = unit * (prm->c0 + Au[b] + prm->Bmax + Cu[b] * prm->Dmax);
        t2 = (thr - bpv) * unit - Eu[b] - 2.f * 3.814697265625e-06f * scale;  // 2 x 2^-18
        t2 -= fabsf(t2) * 1.9073486328125e-06f;                                 // 2 x 2^-20
        usable = __builtin_isfinite(t2);
      }
      for (int c0 = 0; c0 < (phase == 0 ? 1 : n); c0 += 64) {
        if (phase != 0) {
          const int g = c0 + lane;
          bool keep = g < n;
          if (keep && phase == 1) {
            const float d = rowd[slot(g)];
            const bool top = !hnm_better(v63, i63, d != d ? __builtin_inff() : d, g);
            keep = !top && (!usable || !(d + tb < t2));
          }
          const uint64_t m = __ballot(keep);
          if (keep) st[ns + __popcll(m & ((1ull << lane) - 1))] = g;
          ns += __popcll(m);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const bool last = phase == 0 || c0 + 64 >= n;
        while (ns >= 32 || (last && ns > 0)) {
          const int nv = ns < 32 ? ns : 32;
          score_item(cand(st[j < nv ? j : 0]), j < nv);
          nscored += nv;
          const int rest = ns - nv;
          const int mv = lane < rest ? st[32 + lane] : 0;
          __builtin_amdgcn_wave_barrier();
          if (lane < rest) st[lane] = mv;
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          __builtin_amdgcn_wave_barrier();
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
          ns = rest;
        }
      }
    }
    if (stats && lane == 0) {
      atomicAdd(&stats[1], (unsigned long long)nscored);
      if (b == 0) atomicAdd(&stats[0], (unsigned long long)B);
    }
    L.store(ov ? ov + b * K : nullptr, oi + b * K, K);
  }
}

template <bool DEEP>
void launch_rescore(hnm_ctx* ctx, const hnm_ncf_weights* w, const NcfTabs& t, int64_t B,
                    const CertPlan& pl, int K, int short_ok, float* ov, int64_t* oi,
                    const CertDeep& dv) {
  const CertWs& x = pl.ws;
  const int64_t rgrid = std::min<int64_t>(hnm_cdiv(B, 4), (int64_t)RESCORE_PERSIST * ctx->num_cus);
  hipLaunchKernelGGL(ncf_rescore_kernel<DEEP>, dim3((unsigned)rgrid), dim3(256), 0, ctx->stream, t,
                     w->mf, w->w2, w->h1, w->h2, w->b2, w->wp + w->mf, w->bp, B, x.flag, x.cnt,
                     x.buf, x.bufd, x.tau, x.Eu, x.Au, x.Cu, x.prm, pl.sh.part.np, pl.sh.capp, K,
                     short_ok, ov, oi, x.ovf_rows, x.ovf_cnt,
                     ctx->stats_on ? ctx->stats_dev : nullptr, dv, w->num_users);
}

}  // namespace

void cert_launch_rescore(hnm_ctx* ctx, const hnm_ncf_weights* w, const NcfTabs& t, int64_t B,
                         const CertPlan& pl, int K, int short_ok, float* ov, int64_t* oi,
                         const CertDeep* dp) {
  if (dp) launch_rescore<true>(ctx, w, t, B, pl, K, short_ok, ov, oi, *dp);
  else launch_rescore<false>(ctx, w, t, B, pl, K, short_ok, ov, oi, CertDeep{});
}
