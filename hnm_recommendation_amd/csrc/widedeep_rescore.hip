// Wide&Deep certified top-K, after the scan (widedeep_cert.hip): the cascade that refines the
// scan's survivors with a three-pass split-f16 tile, best first, and re-scores what is left with
// wd_tile_fp32, the exact kernel's own arithmetic (widedeep_internal.h) -- so the certified
// path's outputs are bitwise those of the exact path.
#include <algorithm>

#include "widedeep_internal.h"

// Refined certified score of the re-scoring cascade (round 5): one user against the 32 gathered
// items of a tile (lane (j, h): item j), both layers as three split-f16 MFMA passes
// (W_hi x_hi + W_hi x_lo + W_lo x_hi; the dropped W_lo x_lo is 2^-22 relative), fp32
// accumulation -- the configuration the header's g1 / g2 constants were derived for, so the
// bound there holds with the PLAIN v1 / v2 (the scan's one-pass vectors carry dropped-pass
// terms): |approx - exact| <= e.  About 3/16 of the fp32 tile's matrix-pipe time.  Layer 2 in
// RB2 / G2 passes over k of G2 row blocks each (the x operands re-formed per pass), each pass's
// x2 feeding layer 3 at once: G2 = 4 keeps the tile within 256 registers (two waves a SIMD).
//   psr: the user's layer-1 row scaled by s1, offset 8 h (LDS); qrow: item j's row + 8 h
//   (global); v1s / b2l / v2l / b3l / wdl: LDS copies.  Returns (score - cu - wI) in every lane
//   and the bound's three dot products (real units, summed over the halves).
template <int RB2, int OB, int G2>
__device__ __forceinline__ void wd_tile_f16x3(const float* __restrict__ psr,
                                              const float* __restrict__ qrow, int KB,
                                              __amdgpu_buffer_rsrc_t w2rs,
                                              __amdgpu_buffer_rsrc_t w3rs,
                                              const float* __restrict__ v1s,
                                              const float* __restrict__ b2l,
                                              const float* __restrict__ v2l,
                                              const float* __restrict__ b3l,
                                              const float* __restrict__ wdl, float s1, float c2,
                                              float c3, float inv_s2, int lane, int h,
                                              float& fv, float& b1, float& b2, float& b3) {
  constexpr int NOB = OB > 0 ? OB : 1;
  f32x16 acc3[NOB];
#pragma unroll
  for (int ob = 0; ob < NOB; ++ob)
    acc3[ob] = f32x16{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float bx1 = 0.f, bx2 = 0.f, fin = 0.f, bx3 = 0.f;
  auto qload = [&](int kb, float4 (&q)[2]) {
    q[0] = *reinterpret_cast<const float4*>(qrow + 16 * kb);
    q[1] = *reinterpret_cast<const float4*>(qrow + 16 * kb + 4);
  };
#pragma unroll 1
  for (int g = 0; g < RB2 / G2; ++g) {
    f32x16 acc2[G2];
#pragma unroll
    for (int gi = 0; gi < G2; ++gi)
      acc2[gi] = f32x16{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    // item rows two k steps ahead (gathered rows); each weight fragment is reloaded for step
    // kb + 1 right after step kb's MFMAs read it (one register set, a whole step of lead)
    wfr w[G2][2];
#pragma unroll
    for (int gi = 0; gi < G2; ++gi)
#pragma unroll
      for (int hl = 0; hl < 2; ++hl) w[gi][hl] = wd_frag(w2rs, lane, ((g * G2 + gi) * KB * 2 + hl) * 1024);
    auto step = [&](int kb, const float4 (&q)[2]) {
      const float4 p0 = *reinterpret_cast<const float4*>(psr + 16 * kb);
      const float4 p1 = *reinterpret_cast<const float4*>(psr + 16 * kb + 4);
      const float pv[8] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w};
      const float qv[8] = {q[0].x, q[0].y, q[0].z, q[0].w, q[1].x, q[1].y, q[1].z, q[1].w};
      float x[8];
#pragma unroll
      for (int t = 0; t < 8; ++t) x[t] = fmaxf(fmaf(qv[t], s1, pv[t]), 0.f);  // s1 x1 exactly
      if (g == 0) {  // the layer-2 bound term, once
        const float4 w0 = *reinterpret_cast<const float4*>(v1s + 16 * kb + 8 * h);
        const float4 w1 = *reinterpret_cast<const float4*>(v1s + 16 * kb + 8 * h + 4);
        const float vv[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
#pragma unroll
        for (int t = 0; t < 8; ++t) bx1 = fmaf(vv[t], x[t], bx1);
      }
      wh8 xh, xl;
      wd_split8(x, xh, xl);
      const int kn = kb + 1 < KB ? kb + 1 : kb;
#pragma unroll
      for (int gi = 0; gi < G2; ++gi) {
        acc2[gi] = wd_mfma16(wd_h(w[gi][0]), xh, acc2[gi]);
        acc2[gi] = wd_mfma16(wd_h(w[gi][0]), xl, acc2[gi]);
        acc2[gi] = wd_mfma16(wd_h(w[gi][1]), xh, acc2[gi]);
#pragma unroll
        for (int hl = 0; hl < 2; ++hl)
          w[gi][hl] = wd_frag(w2rs, lane, (((g * G2 + gi) * KB + kn) * 2 + hl) * 1024);
      }
    };
    {
      // item rows QD k steps ahead: four register sets in rotation (the gathered rows come from
      // MALL / HBM; two steps of lead left the MFMAs waiting on them)
      constexpr int QD = 4;
      float4 qr[QD][2];
      auto kc = [&](int k) { return k < KB ? k : KB - 1; };
#pragma unroll
      for (int d = 0; d < QD; ++d) qload(kc(d), qr[d]);
      int kb = 0;
      for (; kb + QD <= KB; kb += QD) {
#pragma unroll
        for (int d = 0; d < QD; ++d) {
          step(kb + d, qr[d]);
          qload(kc(kb + d + QD), qr[d]);
        }
      }
#pragma unroll
      for (int d = 0; d < QD; ++d)
        if (kb + d < KB) step(kb + d, qr[d]);
    }
    // x2 = relu(D2 + b2') in s2 units, its bound term, then its layer-3 passes (or the final
    // dot of a two-layer tower).  Layer-3 fragments run W3D kb3 steps ahead in a ring of
    // W3D + 1 register sets (the steps are unrolled: compile-time slots); bias / bound rows are
    // read as float4 (rows 8 r4 + 4 h + 0..3 of a row block hold registers 4 r4 .. 4 r4 + 3).
    constexpr int W3D = 2, NK3 = 2 * G2;
    wfr w3b[W3D + 1][NOB][2];
    auto w3load = [&](int k3) {  // k3: this pass's kb3 step (2 gi + half2)
      const int kb3 = 2 * g * G2 + k3;
#pragma unroll
      for (int ob = 0; ob < NOB; ++ob)
#pragma unroll
        for (int hl = 0; hl < 2; ++hl)
          w3b[k3 % (W3D + 1)][ob][hl] = wd_frag(w3rs, lane, ((ob * 2 * RB2 + kb3) * 2 + hl) * 1024);
    };
    if constexpr (OB > 0) {
#pragma unroll
      for (int k3 = 0; k3 < W3D && k3 < NK3; ++k3) w3load(k3);
    }
#pragma unroll
    for (int gi = 0; gi < G2; ++gi) {
      const int rb = g * G2 + gi;
      float y[16];
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        const float4 bb = *reinterpret_cast<const float4*>(b2l + rb * 32 + 8 * r4 + 4 * h);
        const float4 vq = *reinterpret_cast<const float4*>(v2l + rb * 32 + 8 * r4 + 4 * h);
        const float bq[4] = {bb.x, bb.y, bb.z, bb.w}, vv[4] = {vq.x, vq.y, vq.z, vq.w};
        float wq[4] = {0.f, 0.f, 0.f, 0.f};
        if (OB == 0) {
          const float4 w4 = *reinterpret_cast<const float4*>(wdl + rb * 32 + 8 * r4 + 4 * h);
          wq[0] = w4.x; wq[1] = w4.y; wq[2] = w4.z; wq[3] = w4.w;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 4 * r4 + e;
          y[r] = fmaxf(fmaf(acc2[gi][r], c2, bq[e]), 0.f);
          bx2 = fmaf(vv[e], y[r], bx2);
          if (OB == 0) fin = fmaf(y[r], wq[e], fin);
        }
      }
      if constexpr (OB > 0) {
#pragma unroll
        for (int half2 = 0; half2 < 2; ++half2) {
          const int k3 = 2 * gi + half2;
          if (k3 + W3D < NK3) w3load(k3 + W3D);
          wh8 yh, yl;
          wd_split8(&y[8 * half2], yh, yl);
#pragma unroll
          for (int ob = 0; ob < NOB; ++ob) {
            const wh8 bh = wd_h(w3b[k3 % (W3D + 1)][ob][0]);
            const wh8 bl = wd_h(w3b[k3 % (W3D + 1)][ob][1]);
            acc3[ob] = wd_mfma16(bh, yh, acc3[ob]);
            acc3[ob] = wd_mfma16(bh, yl, acc3[ob]);
            acc3[ob] = wd_mfma16(bl, yh, acc3[ob]);
          }
        }
      }
    }
  }
  if constexpr (OB > 0) {
    float fp[4] = {0.f, 0.f, 0.f, 0.f}, bp[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ob = 0; ob < NOB; ++ob)
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        const float4 b3 = *reinterpret_cast<const float4*>(b3l + ob * 32 + 8 * r4 + 4 * h);
        const float4 w4 = *reinterpret_cast<const float4*>(wdl + ob * 32 + 8 * r4 + 4 * h);
        const float bq[4] = {b3.x, b3.y, b3.z, b3.w}, wq[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float z = fmaxf(fmaf(acc3[ob][4 * r4 + e], c3, bq[e]), 0.f);
          fp[e] = fmaf(z, wq[e], fp[e]);
          bp[e] = fmaf(fabsf(wq[e]), z, bp[e]);
        }
      }
    fin = (fp[0] + fp[1]) + (fp[2] + fp[3]);
    bx3 = (bp[0] + bp[1]) + (bp[2] + bp[3]);
  } else {
    fin *= inv_s2;
  }
  fv = hnm_sum_halves(fin);
  b1 = hnm_sum_halves(bx1) / s1;
  b2 = hnm_sum_halves(bx2) * inv_s2;
  b3 = hnm_sum_halves(bx3);
}

// The re-scoring cascade (round 5; round 4 sent all ~1,145 scan survivors a row through the
// fp32 tile: 15.7 ms a batch):
//   wdc_collect_kernel  one wave per row: fallback rows queued; the row's scan survivors
//                       (ub >= L_u) compacted to the front of its segment area, their count;
//   wdc_best_kernel     (round 6) one wave per row: the refining list's first phase -- the
//                       WDC_BF survivors of best scan upper bound (rows of <= WDC_BF_MIN: all);
//   wdc_tiles_kernel    exclusive prefix of the rows' 32-item refining tiles (one block);
//   wdc_refine_kernel   a fixed grid, each wave a contiguous run of tiles (balanced whatever
//                       the rows' survivor counts): wd_tile_f16x3 -> refined bounds
//                       lb2 <= exact <= ub2 per listed survivor;
//   wdc_filter_kernel   (round 6) one wave per row: the remaining survivors whose scan upper
//                       bound reaches the first phase's K-th refined lower bound appended to
//                       the list, then tiles + refine again over them (~1,145 -> ~570 refined
//                       a row at configs[3]: profiles/r10c_wd_best_first_probe.txt);
//   wdc_rescore_kernel  one wave per row: L2 = the K-th best lb2 (a lower bound of the row's
//                       exact K-th best), then the survivors with ub2 >= max(L2, L_u) -- every
//                       item that can be in the top-K -- through wd_tile_fp32, the exact
//                       kernel's arithmetic, into a wave top-K: bitwise the exact path's output.
__global__ __launch_bounds__(256) void wdc_collect_kernel(WdRescoreArgs R) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= R.B) return;
  const float Lu = R.Lk[b * R.K + R.K - 1];
  bool fb = R.prm->bad || !(Lu > -__builtin_inff());
  for (int p = 0; p < R.NP; ++p) fb |= R.cnt[b * R.NP + p] > R.cap;
  if (fb) {
    if (lane == 0) {
      R.ns[b] = -1;
      R.fbrows[atomicAdd(R.nfb, 1)] = (int32_t)b;
      if (R.stats) {
        atomicAdd(R.stats + 0, 1ull);
        atomicAdd(R.stats + 2, 1ull);
      }
    }
    return;
  }
  // in place: the write position never passes the read position, and a chunk's loads are
  // issued before its stores
  const int64_t rowbase = b * R.rstride;
  int no = 0;
  for (int p = 0; p < R.NP; ++p) {
    const int n = R.cnt[b * R.NP + p];
    const int64_t base = rowbase + (int64_t)p * R.cap;
    for (int c0 = 0; c0 < n; c0 += 64) {
      const int e = c0 + lane;
      const bool in = e < n;
      const int32_t it = in ? R.segi[base + e] : 0;
      const float u = in ? R.segu[base + e] : 0.f;
      const bool ok = in && u >= Lu;
      const uint64_t m = __ballot(ok);
      if (ok) {
        const int64_t o = rowbase + no + __popcll(m & ((1ull << lane) - 1));
        R.segi[o] = it;
        R.segs[o] = u;  // a separate array: the scan's upper bounds are read in place above
      }
      no += __popcll(m);
    }
  }
  if (lane == 0) R.ns[b] = no;
}

__global__ __launch_bounds__(1024) void wdc_tiles_kernel(const int* __restrict__ ns,
                                                         const int* __restrict__ start, int64_t B,
                                                         int* __restrict__ toff) {
  __shared__ int wsum[16];
  __shared__ int carry;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) carry = 0;
  __syncthreads();
  for (int64_t b0 = 0; b0 < B; b0 += 1024) {
    const int64_t b = b0 + tid;
    const int t = b < B ? (int)hnm_cdiv(std::max(ns[b] - (start ? start[b] : 0), 0), TILE) : 0;
    int incl = t;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int v = __shfl_up(incl, o);
      if (lane >= o) incl += v;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int before = carry;
    for (int w = 0; w < wave; ++w) before += wsum[w];
    if (b < B) toff[b] = before + incl - t;
    __syncthreads();
    if (tid == 1023) carry = before + incl;
    __syncthreads();
  }
  if (tid == 0) toff[B] = carry;
}

template <int RB2, int OB>
__global__ __launch_bounds__(256, 1) void wdc_refine_kernel(WdRescoreArgs R) {
  constexpr int NOB = OB > 0 ? OB : 1, NL = OB > 0 ? OB : RB2;
  constexpr int G2 = RB2;
  extern __shared__ __attribute__((aligned(16))) float wsm[];
  const int K1P = R.K1P, KB = K1P / 16;
  float* const v1s = wsm;                  // [K1P]
  float* const b2l = v1s + K1P;            // [RB2 * 32]
  float* const v2l = b2l + RB2 * 32;       // [RB2 * 32]
  float* const b3l = v2l + RB2 * 32;       // [NOB * 32]
  float* const wdl = b3l + NOB * 32;       // [NL * 32]
  float* const psm = wdl + NL * 32;        // [4][K1P] the wave's current user row, scaled by s1
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, j = lane & 31;
  for (int e = tid; e < K1P; e += 256) v1s[e] = R.v1p[e];
  for (int e = tid; e < RB2 * 32; e += 256) {
    b2l[e] = R.b2s[e];
    v2l[e] = R.v2p[e];
  }
  for (int e = tid; e < NOB * 32; e += 256) b3l[e] = OB > 0 ? R.b3p[e] : 0.f;
  for (int e = tid; e < NL * 32; e += 256) wdl[e] = R.wdp[e];
  __syncthreads();  // the only block-level barrier
  const WdCertParams& P = *R.prm;
  const float s1 = P.s1, c2 = P.c2, c3 = P.c3, inv_s2 = P.inv_s2;
  const float g1 = P.g1, g2 = P.g2, g3 = P.g3, g4 = P.g4, cbd = P.cb, absb = P.absb, rho = P.rho;
  const __amdgpu_buffer_rsrc_t w2rs =
      __builtin_amdgcn_make_buffer_rsrc((void*)R.W2hl, 0, RB2 * KB * 2 * 1024, 0x00020000);
  const __amdgpu_buffer_rsrc_t w3rs =
      __builtin_amdgcn_make_buffer_rsrc((void*)R.W3hl, 0, NOB * 2 * RB2 * 2 * 1024, 0x00020000);
  // this wave's tiles: a contiguous run of the T tiles (rows in order)
  const int64_t T = R.toff[R.B];
  const int64_t nw = (int64_t)gridDim.x * 4, w = (int64_t)blockIdx.x * 4 + wave;
  const int64_t t0 = T * w / nw, t1 = T * (w + 1) / nw;
  if (t0 >= t1) return;
  int64_t lo = 0, hi = R.B;  // the row holding tile t0: last b with toff[b] <= t0
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (R.toff[mid] <= t0) lo = mid;
    else hi = mid;
  }
  int64_t b = lo, cb = -1;
  float* const ps = psm + wave * K1P;
  float cub = 0.f;
  for (int64_t t = t0; t < t1; ++t) {
    while (R.toff[b + 1] <= t) ++b;  // rows without tiles are skipped
    if (b != cb) {
      __builtin_amdgcn_wave_barrier();
      for (int e = lane; e < K1P; e += 64) ps[e] = R.Pu[b * K1P + e] * s1;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      cub = R.cu[b];
      cb = b;
    }
    const int k = (int)(t - R.toff[b]);
    const int st = R.rstart ? R.rstart[b] : 0;
    const int nv = std::min(TILE, R.ns[b] - st - TILE * k);
    const int64_t at = b * R.rstride + st + (int64_t)TILE * k;
    const bool ivalid = lane < 32 && j < nv;
    const int it = R.segi[at + (j < nv ? j : 0)];
    float fv, b1, b2, b3;
    wd_tile_f16x3<RB2, OB, G2>(ps + 8 * h, R.Qi + (int64_t)it * K1P + 8 * h, KB, w2rs, w3rs, v1s,
                               b2l, v2l, b3l, wdl, s1, c2, c3, inv_s2, lane, h, fv, b1, b2, b3);
    const float wi = R.wI[it];
    const float score = fv + cub + wi;
    const float e = rho * (g1 * b1 + g2 * b2 + g3 * b3 +
                           g4 * (fabsf(fv) + fabsf(cub) + fabsf(wi)) + cbd) + absb;
    if (ivalid) {
      if (R.dbg_a) {
        R.dbg_a[b * R.lda + it] = score;
        R.dbg_e[b * R.lda + it] = e;
      } else {
        R.segl[at + j] = score - e;
        R.segu[at + j] = score + e;
      }
    }
  }
}

// Best-first refining (round 6).  A row of more than WDC_BF_MIN survivors
// refines its WDC_BF survivors of best scan upper bound first (wdc_best_kernel); their K-th best
// refined lower bound L2' is a certified lower bound of the row's exact K-th, so a remaining
// survivor is refined only if its scan upper bound reaches max(L2', L_u) (wdc_filter_kernel):
// otherwise exact <= scan ub < L2' <= the exact K-th, and it cannot be in the top-K.  The rows'
// refining lists (cli: the first phase, then the filtered rest) replace the survivor lists in
// the refining stage and in wdc_rescore_kernel, whose output is unchanged (bitwise the exact
// path).  Rows of at most WDC_BF_MIN survivors refine them all in the first phase.
constexpr int WDC_BF = 64;
constexpr int WDC_BF_MIN = 96;

// one wave per row: cli[0, nA) = the first phase's items (the WDC_BF best by (scan ub desc,
// survivor position asc), or every survivor), tv / tg = the WDC_BF-th (ub, position)
__global__ __launch_bounds__(256) void wdc_best_kernel(WdRescoreArgs R, int32_t* __restrict__ cli,
                                                       int* __restrict__ nA,
                                                       float* __restrict__ tv,
                                                       int* __restrict__ tg) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= R.B) return;
  const int ns = R.ns[b];
  const int64_t rowbase = b * R.rstride;
  if (ns <= WDC_BF_MIN) {  // incl. the exact kernel's rows (-1)
    for (int e = lane; e < ns; e += 64) cli[rowbase + e] = R.segi[rowbase + e];
    if (lane == 0) nA[b] = ns;
    return;
  }
  float v0 = -__builtin_inff();
  int i0 = HNM_SENTINEL_IDX;
  for (int c0 = 0; c0 < ns; c0 += 64) {  // running WDC_BF best; survivors' ubs are finite
    const int g = c0 + lane;
    float v1 = g < ns ? R.segs[rowbase + g] : -__builtin_inff();
    int i1 = g < ns ? g : HNM_SENTINEL_IDX;
    const float c63 = hnm_readlane_f(v0, 63);
    const int c63i = hnm_readlane_i(i0, 63);
    if (__ballot(hnm_better(v1, i1, c63, c63i))) hnm_sort128(v0, i0, v1, i1);
  }
  cli[rowbase + lane] = R.segi[rowbase + i0];
  if (lane == 63) {
    tv[b] = v0;
    tg[b] = i0;
  }
  if (lane == 0) nA[b] = WDC_BF;
}

// one wave per row (after the first phase's refining): L2' from the first phase's refined lower
// bounds; the remaining survivors with scan ub >= max(L2', L_u) appended to cli; ns = the list's
// final length
__global__ __launch_bounds__(256) void wdc_filter_kernel(WdRescoreArgs R, int32_t* __restrict__ cli,
                                                         const float* __restrict__ tv,
                                                         const int* __restrict__ tg) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= R.B) return;
  const int ns = R.ns[b];
  if (ns <= WDC_BF_MIN) return;  // single phase (or the exact kernel's row): the list is complete
  if (R.stats && lane == 0) atomicAdd(R.stats + 6, 1ull);  // rows that run the second phase
  const int K = R.K;
  const int64_t rowbase = b * R.rstride;
  WaveTopK<1> T2;  // K <= 64 = WDC_BF distinct items
  T2.init();
  T2.offer(R.segl[rowbase + lane], cli[rowbase + lane], true, K);
  const float thr = fmaxf(T2.thr_v, R.Lk[b * K + K - 1]);
  const float v64 = tv[b];
  const int g64 = tg[b];
  int no = WDC_BF;
  for (int c0 = 0; c0 < ns; c0 += 64) {
    const int g = c0 + lane;
    const bool in = g < ns;
    const float u = in ? R.segs[rowbase + g] : -__builtin_inff();
    const bool first = u > v64 || (u == v64 && g <= g64);  // refined in the first phase
    const bool keep = in && !first && u >= thr;
    const uint64_t m = __ballot(keep);
    if (keep) cli[rowbase + no + __popcll(m & ((1ull << lane) - 1))] = R.segi[rowbase + g];
    no += __popcll(m);
  }
  if (lane == 0) R.ns[b] = no;
}

template <int RB2, int OB>
__global__ __launch_bounds__(256, 1) void wdc_rescore_kernel(WdRescoreArgs R) {
  __shared__ int stage[4][96];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, j = lane & 31;
  const int64_t b = (int64_t)blockIdx.x * 4 + wave;
  if (b >= R.B) return;  // no block-level barriers below
  const int ns = R.ns[b];
  if (ns < 0) return;  // queued for the exact kernel by wdc_collect
  const int K = R.K;
  const float Lu = R.Lk[b * K + K - 1];
  const int64_t rowbase = b * R.rstride;
  // L2: the K-th best refined lower bound (K distinct items)
  WaveTopK<1> T2;
  T2.init();
  for (int c0 = 0; c0 < ns; c0 += 64) {
    const int e = c0 + lane;
    const bool in = e < ns;
    T2.offer(in ? R.segl[rowbase + e] : -__builtin_inff(), in ? R.segi[rowbase + e] : 0, in, K);
  }
  const float thr = fmaxf(T2.thr_v, Lu);
  const int KS1 = R.K1P / 2, S4 = R.K1P / 8;
  const float cub = R.cu[b];
  const float* prow = R.Pu + b * R.K1P + h * KS1;
  int* st = stage[wave];
  WaveTopK<1> T;
  T.init();
  int nsurv = 0, nst = 0;
  auto run_tile = [&](int nv) {
    const int it = st[j < nv ? j : 0];
    const float* qrow = R.Qi + (int64_t)it * R.K1P + h * KS1;
    float fin = wd_tile_fp32<RB2, OB>(prow, qrow, S4, R.W2f, R.W3f, R.b2p, R.b3p, R.wdp, lane, h);
    fin += __shfl_xor(fin, 32);
    const bool ivalid = lane < 32 && j < nv;
    const float score = fin + cub + (ivalid ? R.wI[it] : 0.f);
    T.offer(score, it, ivalid, K);
  };
  for (int c0 = 0; c0 < ns; c0 += 64) {
    const int e = c0 + lane;
    const bool ok = e < ns && R.segu[rowbase + e] >= thr;
    const uint64_t m = __ballot(ok);
    if (ok) st[nst + __popcll(m & ((1ull << lane) - 1))] = R.segi[rowbase + e];
    nst += __popcll(m);
    nsurv += __popcll(m);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    while (nst >= 32) {
      run_tile(32);
      const int rest = nst - 32;
      const int mv = lane < rest ? st[32 + lane] : 0;
      __builtin_amdgcn_wave_barrier();
      if (lane < rest) st[lane] = mv;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      nst = rest;
    }
  }
  if (nst > 0) run_tile(nst);
  T.store(R.ov + b * K, R.oi + b * K, K);
  if (R.stats && lane == 0) {
    atomicAdd(R.stats + 0, 1ull);
    atomicAdd(R.stats + 1, (unsigned long long)nsurv);
  }
}

// out rows <- the fallback's compact rows
__global__ void wdc_scatter_kernel(const float* __restrict__ cv, const int64_t* __restrict__ ci,
                                   const int32_t* __restrict__ rows, int n, int K,
                                   float* __restrict__ ov, int64_t* __restrict__ oi) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n * K) return;
  const int r = e / K, s = e % K;
  const int64_t b = rows[r];
  if (ov) ov[b * K + s] = cv[e];
  oi[b * K + s] = ci[e];
}

template <int RB2, int OB>
static void wdc_launch_refine(hnm_ctx* ctx, const WdRescoreArgs& r) {
  constexpr int NOB = OB > 0 ? OB : 1, NL = OB > 0 ? OB : RB2;
  hipLaunchKernelGGL(wdc_tiles_kernel, dim3(1), dim3(1024), 0, ctx->stream, r.ns, r.rstart, r.B,
                     r.toff);
  const size_t lds = (size_t)(5 * r.K1P + 2 * RB2 * 32 + NOB * 32 + NL * 32) * 4;
  auto kern = wdc_refine_kernel<RB2, OB>;
  (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(kern, dim3(ctx->num_cus), dim3(256), lds, ctx->stream, r);
}

struct WdcBestFirst {
  int32_t* cli;  // [B, rstride] the rows' refining lists
  int* nA;       // [B] first-phase length
  float* tv;     // [B] the first phase's last (scan ub, position)
  int* tg;
};

template <int RB2, int OB>
static void wdc_launch_rescore(hnm_ctx* ctx, dim3 grid, const WdRescoreArgs& r,
                               const WdcBestFirst& bf) {
  hipStream_t s = ctx->stream;
  hipLaunchKernelGGL(wdc_collect_kernel, grid, dim3(256), 0, s, r);
  hipLaunchKernelGGL(wdc_best_kernel, grid, dim3(256), 0, s, r, bf.cli, bf.nA, bf.tv, bf.tg);
  WdRescoreArgs q = r;  // the refining lists replace the survivor lists from here on
  q.segi = bf.cli;
  WdRescoreArgs qa = q;  // first phase: cli[0, nA)
  qa.ns = bf.nA;
  qa.rstart = nullptr;
  wdc_launch_refine<RB2, OB>(ctx, qa);
  hipLaunchKernelGGL(wdc_filter_kernel, grid, dim3(256), 0, s, r, bf.cli, bf.tv, bf.tg);
  WdRescoreArgs qb = q;  // second phase: cli[nA, ns)
  qb.rstart = bf.nA;
  wdc_launch_refine<RB2, OB>(ctx, qb);
  hipLaunchKernelGGL((wdc_rescore_kernel<RB2, OB>), grid, dim3(256), 0, s, q);
}

// the call's tables for the cascade's kernels; the lists they work on are the caller's to fill in
static WdRescoreArgs wdc_rescore_args(const hnm_widedeep_weights* w, const WdSetup& S, int64_t B,
                                      const WdcWs& c) {
  WdRescoreArgs r{};
  r.Pu = S.Pu;
  r.Qi = S.Qi;
  r.K1P = S.K1P;
  r.W2f = S.pr.W2f;
  r.W3f = S.pr.W3f;
  r.b2p = S.pr.b2p;
  r.b3p = S.pr.b3p;
  r.wdp = S.pr.wdp;
  r.cu = S.cu;
  r.wI = S.wI;
  r.prm = c.prm;
  r.B = B;
  r.W2hl = c.W2hl;
  r.W3hl = c.W3hl;
  r.v1p = c.v1o;
  r.v2p = c.v2o;
  r.b2s = c.b2s;
  return r;
}

hnm_status wdc_topk(hnm_ctx* ctx, const hnm_widedeep_weights* w, const WdSetup& S, int64_t B,
                    const int64_t* mptr, const int32_t* midx, int K, const WdcWs& c, float* ov,
                    int64_t* oi) {
  hnm_status st = wdc_prepare(ctx, w, S, B, c);
  if (st) return st;
  st = wdc_scan(ctx, w, S, B, mptr, midx, K, c, WDC_THRESH, nullptr, nullptr, 0);
  if (st) return st;
  st = hnm_topk_merge_i32(ctx, c.lbv, c.lbi, B, 1, 0, c.np * K, (int)(c.np * K), K, c.Lv, c.Li);
  if (st) return st;
  hipStream_t s = ctx->stream;
  HNM_HIP_CHECK(hipMemsetAsync(c.nfb, 0, sizeof(int), s));
  const WdPrep& pr = S.pr;
  WdRescoreArgs r = wdc_rescore_args(w, S, B, c);
  r.NP = (int)c.np;
  r.K = K;
  r.cap = c.cap;
  r.Lk = c.Lv;
  r.segi = c.segi;
  r.segu = c.segu;
  r.cnt = c.cnt;
  r.fbrows = c.fbrows;
  r.nfb = c.nfb;
  r.ov = ov;
  r.oi = oi;
  r.stats = ctx->stats_on ? ctx->stats_dev : nullptr;
  r.segl = c.segl;
  r.rstride = c.np * (int64_t)c.cap;
  r.ns = c.ns;
  r.toff = c.toff;
  r.segs = c.segs;
  const WdcBestFirst bf = {c.cli, c.nA, c.tv, c.tg};
  dim3 grid((unsigned)hnm_cdiv(B, 4));
  if (!wd_dispatch<true>(pr.RB2, pr.OB, [&](auto R, auto O) {
        wdc_launch_rescore<R(), O()>(ctx, grid, r, bf);
      }))
    return wd_not_instantiated(pr);
  HNM_LAUNCH_CHECK();
  // fallback rows: the count comes back to the host (a W&D call is long; one sync is noise)
  int nfb = 0;
  HNM_HIP_CHECK(hipMemcpyAsync(&nfb, c.nfb, sizeof(int), hipMemcpyDeviceToHost, s));
  HNM_HIP_CHECK(hipStreamSynchronize(s));
  if (nfb > 0) {
    st = wd_exact(ctx, w, S, nfb, mptr, midx, K, c.fbrows, c.fcv, c.fci, c.fov, c.foi, nullptr,
                  0, false);
    if (st) return st;
    hipLaunchKernelGGL(wdc_scatter_kernel, dim3((unsigned)hnm_cdiv((int64_t)nfb * K, 256)),
                       dim3(256), 0, s, c.fov, c.foi, c.fbrows, nfb, K, ov, oi);
    HNM_LAUNCH_CHECK();
  }
  return HNM_OK;
}

// every row's item list = the whole catalogue (the refine stage's debug input)
__global__ void wdc_debug_rows_kernel(int32_t* __restrict__ segi, int* __restrict__ ns, int64_t B,
                                      int64_t I) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e < B * I) segi[e] = (int32_t)(e % I);
  if (e < B) ns[e] = (int)I;
}

extern "C" hnm_status hnm_widedeep_refine_debug_ex_f32(
    hnm_ctx* ctx, const hnm_widedeep_weights* w, const int64_t* user_ids, int64_t B,
    const float* user_features, float* approx, int64_t lda, float* bound,
    const hnm_widedeep_item_features* itf, const float* item_features, int64_t ldf) {
  HNM_CTX_DEVICE(ctx);
  HNM_REQUIRE(ctx && user_ids && approx && bound && w && lda >= w->num_items, HNM_EINVAL,
              "widedeep_refine_debug: bad argument");
  WdItemFeat F;
  F.itf = itf;
  F.f = item_features;
  F.ldf = ldf;
  WdSetup S;
  hnm_status st = wd_shape(w, &S.pr, F);
  if (st) return st;
  HNM_REQUIRE(wdc_eligible(ctx, S.pr, w->num_items, 1, true), HNM_EUNSUPPORTED,
              "widedeep_refine_debug: tower shape not covered by the certified scan");
  if (B <= 0) return HNM_OK;
  const int64_t I = w->num_items;
  HNM_REQUIRE(B * I < ((int64_t)1 << 31), HNM_EINVAL, "widedeep_refine_debug: B * I >= 2^31");
  const size_t cb = wdc_carve(ctx, S.pr, B, I, 1, nullptr, nullptr);
  const size_t lb = hnm_align((size_t)B * I * 4) + hnm_align((size_t)B * 4) + hnm_align((size_t)(B + 1) * 4);
  st = wd_setup(ctx, w, user_ids, B, user_features, cb + lb, &S, F);
  if (st) return st;
  WdcWs c;
  wdc_carve(ctx, S.pr, B, I, 1, S.extra, &c);
  st = wdc_prepare(ctx, w, S, B, c);
  if (st) return st;
  char* x = (char*)S.extra + cb;
  int32_t* segi = (int32_t*)x;
  int* ns = (int*)(x + hnm_align((size_t)B * I * 4));
  int* toff = (int*)(x + hnm_align((size_t)B * I * 4) + hnm_align((size_t)B * 4));
  hipLaunchKernelGGL(wdc_debug_rows_kernel, dim3((unsigned)hnm_cdiv(B * I, 256)), dim3(256), 0,
                     ctx->stream, segi, ns, B, I);
  WdRescoreArgs r = wdc_rescore_args(w, S, B, c);
  r.segi = segi;
  r.ns = ns;
  r.toff = toff;
  r.rstride = I;
  r.dbg_a = approx;
  r.dbg_e = bound;
  r.lda = lda;
  if (!wd_dispatch<true>(S.pr.RB2, S.pr.OB,
                         [&](auto R, auto O) { wdc_launch_refine<R(), O()>(ctx, r); }))
    return wd_not_instantiated(S.pr);
  HNM_LAUNCH_CHECK();
  return HNM_OK;
}

extern "C" hnm_status hnm_widedeep_refine_debug_f32(hnm_ctx* ctx, const hnm_widedeep_weights* w,
                                                    const int64_t* user_ids, int64_t B,
                                                    const float* user_features, float* approx,
                                                    int64_t lda, float* bound) {
  return hnm_widedeep_refine_debug_ex_f32(ctx, w, user_ids, B, user_features, approx, lda, bound,
                                          nullptr, nullptr, 0);
}
