// Certified NeuralCF path, per-call parameters: the bound statistics (A_u, C_u, B_i, D_i and the
// maxima), the one-launch tables kernel that forms them with the tables, the scales and slack
// (CertParams) and the f16 operand tables of the scan.  Which kernels a call runs, and the bound
// (*) whose terms they compute: the header of ncf_cert.hip.
#include <algorithm>

#include "ncf_cert_internal.h"
#include "linear_mfma.h"

namespace {

// ------------------------------------------------------------------ bound statistics
// The pieces of cert_stats_kernel that ncf_tables_kernel shares (one definition of every sum and
// maximum: the statistics are bitwise the same whichever kernel forms them).

// v_k = sum_j |wm_j| |W2_jk| of the layer-1 unit k < h1, term by term in j order
__device__ __forceinline__ float cert_vk(const float* W2, int h1, int h2, const float* wm, int k) {
  float v = 0.f;
  for (int j = 0; j < h2; ++j) v += fabsf(wm[j]) * fabsf(W2[j * h1 + k]);
  return v;
}

// vs[t] = v_k of the layer-1 unit k stored at pair-permuted position t (0 past h1)
__device__ __forceinline__ void cert_fill_vs(float* vs, const float* __restrict__ W2, int h1,
                                             int h2, const float* __restrict__ wm) {
  const int tid = threadIdx.x;
  if (tid < 64) {
    const int k = korig(tid);
    vs[tid] = k < h1 ? cert_vk(W2, h1, h2, wm, k) : 0.f;
  }
}

// The 8 wave sums of v8[0..7] as one reduce-scatter butterfly: each xor step halves the values a
// lane carries (10 shuffles instead of 48); every sum is formed along the same xor 32, 16, ..., 1
// pairing as wave_sum, so bitwise the same.  Returns sum number cert_sum8_idx(lane).
__device__ __forceinline__ float cert_sum8(const float (&v8)[8], int lane) {
  const bool b5 = lane & 32, b4 = lane & 16, b3 = lane & 8;
  float w4[4], w2[2];
#pragma unroll
  for (int q = 0; q < 4; ++q)
    w4[q] = (b5 ? v8[2 * q + 1] : v8[2 * q]) + __shfl_xor(b5 ? v8[2 * q] : v8[2 * q + 1], 32);
#pragma unroll
  for (int q = 0; q < 2; ++q)
    w2[q] = (b4 ? w4[2 * q + 1] : w4[2 * q]) + __shfl_xor(b4 ? w4[2 * q] : w4[2 * q + 1], 16);
  float w1 = (b3 ? w2[1] : w2[0]) + __shfl_xor(b3 ? w2[0] : w2[1], 8);
  w1 += __shfl_xor(w1, 4);
  w1 += __shfl_xor(w1, 2);
  w1 += __shfl_xor(w1, 1);
  return w1;
}
__device__ __forceinline__ int cert_sum8_idx(int lane) {  // the sum this lane holds
  return ((lane & 32) ? 1 : 0) + ((lane & 16) ? 2 : 0) + ((lane & 8) ? 4 : 0);
}

// Four items i0 + u * stride (u = 0..3; the wave holds |Q| and G of each, one column a lane):
// B_i = v . |Q_i|, D_i = ||g_i||_2 and the running maxima of |Q|, |G|, B, D.
__device__ __forceinline__ void cert_item_stats4(float vt, const float (&aq)[4],
                                                 const float (&g)[4], int64_t i0, int64_t stride,
                                                 int64_t I, int lane, float* __restrict__ Bi,
                                                 float* __restrict__ Di, float& m0, float& m1,
                                                 float& m2, float& m3) {
  float v8[8];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    v8[u] = vt * aq[u];
    v8[4 + u] = g[u] * g[u];
    if (i0 + u * stride < I) {  // uniform
      m0 = nmax(m0, aq[u]);
      m1 = nmax(m1, fabsf(g[u]));
    }
  }
  const float w1 = cert_sum8(v8, lane);
  const int idx = cert_sum8_idx(lane);
  const int64_t i = i0 + (idx & 3) * stride;
  if (i < I) {
    if (idx < 4) {
      m2 = nmax(m2, w1);
      if ((lane & 7) == 0) Bi[i] = w1;
    } else {
      const float dq = sqrtf(w1);
      m3 = nmax(m3, dq);
      if ((lane & 7) == 0) Di[i] = dq;
    }
  }
}

// One batch row (|P_u| and wp * g_u, one column a lane): A_u = v . |P_u|, C_u = ||wp * g_u||_2
// and the running maxima of |P| and |WG|.
__device__ __forceinline__ void cert_user_stats(float vt, float ap, float wg, int64_t b, int lane,
                                                float* __restrict__ Au, float* __restrict__ Cu,
                                                float& m0, float& m1) {
  m0 = nmax(m0, ap);
  m1 = nmax(m1, fabsf(wg));
  const float a = wave_sum(vt * ap), c2 = wave_sum(wg * wg);
  if (lane == 0) {
    Au[b] = a;
    Cu[b] = sqrtf(c2);
  }
}

// cert_fill_vs with W2 and wm staged through LDS first (scr: h2 * h1 + 32 <= 2,080 floats): one
// round of independent loads in place of h2 dependent steps; the sum itself is cert_vk's,
// term by term in j order.  Ends with a barrier (vs is set, scr is free).
__device__ __forceinline__ void cert_fill_vs_staged(float* vs, const float* __restrict__ W2,
                                                    int h1, int h2, const float* __restrict__ wm,
                                                    float* scr) {
  const int tid = threadIdx.x;
  float* const wms = scr + h2 * h1;
  for (int e = tid; e < h2 * h1; e += 256) scr[e] = W2[e];
  if (tid < h2) wms[tid] = wm[tid];
  __syncthreads();
  if (tid < 64) {
    const int k = korig(tid);
    vs[tid] = k < h1 ? cert_vk(scr, h1, h2, wms, k) : 0.f;
  }
  __syncthreads();
}

// The workgroup's four maxima -> part[4 * slot ..] (per-block partials, no same-address atomics;
// reduced by cert_scales_kernel).  Called by the whole workgroup.
__device__ __forceinline__ void cert_block_maxima(float m0, float m1, float m2, float m3,
                                                  float (*red)[4], float* __restrict__ part,
                                                  int slot) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  m0 = wave_max(m0);
  m1 = wave_max(m1);
  m2 = wave_max(m2);
  m3 = wave_max(m3);
  if (lane == 0) {
    red[wave][0] = m0;
    red[wave][1] = m1;
    red[wave][2] = m2;
    red[wave][3] = m3;
  }
  __syncthreads();
  if (tid < 4) {
    float m = red[0][tid];
    for (int w = 1; w < 4; ++w) m = nmax(m, red[w][tid]);
    part[slot * 4 + tid] = m;
  }
}

__global__ __launch_bounds__(256) void cert_stats_kernel(NcfTabs t, int64_t B, int64_t I, int mf,
                                                         const float* __restrict__ W2, int h1,
                                                         int h2, const float* __restrict__ wm,
                                                         CertParams* prm, float* __restrict__ Au,
                                                         float* __restrict__ Cu,
                                                         float* __restrict__ Bi,
                                                         float* __restrict__ Di,
                                                         float* __restrict__ part, int item_blocks,
                                                         int user_blocks) {
  __shared__ float vs[64];
  __shared__ float red[4][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  cert_fill_vs(vs, W2, h1, h2, wm);
  __syncthreads();
  const float vt = vs[lane];
  float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f;  // items: Q, G, B, D / users: P, WG
  const bool items = (int)blockIdx.x < item_blocks;
  if (items) {
    // four items per step, their loads issued together (one item a step waited on each)
    const int64_t stride = (int64_t)item_blocks * 4;
    for (int64_t i0 = (int64_t)blockIdx.x * 4 + wave; i0 < I; i0 += 4 * stride) {
      float aq[4], g[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t i = std::min<int64_t>(i0 + u * stride, I - 1);
        aq[u] = fabsf(t.Qi[i * 64 + lane]);
        g[u] = lane < mf ? t.G[i * t.ldg + lane] : 0.f;
      }
      cert_item_stats4(vt, aq, g, i0, stride, I, lane, Bi, Di, m0, m1, m2, m3);
    }
  } else {
    const int ub = (int)blockIdx.x - item_blocks;
    for (int64_t b = (int64_t)ub * 4 + wave; b < B; b += (int64_t)user_blocks * 4)
      cert_user_stats(vt, fabsf(t.Pu[b * 64 + lane]), t.WGu[b * 64 + lane], b, lane, Au, Cu, m0,
                      m1);
  }
  cert_block_maxima(m0, m1, m2, m3, red, part, blockIdx.x);
}

// The per-call tables AND the bound statistics of their rows in one launch (HNM_OPT_NCF_TABLES;
// two-layer towers, h1 <= 64, mf <= 64 a multiple of 4, h0 a multiple of 32, 16-B aligned
// tables).  In place of linear_rows (users), linear_rows (items), gather_scale and
// cert_stats_kernel: Q_i is written once and never read back for its statistics, G is read once.
// Heterogeneous blocks as cert_stats_kernel's, each over 64-row tiles (grid-stride), partials in
// cert_stats_kernel's layout (item blocks' first):
//   item blocks: the Q_i tile by linear_mfma_tile (linear_rows_mfma_kernel's chain: the rows are
//     bitwise hnm_linear_rows_f32's), staged pair-permuted through the LDS the k-loop released,
//     stored fp32 (re-scoring and the exact fallback read it), and B_i, D_i and the maxima of
//     |Q|, |G|, B, D from the staged tile and the items' G rows (loads issued before the k-loop).
//     a.item_proj set (the caller's cached projection): no projection, the tile is read from it.
//   user blocks: P_u = W1u m_u + b1 (ids gathered, out-of-range ids flagged, their rows NaN),
//     wp * g_u (gather_scale_kernel's product), A_u, C_u and the maxima of |P|, |WG|.
// Columns h1..63 of P / Q are written as zero (no memset of the tables).  Every sum and maximum
// is cert_stats_kernel's own (the functions above), so Bi, Di, Au, Cu and the reduced maxima are
// bitwise the separate launches'.
struct NcfTablesArgs {
  const float* mlp_user;   // [num_users, h0]
  const float* mlp_item;   // [I, h0]
  const float* gmf_user;   // [num_users, mf]
  const float* w1;         // [h1, 2 h0]
  const float* b1;         // [h1]
  const float* wp;         // [mf] GMF part of the prediction weights
  const float* item_proj;  // [I, 64] cached Q (nullptr: computed and written to Qi)
  const int64_t* ids;      // [B]
  int64_t num_users;
  int h0, h1, mf;
  float* Pu;               // [B, 64]
  float* WGu;              // [B, 64]
  float* Qi;               // [I, 64]
  const float* G;          // [I, ldg]
  int64_t ldg;
};

__global__ __launch_bounds__(256) void ncf_tables_kernel(
    NcfTablesArgs a, int64_t B, int64_t I, const float* __restrict__ W2, int h2,
    const float* __restrict__ wm, float* __restrict__ Au, float* __restrict__ Cu,
    float* __restrict__ Bi, float* __restrict__ Di, float* __restrict__ part, int item_blocks,
    int user_blocks, unsigned* err) {
  __shared__ __attribute__((aligned(16))) float lds[2 * 64 * LIN_RS];  // xs | ws, then the tile
  __shared__ float vs[64];
  __shared__ float red[4][4];
  float* const xs = lds;
  float* const ws = lds + 64 * LIN_RS;
  float* const stage = lds;  // [64 rows][64 pair-permuted columns] (<= the k-loop's 2 * 64 * 33)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = lane >> 5;
  const int wr = 32 * (wave >> 1);
  const int n = 32 * (wave & 1) + (lane & 31);  // this lane's output unit in the k-loop's tile
  const int nc = (n & 1) * 32 + (n >> 1);        // its pair-permuted column
  cert_fill_vs_staged(vs, W2, a.h1, h2, wm, lds);
  const float vt = vs[lane];
  float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f;  // items: Q, G, B, D / users: P, WG
  const int r0 = wave * 16;  // the wave's rows of a tile for the statistics
  // the (few, one-tile) user blocks are dispatched first, so they run beside the item blocks and
  // not behind them; the partials keep cert_stats_kernel's layout, item blocks first
  const bool items = (int)blockIdx.x >= user_blocks;
  const int blk = items ? (int)blockIdx.x - user_blocks : (int)blockIdx.x;
  if (items) {
    const int64_t ntiles = hnm_cdiv(I, 64);
    for (int64_t tile = blk; tile < ntiles; tile += item_blocks) {
      const int64_t t0 = tile * 64;
      float g[16];  // G of the wave's rows, issued before the k-loop (rows past I: unused zeros)
      const float* gp = a.G + (t0 + r0) * a.ldg + lane;
      const int nrow = (int)std::min<int64_t>(16, I - t0 - r0);  // may be <= 0
#pragma unroll
      for (int r = 0; r < 16; ++r) g[r] = (lane < a.mf && r < nrow) ? gp[r * a.ldg] : 0.f;
      if (!a.item_proj) {
        const f32x16 acc = linear_mfma_tile(a.mlp_item, a.h0, nullptr, I, I, a.h0, a.w1 + a.h0,
                                            2 * a.h0, a.h1, t0, 0, xs, ws, err);
#pragma unroll
        for (int r = 0; r < 16; ++r)
          stage[(wr + mfma32_row(r, h)) * 64 + nc] = n < a.h1 ? acc[r] : 0.f;
        __syncthreads();
      }
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) {
        const int64_t i0 = t0 + r0 + 4 * q4;
        if (i0 < I) {  // uniform
          float aq[4], g4[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            float qv;
            if (a.item_proj) {
              qv = a.item_proj[std::min<int64_t>(i0 + u, I - 1) * 64 + lane];
            } else {
              qv = stage[(r0 + 4 * q4 + u) * 64 + lane];
              if (i0 + u < I) a.Qi[(i0 + u) * 64 + lane] = qv;
            }
            aq[u] = fabsf(qv);
            g4[u] = g[4 * q4 + u];
          }
          cert_item_stats4(vt, aq, g4, i0, 1, I, lane, Bi, Di, m0, m1, m2, m3);
        }
      }
      __syncthreads();  // the tile is consumed: the next k-loop may stage over it
    }
  } else {
    const int64_t ntiles = hnm_cdiv(B, 64);
    const int kc = korig(lane);  // the GMF column stored at pair-permuted position `lane`
    for (int64_t tile = blk; tile < ntiles; tile += user_blocks) {
      const int64_t t0 = tile * 64;
      const f32x16 acc = linear_mfma_tile(a.mlp_user, a.h0, a.ids, a.num_users, B, a.h0, a.w1,
                                          2 * a.h0, a.h1, t0, 0, xs, ws, err);
      const float bn = n < a.h1 ? a.b1[n] : 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r)
        stage[(wr + mfma32_row(r, h)) * 64 + nc] = n < a.h1 ? acc[r] + bn : 0.f;
      __syncthreads();
      // row by row with cert_user_stats' own wave sums (the compiler fuses their first step
      // into an fma, which the items' butterfly does not reproduce): 16 independent chains
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t b = t0 + r0 + r;
        if (b < B) {  // uniform
          // wp * g_u of the row (the one-tile user blocks end before the item blocks: the
          // gather's latency is not hidden and need not be)
          const int64_t id = a.ids[b];
          const bool ok = id >= 0 && id < a.num_users;
          if (!ok && lane == 0) hnm_flag(err, HNM_ERR_OOB);
          const float wg = ncf_gather_scale(a.gmf_user, id, a.mf, a.mf, a.wp, kc, ok);
          const float pv = stage[(r0 + r) * 64 + lane];
          a.Pu[b * 64 + lane] = pv;
          a.WGu[b * 64 + lane] = wg;
          cert_user_stats(vt, fabsf(pv), wg, b, lane, Au, Cu, m0, m1);
        }
      }
      __syncthreads();
    }
  }
  cert_block_maxima(m0, m1, m2, m3, red, part, items ? blk : item_blocks + blk);
}

__device__ __forceinline__ float pow2_below_inv(float m) {  // 2^-e with m < 2^e (m > 0)
  int e;
  (void)frexpf(m, &e);
  return ldexpf(1.f, -e);
}

// One block: weight statistics, scales, slack.
__global__ __launch_bounds__(256) void cert_scales_kernel(const float* __restrict__ W2, int h1,
                                                          int h2, const float* __restrict__ b2,
                                                          const float* __restrict__ wm,
                                                          const float* __restrict__ bp,
                                                          CertParams* prm,
                                                          const float* __restrict__ part,
                                                          int item_blocks, int user_blocks,
                                                          int* __restrict__ ovf_cnt, CertDeep dp) {
  __shared__ float red[7][4];
  __shared__ float pm[4][6];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  {  // per-block partial maxima of cert_stats_kernel: items Q G B D, users P WG
    float q = 0.f, g = 0.f, bb = 0.f, dd = 0.f, pp = 0.f, wg = 0.f;
    // partials in batches of 8 per thread: every load of a batch issued before the first use
    // (one L2 round trip per batch instead of one per partial: this single block is latency)
    const int nblk = item_blocks + user_blocks;
    for (int b0 = 0; b0 < nblk; b0 += 8 * 256) {
      float4 v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k)
        v[k] = *reinterpret_cast<const float4*>(part + 4 * std::min(b0 + 256 * k + tid, nblk - 1));
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int blk = b0 + 256 * k + tid;
        if (blk < item_blocks) {
          q = nmax(q, v[k].x); g = nmax(g, v[k].y); bb = nmax(bb, v[k].z); dd = nmax(dd, v[k].w);
        } else if (blk < nblk) {
          pp = nmax(pp, v[k].x); wg = nmax(wg, v[k].y);
        }
      }
    }
    q = wave_max(q); g = wave_max(g); bb = wave_max(bb); dd = wave_max(dd);
    pp = wave_max(pp); wg = wave_max(wg);
    if (lane == 0) {
      pm[wave][0] = q; pm[wave][1] = g; pm[wave][2] = bb; pm[wave][3] = dd;
      pm[wave][4] = pp; pm[wave][5] = wg;
    }
    __syncthreads();
    if (tid < 6) {
      float m = pm[0][tid];
      for (int w = 1; w < 4; ++w) m = nmax(m, pm[w][tid]);
      const int slot = tid == 0 ? CM_Q : tid == 1 ? CM_G : tid == 2 ? CM_B : tid == 3 ? CM_D
                     : tid == 4 ? CM_P : CM_WG;
      prm->mx[slot] = __float_as_uint(m);
    }
    if (tid == 0 && ovf_cnt) *ovf_cnt = 0;
    __syncthreads();
  }
  float mW = 0.f, vsum = 0.f, mwm = 0.f, mb2 = 0.f, c0 = 0.f, swm = 0.f;
  for (int e = tid; e < h2 * h1; e += 256) {
    const float w = fabsf(W2[e]);
    mW = nmax(mW, w);
    vsum += fabsf(wm[e / h1]) * w;
  }
  float mrow = 0.f;  // max_j sum_k |W2_jk|: 8 threads a row, strided partials + 3 xor steps
  for (int j0 = 0; j0 < h2; j0 += 32) {
    const int j = j0 + (tid >> 3);
    float rs = 0.f;
    if (j < h2)
      for (int k = tid & 7; k < h1; k += 8) rs += fabsf(W2[j * h1 + k]);
    rs += __shfl_xor(rs, 1);
    rs += __shfl_xor(rs, 2);
    rs += __shfl_xor(rs, 4);
    mrow = nmax(mrow, rs);
  }
  for (int j = tid; j < h2; j += 256) {
    mwm = nmax(mwm, fabsf(wm[j]));
    mb2 = nmax(mb2, fabsf(b2[j]));
    c0 += fabsf(wm[j]) * fabsf(b2[j]);
    swm += fabsf(wm[j]);
  }
  mW = wave_max(mW);
  mrow = wave_max(mrow);
  mwm = wave_max(mwm);
  mb2 = wave_max(mb2);
  vsum = wave_sum(vsum);
  c0 = wave_sum(c0);
  swm = wave_sum(swm);
  if (lane == 0) {
    red[0][wave] = mW;
    red[1][wave] = mwm;
    red[2][wave] = mb2;
    red[3][wave] = vsum;
    red[4][wave] = c0;
    red[5][wave] = swm;
    red[6][wave] = mrow;
  }
  __syncthreads();
  if (tid != 0) return;
  for (int w = 1; w < 4; ++w) {
    red[0][0] = nmax(red[0][0], red[0][w]);
    red[1][0] = nmax(red[1][0], red[1][w]);
    red[2][0] = nmax(red[2][0], red[2][w]);
    red[3][0] += red[3][w];
    red[4][0] += red[4][w];
    red[5][0] += red[5][w];
    red[6][0] = nmax(red[6][0], red[6][w]);
  }
  mW = red[0][0];
  mwm = red[1][0];
  mb2 = red[2][0];
  vsum = red[3][0];
  c0 = red[4][0];
  swm = red[5][0];
  mrow = red[6][0];
  const float mP = __uint_as_float(prm->mx[CM_P]), mQ = __uint_as_float(prm->mx[CM_Q]);
  const float mWG = __uint_as_float(prm->mx[CM_WG]), mG = __uint_as_float(prm->mx[CM_G]);
  const float Bmax = __uint_as_float(prm->mx[CM_B]), Dmax = __uint_as_float(prm->mx[CM_D]);
  const float lim = 1099511627776.f;  // 2^40
  bool bad = false;
  for (float m : {mP, mQ, mWG, mG, Bmax, Dmax, mW, mrow, mwm, mb2, vsum, c0, fabsf(bp[0])})
    bad |= !(m <= lim);  // also catches NaN / inf
  const float zmax = mP + mQ;
  const float s1 = zmax > 0.f ? 0.5f * pow2_below_inv(zmax) : 1.f;  // s1 * z <= 0.5
  // W2 / b2 scale: |H~| <= s1 sw |b2| + sw sum_k |W2_jk| x~_k (x~ <= 0.5 (1 + u)^2) stays
  // below 1, so the [0, 1] clamp of the f32 -> f16 convert is an exact ReLU
  const float hmax = (s1 * mb2 + 0.51f * mrow) * 1.01f;
  const float sw = hmax > 0.f ? pow2_below_inv(hmax) : 1.f;
  float sm = mwm > 0.f ? pow2_below_inv(mwm) : 1.f;
  const float sgu = mWG > 0.f ? pow2_below_inv(mWG) : 1.f;
  const float sgi = mG > 0.f ? pow2_below_inv(mG) : 1.f;
  const float phi = 2.98023224e-08f;  // 2^-25: half the f16 subnormal spacing
  const float rmax = mb2 + 64.f * mW * zmax;
  float s3 = 1.f, rho = CERT_RHO;
  // the per-rounding absolute slack terms (real units, x 16 phi below): layer-1 operands and
  // sum, W2 rounding, relu(H) rounding, GMF operands -- and the last weights' rounding
  float abst = 3.f * vsum / s1 + 64.f * swm * zmax / sw + swm / (s1 * sw) + 64.f * mG / sgu +
               64.f * mWG / sgi;
  if (dp.W3) {
    // Deep tower (round 6).  `wm` is u = |wp3|^T |W3| here, so vsum = sum_k v_k, swm = sum_l u_l
    // and c0 = u . |b2| with v = |wp3|^T |W3| |W2| (the stats kernel's A_u / B_i).  Error of the
    // scan against the exact chain, u = 2^-11: layer-2 output dH_l <= 3.02u sum_k |W2_lk| z_k as
    // before; y~ = f16(relu(H~)) adds u R_l (R_l = |b2_l| + sum_k |W2_lk| z_k >= |H_l|); the f16
    // W3 and layer-3 accumulation give dH3_m <= sum_l |W3_ml| ((1 + u) dH_l + 2u R_l); z~ =
    // f16(relu(H3~)) adds u R3_m (R3_m = |b3_m| + sum_l |W3_ml| R_l) and the f16 wp3 another u
    // R3_m: |err| <= u (7.03 (A_u + B_i) + 4 c0 + 2 cb3) + 2.01u C_u D_i + O(u^2) <= 8u (c0 + cb3
    // + A_u + B_i + C_u D_i) (fp32 accumulation ~2^-22 relative, inside the margin); absolute
    // slack for f16 subnormals per rounding site, each through the weights after it.
    float mW3 = 0.f, mrow3 = 0.f, mb3 = 0.f, mwp = 0.f, swp = 0.f, cb3 = 0.f;
    for (int m = 0; m < dp.h3; ++m) {
      float rs = 0.f;
      for (int l = 0; l < h2; ++l) {
        const float a = fabsf(dp.W3[m * h2 + l]);
        mW3 = nmax(mW3, a);
        rs += a;
      }
      mrow3 = nmax(mrow3, rs);
      mb3 = nmax(mb3, fabsf(dp.b3[m]));
      mwp = nmax(mwp, fabsf(dp.wp3[m]));
      swp += fabsf(dp.wp3[m]);
      cb3 += fabsf(dp.wp3[m]) * fabsf(dp.b3[m]);
    }
    for (float m : {mW3, mrow3, mb3, mwp, swp, cb3}) bad |= !(m <= lim);
    // relu(H~) <= 1 after the clamp, so |H3~| <= s3 (s1 sw |b3| + sum_l |W3_ml|) <= 1
    const float hmax3 = (s1 * sw * mb3 + mrow3) * 1.01f;
    s3 = hmax3 > 0.f ? pow2_below_inv(hmax3) : 1.f;
    sm = mwp > 0.f ? pow2_below_inv(mwp) : 1.f;
    const float r3max = mb3 + (float)h2 * mW3 * rmax;
    c0 += cb3;
    abst += 32.f * swp * rmax / s3 + swp / (s1 * sw * s3) + 16.f * r3max / sm;
    rho = CERT_RHO_DEEP;
  } else {
    abst += 32.f * rmax / sm;  // wm rounding
  }
  const float unit = s1 * sw * s3 * sm;
  const float cg = unit / (sgu * sgi);
  bad |= !(unit >= 1e-30f && unit <= 1e30f && cg >= 1e-30f && cg <= 1e30f);
  const float absb = 16.f * phi * abst + 2.4e-7f * fabsf(bp[0]);
  prm->s1 = s1;
  prm->sw = sw;
  prm->sm = sm;
  prm->s3 = s3;
  prm->sgu = sgu;
  prm->sgi = sgi;
  prm->unit = unit;
  prm->cg = cg;
  prm->rho = rho;
  prm->c0 = c0;
  prm->absb = absb;
  prm->Bmax = Bmax;
  prm->Dmax = Dmax;
  prm->bad = bad || !(absb <= lim);
}

// f16 operand tables.  Q16/P16 keep the pair-permuted order (the layer-1 unit order is
// free as long as W2h's columns follow it); G16/WG16 use the natural GMF order.
__global__ __launch_bounds__(256) void cert_convert_kernel(
    NcfTabs t, int64_t B, int64_t I, int mf, const CertParams* __restrict__ prm,
    _Float16* __restrict__ P16, _Float16* __restrict__ WG16, _Float16* __restrict__ Q16,
    _Float16* __restrict__ G16, const float* __restrict__ W2, int h1, int h2,
    const float* __restrict__ b2, const float* __restrict__ wm, _Float16* __restrict__ W2h,
    _Float16* __restrict__ wmh, float* __restrict__ b2s, const float* __restrict__ Bi,
    const float* __restrict__ Cu, float* __restrict__ Bs, float* __restrict__ Cs, CertDeep dp,
    _Float16* __restrict__ W3h, _Float16* __restrict__ wph, float* __restrict__ b3s) {
  const float s1 = prm->s1, sgu = prm->sgu, sgi = prm->sgi;
  // the scan's bound terms in test units (rho * unit * B_i, ... * C_u): the same fp32
  // products the scan formed itself before, computed once here so the scan keeps no scale
  // factor live across its tile loop
  const int64_t nthreads = (int64_t)gridDim.x * 256;
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const float ru = prm->rho * prm->unit;
  for (int64_t e = g; e < I; e += nthreads) Bs[e] = ru * Bi[e];
  for (int64_t e = g; e < B; e += nthreads) Cs[e] = ru * Cu[e];
  // items: 16 chunks of 4 per row
  for (int64_t e = g; e < I * 16; e += nthreads) {
    const int64_t i = e >> 4;
    const int c = (int)(e & 15);
    const float4 q = *reinterpret_cast<const float4*>(t.Qi + i * 64 + 4 * c);
    _Float16* qo = Q16 + i * 64 + 4 * c;
    qo[0] = (_Float16)(q.x * s1);
    qo[1] = (_Float16)(q.y * s1);
    qo[2] = (_Float16)(q.z * s1);
    qo[3] = (_Float16)(q.w * s1);
    float4 gv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (4 * c < mf) gv = *reinterpret_cast<const float4*>(t.G + i * t.ldg + 4 * c);
    _Float16* go = G16 + i * 64 + 4 * c;
    go[0] = (_Float16)(4 * c + 0 < mf ? gv.x * sgi : 0.f);
    go[1] = (_Float16)(4 * c + 1 < mf ? gv.y * sgi : 0.f);
    go[2] = (_Float16)(4 * c + 2 < mf ? gv.z * sgi : 0.f);
    go[3] = (_Float16)(4 * c + 3 < mf ? gv.w * sgi : 0.f);
  }
  for (int64_t e = g; e < B * 64; e += nthreads) {
    const int64_t b = e >> 6;
    const int k = (int)(e & 63);
    P16[e] = (_Float16)(t.Pu[e] * s1);
    WG16[e] = (_Float16)(t.WGu[b * 64 + (k & 1) * 32 + (k >> 1)] * sgu);
  }
  if (blockIdx.x == 0) {
    const float sw = prm->sw, sm = prm->sm;
    for (int e = threadIdx.x; e < 32 * 64; e += 256) {
      const int j = e >> 6, k = korig(e & 63);
      W2h[e] = (_Float16)((j < h2 && k < h1) ? W2[j * h1 + k] * sw : 0.f);
    }
    if (threadIdx.x < 32) {
      const int j = threadIdx.x;
      wmh[j] = (_Float16)(j < h2 && !dp.W3 ? wm[j] * sm : 0.f);
      b2s[j] = j < h2 ? b2[j] * s1 * sw : 0.f;
    }
    if (dp.W3) {  // layer 3 (unit m, hidden l) x s3, its bias x s1 sw s3, wp3 x sm
      const float s3 = prm->s3;
      for (int e = threadIdx.x; e < 16 * 32; e += 256) {
        const int m = e >> 5, l = e & 31;
        W3h[e] = (_Float16)((m < dp.h3 && l < h2) ? dp.W3[m * h2 + l] * s3 : 0.f);
      }
      if (threadIdx.x < 16) {
        const int m = threadIdx.x;
        wph[m] = (_Float16)(m < dp.h3 ? dp.wp3[m] * sm : 0.f);
        b3s[m] = m < dp.h3 ? dp.b3[m] * s1 * sw * s3 : 0.f;
      }
    }
  }
}

// Deep towers: u_l = sum_m |wp3_m| |W3_ml| (l < h2), the weights the bound statistics take in
// place of the two-layer tower's |wm| (v = |wp3|^T |W3| |W2|)
__global__ __launch_bounds__(64) void cert_deep_u_kernel(CertDeep dp, int h2, float* __restrict__ u) {
  const int l = threadIdx.x;
  if (l >= 32) return;
  float v = 0.f;
  if (l < h2)
    for (int m = 0; m < dp.h3; ++m) v += fabsf(dp.wp3[m]) * fabsf(dp.W3[m * h2 + l]);
  u[l] = v;
}

StatBlocks cert_stat_blocks(int64_t B, int64_t I, bool fused) {
  const int rows = fused ? 64 : 4;
  return {(int)std::min<int64_t>(1024, hnm_cdiv(I, rows)),
          (int)std::min<int64_t>(256, hnm_cdiv(B, rows))};
}

}  // namespace

hnm_status cert_prepare(hnm_ctx* ctx, const hnm_ncf_weights* w, const NcfTabs& t, int64_t B,
                        const CertWs& x, const CertDeep* dp) {
  const int64_t I = w->num_items;
  const StatBlocks sb = cert_stat_blocks(B, I, t.stats);
  const int ib = sb.items, ub = sb.users;
  // the weights behind layer 2's outputs: wm (two-layer tower) or u = |wp3|^T |W3| (deep)
  const float* wm = w->wp + w->mf;
  const CertDeep dv = dp ? *dp : CertDeep{};
  if (dp) {
    hipLaunchKernelGGL(cert_deep_u_kernel, dim3(1), dim3(64), 0, ctx->stream, dv, w->h2, x.u);
    HNM_LAUNCH_CHECK();
    wm = x.u;
  }
  if (!t.stats) {  // else ncf_cert_tables left Au, Cu, Bi, Di and the partials with the tables
    hipLaunchKernelGGL(cert_stats_kernel, dim3(ib + ub), dim3(256), 0, ctx->stream, t, B, I, w->mf,
                       w->w2, w->h1, w->h2, wm, x.prm, x.Au, x.Cu, x.Bi, x.Di, x.part, ib, ub);
    HNM_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(cert_scales_kernel, dim3(1), dim3(256), 0, ctx->stream, w->w2, w->h1, w->h2,
                     w->b2, wm, w->bp, x.prm, x.part, ib, ub, x.ovf_cnt, dv);
  HNM_LAUNCH_CHECK();
  const int cb = (int)std::min<int64_t>(2048, std::max<int64_t>(1, hnm_cdiv(I * 16, 256)));
  hipLaunchKernelGGL(cert_convert_kernel, dim3(cb), dim3(256), 0, ctx->stream, t, B, I, w->mf,
                     x.prm, x.P16, x.WG16, x.Q16, x.G16, w->w2, w->h1, w->h2, w->b2, wm, x.W2h,
                     x.wmh, x.b2s, x.Bi, x.Cu, x.Bs, x.Cs, dv, x.W3h, x.wph, x.b3s);
  HNM_LAUNCH_CHECK();
  return HNM_OK;
}

hnm_status ncf_cert_tables(hnm_ctx* ctx, const hnm_ncf_weights* w, const int64_t* ids, int64_t B,
                           float* Pu, float* WGu, float* Qi, int K, void* scratch, bool strided) {
  const int64_t I = w->num_items;
  const CertWs x = cert_plan(ctx, B, I, K, scratch, strided).ws;
  const StatBlocks sb = cert_stat_blocks(B, I, true);
  const NcfTablesArgs a{w->mlp_user, w->mlp_item, w->gmf_user, w->w1,  w->b1, w->wp,
                        w->item_proj, ids,         w->num_users, w->h0, w->h1, w->mf,
                        Pu,           WGu,         Qi,           w->gmf_item, w->mf};
  hipLaunchKernelGGL(ncf_tables_kernel, dim3(sb.items + sb.users), dim3(256), 0, ctx->stream, a, B,
                     I, w->w2, w->h2, w->wp + w->mf, x.Au, x.Cu, x.Bi, x.Di, x.part, sb.items,
                     sb.users, ctx->err_dev);
  HNM_LAUNCH_CHECK();
  return HNM_OK;
}
