// ItemCF: item-based collaborative filtering over the de-duplicated user -> item CSR
// (UserHistory.hist_ptr / hist_idx: rows ascending and unique).  No reference counterpart: the
// contract is stated in include/hnm.h and restated in numpy by tests/itemcf_oracle.py.
//
// Fit.  Users with more than max_history items are dropped.  Over the kept users
//   n[i]     = users holding i                         (int32 atomics -> item_count int64)
//   C[i, j]  = users holding i and j, i != j           (int32 LDS atomics)
//   sim[i,j] = float( double(C) / ( sqrt(double(n_i) * double(n_j)) + shrink ) )   for C > 0
// one rounding per operation, contraction off; row i keeps the N best in (sim desc, j asc) order,
// padded with (-1, 0.0f).  Counts are integers, so the result is the same bits on every run.
// Shape: histogram -> scan -> fill give the item -> user transpose; then one workgroup per item
// walks the catalogue in windows of `window` columns of LDS counters: a thread per user of the
// item finds the window's lower bound in that user's sorted row by binary search and adds 1 per
// item inside the window; each wave then turns its share of the non-zero counters into sim and
// offers them to its wave-resident top-N list (clearing the counters as it reads); the four
// lists are merged at the end.  (sim desc, j asc) is a total order, so the merge order is free.
//
// Scores.  score[i] = the fp32 sum of val(j -> i) over the history items j in ascending order,
// plain adds: one step per j, the up-to-64 neighbours of one j are distinct items (one lane
// each, no atomics), a workgroup barrier between steps (a lane reads what another wrote).
//
// Top-K.  One wave per row with an LDS open-addressing table keyed by item id, sized from
// h * N (h = history length); slots are claimed by compare-and-swap (two new items of one step
// may hash alike), the adds are plain.  Then the unmasked entries with score > 0 go through
// the wave list.  Rows with h * N > ICF_TABLE queue themselves for the dense route: a pool of
// workspace rows, the same steps, the same selection -- the same bits.
//
// Weighted (hist_w: an fp32 weight per history entry; the *_weighted_* entries, WT = true below).
// The fit counts in fixed point so that it stays integer and order-free: w_max = the largest
// weight of the kept users (an integer max on the float's bit pattern), s = 32768 / w_max,
// q = rint(w * s) in float64 (w_max -> 2^15), n_w[i] = sum q_ui^2, C_w[i, j] = sum q_ui q_uj in
// uint64 (a product <= 2^30, fewer than 2^31 users: < 2^61), 64-bit LDS counters, and
//   sim = float( double(C_w) / ( sqrt(double(n_i) * double(n_j)) + (shrink * s) * s ) ).
// Entries with q = 0 stay out of the transpose.  Serving multiplies val(j -> i) by the row's raw
// weight w_j (one fp32 rounding) before the same plain add.  The unweighted kernels are the
// WT = false instantiations: no extra loads, registers or LDS.  The numpy restatement of this
// paragraph is tests/itemcf_oracle.py too.
#include "hnm_device.h"
#include "hnm_internal.h"
#include "itemcf_internal.h"

#include <cfloat>
#include <cmath>
#include <type_traits>

namespace {

constexpr int ICF_MAX_N = 64;
// int32 counters per LDS pass.  Measured at the H&M shape (tools/itemcf_bench.py): 4,096 -> 307 ms,
// 8,192 -> 190 ms, 16,384 (64 KiB, two workgroups a CU) -> 139 ms: fewer passes beat occupancy.
constexpr int ICF_WINDOW_DEFAULT = 16384;
constexpr int ICF_WINDOW_MAX = 16384;
// uint64 counters per LDS pass of the weighted fit.  Measured at the H&M shape (tools/
// itemcf_bench.py, profiles/witemcf_bench.txt): 4,096 -> 455 ms, 8,192 (64 KiB, two workgroups a
// CU) -> 299 ms, 16,384 (128 KiB, one workgroup a CU) -> 229 ms: fewer passes beat occupancy here
// too (the unweighted fit on the same CSR: 139 ms).
constexpr int ICF_WWINDOW_DEFAULT = 16384;
constexpr int ICF_TABLE = 4096;           // LDS table slots of the fused top-K (32 KiB)
constexpr int ICF_DENSE_POOL = 128;       // workspace rows (and workgroups) of the dense route
constexpr int ICF_GRID_USERS = 4096;

// ------------------------------------------------------------------ shared device pieces
// (icf_offer and icf_merge4, the wave list: itemcf_internal.h)
__device__ __forceinline__ bool icf_masked(const int32_t* midx, int64_t m0, int64_t m1, int item) {
  const int64_t p = mask_lower_bound(midx, m0, m1, item);
  return p < m1 && midx[p] == item;
}

// The history row of batch row b: (first entry, length); a user id out of range raises the
// error word and gives an empty row.
__device__ __forceinline__ void icf_row(const int64_t* hist_ptr, int64_t num_users,
                                        const int64_t* user_ids, int64_t b, unsigned* err,
                                        int64_t& p0, int64_t& h) {
  const int64_t u = user_ids ? user_ids[b] : b;
  p0 = 0;
  h = 0;
  if (u < 0 || u >= num_users) {
    if (threadIdx.x == 0) hnm_flag(err, HNM_ERR_OOB);
    return;
  }
  p0 = hist_ptr[u];
  h = hist_ptr[u + 1] - p0;
  if (h < 0) h = 0;
}

// A history weight as served: negative or non-finite raises the error word and counts as 0.
__device__ __forceinline__ float icf_weight(const float* __restrict__ hist_w, int64_t p,
                                            unsigned* err) {
  const float w = hist_w[p];
  if (!(w >= 0.f) || w > FLT_MAX) {
    hnm_flag(err, HNM_ERR_WEIGHT);
    return 0.f;
  }
  return w;
}

// w * val rounded to fp32; the add that follows must stay an add (no fma).
__device__ __forceinline__ float icf_wmul(float w, float val) {
#pragma clang fp contract(off)
  const float prod = w * val;
  return prod;
}

// The (idx, val) lane t < N holds for step s of a history row (idx -1: nothing to add); WT: val
// is the weighted term fl(w_j * val).
template <bool WT>
__device__ __forceinline__ void icf_step_load(const int32_t* __restrict__ nbr_idx,
                                              const float* __restrict__ nbr_val, int64_t I, int N,
                                              const int32_t* __restrict__ hist_idx,
                                              const float* __restrict__ hist_w, int64_t p0,
                                              int64_t h, int64_t s, unsigned* err, int& idx,
                                              float& val) {
  idx = -1;
  val = 0.f;
  const int t = threadIdx.x;
  if (t < N && s < h) {
    const int32_t j = hist_idx[p0 + s];
    if (j < 0 || j >= I) {
      hnm_flag(err, HNM_ERR_OOB);
    } else {
      idx = nbr_idx[(int64_t)j * N + t];
      val = nbr_val[(int64_t)j * N + t];
      if (idx >= I) idx = -1;  // a table that was not produced by the fit: never write outside
      if constexpr (WT) val = icf_wmul(icf_weight(hist_w, p0 + s, err), val);
    }
  }
}

// row[0, I) (zeroed, visible to the workgroup) += the history row, one step per history item in
// ascending order.  Every thread of the workgroup calls it (h is uniform); step s + 1 is loaded
// before step s's barrier.
template <bool WT>
__device__ __forceinline__ void icf_accumulate_dense(float* row, const int32_t* nbr_idx,
                                                     const float* nbr_val, int64_t I, int N,
                                                     const int32_t* hist_idx, const float* hist_w,
                                                     int64_t p0, int64_t h, unsigned* err) {
  int nidx;
  float nval;
  icf_step_load<WT>(nbr_idx, nbr_val, I, N, hist_idx, hist_w, p0, h, 0, err, nidx, nval);
  for (int64_t s = 0; s < h; ++s) {
    const int cidx = nidx;
    const float cval = nval;
    icf_step_load<WT>(nbr_idx, nbr_val, I, N, hist_idx, hist_w, p0, h, s + 1, err, nidx, nval);
    if (cidx >= 0) row[cidx] = row[cidx] + cval;
    __syncthreads();  // the next step reads what this one wrote (another lane's item)
  }
}

// ------------------------------------------------------------------ fit
// A user's row if the fit keeps the user (len <= max_history, bounds sane).
__device__ __forceinline__ bool icf_kept(const int64_t* hist_ptr, int64_t u, int64_t nnz,
                                         int64_t max_history, unsigned* err, int64_t& p0,
                                         int64_t& p1) {
  p0 = hist_ptr[u];
  p1 = hist_ptr[u + 1];
  if (p0 < 0 || p1 < p0 || p1 > nnz) {
    hnm_flag(err, HNM_ERR_OOB);
    return false;
  }
  return max_history <= 0 || p1 - p0 <= max_history;
}

// The scale of the weighted fit's fixed point, from the bit pattern of w_max (> 0).
__device__ __forceinline__ double icf_scale(unsigned wmax_bits) {
  return 32768.0 / (double)__uint_as_float(wmax_bits);
}

// *wmax = the bit pattern of the largest valid weight among the kept users' entries (0: none is
// positive).  Non-negative floats order as their bit patterns, and a max is order-free.
__global__ __launch_bounds__(256) void icf_wmax_kernel(
    const int64_t* __restrict__ hist_ptr, const int32_t* __restrict__ hist_idx,
    const float* __restrict__ hist_w, int64_t num_users, int64_t I, int64_t nnz,
    int64_t max_history, unsigned* __restrict__ wmax) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  unsigned m = 0;
  for (int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x; u < num_users; u += stride) {
    int64_t p0, p1;
    if (!icf_kept(hist_ptr, u, nnz, max_history, nullptr, p0, p1)) continue;
    for (int64_t p = p0; p < p1; ++p) {
      const int32_t j = hist_idx[p];
      const float w = hist_w[p];
      if (j >= 0 && j < I && w > 0.f && w <= FLT_MAX) m = std::max(m, __float_as_uint(w));
    }
  }
  if (m) atomicMax(wmax, m);
}

// FILL = false: cnt[j] += 1 per (kept user, item j).  FILL = true: tusers[cursor[j]++] = u.
// WT: the count pass also writes q next to hist_idx (hist_q) and adds q^2 to nsq[j]; entries with
// q = 0 are left out; the fill pass carries q beside the user (tq).
template <bool FILL, bool WT>
__global__ __launch_bounds__(256) void icf_transpose_kernel(
    const int64_t* __restrict__ hist_ptr, const int32_t* __restrict__ hist_idx, int64_t num_users,
    int64_t I, int64_t nnz, int64_t max_history, int* __restrict__ cnt, int* __restrict__ tusers,
    unsigned* err, const float* __restrict__ hist_w, const unsigned* __restrict__ wmax,
    uint32_t* __restrict__ hist_q, uint32_t* __restrict__ tq,
    unsigned long long* __restrict__ nsq) {
  unsigned wbits = 0;
  double scale = 0.0;
  if constexpr (WT && !FILL) {
    wbits = *wmax;
    if (wbits) scale = icf_scale(wbits);
  }
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x; u < num_users; u += stride) {
    int64_t p0, p1;
    if (!icf_kept(hist_ptr, u, nnz, max_history, FILL ? nullptr : err, p0, p1)) continue;
    for (int64_t p = p0; p < p1; ++p) {
      const int32_t j = hist_idx[p];
      uint32_t q = 1;
      if constexpr (WT && !FILL) {
        const float w = hist_w[p];
        q = 0;
        if (!(w >= 0.f) || w > FLT_MAX) hnm_flag(err, HNM_ERR_WEIGHT);
        else if (wbits) q = (uint32_t)rint((double)w * scale);  // w <= w_max: q <= 2^15
        hist_q[p] = q;
      }
      if constexpr (WT && FILL) q = hist_q[p];
      if (j < 0 || j >= I) {
        if (!FILL) hnm_flag(err, HNM_ERR_OOB);
        continue;
      }
      if constexpr (WT) {
        if (q == 0) continue;
      }
      const int at = atomicAdd(&cnt[j], 1);
      if (FILL) tusers[at] = (int)u;
      if constexpr (WT && FILL) tq[at] = q;
      if constexpr (WT && !FILL) atomicAdd(&nsq[j], (unsigned long long)q * q);
    }
  }
}

// (icf_scan_kernel, the exclusive scan of the transpose: itemcf_internal.h)
__device__ __forceinline__ float icf_sim(int c, int ni, int nj, double shrink) {
#pragma clang fp contract(off)
  const double prod = (double)ni * (double)nj;
  const double den = sqrt(prod) + shrink;
  return (float)((double)c / den);
}

// The weighted sim: c, ni, nj in fixed point, shrink_ss = (shrink * s) * s.
__device__ __forceinline__ float icf_sim_w(unsigned long long c, unsigned long long ni,
                                           unsigned long long nj, double shrink_ss) {
#pragma clang fp contract(off)
  const double prod = (double)ni * (double)nj;
  const double den = sqrt(prod) + shrink_ss;
  return (float)((double)c / den);
}

// One workgroup per item i; W counters of dynamic LDS (at least 2 KiB: the merge reuses it).
// WT: the counters are uint64 and a thread adds q_ui * q_uj.
template <bool WT>
__global__ __launch_bounds__(256) void icf_cooc_kernel(
    const int64_t* __restrict__ hist_ptr, const int32_t* __restrict__ hist_idx,
    const int* __restrict__ cnt, const int* __restrict__ tptr, const int* __restrict__ tusers,
    int64_t I, int N, double shrink, int W, int32_t* __restrict__ nbr_idx,
    float* __restrict__ nbr_val, const uint32_t* __restrict__ hist_q,
    const uint32_t* __restrict__ tq, const unsigned long long* __restrict__ nsq,
    const unsigned* __restrict__ wmax) {
  extern __shared__ int icf_lds[];
  using counter_t = std::conditional_t<WT, unsigned long long, int>;
  counter_t* c = reinterpret_cast<counter_t*>(icf_lds);
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int i = blockIdx.x;
  const int ni = cnt[i];
  const int t0 = tptr[i];
  unsigned long long nwi = 0;
  double shrink_ss = 0.0;
  if constexpr (WT) {
    if (ni > 0) {  // then w_max > 0
#pragma clang fp contract(off)
      const double s = icf_scale(*wmax);
      shrink_ss = (shrink * s) * s;
      nwi = nsq[i];
    }
  }
  float lv = -__builtin_inff();
  int li = HNM_SENTINEL_IDX;
  if (ni > 0) {  // uniform over the workgroup
    for (int x = t; x < W; x += 256) c[x] = 0;
    __syncthreads();
    for (int64_t w0 = 0; w0 < I; w0 += W) {
      const int64_t w1 = std::min<int64_t>(I, w0 + W);
      const int len = (int)(w1 - w0);
      for (int q = t; q < ni; q += 256) {
        const int u = tusers[t0 + q];
        const int64_t p1 = hist_ptr[u + 1];
        int64_t p = mask_lower_bound(hist_idx, hist_ptr[u], p1, (int)w0);
        if constexpr (WT) {
          const unsigned long long qi = tq[t0 + q];
          for (; p < p1; ++p) {
            const int64_t j = hist_idx[p];
            if (j >= w1) break;
            const unsigned long long qq = qi * hist_q[p];  // <= 2^30
            if (j >= w0 && qq) atomicAdd(&c[j - w0], qq);  // a non-returning 64-bit ds_add
          }
        } else {
          for (; p < p1; ++p) {
            const int64_t j = hist_idx[p];
            if (j >= w1) break;
            if (j >= w0) atomicAdd(&c[j - w0], 1);  // result unused: a non-returning ds_add
          }
        }
      }
      __syncthreads();
      for (int g = wave * 64; g < len; g += 256) {  // trip count uniform over the wave
        const int x = g + lane;
        counter_t cc = 0;
        if (x < len) {
          cc = c[x];
          if (cc) c[x] = 0;
        }
        const int j = (int)w0 + x;
        const bool valid = cc > 0 && j != i;
        float sim = 0.f;
        if constexpr (WT) {
          if (valid) sim = icf_sim_w(cc, nwi, nsq[j], shrink_ss);
        } else {
          sim = valid ? icf_sim(cc, ni, cnt[j], shrink) : 0.f;
        }
        icf_offer(lv, li, sim, j, valid, N);
      }
      __syncthreads();
    }
  }
  icf_merge4(lv, li, reinterpret_cast<float*>(icf_lds), icf_lds + 256, N);
  if (t < N) {
    const bool pad = li == HNM_SENTINEL_IDX;
    nbr_idx[(int64_t)i * N + t] = pad ? -1 : li;
    nbr_val[(int64_t)i * N + t] = pad ? 0.f : lv;
  }
}

// ------------------------------------------------------------------ scores, top-K
// One 256-thread workgroup per batch row: out[b, 0 .. I) = the row's scores.
template <bool WT>
__global__ __launch_bounds__(256) void icf_scores_kernel(
    const int32_t* __restrict__ nbr_idx, const float* __restrict__ nbr_val, int64_t I, int N,
    const int64_t* __restrict__ hist_ptr, const int32_t* __restrict__ hist_idx, int64_t num_users,
    const int64_t* __restrict__ user_ids, float* out, int64_t ld, unsigned* err,
    const float* __restrict__ hist_w) {
  const int64_t b = blockIdx.x;
  int64_t p0, h;
  icf_row(hist_ptr, num_users, user_ids, b, err, p0, h);
  float* row = out + b * ld;
  for (int64_t x = threadIdx.x; x < I; x += 256) row[x] = 0.f;
  __syncthreads();
  icf_accumulate_dense<WT>(row, nbr_idx, nbr_val, I, N, hist_idx, hist_w, p0, h, err);
}

__device__ __forceinline__ void icf_store_topk(float lv, int li, int k, float* ov, int64_t* oi) {
  const int lane = threadIdx.x;
  if (lane < k) {
    const bool pad = li == HNM_SENTINEL_IDX;
    ov[lane] = pad ? -__builtin_inff() : lv;
    oi[lane] = pad ? -1 : li;
  }
}

// One wave per batch row.  Rows whose h * N exceeds the table append themselves to dense_rows.
template <bool WT>
__global__ __launch_bounds__(64) void icf_topk_kernel(
    const int32_t* __restrict__ nbr_idx, const float* __restrict__ nbr_val, int64_t I, int N,
    const int64_t* __restrict__ hist_ptr, const int32_t* __restrict__ hist_idx, int64_t num_users,
    const int64_t* __restrict__ user_ids, const int64_t* __restrict__ mptr,
    const int32_t* __restrict__ midx, int k, float* __restrict__ out_val,
    int64_t* __restrict__ out_idx, int* __restrict__ dense_rows, int* ndense, unsigned* err,
    const float* __restrict__ hist_w) {
  __shared__ int key[ICF_TABLE];
  __shared__ float val[ICF_TABLE];
  const int64_t b = blockIdx.x;
  const int lane = threadIdx.x;
  int64_t p0, h;
  icf_row(hist_ptr, num_users, user_ids, b, err, p0, h);
  if (h * N > ICF_TABLE) {  // uniform
    if (lane == 0) dense_rows[atomicAdd(ndense, 1)] = (int)b;
    return;
  }
  int bits = 6;
  while ((1 << bits) < 2 * h * N && (1 << bits) < ICF_TABLE) ++bits;
  const int cap = 1 << bits;  // >= h * N: every distinct item finds a slot
  for (int x = lane; x < cap; x += 64) {
    key[x] = -1;
    val[x] = 0.f;
  }
  __syncthreads();
  int nidx;
  float nval;
  icf_step_load<WT>(nbr_idx, nbr_val, I, N, hist_idx, hist_w, p0, h, 0, err, nidx, nval);
  for (int64_t s = 0; s < h; ++s) {
    const int cidx = nidx;
    const float cval = nval;
    icf_step_load<WT>(nbr_idx, nbr_val, I, N, hist_idx, hist_w, p0, h, s + 1, err, nidx, nval);
    if (cidx >= 0) {
      unsigned slot = ((unsigned)cidx * 2654435761u) >> (32 - bits);
      for (;;) {
        const int prev = atomicCAS(&key[slot], -1, cidx);
        if (prev == -1 || prev == cidx) break;
        slot = (slot + 1) & (cap - 1);
      }
      val[slot] = val[slot] + cval;  // this step's items are distinct: the slot is this lane's
    }
    __syncthreads();  // the next step reads what this one wrote (another lane's item)
  }
  int64_t m0 = 0, m1 = 0;
  if (mptr) {
    m0 = mptr[b];
    m1 = mptr[b + 1];
  }
  float lv = -__builtin_inff();
  int li = HNM_SENTINEL_IDX;
  for (int g = 0; g < cap; g += 64) {
    const int kx = key[g + lane];
    const float vx = val[g + lane];
    bool ok = kx >= 0 && vx > 0.f &&
              hnm_better(vx, kx, hnm_readlane_f(lv, k - 1), hnm_readlane_i(li, k - 1));
    if (ok && m1 > m0) ok = !icf_masked(midx, m0, m1, kx);
    icf_offer(lv, li, vx, kx, ok, k);
  }
  icf_store_topk(lv, li, k, out_val + b * k, out_idx + b * k);
}

// The dense route: workgroup w owns workspace row w and takes the queued rows w, w + grid, ...
template <bool WT>
__global__ __launch_bounds__(256) void icf_topk_dense_kernel(
    const int32_t* __restrict__ nbr_idx, const float* __restrict__ nbr_val, int64_t I, int N,
    const int64_t* __restrict__ hist_ptr, const int32_t* __restrict__ hist_idx, int64_t num_users,
    const int64_t* __restrict__ user_ids, const int64_t* __restrict__ mptr,
    const int32_t* __restrict__ midx, int k, float* __restrict__ out_val,
    int64_t* __restrict__ out_idx, const int* __restrict__ dense_rows, const int* ndense,
    float* pool, unsigned* err, const float* __restrict__ hist_w) {
  __shared__ float mv[256];
  __shared__ int mi[256];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int n = *ndense;
  float* row = pool + (int64_t)blockIdx.x * I;
  for (int r = blockIdx.x; r < n; r += gridDim.x) {
    const int64_t b = dense_rows[r];
    int64_t p0, h;
    icf_row(hist_ptr, num_users, user_ids, b, err, p0, h);
    for (int64_t x = t; x < I; x += 256) row[x] = 0.f;
    __syncthreads();
    icf_accumulate_dense<WT>(row, nbr_idx, nbr_val, I, N, hist_idx, hist_w, p0, h, err);
    int64_t m0 = 0, m1 = 0;
    if (mptr) {
      m0 = mptr[b];
      m1 = mptr[b + 1];
    }
    float lv = -__builtin_inff();
    int li = HNM_SENTINEL_IDX;
    for (int64_t g = wave * 64; g < I; g += 256) {  // trip count uniform over the wave
      const int64_t x = g + lane;
      const float vx = x < I ? row[x] : 0.f;
      bool ok = vx > 0.f && hnm_better(vx, (int)x, hnm_readlane_f(lv, k - 1),
                                       hnm_readlane_i(li, k - 1));
      if (ok && m1 > m0) ok = !icf_masked(midx, m0, m1, (int)x);
      icf_offer(lv, li, vx, (int)x, ok, k);
    }
    icf_merge4(lv, li, mv, mi, k);
    if (t < 64) icf_store_topk(lv, li, k, out_val + b * k, out_idx + b * k);
    __syncthreads();  // mv / mi and the workspace row are reused by the next queued row
  }
}

hnm_status icf_table_check(const char* what, hnm_ctx* ctx, const int32_t* nbr_idx,
                           const float* nbr_val, int64_t num_items, int N, const int64_t* hist_ptr,
                           const int32_t* hist_idx, int64_t num_users, int64_t B) {
  HNM_REQUIRE(ctx, HNM_EINVAL, "%s: ctx is NULL", what);
  HNM_REQUIRE(N >= 1 && N <= ICF_MAX_N, HNM_EINVAL, "%s: 1 <= N <= %d", what, ICF_MAX_N);
  HNM_REQUIRE(B >= 0 && num_items >= 0 && num_users >= 0, HNM_EINVAL, "%s: bad size", what);
  HNM_REQUIRE(B <= INT32_MAX && num_items < INT_BIG, HNM_EUNSUPPORTED,
              "%s: B or num_items exceeds 2^31 - 1", what);
  if (B == 0) return HNM_OK;
  HNM_REQUIRE((nbr_idx && nbr_val) || num_items == 0, HNM_EINVAL, "%s: NULL neighbour table", what);
  HNM_REQUIRE((hist_ptr && hist_idx) || num_users == 0, HNM_EINVAL, "%s: NULL history", what);
  return HNM_OK;
}

// The fit of both entries; hist_w NULL: the unweighted kernels.
template <bool WT>
hnm_status icf_fit(hnm_ctx* ctx, const int64_t* hist_ptr, const int32_t* hist_idx,
                   const float* hist_w, int64_t num_users, int64_t num_items, int N, double shrink,
                   int64_t max_history, int window, int32_t* nbr_idx, float* nbr_val,
                   int64_t* item_count) {
  HNM_CTX_DEVICE(ctx);
  HNM_REQUIRE(ctx, HNM_EINVAL, "itemcf_fit: ctx is NULL");
  HNM_REQUIRE(N >= 1 && N <= ICF_MAX_N, HNM_EINVAL, "itemcf_fit: 1 <= N <= %d", ICF_MAX_N);
  HNM_REQUIRE(num_users >= 0 && num_items >= 0 && max_history >= 0, HNM_EINVAL,
              "itemcf_fit: bad size");
  HNM_REQUIRE(shrink >= 0.0 && std::isfinite(shrink), HNM_EINVAL,
              "itemcf_fit: shrink must be finite and >= 0");
  HNM_REQUIRE(window == 0 || (window >= 64 && window <= ICF_WINDOW_MAX && window % 64 == 0),
              HNM_EINVAL, "itemcf_fit: window must be 0 or a multiple of 64 in [64, %d]",
              ICF_WINDOW_MAX);
  HNM_REQUIRE(num_users <= INT32_MAX && num_items < INT_BIG, HNM_EUNSUPPORTED,
              "itemcf_fit: num_users or num_items exceeds 2^31 - 1");
  if (num_items == 0) return HNM_OK;
  HNM_REQUIRE(nbr_idx && nbr_val && item_count, HNM_EINVAL, "itemcf_fit: NULL output");
  HNM_REQUIRE((hist_ptr && hist_idx) || num_users == 0, HNM_EINVAL, "itemcf_fit: NULL history");
  const int64_t I = num_items;
  int64_t nnz = 0;
  if (num_users > 0) {  // the transpose is sized by the CSR's last offset
    HNM_HIP_CHECK(hipMemcpyAsync(&nnz, hist_ptr + num_users, sizeof(int64_t),
                                 hipMemcpyDeviceToHost, ctx->stream));
    HNM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  }
  HNM_REQUIRE(nnz >= 0 && nnz <= INT32_MAX, HNM_EUNSUPPORTED,
              "itemcf_fit: the history holds %lld entries (0 .. 2^31 - 1 supported)",
              (long long)nnz);
  const size_t s_cnt = hnm_align((size_t)I * 4), s_ptr = hnm_align((size_t)(I + 1) * 4),
               s_usr = hnm_align((size_t)std::max<int64_t>(nnz, 1) * 4);
  // weighted: + tq and hist_q (an entry each), nsq (uint64 per item), w_max
  const size_t s_nsq = hnm_align((size_t)I * 8), s_max = 256;
  const size_t plain = 2 * s_cnt + s_ptr + s_usr;
  char* ws = nullptr;
  hnm_status st = hnm_workspace(ctx, plain + (WT ? 2 * s_usr + s_nsq + s_max : 0), (void**)&ws);
  if (st != HNM_OK) return st;
  int* cnt = (int*)ws;
  int* cursor = (int*)(ws + s_cnt);
  int* tptr = (int*)(ws + 2 * s_cnt);
  int* tusers = (int*)(ws + 2 * s_cnt + s_ptr);
  uint32_t* tq = WT ? (uint32_t*)(ws + plain) : nullptr;
  uint32_t* hist_q = WT ? (uint32_t*)(ws + plain + s_usr) : nullptr;
  unsigned long long* nsq = WT ? (unsigned long long*)(ws + plain + 2 * s_usr) : nullptr;
  unsigned* wmax = WT ? (unsigned*)(ws + plain + 2 * s_usr + s_nsq) : nullptr;
  HNM_HIP_CHECK(hipMemsetAsync(cnt, 0, (size_t)I * 4, ctx->stream));
  if (WT) HNM_HIP_CHECK(hipMemsetAsync(nsq, 0, s_nsq + s_max, ctx->stream));  // nsq and w_max
  const unsigned ugrid = (unsigned)std::min<int64_t>(ICF_GRID_USERS, hnm_cdiv(num_users, 256));
  if (num_users > 0) {
    if (WT) {
      hipLaunchKernelGGL(icf_wmax_kernel, dim3(ugrid), dim3(256), 0, ctx->stream, hist_ptr,
                         hist_idx, hist_w, num_users, I, nnz, max_history, wmax);
      HNM_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL((icf_transpose_kernel<false, WT>), dim3(ugrid), dim3(256), 0, ctx->stream,
                       hist_ptr, hist_idx, num_users, I, nnz, max_history, cnt, (int*)nullptr,
                       ctx->err_dev, hist_w, wmax, hist_q, tq, nsq);
    HNM_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(icf_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, cnt, I, tptr, cursor,
                     item_count);
  HNM_LAUNCH_CHECK();
  if (num_users > 0) {
    hipLaunchKernelGGL((icf_transpose_kernel<true, WT>), dim3(ugrid), dim3(256), 0, ctx->stream,
                       hist_ptr, hist_idx, num_users, I, nnz, max_history, cursor, tusers,
                       ctx->err_dev, hist_w, wmax, hist_q, tq, nsq);
    HNM_LAUNCH_CHECK();
  }
  int W = window ? window : (WT ? ICF_WWINDOW_DEFAULT : ICF_WINDOW_DEFAULT);
  W = (int)std::min<int64_t>(W, hnm_cdiv(I, 64) * 64);
  const size_t lds = WT ? (size_t)std::max(W, 256) * 8 : (size_t)std::max(W, 512) * 4;
  if (lds > 64 * 1024)  // the weighted fit at more than 8,192 columns: one workgroup a CU
    (void)hipFuncSetAttribute((const void*)icf_cooc_kernel<WT>,
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(icf_cooc_kernel<WT>, dim3((unsigned)I), dim3(256), lds, ctx->stream, hist_ptr,
                     hist_idx, cnt, tptr, tusers, I, N, shrink, W, nbr_idx, nbr_val, hist_q, tq,
                     nsq, wmax);
  HNM_LAUNCH_CHECK();
  return HNM_OK;
}

template <bool WT>
hnm_status icf_scores(hnm_ctx* ctx, const int32_t* nbr_idx, const float* nbr_val,
                      int64_t num_items, int N, const int64_t* hist_ptr, const int32_t* hist_idx,
                      const float* hist_w, int64_t num_users, const int64_t* user_ids, int64_t B,
                      float* out, int64_t ld) {
  HNM_CTX_DEVICE(ctx);
  hnm_status st = icf_table_check("itemcf_scores", ctx, nbr_idx, nbr_val, num_items, N, hist_ptr,
                                  hist_idx, num_users, B);
  if (st != HNM_OK) return st;
  if (B == 0 || num_items == 0) return HNM_OK;
  HNM_REQUIRE(out && ld >= num_items, HNM_EINVAL, "itemcf_scores: NULL output or ld < num_items");
  hipLaunchKernelGGL(icf_scores_kernel<WT>, dim3((unsigned)B), dim3(256), 0, ctx->stream, nbr_idx,
                     nbr_val, num_items, N, hist_ptr, hist_idx, num_users, user_ids, out, ld,
                     ctx->err_dev, hist_w);
  HNM_LAUNCH_CHECK();
  return HNM_OK;
}

template <bool WT>
hnm_status icf_topk(hnm_ctx* ctx, const int32_t* nbr_idx, const float* nbr_val, int64_t num_items,
                    int N, const int64_t* hist_ptr, const int32_t* hist_idx, const float* hist_w,
                    int64_t num_users, const int64_t* user_ids, int64_t B,
                    const int64_t* mask_ptr, const int32_t* mask_idx, int k, float* out_val,
                    int64_t* out_idx) {
  HNM_CTX_DEVICE(ctx);
  hnm_status st = icf_table_check("itemcf_topk", ctx, nbr_idx, nbr_val, num_items, N, hist_ptr,
                                  hist_idx, num_users, B);
  if (st != HNM_OK) return st;
  HNM_REQUIRE(k >= 0 && k <= 64, HNM_EINVAL, "itemcf_topk: 0 <= k <= 64");
  if (B == 0 || k == 0) return HNM_OK;
  HNM_REQUIRE(out_val && out_idx, HNM_EINVAL, "itemcf_topk: NULL output");
  HNM_REQUIRE(!mask_ptr || mask_idx, HNM_EINVAL, "itemcf_topk: mask_ptr without mask_idx");
  const int pool_rows = (int)std::min<int64_t>(B, ICF_DENSE_POOL);
  const size_t s_rows = hnm_align((size_t)B * 4), s_n = 256;
  char* ws = nullptr;
  st = hnm_workspace(ctx, s_n + s_rows + (size_t)pool_rows * (size_t)num_items * 4, (void**)&ws);
  if (st != HNM_OK) return st;
  int* ndense = (int*)ws;
  int* dense_rows = (int*)(ws + s_n);
  float* pool = (float*)(ws + s_n + s_rows);
  HNM_HIP_CHECK(hipMemsetAsync(ndense, 0, sizeof(int), ctx->stream));
  hnm_timer_begin(ctx, HNM_TIME_SCORE);
  hipLaunchKernelGGL(icf_topk_kernel<WT>, dim3((unsigned)B), dim3(64), 0, ctx->stream, nbr_idx,
                     nbr_val, num_items, N, hist_ptr, hist_idx, num_users, user_ids, mask_ptr,
                     mask_idx, k, out_val, out_idx, dense_rows, ndense, ctx->err_dev, hist_w);
  hnm_timer_end(ctx, HNM_TIME_SCORE);
  HNM_LAUNCH_CHECK();
  hipLaunchKernelGGL(icf_topk_dense_kernel<WT>, dim3((unsigned)pool_rows), dim3(256), 0,
                     ctx->stream, nbr_idx, nbr_val, num_items, N, hist_ptr, hist_idx, num_users,
                     user_ids, mask_ptr, mask_idx, k, out_val, out_idx, dense_rows, ndense, pool,
                     ctx->err_dev, hist_w);
  HNM_LAUNCH_CHECK();
  return HNM_OK;
}

}  // namespace

extern "C" hnm_status hnm_itemcf_fit_f32(hnm_ctx* ctx, const int64_t* hist_ptr,
                                         const int32_t* hist_idx, int64_t num_users,
                                         int64_t num_items, int N, double shrink,
                                         int64_t max_history, int window, int32_t* nbr_idx,
                                         float* nbr_val, int64_t* item_count) {
  return icf_fit<false>(ctx, hist_ptr, hist_idx, nullptr, num_users, num_items, N, shrink,
                        max_history, window, nbr_idx, nbr_val, item_count);
}

extern "C" hnm_status hnm_itemcf_fit_weighted_f32(hnm_ctx* ctx, const int64_t* hist_ptr,
                                                  const int32_t* hist_idx, const float* hist_w,
                                                  int64_t num_users, int64_t num_items, int N,
                                                  double shrink, int64_t max_history, int window,
                                                  int32_t* nbr_idx, float* nbr_val,
                                                  int64_t* item_count) {
  if (!hist_w)
    return icf_fit<false>(ctx, hist_ptr, hist_idx, nullptr, num_users, num_items, N, shrink,
                          max_history, window, nbr_idx, nbr_val, item_count);
  return icf_fit<true>(ctx, hist_ptr, hist_idx, hist_w, num_users, num_items, N, shrink,
                       max_history, window, nbr_idx, nbr_val, item_count);
}

extern "C" hnm_status hnm_itemcf_scores_f32(hnm_ctx* ctx, const int32_t* nbr_idx,
                                            const float* nbr_val, int64_t num_items, int N,
                                            const int64_t* hist_ptr, const int32_t* hist_idx,
                                            int64_t num_users, const int64_t* user_ids, int64_t B,
                                            float* out, int64_t ld) {
  return icf_scores<false>(ctx, nbr_idx, nbr_val, num_items, N, hist_ptr, hist_idx, nullptr,
                           num_users, user_ids, B, out, ld);
}

extern "C" hnm_status hnm_itemcf_scores_weighted_f32(hnm_ctx* ctx, const int32_t* nbr_idx,
                                                     const float* nbr_val, int64_t num_items,
                                                     int N, const int64_t* hist_ptr,
                                                     const int32_t* hist_idx, const float* hist_w,
                                                     int64_t num_users, const int64_t* user_ids,
                                                     int64_t B, float* out, int64_t ld) {
  if (!hist_w)
    return icf_scores<false>(ctx, nbr_idx, nbr_val, num_items, N, hist_ptr, hist_idx, nullptr,
                             num_users, user_ids, B, out, ld);
  return icf_scores<true>(ctx, nbr_idx, nbr_val, num_items, N, hist_ptr, hist_idx, hist_w,
                          num_users, user_ids, B, out, ld);
}

extern "C" hnm_status hnm_itemcf_topk_f32(hnm_ctx* ctx, const int32_t* nbr_idx,
                                          const float* nbr_val, int64_t num_items, int N,
                                          const int64_t* hist_ptr, const int32_t* hist_idx,
                                          int64_t num_users, const int64_t* user_ids, int64_t B,
                                          const int64_t* mask_ptr, const int32_t* mask_idx, int k,
                                          float* out_val, int64_t* out_idx) {
  return icf_topk<false>(ctx, nbr_idx, nbr_val, num_items, N, hist_ptr, hist_idx, nullptr,
                         num_users, user_ids, B, mask_ptr, mask_idx, k, out_val, out_idx);
}

extern "C" hnm_status hnm_itemcf_topk_weighted_f32(hnm_ctx* ctx, const int32_t* nbr_idx,
                                                   const float* nbr_val, int64_t num_items, int N,
                                                   const int64_t* hist_ptr,
                                                   const int32_t* hist_idx, const float* hist_w,
                                                   int64_t num_users, const int64_t* user_ids,
                                                   int64_t B, const int64_t* mask_ptr,
                                                   const int32_t* mask_idx, int k, float* out_val,
                                                   int64_t* out_idx) {
  if (!hist_w)
    return icf_topk<false>(ctx, nbr_idx, nbr_val, num_items, N, hist_ptr, hist_idx, nullptr,
                           num_users, user_ids, B, mask_ptr, mask_idx, k, out_val, out_idx);
  return icf_topk<true>(ctx, nbr_idx, nbr_val, num_items, N, hist_ptr, hist_idx, hist_w,
                        num_users, user_ids, B, mask_ptr, mask_idx, k, out_val, out_idx);
}

extern "C" hnm_status hnm_itemcf_route(hnm_ctx* ctx, int N, int64_t history_len, int* route) {
  HNM_REQUIRE(ctx && route, HNM_EINVAL, "itemcf_route: NULL argument");
  HNM_REQUIRE(N >= 1 && N <= ICF_MAX_N && history_len >= 0, HNM_EINVAL,
              "itemcf_route: 1 <= N <= %d, history_len >= 0", ICF_MAX_N);
  *route = history_len * N > ICF_TABLE ? 1 : 0;
  return HNM_OK;
}

