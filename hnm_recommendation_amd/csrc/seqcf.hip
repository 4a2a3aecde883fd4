// SequentialCF: the directed "bought a, then b within max_gap days" table, fitted over the
// time-ordered user -> event CSR (UserSequence.seq_ptr / seq_item / seq_day: a user's events by
// day ascending, then item ascending).  No reference counterpart: the contract is stated in
// include/hnm.h and restated in numpy by tests/seqcf_oracle.py.
//
// Fit.  Users with more than max_history events are dropped.  Over the kept users
//   n[a]    = events of item a                                  (int32 atomics -> item_count)
//   T[a, b] = sum of gap_q[t - s - 1] over the ordered pairs of one user's events (a, day s),
//             (b, day t) with 1 <= t - s <= max_gap; a != b unless repeat_buys   (uint64, LDS)
//   sim(a -> b) = float( double(T) / ( 32768.0 * ( sqrt(double(n_a) * double(n_b)) + shrink ) ) )
// for T > 0, one rounding per operation, contraction off; row a keeps the N best in (sim desc, b
// asc) order, padded with (-1, 0.0f).  T is an integer below 2^60 (hnm.h has the bound), so the
// result is the same bits on every run and at every window.
//
// Shape: histogram -> scan -> fill give the item -> event transpose, as in itemcf.hip; here the
// fill pass (a thread per user, two pointers that only move forward) also finds each event's
// forward range [lo, hi): the user's later events from the first of a later day to the last
// within max_gap days, and stores (lo, hi, day) beside the item.  Then one workgroup per item a,
// a thread per event of a, on one of two routes that give the same T and therefore the same bits:
//   table   -- rows whose forward ranges hold at most SQ_TABLE / 2 events in all (an upper bound
//              of their distinct successors): an LDS open-addressing table keyed by b, sized
//              from that sum, slots claimed by compare-and-swap (icf_topk_kernel's idiom), a
//              64-bit LDS add per range entry; every range is read once.
//   windows -- the other rows queue themselves; a second kernel walks the catalogue for each in
//              windows of `window` uint64 LDS counters, the gap table in LDS behind them, as the
//              weighted icf_cooc_kernel does.  The rows are ordered by day, not by item, so there
//              is nothing to search for: every window pass re-reads the whole range.
// Measured at the H&M shape (tools/seqcf_bench.py; max_gap 28, 24 M range entries): the windows
// alone 188 ms (profiles/seqcf_bench_windows_only.txt), with the table 181 ms
// (profiles/seqcf_bench.txt): the sweep of 7 x 16,384 counters for each of 105,542 mostly small
// rows was not what the time goes to.  Halving the window adds 90 ms, so the windows of the
// queued rows are: the most popular item's 1.4 M events are walked by ONE workgroup once a
// window, and that row's passes run one after another.  Giving each (row, window) its own
// workgroup and merging the per-window lists is the open item.  The counter -> sim -> wave list ->
// merge tail is ItemCF's (itemcf_internal.h) on both routes.
#include "hnm_device.h"
#include "hnm_internal.h"
#include "itemcf_internal.h"
#include "seqcf_args.h"

#include <cmath>

namespace {

// uint64 counters per LDS pass of the window route (128 KiB, plus the gap table: one workgroup a
// CU).  Every pass re-reads every forward range of the row, so fewer passes weigh more here than
// in the weighted ItemCF fit: 16,384 -> 181 ms, 8,192 -> 273 ms at max_gap 28.
constexpr int SQ_WINDOW_DEFAULT = 16384;
// Slots of the table route (4 B keys + 8 B sums: 24 KiB, six workgroups a CU); a row takes it when
// its ranges hold at most half as many entries, so a probe sequence always ends.
constexpr int SQ_TABLE = 2048;
constexpr int SQ_GRID_WINDOWS = 512;  // workgroups that share the queued rows
constexpr int SQ_GRID_USERS = 4096;

// A user's row if the fit keeps the user (1 <= len <= max_history is not required: an empty row
// is kept and holds nothing).
__device__ __forceinline__ bool sq_kept(const int64_t* seq_ptr, int64_t u, int64_t nnz,
                                        int64_t max_history, unsigned* err, int64_t& p0,
                                        int64_t& p1) {
  p0 = seq_ptr[u];
  p1 = seq_ptr[u + 1];
  if (p0 < 0 || p1 < p0 || p1 > nnz) {
    hnm_flag(err, HNM_ERR_OOB);
    return false;
  }
  return p1 - p0 <= max_history;
}

// FILL = false: cnt[a] += 1 per (kept user, event of a).  FILL = true: the event's forward range
// and day go to slot cursor[a]++ of the transpose.
template <bool FILL>
__global__ __launch_bounds__(256) void sq_transpose_kernel(
    const int64_t* __restrict__ seq_ptr, const int32_t* __restrict__ seq_item,
    const int32_t* __restrict__ seq_day, int64_t num_users, int64_t I, int64_t nnz,
    int64_t max_history, int max_gap, int* __restrict__ cnt, int* __restrict__ tlo,
    int* __restrict__ thi, int* __restrict__ tday, unsigned* err) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x; u < num_users; u += stride) {
    int64_t p0, p1;
    if (!sq_kept(seq_ptr, u, nnz, max_history, FILL ? nullptr : err, p0, p1)) continue;
    int64_t lo = p0, hi = p0;  // both only move forward: one pass over the row
    for (int64_t p = p0; p < p1; ++p) {
      const int32_t a = seq_item[p];
      if (a < 0 || a >= I) {
        if (!FILL) hnm_flag(err, HNM_ERR_OOB);
        continue;
      }
      if constexpr (FILL) {
        const int64_t s = seq_day[p];
        if (lo <= p) lo = p + 1;
        while (lo < p1 && (int64_t)seq_day[lo] <= s) ++lo;  // same-day events do not count
        if (hi < lo) hi = lo;
        while (hi < p1 && (int64_t)seq_day[hi] - s <= max_gap) ++hi;
        const int at = atomicAdd(&cnt[a], 1);
        tlo[at] = (int)lo;  // positions < nnz < 2^31
        thi[at] = (int)hi;
        tday[at] = (int)s;
      } else {
        atomicAdd(&cnt[a], 1);
      }
    }
  }
}

__device__ __forceinline__ float sq_sim(unsigned long long T, int na, int nb, double shrink) {
#pragma clang fp contract(off)
  const double prod = (double)na * (double)nb;
  const double root = sqrt(prod);
  const double den = 32768.0 * (root + shrink);
  return (float)((double)T / den);
}

// Whether the range entry at r counts for item a, and with which weight (0: not at all).  The day
// test is made on every entry, so a sequence that is not sorted by day still stays in bounds.
__device__ __forceinline__ unsigned long long sq_entry(const int32_t* __restrict__ seq_day, int r,
                                                       int s, int a, int b, int max_gap,
                                                       bool repeat, const uint32_t* gq) {
  if (b == a && !repeat) return 0;
  const int64_t d = (int64_t)seq_day[r] - s;
  if (d < 1 || d > max_gap) return 0;
  return gq[d - 1];
}

// The table route, one workgroup per item a; rows that do not fit append themselves to big_items.
__global__ __launch_bounds__(256) void sq_table_kernel(
    const int32_t* __restrict__ seq_item, const int32_t* __restrict__ seq_day,
    const int* __restrict__ cnt, const int* __restrict__ tptr, const int* __restrict__ tlo,
    const int* __restrict__ thi, const int* __restrict__ tday, int64_t I, int N, double shrink,
    int max_gap, const uint32_t* __restrict__ gap_q, int repeat_buys,
    int32_t* __restrict__ nbr_idx, float* __restrict__ nbr_val, int* __restrict__ big_items,
    int* nbig) {
  __shared__ int key[SQ_TABLE];
  __shared__ unsigned long long val[SQ_TABLE];
  __shared__ unsigned long long rtot;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int a = blockIdx.x;
  const int na = cnt[a];
  const int t0 = tptr[a];
  const bool repeat = repeat_buys != 0;
  float lv = -__builtin_inff();
  int li = HNM_SENTINEL_IDX;
  if (na > 0) {  // uniform over the workgroup
    if (t == 0) rtot = 0;
    __syncthreads();
    unsigned long long mine = 0;
    for (int q = t; q < na; q += 256) mine += (unsigned)(thi[t0 + q] - tlo[t0 + q]);
    if (mine) atomicAdd(&rtot, mine);
    __syncthreads();
    const unsigned long long R = rtot;  // at least the row's distinct successors
    if (R > SQ_TABLE / 2) {             // uniform: the window route writes this row
      if (t == 0) big_items[atomicAdd(nbig, 1)] = a;
      return;
    }
    if (R > 0) {
      int bits = 6;
      while ((1u << bits) < 2 * R) ++bits;
      const int cap = 1 << bits;  // a multiple of 64, <= SQ_TABLE, at most half full
      for (int x = t; x < cap; x += 256) {
        key[x] = -1;
        val[x] = 0;
      }
      __syncthreads();
      for (int q = t; q < na; q += 256) {  // an item with more events than threads
        const int hi = thi[t0 + q], s = tday[t0 + q];
        for (int r = tlo[t0 + q]; r < hi; ++r) {  // a range of any length
          const int b = seq_item[r];
          if (b < 0 || b >= I) continue;
          const unsigned long long g = sq_entry(seq_day, r, s, a, b, max_gap, repeat, gap_q);
          if (!g) continue;
          unsigned slot = ((unsigned)b * 2654435761u) >> (32 - bits);
          for (;;) {
            const int prev = atomicCAS(&key[slot], -1, b);
            if (prev == -1 || prev == b) break;
            slot = (slot + 1) & (cap - 1);
          }
          atomicAdd(&val[slot], g);  // result unused: a non-returning 64-bit ds_add
        }
      }
      __syncthreads();
      for (int g = wave * 64; g < cap; g += 256) {  // trip count uniform over the wave
        const int b = key[g + lane];
        const unsigned long long cc = val[g + lane];
        const bool valid = b >= 0 && cc > 0;
        const float sim = valid ? sq_sim(cc, na, cnt[b], shrink) : 0.f;
        icf_offer(lv, li, sim, b, valid, N);
      }
      __syncthreads();  // the merge reuses val
    }
  }
  icf_merge4(lv, li, reinterpret_cast<float*>(val), reinterpret_cast<int*>(val) + 256, N);
  if (t < N) {
    const bool pad = li == HNM_SENTINEL_IDX;
    nbr_idx[(int64_t)a * N + t] = pad ? -1 : li;
    nbr_val[(int64_t)a * N + t] = pad ? 0.f : lv;
  }
}

// One event's forward range [lo, hi) against the window [w0, w1) of counters c.
__device__ __forceinline__ void sq_walk(const int32_t* __restrict__ seq_item,
                                        const int32_t* __restrict__ seq_day, int lo, int hi,
                                        int s, int a, int w0, int w1, int max_gap, bool repeat,
                                        const uint32_t* gq, unsigned long long* c) {
  for (int r = lo; r < hi; ++r) {
    const int b = seq_item[r];
    if (b < w0 || b >= w1) continue;
    const unsigned long long g = sq_entry(seq_day, r, s, a, b, max_gap, repeat, gq);
    if (g) atomicAdd(&c[b - w0], g);  // result unused: a non-returning 64-bit ds_add
  }
}

// The window route: workgroup w takes the queued rows w, w + grid, ...  Dynamic LDS: max(W, 256)
// uint64 counters (the merge reuses the first 2 KiB), then max_gap uint32 of the gap table.
__global__ __launch_bounds__(256) void sq_window_kernel(
    const int32_t* __restrict__ seq_item, const int32_t* __restrict__ seq_day,
    const int* __restrict__ cnt, const int* __restrict__ tptr, const int* __restrict__ tlo,
    const int* __restrict__ thi, const int* __restrict__ tday, int64_t I, int N, double shrink,
    int W, int max_gap, const uint32_t* __restrict__ gap_q, int repeat_buys,
    int32_t* __restrict__ nbr_idx, float* __restrict__ nbr_val,
    const int* __restrict__ big_items, const int* nbig) {
  extern __shared__ unsigned long long sq_lds[];
  unsigned long long* c = sq_lds;
  uint32_t* gq = reinterpret_cast<uint32_t*>(sq_lds + std::max(W, 256));
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const bool repeat = repeat_buys != 0;
  const int n = *nbig;
  if ((int)blockIdx.x >= n) return;  // uniform
  for (int x = t; x < std::max(W, 256); x += 256) c[x] = 0;
  for (int x = t; x < max_gap; x += 256) gq[x] = gap_q[x];
  __syncthreads();
  for (int row = blockIdx.x; row < n; row += gridDim.x) {
    const int a = big_items[row];
    const int na = cnt[a];  // > 0: the row queued itself
    const int t0 = tptr[a];
    float lv = -__builtin_inff();
    int li = HNM_SENTINEL_IDX;
    int lo0 = 0, hi0 = 0, s0 = 0;  // the thread's first event
    if (t < na) {
      lo0 = tlo[t0 + t];
      hi0 = thi[t0 + t];
      s0 = tday[t0 + t];
    }
    for (int64_t w0 = 0; w0 < I; w0 += W) {
      const int64_t w1 = std::min<int64_t>(I, w0 + W);
      const int len = (int)(w1 - w0);
      sq_walk(seq_item, seq_day, lo0, hi0, s0, a, (int)w0, (int)w1, max_gap, repeat, gq, c);
      for (int q = t + 256; q < na; q += 256)  // an item with more events than threads
        sq_walk(seq_item, seq_day, tlo[t0 + q], thi[t0 + q], tday[t0 + q], a, (int)w0, (int)w1,
                max_gap, repeat, gq, c);
      __syncthreads();
      for (int g = wave * 64; g < len; g += 256) {  // trip count uniform over the wave
        const int x = g + lane;
        unsigned long long cc = 0;
        if (x < len) {
          cc = c[x];
          if (cc) c[x] = 0;
        }
        const int b = (int)w0 + x;
        const bool valid = cc > 0;
        const float sim = valid ? sq_sim(cc, na, cnt[b], shrink) : 0.f;
        icf_offer(lv, li, sim, b, valid, N);
      }
      __syncthreads();
    }
    icf_merge4(lv, li, reinterpret_cast<float*>(sq_lds), reinterpret_cast<int*>(sq_lds) + 256, N);
    if (t < N) {
      const bool pad = li == HNM_SENTINEL_IDX;
      nbr_idx[(int64_t)a * N + t] = pad ? -1 : li;
      nbr_val[(int64_t)a * N + t] = pad ? 0.f : lv;
    }
    __syncthreads();  // wave 0 has read the merge area: counters again for the next queued row
    c[t] = 0;
    __syncthreads();
  }
}

}  // namespace

extern "C" hnm_status hnm_seqcf_fit_f32(hnm_ctx* ctx, const int64_t* seq_ptr,
                                        const int32_t* seq_item, const int32_t* seq_day,
                                        int64_t num_users, int64_t num_items, int N, double shrink,
                                        int64_t max_history, int max_gap, const uint32_t* gap_q,
                                        int repeat_buys, int window, int32_t* nbr_idx,
                                        float* nbr_val, int64_t* item_count) {
  HNM_CTX_DEVICE(ctx);
  HNM_REQUIRE(ctx, HNM_EINVAL, "seqcf_fit: ctx is NULL");
  const char* bad = sq_bad_args(N, shrink, max_history, max_gap, repeat_buys, window, num_users,
                                num_items);
  HNM_REQUIRE(!bad, HNM_EINVAL, "%s", bad);
  HNM_REQUIRE(num_users <= INT32_MAX && num_items < INT_BIG, HNM_EUNSUPPORTED,
              "seqcf_fit: num_users or num_items exceeds 2^31 - 1");
  if (num_items == 0) return HNM_OK;
  HNM_REQUIRE(nbr_idx && nbr_val && item_count && gap_q, HNM_EINVAL,
              "seqcf_fit: NULL output or gap table");
  HNM_REQUIRE((seq_ptr && seq_item && seq_day) || num_users == 0, HNM_EINVAL,
              "seqcf_fit: NULL sequence");
  const int64_t I = num_items;
  uint32_t gap_host[SQ_MAX_GAP];
  int64_t nnz = 0;
  HNM_HIP_CHECK(hipMemcpyAsync(gap_host, gap_q, (size_t)max_gap * sizeof(uint32_t),
                               hipMemcpyDeviceToHost, ctx->stream));
  if (num_users > 0)  // the transpose is sized by the CSR's last offset
    HNM_HIP_CHECK(hipMemcpyAsync(&nnz, seq_ptr + num_users, sizeof(int64_t), hipMemcpyDeviceToHost,
                                 ctx->stream));
  HNM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  const int bad_gap = sq_bad_gap_entry(gap_host, max_gap);
  HNM_REQUIRE(bad_gap < 0, HNM_EINVAL, "seqcf_fit: gap_q[%d] = %u exceeds 32768", bad_gap,
              gap_host[bad_gap < 0 ? 0 : bad_gap]);
  HNM_REQUIRE(nnz >= 0 && nnz <= INT32_MAX, HNM_EUNSUPPORTED,
              "seqcf_fit: the sequence holds %lld events (0 .. 2^31 - 1 supported)",
              (long long)nnz);
  const size_t s_cnt = hnm_align((size_t)I * 4), s_ptr = hnm_align((size_t)(I + 1) * 4),
               s_ev = hnm_align((size_t)std::max<int64_t>(nnz, 1) * 4);
  char* ws = nullptr;
  // + the queue of the window route (an item each) and its length
  hnm_status st = hnm_workspace(ctx, 3 * s_cnt + s_ptr + 3 * s_ev + 256, (void**)&ws);
  if (st != HNM_OK) return st;
  int* cnt = (int*)ws;
  int* cursor = (int*)(ws + s_cnt);
  int* tptr = (int*)(ws + 2 * s_cnt);
  int* tlo = (int*)(ws + 2 * s_cnt + s_ptr);
  int* thi = (int*)(ws + 2 * s_cnt + s_ptr + s_ev);
  int* tday = (int*)(ws + 2 * s_cnt + s_ptr + 2 * s_ev);
  int* big_items = (int*)(ws + 2 * s_cnt + s_ptr + 3 * s_ev);
  int* nbig = (int*)(ws + 3 * s_cnt + s_ptr + 3 * s_ev);
  HNM_HIP_CHECK(hipMemsetAsync(cnt, 0, (size_t)I * 4, ctx->stream));
  HNM_HIP_CHECK(hipMemsetAsync(nbig, 0, sizeof(int), ctx->stream));
  const unsigned ugrid = (unsigned)std::min<int64_t>(SQ_GRID_USERS, hnm_cdiv(num_users, 256));
  if (num_users > 0) {
    hipLaunchKernelGGL(sq_transpose_kernel<false>, dim3(ugrid), dim3(256), 0, ctx->stream, seq_ptr,
                       seq_item, seq_day, num_users, I, nnz, max_history, max_gap, cnt,
                       (int*)nullptr, (int*)nullptr, (int*)nullptr, ctx->err_dev);
    HNM_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(icf_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, cnt, I, tptr, cursor,
                     item_count);
  HNM_LAUNCH_CHECK();
  if (num_users > 0) {
    hipLaunchKernelGGL(sq_transpose_kernel<true>, dim3(ugrid), dim3(256), 0, ctx->stream, seq_ptr,
                       seq_item, seq_day, num_users, I, nnz, max_history, max_gap, cursor, tlo,
                       thi, tday, ctx->err_dev);
    HNM_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(sq_table_kernel, dim3((unsigned)I), dim3(256), 0, ctx->stream, seq_item,
                     seq_day, cnt, tptr, tlo, thi, tday, I, N, shrink, max_gap, gap_q, repeat_buys,
                     nbr_idx, nbr_val, big_items, nbig);
  HNM_LAUNCH_CHECK();
  int W = window ? window : SQ_WINDOW_DEFAULT;
  W = (int)std::min<int64_t>(W, hnm_cdiv(I, 64) * 64);
  const size_t lds = (size_t)std::max(W, 256) * 8 + (size_t)max_gap * 4;
  if (lds > 64 * 1024)
    (void)hipFuncSetAttribute((const void*)sq_window_kernel,
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  const unsigned wgrid = (unsigned)std::min<int64_t>(SQ_GRID_WINDOWS, I);
  hipLaunchKernelGGL(sq_window_kernel, dim3(wgrid), dim3(256), lds, ctx->stream, seq_item, seq_day,
                     cnt, tptr, tlo, thi, tday, I, N, shrink, W, max_gap, gap_q, repeat_buys,
                     nbr_idx, nbr_val, big_items, nbig);
  HNM_LAUNCH_CHECK();
  return HNM_OK;
}
