// Shared by the LightGCN graph units: graph_csr.hip (normalized-adjacency CSR build),
// graph_plan.hip (host-only SpMM planning: binding, the walks' schedules, plan create / restrict /
// destroy) and graph.hip (the SpMM kernels and their launches).  Only host functions cross the
// units; no __global__ or __device__ symbol is shared between objects.
#pragma once
#include <memory>
#include <mutex>
#include <vector>

#include "hnm_internal.h"

// Fixed design constants (round 5: the measured-and-dropped A/B switches of rounds 2-4 --
// walk launch order / side stream, record prefetch in the long-row walk, column windows in the
// short walk, the CSR-order short rows, ... -- are gone; DESIGN.md §4 keeps their numbers).
//
// Row classes by entry count L (self-loop included), decided per row so that every kernel that
// sums a row (the layer kernels, rows_combine) uses the same order:
//   short  L <= SPMM_SHORT           one LPR-lane group per row, 64 / LPR rows per wave
//   long   SPMM_SHORT < L <= HEAVY   one wave per row (4 neighbour groups + a fixed tree)
//   heavy  L > HEAVY                 SEG-long segments + a finish kernel
// Graphs of up to 2^22 nodes (every BASELINE graph) run the two walks below instead: short rows
// by the column-ordered short walk, the others by the user-ordered walk; the classes above
// remain the plan-less path and the path of larger graphs (both tested).
#define HEAVY 2048
#define SEG 2048
#define SPMM_SHORT 128
// the long-row walk: 1024-thread workgroups (one per CU), 144 KiB of float4 row accumulators,
// lists cut at WALK_WIN column windows with a workgroup barrier after each (d=64 layer: no
// windows 1.635 ms, 4: 1.499, 8: 1.448, 16: 1.431-1.451, 32: 1.474), WALK_STEP entries a step
// (round 4, whole-graph layer d=64 / d=128: 4 entries 1.308 / 2.676 ms, 4 + records prefetched a
// step ahead 1.415 / 2.920, 8 entries 1.435 / 3.017), pieces cut for ~WALK_GROUPS_TARGET groups
#define WALK_THREADS 1024
#define WALK_WIN 12
// d >= 128 (512-B rows): more, narrower windows (round 6, A/B on one box, configs[4] d = 128
// step: 16 windows 7.09 ms, 24: 7.01, 32: 7.02, 64: 7.29; the d = 64 step: 8: 3.464, 12: 3.462,
// 16: 3.474, 32: 3.58 -- profiles/r11d_spmm_windows_ab.txt)
#define WALK_WIN_WIDE 24
static inline int walk_windows(int d) { return d >= 128 ? WALK_WIN_WIDE : WALK_WIN; }
#define WALK_STEP 4
#define WALK_LDS_F4 9216
#define WALK_GROUPS_TARGET 16384
// the short walk (round 4): 2 persistent 512-thread workgroups per CU, 72 KiB of float4 row
// accumulators each, 8 entries a step with the records loaded a step ahead.  Measured and
// dropped (A/B on one box, d = 64 layer, `git show a7c47dc`): the short rows one lane group
// each in CSR order 1.44 ms, two rows per group interleaved 1.72 ms, the ~600 most gathered item
// rows held in LDS 1.46-1.65 ms, column windows with barriers 1.537 / 1.602 ms (4 / 8 windows),
// vs 1.305 ms for this walk.
#define SWALK_WG_PER_CU 2
#define SWALK_THREADS 512
#define SWALK_LDS_F4 4608
#define SWALK_STEP 8
// d >= 128 (LPR >= 32): 4 entries a step (round 6, A/B on one box: configs[4] d = 128 step
// 7.02 -> 6.94 ms; 2 entries 7.33-7.37, 16 entries 8.21; d = 64 the same at 4 and 8; the long
// walk's WALK_STEP at d = 128: 2 entries 8.42, 8 entries 7.79 vs 6.94 ms at 4 --
// profiles/r11f_swalk_step_ab.txt)
#define SWALK_STEP_WIDE 4
__host__ __device__ constexpr int swalk_step(int lpr) { return lpr >= 32 ? SWALK_STEP_WIDE : SWALK_STEP; }
// Round 4, measured and dropped: aligning the workgroups of an XCD -- a bounded wait (per-XCD
// progress counters, atomics at agent scope) before each short-walk round until all but 1/8 of
// the XCD's workgroups finished the previous one, and the same before each of the long-row
// walk's column windows -- so their gathers share one window of the table in that L2: d=64
// layer 1.304 -> 1.586 ms (short walk aligned), 1.430 (walk windows), 1.699 (both); d=128
// 2.672 -> 3.235 / 2.680 / 3.237 ms.  The waits cost more than the L2 locality returns.
// (tools/gather_probe.hip: uniformly random 256-B rows gather at 8.4-8.6 TB/s from a 27 MB
// table and 7.0-7.3 TB/s from 351 MB whatever the loads in flight, 23 TB/s from an
// L2-resident 4 MB one; the two walks' 12.8 TB/s lies between: their column order already
// serves ~62 % of the gathered bytes from L2.  Round 5, tools/granule_probe.hip: gathers of
// column slices -- 32 / 64 / 128-B granules from slice tables of 3.4 / 6.8 / 13.5 MB -- run at
// 4.3 / 5.3 / 8.8 TB/s, below the walks' rate: slicing the item table per XCD cannot pay.)
// Also measured and dropped (round 4): the long-row walk split by XCD column ranges (668 ->
// 1,155 us a launch: ~4x the pieces for the same LDS slots), and the walk on the side stream
// beside the short rows (1.318 / 2.928 ms vs 1.308 / 2.676).

// Epilogue of row r (layer combine, lightgcn.py:156-158): Y[r] = y and, for rows with an
// accumulator (r >= acc_row0), acc_out = fma(alpha, y, acc_in) where acc_in == NULL means
// beta * X[r] (the alpha_0 E_0 term folded into layer 1).  Accumulators are stored from
// row acc_row0 on (items only when acc_row0 = num_users).
struct SpmmEpi {
  float* Y;
  float alpha, beta;
  const float* acc_in;
  float* acc_out;
  int64_t acc_row0;
};

// rows_combine's layer inputs E_0 .. E_{L-1} and weights alpha_0 .. alpha_L
struct CombineLayers {
  const float* E[8];
  float a[9];
  int L;
};

// The summation order rows_combine must repeat (the plan's): mode 0 plan-less (one wave per
// row, row_sum, every row: spmm_light_kernel with no heavy class); mode 1 a plan without the
// walks (short rows grouped in CSR order, long rows one wave, heavy rows segments); mode 2 a
// walk plan (long rows in the walk's piece order over the sorted copy scol / sval; short rows
// grouped over the sorted copy when the short walk is on, else over col / val).
struct CombineOrder {
  int mode;
  int short_sorted;
  const int32_t* scol;
  const float* sval;
  int64_t cap;
};

// A device array owned by a plan or a schedule: hipMalloc in alloc / upload / dup, hipFree in
// the destructor (and at once when the copy fails), move-only.  The owner is destroyed with its
// device current (hnm_spmm_plan_destroy, or a local inside an entry point's device guard).
template <typename T>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      reset();
      p_ = o.p_;
      o.p_ = nullptr;
    }
    return *this;
  }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { reset(); }

  T* get() const { return p_; }
  void reset() {
    if (p_) (void)hipFree(p_);
    p_ = nullptr;
  }
  // n elements (at least one is allocated, so an empty array still has an address)
  hnm_status alloc(size_t n) {
    reset();
    if (hipMalloc((void**)&p_, std::max<size_t>(n, 1) * sizeof(T)) != hipSuccess) {
      p_ = nullptr;
      hnm_set_error("spmm plan: hipMalloc of %zu bytes failed", n * sizeof(T));
      return HNM_ENOMEM;
    }
    return HNM_OK;
  }
  hnm_status upload(const T* host, size_t n) { return fill(host, n, hipMemcpyHostToDevice); }
  // a copy of dev[0, n); stays NULL for a NULL or empty source
  hnm_status dup(const T* dev, size_t n) {
    if (!dev || n == 0) {
      reset();
      return HNM_OK;
    }
    return fill(dev, n, hipMemcpyDeviceToDevice);
  }

 private:
  hnm_status fill(const T* src, size_t n, hipMemcpyKind kind) {
    hnm_status s = alloc(n);
    if (s) return s;
    if (n && hipMemcpy(p_, src, n * sizeof(T), kind) != hipSuccess) {
      reset();
      hnm_set_error("spmm plan: hipMemcpy of %zu bytes failed", n * sizeof(T));
      return HNM_EHIP;
    }
    return HNM_OK;
  }
  T* p_ = nullptr;
};

// user-ordered walk of the rows of more than SPMM_SHORT entries (graph_plan.hip walk_build)
struct WalkSched {
  int lpr = 0, ng = 0, nwg = 0, maxloc = 0, nwin = 0;
  DevBuf<int64_t> gptr;       // [nwg * ng * nwin + 1] (nwin column windows per group list)
  DevBuf<uint32_t> ent;       // [walk_nnz] col << 10 | slot
  DevBuf<float> wt;
  DevBuf<int32_t> slot_out;   // [nwg * maxloc]: row (unsplit piece) or -(partial index) - 1
  DevBuf<int32_t> nslot;      // [nwg]
  int64_t n_split = 0, n_part = 0;
  DevBuf<int32_t> split_rows;  // [n_split]
  DevBuf<int64_t> split_ptr;   // [n_split + 1] partial indices, pieces in order
};

// short walk: nb blocks of up to S consecutive short rows, ng lists per block
struct ShortSched {
  int lpr = 0, ng = 0, S = 0, nwg = 0;
  int64_t nb = 0;
  DevBuf<int64_t> gptr;     // [nb * ng + 1]
  DevBuf<uint32_t> ent;     // col << 10 | slot (slot S: padding, weight 0)
  DevBuf<float> wt;
  DevBuf<int32_t> srow;     // [nb * S] row of each slot
  DevBuf<int32_t> nslot;    // [nb]
  std::vector<int32_t> first, last;  // first / last row of each block (row-range launches)
};

struct hnm_spmm_plan {
  int device = 0;
  int num_cus = 0;
  int64_t N = 0, nnz = 0;
  std::vector<int64_t> h_rowptr;
  int64_t n_heavy = 0;
  int64_t n_seg = 0;
  DevBuf<int32_t> heavy_rows;  // [n_heavy]
  int64_t n_long = 0;
  DevBuf<int32_t> long_rows;   // [n_long] rows of the long class, ascending (SPMM_SHORT > 0)
  std::vector<int32_t> h_long;
  DevBuf<int64_t> seg_ptr;     // [n_heavy + 1]
  DevBuf<int32_t> seg_hrow;    // [n_seg]  index into heavy_rows
  DevBuf<int64_t> seg_start;   // [n_seg]
  DevBuf<int64_t> seg_end;     // [n_seg]
  std::vector<int32_t> h_heavy;  // host copies (row-range launches)
  std::vector<int64_t> h_seg_ptr;
  // user-ordered walk of the rows of more than SPMM_SHORT entries
  int walk = 0;
  int swalk = 0;            // short rows by the column-ordered short walk
  int64_t walk_cap = 0;     // entries per piece: a row of L entries is cut into cdiv(L, cap) pieces
  int64_t n_walk = 0, walk_nnz = 0;
  std::vector<int32_t> h_walk_rows;   // ascending
  std::vector<int32_t> h_short_rows;  // rows of <= SPMM_SHORT entries, ascending
  // The graph values the plan is bound to (first prepare / SpMM / rows_combine call): every
  // row's entries sorted by (col, CSR position) in CSR layout, on the device (rows_combine) and
  // on the host (schedule builds).  Later calls must pass the same col / val pointers.
  const int32_t* bound_col = nullptr;
  const float* bound_val = nullptr;
  DevBuf<int32_t> scol;
  DevBuf<float> sval;
  std::vector<int32_t> h_scol;
  std::vector<float> h_sval;
  mutable std::mutex mu;  // lazy preparation (first call with col/val, first call per d)
  std::unique_ptr<WalkSched> sched[7];  // per d = 4 << i
  std::unique_ptr<ShortSched> ssched[7];
  // hnm_spmm_plan_restrict: the row ranges [keep[2j], keep[2j+1]) this plan computes, and
  // whether it is a restricted plan at all (one with no range keeps nothing)
  bool restricted = false;
  std::vector<int64_t> keep;
};

// Binding + the walk schedules for d, built on first use under the plan's mutex (one-time host
// work with stream syncs; d = 0: the binding check alone).  graph_plan.hip.
hnm_status walk_get(hnm_ctx* ctx, const hnm_spmm_plan* plan, const int32_t* col, const float* val,
                    int d, const WalkSched** out, const ShortSched** sout);
