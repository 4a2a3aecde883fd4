// ContentKNN: item-attribute similarity, the fit of a neighbour table for items nobody has bought
// yet.  No reference counterpart (GEMINI.md stage 5 names it, src/models never built it): the
// contract is stated in include/hnm.h and restated in numpy by tests/content_oracle.py.
//
// Input: attrs int32[I, F], a categorical code per (item, column) in the column's own dense
// vocabulary, and a fixed-point weight per (column, code), code_q <= 2^20.  With q_if the weight of
// item i's code in column f (0 when missing),
//   n_i      = sum_f q_if                                      (<= 16 * 2^20 = 2^24)
//   S[i, j]  = sum_f [a_if == a_jf and a_if >= 0] * q_if       (i != j; symmetric: the weight
//                                                               belongs to the code, not the item)
//   sim[i,j] = float( double(S) / sqrt(double(n_i) * double(n_j)) )   for S > 0
// one rounding per operation, contraction off; row i keeps the N best in (sim desc, j asc) order,
// padded with (-1, 0.0f): hnm_itemcf_fit_f32's table, served by the itemcf entries unchanged.
// Everything up to the float64 expression is integer, so the result is the same bits on every run.
//
// Shape.  There is no sparsity to exploit: every row meets every column (I^2 pairs).
//   prep   a thread per item: cleans the codes (missing / out of range -> -1), gathers q, n,
//          item_count and rinv = float(1 / sqrt(n)), and writes codes and weights COLUMN-major
//          ([F][I]) to the workspace so that lane-consecutive items load coalesced.
//   scan   a wave owns R rows for the whole scan: their codes, n and rinv are wave-uniform and sit
//          in scalar registers, their weights in vector registers (a select that takes the
//          compare's mask has no room for a second scalar operand on this ISA: from scalar
//          registers every term paid a v_mov).
//          A (row, column, attribute) term is one compare against a scalar, one select and half
//          an add3, and each loaded column item is used R times.  The four waves of a
//          workgroup share LDS tiles of `tile` column items (codes, n, rinv), a lane takes one
//          column item per step.  A wave meets the columns in ascending j and keeps each row's
//          list to itself: no merge, no atomics, no barrier beyond the tile's two.
//
// The float64 square root and division are not paid per pair.  Two filters stand before them, and
// the result does not depend on either being tight, only on neither rejecting a pair that would
// enter the list:
//   (a) the estimate.  est = fl(fl(fl(float(S) * rinv_i) * rinv_j) * (1 + 2^-20)) in fp32.  S <=
//       2^24 converts exactly; rinv carries one fp32 rounding of a float64 value that is itself
//       within 2 ulp(f64) of 1/sqrt(n); the three products round three times.  The exact sim is the
//       real quotient after three float64 roundings and one fp32 rounding.  Relative to the real
//       value x = S / sqrt(n_i n_j): sim <= x (1 + 2^-24)(1 + 2^-50), est >= x (1 - 2^-24)^5
//       (1 - 2^-50)(1 + 2^-20), so est >= sim (1 + 2^-20)(1 - 7 * 2^-24) > sim: est bounds sim
//       from above with about 9 * 2^-24 to spare (values are >= 2^-24: no subnormals).  A pair
//       with est < the row's current N-th value cannot enter.
//   (b) the memo.  For a fixed row, sim is a function of (S, n_j) alone, non-decreasing in S and
//       non-increasing in n_j: n_i * n_j is exact (< 2^48), and a correctly rounded sqrt, a
//       correctly rounded division and the conversion to fp32 are each monotone.  The wave keeps,
//       per row, one pair (S*, n*) whose sim was computed and found <= the N-th value of a full
//       list.  A later pair with S <= S* and n_j >= n* has sim <= that value, and because columns
//       arrive in ascending j it loses every tie: rejected without float64.  This is what keeps
//       catalogues with many exact ties (colour variants: identical rows) off the slow path; the
//       N-th value only rises, so a memo never goes stale.
// Only survivors of both get the exact float64 sim, and only that value is ranked: the order is
// the fp32-rounded sim's, not the estimate's.
#include "hnm_device.h"
#include "hnm_internal.h"
#include "itemcf_internal.h"

#include <cmath>

namespace {

constexpr int CNT_MAX_F = 16;
constexpr int CNT_MAX_N = 64;
constexpr unsigned CNT_MAX_Q = 1u << 20;
constexpr int CNT_TILE_MAX = 512;
// Column items per LDS tile.  Measured at the H&M catalogue size, F = 11 (tools/content_bench.py,
// profiles/content_bench.txt): 64 -> 69.6 ms, 128 -> 42.7 ms, 256 -> 31.2 ms, 512 -> 30.0 ms:
// fewer barriers beat the smaller LDS footprint (occupancy is 3 waves a SIMD by registers at
// every size).
constexpr int CNT_TILE_DEFAULT = 512;
constexpr float CNT_MARGIN = 1.0f + 0x1p-20f;

__device__ __forceinline__ float cnt_sim(unsigned s, unsigned ni, unsigned nj) {
#pragma clang fp contract(off)
  const double prod = (double)ni * (double)nj;
  const double den = sqrt(prod);
  return (float)((double)s / den);
}

// A thread per item: ccode / cq [F][I] (column-major), nsum, rinv, item_count.  The grid also
// strides over code_q to raise the error word for a weight above 2^20.
__global__ __launch_bounds__(256) void cnt_prep_kernel(
    const int32_t* __restrict__ attrs, int64_t I, int F, const int64_t* __restrict__ code_ptr,
    const uint32_t* __restrict__ code_q, int32_t* __restrict__ ccode, uint32_t* __restrict__ cq,
    unsigned* __restrict__ nsum, float* __restrict__ rinv, int64_t* __restrict__ item_count,
    unsigned* err) {
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  // a vocabulary table that does not ascend from an offset >= 0: every code counts as missing
  bool sane = code_ptr[0] >= 0;
  for (int f = 0; f < F; ++f) sane = sane && code_ptr[f + 1] >= code_ptr[f];
  if (!sane) {
    if (gid == 0) hnm_flag(err, HNM_ERR_OOB);
  } else {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t x = code_ptr[0] + gid; x < code_ptr[F]; x += stride)
      if (code_q[x] > CNT_MAX_Q) hnm_flag(err, HNM_ERR_CODE_Q);
  }
  if (gid >= I) return;
  unsigned n = 0;
  int cols = 0;
  for (int f = 0; f < F; ++f) {
    int32_t a = attrs[gid * F + f];
    uint32_t q = 0;
    if (a >= 0 && sane) {
      const int64_t base = code_ptr[f];
      if (a >= code_ptr[f + 1] - base) {
        hnm_flag(err, HNM_ERR_OOB);
        a = -1;
      } else {
        q = code_q[base + a];
        if (q > CNT_MAX_Q) q = 0;  // flagged above
      }
    } else {
      a = -1;
    }
    ccode[(int64_t)f * I + gid] = a;
    cq[(int64_t)f * I + gid] = q;
    n += q;
    cols += q > 0;
  }
  nsum[gid] = n;
  rinv[gid] = n ? (float)(1.0 / sqrt((double)n)) : 0.f;
  item_count[gid] = cols;
}

// 256 threads; wave w of workgroup b owns rows (4 b + w) * R .. + R.  FP: F rounded up to a
// multiple of 4 (padding attributes weigh 0).  Dynamic LDS: (FP + 2) * T words.
template <int FP, int R>
__global__ __launch_bounds__(256) void cnt_scan_kernel(
    const int32_t* __restrict__ ccode, const uint32_t* __restrict__ cq,
    const unsigned* __restrict__ nsum, const float* __restrict__ rinv, int64_t I, int F, int N,
    int T, int32_t* __restrict__ nbr_idx, float* __restrict__ nbr_val) {
  extern __shared__ int cnt_lds[];
  int* tc = cnt_lds;                                         // [FP][T] codes
  unsigned* tn = reinterpret_cast<unsigned*>(cnt_lds + FP * T);  // [T] n_j
  float* tr = reinterpret_cast<float*>(cnt_lds + (FP + 1) * T);  // [T] rinv_j
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t row0 = ((int64_t)blockIdx.x * 4 + wave) * R;
  // the rows' side: wave-uniform
  int rc[R][FP];
  unsigned rq[R][FP];
  unsigned rn[R];
  float rr[R];
  float lv[R];
  int li[R];
  unsigned ms[R], mn[R];  // the memo (S*, n*): nothing is rejected by (0, 2^32 - 1)
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int64_t i = row0 + r;
    const bool live = i < I;
#pragma unroll
    for (int f = 0; f < FP; ++f) {
      int c = -1;
      unsigned q = 0;
      if (live && f < F) {
        c = ccode[(int64_t)f * I + i];
        q = cq[(int64_t)f * I + i];
      }
      rc[r][f] = __builtin_amdgcn_readfirstlane(c);  // the compare's scalar operand
      rq[r][f] = q;  // a vector register: a select takes the mask and no second scalar
    }
    rn[r] = (unsigned)__builtin_amdgcn_readfirstlane((int)(live ? nsum[i] : 0u));
    rr[r] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(live ? rinv[i] : 0.f)));
    lv[r] = -__builtin_inff();
    li[r] = HNM_SENTINEL_IDX;
    ms[r] = 0u;
    mn[r] = 0xffffffffu;
  }
  for (int64_t t0 = 0; t0 < I; t0 += T) {
    __syncthreads();  // the previous tile has been read by every wave
#pragma unroll
    for (int f = 0; f < FP; ++f)
      for (int c = t; c < T; c += 256) {
        const int64_t j = t0 + c;
        tc[f * T + c] = (f < F && j < I) ? ccode[(int64_t)f * I + j] : -1;
      }
    for (int c = t; c < T; c += 256) {
      const int64_t j = t0 + c;
      tn[c] = j < I ? nsum[j] : 0u;
      tr[c] = j < I ? rinv[j] : 0.f;
    }
    __syncthreads();
    const int len = (int)std::min<int64_t>(T, I - t0);
    for (int g = 0; g < len; g += 64) {  // T is a multiple of 64: g + lane < T
      const int c = g + lane;
      int cc[FP];
#pragma unroll
      for (int f = 0; f < FP; ++f) cc[f] = tc[f * T + c];
      const unsigned nj = tn[c];
      const float rj = tr[c];
      const int j = (int)t0 + c;  // >= I past the end: code -1 everywhere, S = 0
#pragma unroll
      for (int r = 0; r < R; ++r) {
        unsigned S = 0;
#pragma unroll
        for (int f = 0; f < FP; ++f) S += cc[f] == rc[r][f] ? rq[r][f] : 0u;
        const float thr = hnm_readlane_f(lv[r], N - 1);
        const float est = (float)S * rr[r] * rj * CNT_MARGIN;
        const bool pass = S > 0 && j != (int)(row0 + r) && est >= thr &&
                          !(S <= ms[r] && nj >= mn[r]);
        if (__ballot(pass)) {
          const float sim = pass ? cnt_sim(S, rn[r], nj) : 0.f;
          icf_offer(lv[r], li[r], sim, j, pass, N);
          const float now = hnm_readlane_f(lv[r], N - 1);  // -inf until the list is full
          const uint64_t rej = __ballot(pass && sim <= now);
          if (rej) {
            const uint64_t tie = __ballot(pass && sim == now);
            const int l = __builtin_ctzll(tie ? tie : rej);
            ms[r] = (unsigned)hnm_readlane_i((int)S, l);
            mn[r] = (unsigned)hnm_readlane_i((int)nj, l);
          }
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int64_t i = row0 + r;
    if (i < I && lane < N) {
      const bool pad = li[r] == HNM_SENTINEL_IDX;
      nbr_idx[i * N + lane] = pad ? -1 : li[r];
      nbr_val[i * N + lane] = pad ? 0.f : lv[r];
    }
  }
}

template <int FP, int R>
hnm_status cnt_launch(hnm_ctx* ctx, const int32_t* ccode, const uint32_t* cq, const unsigned* nsum,
                      const float* rinv, int64_t I, int F, int N, int T, int32_t* nbr_idx,
                      float* nbr_val) {
  const size_t lds = (size_t)(FP + 2) * T * 4;  // <= 18 * 512 * 4 = 36 KiB
  const unsigned grid = (unsigned)hnm_cdiv(I, 4 * R);
  hipLaunchKernelGGL((cnt_scan_kernel<FP, R>), dim3(grid), dim3(256), lds, ctx->stream, ccode, cq,
                     nsum, rinv, I, F, N, T, nbr_idx, nbr_val);
  HNM_LAUNCH_CHECK();
  return HNM_OK;
}

}  // namespace

extern "C" hnm_status hnm_content_fit_f32(hnm_ctx* ctx, const int32_t* attrs, int64_t num_items,
                                          int F, const int64_t* code_ptr, const uint32_t* code_q,
                                          int N, int tile, int32_t* nbr_idx, float* nbr_val,
                                          int64_t* item_count) {
  HNM_CTX_DEVICE(ctx);
  HNM_REQUIRE(ctx, HNM_EINVAL, "content_fit: ctx is NULL");
  HNM_REQUIRE(N >= 1 && N <= CNT_MAX_N, HNM_EINVAL, "content_fit: 1 <= N <= %d", CNT_MAX_N);
  HNM_REQUIRE(F >= 1 && F <= CNT_MAX_F, HNM_EINVAL, "content_fit: 1 <= F <= %d", CNT_MAX_F);
  HNM_REQUIRE(num_items >= 0, HNM_EINVAL, "content_fit: bad size");
  HNM_REQUIRE(tile == 0 || (tile >= 64 && tile <= CNT_TILE_MAX && tile % 64 == 0), HNM_EINVAL,
              "content_fit: tile must be 0 or a multiple of 64 in [64, %d]", CNT_TILE_MAX);
  HNM_REQUIRE(num_items < INT_BIG, HNM_EUNSUPPORTED, "content_fit: num_items exceeds 2^31 - 1");
  if (num_items == 0) return HNM_OK;
  HNM_REQUIRE(attrs && code_ptr && code_q, HNM_EINVAL, "content_fit: NULL input");
  HNM_REQUIRE(nbr_idx && nbr_val && item_count, HNM_EINVAL, "content_fit: NULL output");
  const int64_t I = num_items;
  const size_t s_tab = hnm_align((size_t)F * (size_t)I * 4), s_vec = hnm_align((size_t)I * 4);
  char* ws = nullptr;
  hnm_status st = hnm_workspace(ctx, 2 * s_tab + 2 * s_vec, (void**)&ws);
  if (st != HNM_OK) return st;
  int32_t* ccode = (int32_t*)ws;
  uint32_t* cq = (uint32_t*)(ws + s_tab);
  unsigned* nsum = (unsigned*)(ws + 2 * s_tab);
  float* rinv = (float*)(ws + 2 * s_tab + s_vec);
  hipLaunchKernelGGL(cnt_prep_kernel, dim3((unsigned)hnm_cdiv(I, 256)), dim3(256), 0, ctx->stream,
                     attrs, I, F, code_ptr, code_q, ccode, cq, nsum, rinv, item_count,
                     ctx->err_dev);
  HNM_LAUNCH_CHECK();
  int T = tile ? tile : CNT_TILE_DEFAULT;
  T = (int)std::min<int64_t>(T, hnm_cdiv(I, 64) * 64);
  // rows per wave by attribute count: FP * R scalar and FP * R vector registers hold the rows;
  // at F = 11 four rows a wave measured 30.0 ms against three rows' 34.1 ms (both 3 waves a SIMD)
  if (F <= 4) return cnt_launch<4, 4>(ctx, ccode, cq, nsum, rinv, I, F, N, T, nbr_idx, nbr_val);
  if (F <= 8) return cnt_launch<8, 4>(ctx, ccode, cq, nsum, rinv, I, F, N, T, nbr_idx, nbr_val);
  if (F <= 12) return cnt_launch<12, 4>(ctx, ccode, cq, nsum, rinv, I, F, N, T, nbr_idx, nbr_val);
  return cnt_launch<16, 2>(ctx, ccode, cq, nsum, rinv, I, F, N, T, nbr_idx, nbr_val);
}
