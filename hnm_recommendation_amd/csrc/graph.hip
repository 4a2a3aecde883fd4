// LightGCN graph path for gfx950, SpMM with the fused layer combine (a6): the kernels, their
// launches and the three SpMM entry points.  The CSR build is graph_csr.hip, the host-only
// planning (binding, schedules, plan create / restrict / destroy) graph_plan.hip; the design
// constants and the plan / schedule structs are in graph_internal.h.
//
// SpMM (lightgcn.py:152): a row's neighbours are gathered as whole embedding rows, d/4
// lanes x 16 B each, 64/(d/4) neighbours per wave instruction, 4-deep unrolled so ~16
// rows are in flight per wave.  Rows up to HEAVY neighbours take one wave; power-law item
// rows (up to ~1e6 neighbours on the H&M shape) are cut into SEG-long segments whose
// partial sums are added back in segment order, so results are deterministic and the
// longest wave is bounded.  Epilogue: Y = sum, acc_out = acc_in + alpha * Y
// (lightgcn.py:156-158).
//
// Bitwise contract: a row's value does not depend on the call that computes it -- the layer
// kernels, rows_combine and a restricted plan sum it in the same order.  That order is written
// once per level: the entry chains in row_sum / row_sum_grouped / walk_consume, the slice sum +
// pairwise tree over a row's pieces or segments in finish_row (workgroup) and wave_slice_sum
// (wave), which must stay the same sum.
#include <algorithm>
#include <vector>

#include "graph_internal.h"
#include "hnm_device.h"

// ------------------------------------------------------------------ SpMM
// Sum of val[e] * X[col[e], :] over e in [s, e) with the lane layout of LPR lanes per row.
// (A variant issuing a whole batch of indices and then all row gathers before consuming
// any -- no serial remainder loop -- measured 3 % slower per layer: 2.145 vs 2.087 ms.)
template <int LPR>
__device__ __forceinline__ float4 row_sum(const int32_t* __restrict__ col,
                                          const float* __restrict__ val,
                                          const float* __restrict__ X, int d, int64_t s,
                                          int64_t e, int lane) {
  constexpr int G = 64 / LPR;
  const int grp = lane / LPR, sub = lane % LPR;
  float4 acc = f4_zero();
  int64_t p = s + grp;
  for (; p + 3 * G < e; p += 4 * G) {
    int c[4];
    float w[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      c[u] = col[p + u * G];
      w[u] = val[p + u * G];
    }
    float4 x[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) x[u] = f4_load(X + (int64_t)c[u] * d + 4 * sub);
#pragma unroll
    for (int u = 0; u < 4; ++u) f4_fma(w[u], x[u], acc);
  }
  for (; p < e; p += G) {
    const int c = col[p];
    const float w = val[p];
    f4_fma(w, f4_load(X + (int64_t)c * d + 4 * sub), acc);
  }
  // fixed-order tree across the G neighbour groups
#pragma unroll
  for (int o = LPR; o < 64; o <<= 1) f4_add_xor_lane(acc, o);
  return acc;
}

// SpmmEpi (graph_internal.h) applied to row r, float4 column sub
__device__ __forceinline__ void spmm_epilogue(int64_t r, int d, int sub, float4 y,
                                              const float* __restrict__ X, const SpmmEpi& ep) {
  const int64_t off = r * d + 4 * sub;
  if (ep.Y) f4_store(ep.Y + off, y);
  if (ep.acc_out && r >= ep.acc_row0) {
    const int64_t ao = (r - ep.acc_row0) * d + 4 * sub;
    float4 a;
    if (ep.acc_in) {
      a = f4_load(ep.acc_in + ao);
    } else if (ep.beta != 0.f) {
      a = f4_scale(ep.beta, f4_load(X + off));
    } else {
      a = f4_zero();
    }
    f4_fma(ep.alpha, y, a);
    f4_store(ep.acc_out + ao, a);
  }
}

template <int LPR>
__global__ __launch_bounds__(256) void spmm_light_kernel(int64_t r0, int64_t r1,
                                                         const int64_t* __restrict__ rowptr,
                                                         const int32_t* __restrict__ col,
                                                         const float* __restrict__ val,
                                                         const float* __restrict__ X, int d,
                                                         SpmmEpi ep, int64_t heavy) {
  const int64_t r = r0 + (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= r1) return;
  const int lane = threadIdx.x & 63;
  const int64_t s = rowptr[r], e = rowptr[r + 1];
  if (e - s > heavy) return;  // segmented path
  const float4 y = row_sum<LPR>(col, val, X, d, s, e, lane);
  if (lane < LPR) spmm_epilogue(r, d, lane, y, X, ep);
}

// Grouped light rows: lane group g = lane / LPR owns row r, lane sub = lane % LPR its float4
// column; the group walks the row's entries in order (4 loads in flight per group, 64 / LPR
// rows per wave) with one fma chain per column -- no cross-group tree.
template <int LPR>
__device__ __forceinline__ float4 row_sum_grouped(const int32_t* __restrict__ col,
                                                  const float* __restrict__ val,
                                                  const float* __restrict__ X, int d, int64_t s,
                                                  int64_t e, int sub) {
  float4 acc = f4_zero();
  int64_t p = s;
  for (; p + 3 < e; p += 4) {
    int c[4];
    float w[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      c[u] = col[p + u];
      w[u] = val[p + u];
    }
    float4 x[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) x[u] = f4_load(X + (int64_t)c[u] * d + 4 * sub);
#pragma unroll
    for (int u = 0; u < 4; ++u) f4_fma(w[u], x[u], acc);
  }
  for (; p < e; ++p) {
    const int c = col[p];
    const float w = val[p];
    f4_fma(w, f4_load(X + (int64_t)c * d + 4 * sub), acc);
  }
  return acc;
}

// One launch for the light rows of [r0, r1): blocks [0, nlb) take the long rows listed in
// long_rows[l0, l1) (one wave per row, the light kernel's order; first, so the longest work
// starts first), the other blocks the short rows (one LPR-lane group per row), skipping rows
// of the other classes.
template <int LPR>
__global__ __launch_bounds__(256) void spmm_mixed_kernel(int64_t r0, int64_t r1,
                                                         const int32_t* __restrict__ long_rows,
                                                         int64_t l0, int64_t l1, int64_t nlb,
                                                         const int64_t* __restrict__ rowptr,
                                                         const int32_t* __restrict__ col,
                                                         const float* __restrict__ val,
                                                         const float* __restrict__ X, int d,
                                                         SpmmEpi ep) {
  const int lane = threadIdx.x & 63;
  if ((int64_t)blockIdx.x < nlb) {
    const int64_t q = l0 + (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= l1) return;
    const int64_t r = long_rows[q];
    const float4 y = row_sum<LPR>(col, val, X, d, rowptr[r], rowptr[r + 1], lane);
    if (lane < LPR) spmm_epilogue(r, d, lane, y, X, ep);
    return;
  }
  constexpr int RPW = 64 / LPR;
  const int sub = lane % LPR;
  const int64_t r = r0 + ((int64_t)(blockIdx.x - nlb) * 4 + (threadIdx.x >> 6)) * RPW + lane / LPR;
  if (r >= r1) return;
  const int64_t s = rowptr[r], e = rowptr[r + 1];
  if (e - s > SPMM_SHORT) return;  // long / heavy class
  spmm_epilogue(r, d, sub, row_sum_grouped<LPR>(col, val, X, d, s, e, sub), X, ep);
}

template <int LPR>
__global__ __launch_bounds__(256) void spmm_segment_kernel(int64_t sg0, int64_t sg1,
                                                           const int64_t* __restrict__ seg_start,
                                                           const int64_t* __restrict__ seg_end,
                                                           const int32_t* __restrict__ col,
                                                           const float* __restrict__ val,
                                                           const float* __restrict__ X, int d,
                                                           float* __restrict__ partial) {
  const int64_t sg = sg0 + (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (sg >= sg1) return;
  const int lane = threadIdx.x & 63;
  const float4 y = row_sum<LPR>(col, val, X, d, seg_start[sg], seg_end[sg], lane);
  if (lane < LPR) f4_store(partial + (sg - sg0) * d + 4 * lane, y);
}

// The workgroup-level slice sum (the only copy; wave_slice_sum below is the same sum by one
// wave): row r = the sum of its n partial rows partial[a .. a + n) -- a heavy row's segments or
// a split walk row's pieces.  Thread (slice sl, column c) of the 256 adds partials sl, sl + S,
// ... (S = 256 / (d/4) slices) in order from 0 -- 4 loads in flight, added in that same order --
// then a fixed pairwise LDS tree over the slices, w = S/2 .. 1.  Deterministic, with all 256
// lanes busy instead of d/4 lanes walking every partial (a sequential sum over ~1,500 pieces of
// the most popular item took 70 us).
__device__ __forceinline__ void finish_row(const float* __restrict__ partial, int64_t a, int64_t n,
                                           int64_t r, const float* __restrict__ X, int d,
                                           const SpmmEpi& ep) {
  __shared__ float4 red[256];
  // d4 divides 256 (d in 4..256, powers of two)
  const int t = threadIdx.x, d4 = d / 4, S = 256 / d4, c = t % d4, sl = t / d4;
  float4 y = f4_zero();
  int64_t j = sl;
  for (; j + 3 * S < n; j += 4 * S) {
    float4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = f4_load(partial + (a + j + u * S) * d + 4 * c);
#pragma unroll
    for (int u = 0; u < 4; ++u) f4_add(y, v[u]);
  }
  for (; j < n; j += S) f4_add(y, f4_load(partial + (a + j) * d + 4 * c));
  red[t] = y;
  __syncthreads();
  for (int w = S / 2; w >= 1; w >>= 1) {
    if (sl < w) {
      const float4 o = red[t + w * d4];
      float4 m = red[t];
      f4_add(m, o);
      red[t] = m;
    }
    __syncthreads();
  }
  if (sl == 0) spmm_epilogue(r, d, c, red[t], X, ep);
}

// One workgroup per heavy row: its segment partials, finish_row's order.
__global__ __launch_bounds__(256) void spmm_finish_kernel(int64_t h0,
                                                          const int32_t* __restrict__ heavy_rows,
                                                          const int64_t* __restrict__ seg_ptr,
                                                          int64_t sg0,
                                                          const float* __restrict__ partial,
                                                          const float* __restrict__ X, int d,
                                                          SpmmEpi ep) {
  const int64_t hr = h0 + blockIdx.x;
  const int64_t s0 = seg_ptr[hr] - sg0;
  finish_row(partial, s0, seg_ptr[hr + 1] - sg0 - s0, (int64_t)heavy_rows[hr], X, d, ep);
}

// ---------------------------------------------------------------- user-ordered walk
// One step of a walk list, both walks: ST records (col << 10 | slot, weight) -- the ST rows are
// gathered first, then added into their slots' LDS accumulators in list order, so a slot's
// entries stay one fma chain.  acc: the workgroup's accumulators, LPR float4 per slot.
template <int LPR, int ST>
__device__ __forceinline__ void walk_consume(float4* acc, const uint32_t* c, const float* w,
                                             const float* __restrict__ X, int d, int sub) {
  float4 x[ST];
#pragma unroll
  for (int u = 0; u < ST; ++u) x[u] = f4_load(X + (int64_t)(c[u] >> 10) * d + 4 * sub);
#pragma unroll
  for (int u = 0; u < ST; ++u) {
    float4* a = &acc[(c[u] & 1023u) * LPR + sub];
    float4 v = *a;
    f4_fma(w[u], x[u], v);
    *a = v;
  }
}

// Rows of more than SPMM_SHORT entries (the item half: each item row gathers ~300 random rows
// of the 351 MB user table) as ONE persistent launch whose gathers move through the table in
// ascending column order.  Each walk row's entries are sorted by (col, CSR position) and cut
// into pieces: a row of L entries has n = cdiv(L, cap) pieces, piece j holding the sorted
// entries j, j + n, j + 2n, ... (so every piece spans the whole column range).  A workgroup
// (one per CU, 1024 threads) owns up to maxloc pieces with their fp32 accumulators in LDS;
// each LPR-lane group walks ONE list -- its pieces' entries merged by column, packed as
// col << 10 | slot -- and adds val * X[col] into the slot's accumulator.  All lists of the
// chip advance through the columns at the same pace, so the rows gathered at any moment lie
// in a narrow window of X that the XCD L2s hold: measured on the synthetic H&M item half
// (tools/slice_walk_probe.hip) 0.85 ms vs 1.16 ms for the segmented pull in CSR order.
// Order: piece j = fma chain from 0 over its entries in (col, position) order; y = p_0 for an
// unsplit row, else per-slice sums of the pieces and a fixed tree (spmm_walk_finish_kernel);
// rows_combine repeats it from wcol / wval (walk_row_sum), so listed rows stay bitwise equal
// to the layer kernels.
template <int LPR>
__global__ __launch_bounds__(WALK_THREADS) void spmm_walk_kernel(
    const int64_t* __restrict__ gptr, const uint32_t* __restrict__ ent,
    const float* __restrict__ wt, const int32_t* __restrict__ slot_out,
    const int32_t* __restrict__ nslot, int maxloc, int nwin, const float* __restrict__ X, int d,
    float* __restrict__ partial, SpmmEpi ep, int64_t r0, int64_t r1) {
  constexpr int NG = WALK_THREADS / LPR;
  __shared__ float4 acc[WALK_LDS_F4];
  const int tid = threadIdx.x, g = tid / LPR, sub = tid % LPR;
  const int ns = nslot[blockIdx.x];
  for (int i = tid; i < ns * LPR; i += WALK_THREADS) acc[i] = f4_zero();
  __syncthreads();
  // WALK_STEP entries per step (round 3: 2: 1.741 ms per d=64 layer, 4: 1.694, 8: 1.848)
  const int K = nwin;  // column windows (walk_windows)
  constexpr int ST = WALK_STEP;
  for (int k = 0; k < K; ++k) {
    int64_t p = gptr[((int64_t)blockIdx.x * NG + g) * K + k];
    const int64_t e = gptr[((int64_t)blockIdx.x * NG + g) * K + k + 1];
    for (; p + ST - 1 < e; p += ST) {
      uint32_t c[ST];
      float w[ST];
#pragma unroll
      for (int u = 0; u < ST; ++u) {
        c[u] = ent[p + u];
        w[u] = wt[p + u];
      }
      walk_consume<LPR, ST>(acc, c, w, X, d, sub);
    }
    for (; p < e; ++p) {
      const uint32_t c = ent[p];
      const float w = wt[p];
      walk_consume<LPR, 1>(acc, &c, &w, X, d, sub);
    }
    if (K > 1) __syncthreads();
  }
  __syncthreads();
  for (int i = tid; i < ns * LPR; i += WALK_THREADS) {
    const int o = slot_out[(int64_t)blockIdx.x * maxloc + i / LPR], c = i % LPR;
    if (o >= 0) {
      if (o >= r0 && o < r1) spmm_epilogue(o, d, c, acc[i], X, ep);
    } else {
      f4_store(partial + (int64_t)(-o - 1) * d + 4 * c, acc[i]);
    }
  }
}

// ------------------------------------------------------------- short walk (round 4)
// Rows of at most SPMM_SHORT entries (every user row of the bipartite graph: ~24 entries
// gathering the 27 MB item table at d=64) in blocks of up to S consecutive rows.  A persistent
// workgroup (one per CU) takes blocks b0 + blockIdx.x, + gridDim.x, ...; the block's rows hold
// their fp32 accumulators in LDS (slot = row - first row of the block, spare slot S for
// padding), each LPR-lane group owns a set of the block's rows and walks their entries merged by
// column (col << 10 | slot records, padded to 4 per list), adding val * X[col] into the slot.
// Every block's lists span the same column range at a similar pace, so the rows the 32 CUs of
// an XCD gather at any moment lie in a narrow window of the item table that their L2 holds.
// Order: row r's value is one fma chain from 0 over its entries sorted by (col, CSR position)
// -- rows_combine repeats it over the plan's sorted copy (row_sum_grouped on scol / sval).
template <int LPR>
__global__ __launch_bounds__(SWALK_THREADS) void spmm_swalk_kernel(
    const int64_t* __restrict__ gptr, const uint32_t* __restrict__ ent,
    const float* __restrict__ wt, const int32_t* __restrict__ srow,
    const int32_t* __restrict__ nslot, int S, const float* __restrict__ X, int d, SpmmEpi ep,
    int64_t r0, int64_t r1, int64_t b0, int64_t b1) {
  constexpr int NG = SWALK_THREADS / LPR;
  constexpr int ST = swalk_step(LPR);
  __shared__ float4 acc[SWALK_LDS_F4];
  const int tid = threadIdx.x, g = tid / LPR, sub = tid % LPR;
  for (int i = tid; i < SWALK_LDS_F4; i += SWALK_THREADS) acc[i] = f4_zero();
  __syncthreads();
  for (int64_t b = b0 + blockIdx.x; b < b1; b += gridDim.x) {
    int64_t p = gptr[b * NG + g];
    const int64_t e = gptr[b * NG + g + 1];  // lists are padded to multiples of ST
    // the next step's records are loaded before this step's gathers
    uint32_t c[ST], cn[ST];
    float w[ST], wn[ST];
    if (p < e) {
#pragma unroll
      for (int u = 0; u < ST; ++u) {
        cn[u] = ent[p + u];
        wn[u] = wt[p + u];
      }
    }
    for (; p < e; p += ST) {
#pragma unroll
      for (int u = 0; u < ST; ++u) {
        c[u] = cn[u];
        w[u] = wn[u];
      }
      if (p + ST < e) {
#pragma unroll
        for (int u = 0; u < ST; ++u) {
          cn[u] = ent[p + ST + u];
          wn[u] = wt[p + ST + u];
        }
      }
      walk_consume<LPR, ST>(acc, c, w, X, d, sub);
    }
    __syncthreads();
    const int ns = nslot[b];
    for (int i = tid; i < ns * LPR; i += SWALK_THREADS) {
      const int64_t r = srow[b * S + i / LPR];
      if (r >= r0 && r < r1) spmm_epilogue(r, d, i % LPR, acc[i], X, ep);
      acc[i] = f4_zero();
    }
    __syncthreads();
  }
}

// Split walk rows, one workgroup per row: its pieces' partials, finish_row's order.
__global__ __launch_bounds__(256) void spmm_walk_finish_kernel(
    const int32_t* __restrict__ split_rows, const int64_t* __restrict__ split_ptr,
    const float* __restrict__ partial, const float* __restrict__ X, int d, SpmmEpi ep,
    int64_t r0, int64_t r1) {
  const int64_t r = split_rows[blockIdx.x];
  if (r < r0 || r >= r1) return;  // uniform
  const int64_t a = split_ptr[blockIdx.x];
  finish_row(partial, a, split_ptr[blockIdx.x + 1] - a, r, X, d, ep);
}

// finish_row's sum by one wave, for rows_combine (the only wave-level copy; it must stay the
// same sum): the row's n terms -- term(j) valid in every lane, as the whole wave computes it --
// in S = 256 / LPR slices, slice sl adding terms sl, sl + S, ... in order from 0, then the
// pairwise tree over the slices, w = S/2 .. 1.  Each lane only touches its own float4 column of
// the slice sums (red: one S x LPR block of LDS per wave), so the wave needs no barrier.  The
// result is valid in lanes < LPR.
template <int LPR, typename Term>
__device__ __forceinline__ float4 wave_slice_sum(int64_t n, int lane, float4* red, Term term) {
  constexpr int S = 256 / LPR;
  for (int sl = 0; sl < S; ++sl) {
    float4 acc = f4_zero();
    for (int64_t j = sl; j < n; j += S) f4_add(acc, term(j));
    if (lane < LPR) red[sl * LPR + lane] = acc;
  }
  float4 y = f4_zero();
  if (lane < LPR) {
    for (int w = S / 2; w >= 1; w >>= 1)
      for (int sl = 0; sl < w; ++sl) {
        const float4 o = red[(sl + w) * LPR + lane];
        float4 m = red[sl * LPR + lane];
        f4_add(m, o);
        red[sl * LPR + lane] = m;
      }
    y = red[lane];
  }
  return y;
}

// Walk order of one row for a listed-row kernel (the whole wave calls it; valid in lanes <
// LPR): the pieces' fma chains over the sorted entries; one piece -> its chain; several ->
// the slice sum over the pieces, as spmm_walk_finish_kernel.
template <int LPR>
__device__ float4 walk_row_sum(const int32_t* __restrict__ wcol, const float* __restrict__ wval,
                               int64_t ws, int64_t L, int64_t cap, const float* __restrict__ X,
                               int d, int lane, float4* red) {
  const int sub = lane % LPR;
  const int64_t n = hnm_cdiv(L, cap);
  auto chain = [&](int64_t j) {
    float4 v = f4_zero();
    for (int64_t q = j; q < L; q += n)
      f4_fma(wval[ws + q], f4_load(X + (int64_t)wcol[ws + q] * d + 4 * sub), v);
    return v;
  };
  if (n == 1) return chain(0);
  return wave_slice_sum<LPR>(n, lane, red, chain);
}

// y = (A_hat X)[r] for a row of more than HEAVY entries, in the plan's segment + finish
// order: the SEG-long segments (row_sum each, as spmm_segment_kernel), then the slice sum over
// them, as spmm_finish_kernel; the whole wave works on the row, the result is valid in lanes <
// LPR.
template <int LPR>
__device__ float4 heavy_row_sum(const int32_t* __restrict__ col, const float* __restrict__ val,
                                const float* __restrict__ X, int d, int64_t rs, int64_t re,
                                int lane, float4* red) {
  return wave_slice_sum<LPR>(hnm_cdiv(re - rs, SEG), lane, red, [&](int64_t sg) {
    const int64_t a = rs + sg * SEG, z = a + SEG < re ? a + SEG : re;
    return row_sum<LPR>(col, val, X, d, a, z, lane);
  });
}

// out[b] = alpha_0 E_0[r] + sum_l alpha_l E_l[r] (fma chain in layer order) + alpha_L y
__device__ __forceinline__ void combine_store(const CombineLayers& cl, int64_t r, int d, int sub,
                                              float4 y, float* __restrict__ out, int64_t b) {
  const int64_t off = r * d + 4 * sub;
  float4 a = f4_scale(cl.a[0], f4_load(cl.E[0] + off));
  for (int l = 1; l < cl.L; ++l) f4_fma(cl.a[l], f4_load(cl.E[l] + off), a);
  f4_fma(cl.a[cl.L], y, a);
  f4_store(out + b * d + 4 * sub, a);
}

// Final embeddings of listed rows (the batch's users) without their last layer over the
// whole graph: y = (A_hat E_{L-1})[r], out[b] = alpha_0 E_0[r] then
// fma(alpha_l, E_l[r], .) for l = 1..L-1 and fma(alpha_L, y, .) -- the same operations, in
// the same order, as the fused combine.  Every row is summed in the order of its class as the
// layer kernels of the same plan sum it (CombineOrder, graph_internal.h), so listed rows --
// heavy and split ones included -- are bitwise equal to forward() too.
template <int LPR>
__global__ __launch_bounds__(256) void spmm_rows_combine_kernel(
    const int64_t* __restrict__ rows, int64_t n, int64_t N, const int64_t* __restrict__ rowptr,
    const int32_t* __restrict__ col, const float* __restrict__ val, int d, CombineLayers cl,
    CombineOrder co, float* __restrict__ out, unsigned* err) {
  __shared__ float4 slices[4][256];
  const int lane = threadIdx.x & 63;
  const float* Xl = cl.E[cl.L - 1];
  if (co.mode == 0) {
    const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= n) return;
    const int64_t r = rows[b];
    if (r < 0 || r >= N) {
      if (lane == 0) hnm_flag(err, HNM_ERR_OOB);
      for (int c = lane; c < d; c += 64) out[b * d + c] = __builtin_nanf("");
      return;
    }
    const float4 y = row_sum<LPR>(col, val, Xl, d, rowptr[r], rowptr[r + 1], lane);
    if (lane < LPR) combine_store(cl, r, d, lane, y, out, b);
    return;
  }
  // grouped: group g = lane / LPR owns listed row b; short rows in the grouped order, long and
  // heavy rows afterwards by the whole wave (uniform loop over the wave's groups)
  constexpr int RPW = 64 / LPR;
  const int g = lane / LPR, sub = lane % LPR;
  const int64_t b0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * RPW;
  if (b0 >= n) return;
  const int64_t b = b0 + g;
  int64_t r = -1, rs = 0, re = 0;
  bool ok = false;
  const int32_t* scl = co.short_sorted ? co.scol : col;
  const float* svl = co.short_sorted ? co.sval : val;
  if (b < n) {
    r = rows[b];
    ok = r >= 0 && r < N;
    if (!ok) {
      if (sub == 0) hnm_flag(err, HNM_ERR_OOB);
      const float nan = __builtin_nanf("");
      f4_store(out + b * d + 4 * sub, make_float4(nan, nan, nan, nan));
    } else {
      rs = rowptr[r];
      re = rowptr[r + 1];
      if (re - rs <= SPMM_SHORT)
        combine_store(cl, r, d, sub, row_sum_grouped<LPR>(scl, svl, Xl, d, rs, re, sub), out, b);
    }
  }
  // long and heavy rows: the whole wave, one row at a time
  uint64_t hm = __ballot(ok && re - rs > SPMM_SHORT && sub == 0);
  while (hm) {
    const int src = __builtin_ctzll(hm);
    hm &= hm - 1;
    const int64_t hb = b0 + src / LPR;
    const int64_t hr = rows[hb];
    const int64_t hs = rowptr[hr], he = rowptr[hr + 1];
    float4 y;
    if (co.mode == 2) {  // the walk's order (every row of this class is a walk row)
      y = walk_row_sum<LPR>(co.scol, co.sval, hs, he - hs, co.cap, Xl, d, lane,
                            slices[threadIdx.x >> 6]);
    } else {
      y = he - hs <= HEAVY
              ? row_sum<LPR>(col, val, Xl, d, hs, he, lane)
              : heavy_row_sum<LPR>(col, val, Xl, d, hs, he, lane, slices[threadIdx.x >> 6]);
    }
    if (lane < LPR) combine_store(cl, hr, d, lane, y, out, hb);
  }
}

// ------------------------------------------------------------------ launches
static int64_t first_at_least(const std::vector<int32_t>& ascending, int64_t r) {
  return std::lower_bound(ascending.begin(), ascending.end(), (int32_t)std::min<int64_t>(r, INT32_MAX)) -
         ascending.begin();
}

// The rows of [r0, r1) that the plan's row lists hold (a restricted walk plan's hold its kept
// rows only); a restricted plan without the walks is given its kept sub-ranges one at a time by
// spmm_launch.  timed: the live roofline's SpMM timer around the kernels.
template <int LPR>
static hnm_status spmm_range(hnm_ctx* ctx, const hnm_spmm_plan* pl, const int64_t* rowptr,
                             const int32_t* col, const float* val, const float* X, int d,
                             const SpmmEpi& ep, int64_t r0, int64_t r1, bool timed) {
  if (pl && pl->walk) {
    // short rows (<= SPMM_SHORT entries) by the short walk, then the rows of more entries by the
    // user-ordered walk (+ the split rows' finish), one stream, disjoint output rows
    const WalkSched* ws = nullptr;
    const ShortSched* ss = nullptr;
    hnm_status s = walk_get(ctx, pl, col, val, d, &ws, &ss);
    if (s) return s;
    const bool any = first_at_least(pl->h_walk_rows, r0) != first_at_least(pl->h_walk_rows, r1);
    float* partial = nullptr;
    if (any && ws->n_part > 0) {
      void* w;
      s = hnm_workspace(ctx, (size_t)ws->n_part * d * 4, &w);
      if (s) return s;
      partial = (float*)w;
    }
    if (timed) hnm_timer_begin(ctx, HNM_TIME_SPMM);
    if (r1 > r0 && ss) {
      // blocks whose rows meet [r0, r1) (blocks are in ascending row order)
      const int64_t b0 = first_at_least(ss->last, r0), b1 = first_at_least(ss->first, r1);
      if (b1 > b0) {
        const unsigned grid = (unsigned)std::min<int64_t>(b1 - b0, ss->nwg);
        hipLaunchKernelGGL(spmm_swalk_kernel<LPR>, dim3(grid), dim3(SWALK_THREADS), 0, ctx->stream,
                           ss->gptr.get(), ss->ent.get(), ss->wt.get(), ss->srow.get(),
                           ss->nslot.get(), ss->S, X, d, ep, r0, r1, b0, b1);
        HNM_LAUNCH_CHECK();
      }
    } else if (r1 > r0) {
      hipLaunchKernelGGL(spmm_mixed_kernel<LPR>,
                         dim3((unsigned)hnm_cdiv(r1 - r0, 4 * (64 / LPR))), dim3(256), 0,
                         ctx->stream, r0, r1, pl->long_rows.get(), (int64_t)0, (int64_t)0, (int64_t)0,
                         rowptr, col, val, X, d, ep);
      HNM_LAUNCH_CHECK();
    }
    if (any) {
      hipLaunchKernelGGL(spmm_walk_kernel<LPR>, dim3((unsigned)ws->nwg), dim3(WALK_THREADS), 0,
                         ctx->stream, ws->gptr.get(), ws->ent.get(), ws->wt.get(),
                         ws->slot_out.get(), ws->nslot.get(), ws->maxloc, ws->nwin, X, d, partial,
                         ep, r0, r1);
      HNM_LAUNCH_CHECK();
      if (ws->n_split > 0) {
        hipLaunchKernelGGL(spmm_walk_finish_kernel, dim3((unsigned)ws->n_split), dim3(256), 0,
                           ctx->stream, ws->split_rows.get(), ws->split_ptr.get(), partial, X, d,
                           ep, r0, r1);
        HNM_LAUNCH_CHECK();
      }
    }
    if (timed) hnm_timer_end(ctx, HNM_TIME_SPMM);
    return HNM_OK;
  }
  const bool has_heavy = pl && pl->n_heavy > 0;
  if (timed) hnm_timer_begin(ctx, HNM_TIME_SPMM);
  // the heavy rows' segments + finish run on the ctx's side stream, concurrent with the light
  // kernel (disjoint output rows, X read-only): they fill the CUs the light kernel's long item
  // rows leave idle at its tail; the ctx stream joins before anything reads Y
  bool forked = false;
  if (has_heavy) {
    // heavy rows inside [r0, r1): heavy rows are ascending
    const int64_t h0 = first_at_least(pl->h_heavy, r0), h1 = first_at_least(pl->h_heavy, r1);
    if (h1 > h0) {
      const int64_t sg0 = pl->h_seg_ptr[h0], sg1 = pl->h_seg_ptr[h1];
      void* w;
      hnm_status s = hnm_workspace(ctx, (size_t)(sg1 - sg0) * d * 4, &w);
      if (s) return s;
      float* partial = (float*)w;
      HNM_HIP_CHECK(hipEventRecord(ctx->side_in, ctx->stream));
      HNM_HIP_CHECK(hipStreamWaitEvent(ctx->side, ctx->side_in, 0));
      const hipStream_t hs = ctx->side;
      hipLaunchKernelGGL(spmm_segment_kernel<LPR>, dim3((unsigned)hnm_cdiv(sg1 - sg0, 4)),
                         dim3(256), 0, hs, sg0, sg1, pl->seg_start.get(), pl->seg_end.get(), col,
                         val, X, d, partial);
      HNM_LAUNCH_CHECK();
      hipLaunchKernelGGL(spmm_finish_kernel, dim3((unsigned)(h1 - h0)), dim3(256), 0, hs,
                         h0, pl->heavy_rows.get(), pl->seg_ptr.get(), sg0, partial, X, d, ep);
      HNM_LAUNCH_CHECK();
      HNM_HIP_CHECK(hipEventRecord(ctx->side_out, ctx->side));
      forked = true;
    }
  }
  if (r1 > r0) {
    if (pl) {
      // long rows inside [r0, r1) (ascending list) + every short row of the range
      const int64_t l0 = first_at_least(pl->h_long, r0), l1 = first_at_least(pl->h_long, r1);
      const int64_t nlb = hnm_cdiv(l1 - l0, 4), nsb = hnm_cdiv(r1 - r0, 4 * (64 / LPR));
      hipLaunchKernelGGL(spmm_mixed_kernel<LPR>, dim3((unsigned)(nlb + nsb)), dim3(256), 0,
                         ctx->stream, r0, r1, pl->long_rows.get(), l0, l1, nlb, rowptr, col, val, X,
                         d, ep);
    } else {
      // plan-less: every row by the light kernel, no heavy class
      hipLaunchKernelGGL(spmm_light_kernel<LPR>, dim3((unsigned)hnm_cdiv(r1 - r0, 4)), dim3(256), 0,
                         ctx->stream, r0, r1, rowptr, col, val, X, d, ep, (int64_t)INT64_MAX);
    }
    HNM_LAUNCH_CHECK();
  }
  if (forked) HNM_HIP_CHECK(hipStreamWaitEvent(ctx->stream, ctx->side_out, 0));
  if (timed) hnm_timer_end(ctx, HNM_TIME_SPMM);
  return HNM_OK;
}

template <int LPR>
static hnm_status spmm_launch(hnm_ctx* ctx, const hnm_spmm_plan* pl, int64_t N,
                              const int64_t* rowptr, const int32_t* col, const float* val,
                              const float* X, int d, const SpmmEpi& ep, int64_t r0, int64_t r1) {
  // the live roofline times whole-plan layers only (row-range calls do less work; a restricted
  // plan's whole layer is timed as such -- bench.py prices its kept rows)
  const bool timed = r0 == 0 && r1 == N;
  if (pl) {
    hnm_status s = walk_get(ctx, pl, col, val, 0, nullptr, nullptr);  // binding check
    if (s) return s;
  }
  if (!(pl && pl->restricted && !pl->walk))
    return spmm_range<LPR>(ctx, pl, rowptr, col, val, X, d, ep, r0, r1, timed);
  // a restricted plan without the walks: its kept sub-ranges of [r0, r1), one at a time
  if (timed) hnm_timer_begin(ctx, HNM_TIME_SPMM);
  for (size_t j = 0; j + 1 < pl->keep.size(); j += 2) {
    const int64_t a = std::max(r0, pl->keep[j]), b = std::min(r1, pl->keep[j + 1]);
    if (a >= b) continue;
    hnm_status s = spmm_range<LPR>(ctx, pl, rowptr, col, val, X, d, ep, a, b, false);
    if (s) return s;
  }
  if (timed) hnm_timer_end(ctx, HNM_TIME_SPMM);
  return HNM_OK;
}

#define HNM_SPMM_DISPATCH(FN, ...)                                                        \
  switch (d) {                                                                            \
    case 4: return FN<1>(__VA_ARGS__);                                                    \
    case 8: return FN<2>(__VA_ARGS__);                                                    \
    case 16: return FN<4>(__VA_ARGS__);                                                   \
    case 32: return FN<8>(__VA_ARGS__);                                                   \
    case 64: return FN<16>(__VA_ARGS__);                                                  \
    case 128: return FN<32>(__VA_ARGS__);                                                 \
    case 256: return FN<64>(__VA_ARGS__);                                                 \
    default:                                                                              \
      hnm_set_error("spmm: d must be one of 4, 8, 16, 32, 64, 128, 256 (got %d)", d);     \
      return HNM_EUNSUPPORTED;                                                            \
  }

extern "C" hnm_status hnm_spmm_csr_range_f32(hnm_ctx* ctx, const hnm_spmm_plan* plan, int64_t N,
                                             const int64_t* rowptr, const int32_t* col,
                                             const float* val, const float* X, int d, float* Y,
                                             float alpha, const float* acc_in, float* acc_out,
                                             float beta, int64_t row_begin, int64_t row_end,
                                             int64_t acc_row0) {
  HNM_CTX_DEVICE(ctx);
  HNM_REQUIRE(ctx && rowptr && col && val && X, HNM_EINVAL, "spmm: NULL argument");
  HNM_REQUIRE(!plan || plan->N == N, HNM_EINVAL, "spmm: plan built for a different graph");
  HNM_REQUIRE((uintptr_t)X % 16 == 0 && (!Y || (uintptr_t)Y % 16 == 0) &&
                  (!acc_out || (uintptr_t)acc_out % 16 == 0) &&
                  (!acc_in || (uintptr_t)acc_in % 16 == 0),
              HNM_EUNSUPPORTED, "spmm: buffers must be 16-B aligned");
  HNM_REQUIRE(0 <= row_begin && row_begin <= row_end && row_end <= N && 0 <= acc_row0 &&
                  acc_row0 <= N,
              HNM_EINVAL, "spmm: bad row range");
  if (N <= 0) return HNM_OK;
  const SpmmEpi ep{Y, alpha, beta, acc_in, acc_out, acc_row0};
  HNM_SPMM_DISPATCH(spmm_launch, ctx, plan, N, rowptr, col, val, X, d, ep, row_begin, row_end)
}

extern "C" hnm_status hnm_spmm_csr_f32(hnm_ctx* ctx, const hnm_spmm_plan* plan, int64_t N,
                                       const int64_t* rowptr, const int32_t* col,
                                       const float* val, const float* X, int d, float* Y,
                                       float alpha, const float* acc_in, float* acc_out) {
  HNM_CTX_DEVICE(ctx);
  return hnm_spmm_csr_range_f32(ctx, plan, N, rowptr, col, val, X, d, Y, alpha, acc_in, acc_out,
                                0.f, 0, N, 0);
}

template <int LPR>
static hnm_status combine_launch(hnm_ctx* ctx, const int64_t* rows, int64_t n, int64_t N,
                                 const int64_t* rowptr, const int32_t* col, const float* val,
                                 int d, const CombineLayers& cl, const CombineOrder& co, float* out) {
  const int64_t rows_per_block = co.mode != 0 ? 4 * (64 / LPR) : 4;
  hipLaunchKernelGGL(spmm_rows_combine_kernel<LPR>, dim3((unsigned)hnm_cdiv(n, rows_per_block)),
                     dim3(256), 0,
                     ctx->stream, rows, n, N, rowptr, col, val, d, cl, co, out, ctx->err_dev);
  HNM_LAUNCH_CHECK();
  return HNM_OK;
}

extern "C" hnm_status hnm_spmm_rows_combine_f32(hnm_ctx* ctx, const hnm_spmm_plan* plan,
                                                int64_t N, const int64_t* rowptr,
                                                const int32_t* col, const float* val,
                                                const int64_t* rows, int64_t n, int d,
                                                const float* const* layers, const float* alphas,
                                                int L, float* out) {
  HNM_CTX_DEVICE(ctx);
  HNM_REQUIRE(ctx && rowptr && col && val && layers && alphas && ((rows && out) || n == 0),
              HNM_EINVAL, "spmm_rows_combine: NULL argument");
  HNM_REQUIRE(!plan || plan->N == N, HNM_EINVAL, "spmm_rows_combine: plan built for a different graph");
  HNM_REQUIRE(L >= 1 && L <= 8, HNM_EUNSUPPORTED, "spmm_rows_combine: 1 <= L <= 8");
  CombineOrder co{};
  co.mode = plan ? 1 : 0;
  if (plan) {
    hnm_status s = walk_get(ctx, plan, col, val, 0, nullptr, nullptr);
    if (s) return s;
    if (plan->walk) {
      co.mode = 2;
      co.short_sorted = plan->swalk;
      co.scol = plan->scol.get();
      co.sval = plan->sval.get();
      co.cap = plan->walk_cap;
    }
  }
  CombineLayers cl;
  cl.L = L;
  for (int l = 0; l < L; ++l) {
    HNM_REQUIRE(layers[l] && (uintptr_t)layers[l] % 16 == 0, HNM_EINVAL,
                "spmm_rows_combine: layer %d NULL or not 16-B aligned", l);
    cl.E[l] = layers[l];
  }
  for (int l = 0; l <= L; ++l) cl.a[l] = alphas[l];
  if (n <= 0) return HNM_OK;
  HNM_REQUIRE((uintptr_t)out % 16 == 0, HNM_EINVAL, "spmm_rows_combine: out not 16-B aligned");
  HNM_SPMM_DISPATCH(combine_launch, ctx, rows, n, N, rowptr, col, val, d, cl, co, out)
}
