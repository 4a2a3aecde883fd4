// LightGCN graph path, SpMM planning (host only, no kernels): the row classes of a graph, the
// plan's binding to col / val with the column-sorted copy, the bipartite side routing, the two
// walks' schedules per embedding width, and plan create / prepare / restrict / destroy.
//
// Ownership: a plan is a C++ object created with new; its host arrays are vectors, its device
// arrays and those of its schedules are DevBuf (graph_internal.h).  Create, restrict, bind and
// the schedule builders fill a local object and install it only when every step succeeded, so
// every early return frees what it made and leaves the plan as it was.
#include <algorithm>
#include <memory>
#include <mutex>
#include <queue>
#include <thread>
#include <vector>

#include "graph_internal.h"

template <typename F>
static void parallel_for(int64_t n, F fn) {
  const int nt = (int)std::max<int64_t>(1, std::min<int64_t>(
      std::min<unsigned>(16, std::max(1u, std::thread::hardware_concurrency())), n / 64 + 1));
  std::vector<std::thread> th;
  for (int t = 0; t < nt; ++t)
    th.emplace_back([&, t] {
      for (int64_t i = t; i < n; i += nt) fn(i);
    });
  for (auto& x : th) x.join();
}

// A bipartite graph stored with contiguous sides -- rows [0, S) connected only to [S, N) and
// back, self-loops aside (the reference's user / item layout, lightgcn.py:81-112) -- has one
// side whose rows all gather the OTHER side's table.  The short walk suits the side that gathers
// the smaller table (users: the 27 MB item table at d = 64); the short rows of the side that
// gathers the larger table (the tail items, < 129 entries into the 351 MB user table) join the
// user-ordered walk instead, where their gathers ride the same column sweep as the long item
// rows.  A short row is one piece there, so its value is the same sorted-order fma chain
// either way (rows_combine is unchanged).  Called once at binding, before any schedule.
static void plan_bipartite_sides(hnm_spmm_plan* pl) {
  const std::vector<int64_t>& rp = pl->h_rowptr;
  const std::vector<int32_t>& hc = pl->h_scol;
  const int64_t N = pl->N;
  // per row the smallest / largest neighbour other than itself (entries are column-sorted);
  // a split S is valid when every row below it only reaches [S, N) and every row from it on
  // only reaches [0, S): prefix min of the minima >= S and suffix max of the maxima < S
  std::vector<int64_t> mn((size_t)N), mx((size_t)N);
  parallel_for(hnm_cdiv(N, 4096), [&](int64_t ch) {
    const int64_t r1 = std::min<int64_t>(N, (ch + 1) * 4096);
    for (int64_t r = ch * 4096; r < r1; ++r) {
      int64_t lo = N, hi = -1;
      for (int64_t q = rp[r]; q < rp[r + 1]; ++q)
        if (hc[q] != r) {
          lo = std::min<int64_t>(lo, hc[q]);
          hi = std::max<int64_t>(hi, hc[q]);
        }
      mn[r] = lo;
      mx[r] = hi;
    }
  });
  std::vector<int64_t> smax((size_t)N + 1, -1);
  for (int64_t r = N - 1; r >= 0; --r) smax[r] = std::max(smax[r + 1], mx[r]);
  int64_t S = -1, pmin = N;
  for (int64_t c = 1; c < N; ++c) {
    pmin = std::min(pmin, mn[c - 1]);
    if (pmin >= c && smax[c] < c && pmin < N && smax[c] >= 0) {
      S = c;
      break;
    }
  }
  if (S <= 0) return;
  // the side whose neighbours form the larger table moves its short rows into the walk
  const bool upper = S > N - S;  // rows [S, N) gather the S-row table
  const int64_t lo = upper ? S : 0, hi = upper ? N : S;
  std::vector<int32_t>& sr = pl->h_short_rows;
  std::vector<int32_t>& wr = pl->h_walk_rows;
  std::vector<int32_t> keep, moved;
  for (int32_t r : sr) (r >= lo && r < hi && rp[r + 1] > rp[r] ? moved : keep).push_back(r);
  if (moved.empty() || keep.empty()) return;
  std::vector<int32_t> merged((size_t)(wr.size() + moved.size()));
  std::merge(wr.begin(), wr.end(), moved.begin(), moved.end(), merged.begin());
  for (int32_t r : moved) pl->walk_nnz += rp[r + 1] - rp[r];
  wr.swap(merged);
  sr.swap(keep);
  pl->n_walk = (int64_t)wr.size();
  pl->walk_cap = std::max<int64_t>(512, hnm_cdiv(pl->walk_nnz, 2 * WALK_GROUPS_TARGET));
}

// Binds the plan to col / val on first use.  A walk plan then copies the CSR to the host,
// stable-sorts every row's entries by column (the walks' summation order: (col, CSR position))
// and uploads the sorted copy (rows_combine repeats the walks' order from it).  Later calls
// must pass the same col / val: a plan snapshots the graph's values.  Caller holds pl->mu.
static hnm_status plan_bind(hnm_ctx* ctx, hnm_spmm_plan* pl, const int32_t* col, const float* val) {
  if (pl->bound_col) {
    HNM_REQUIRE(col == pl->bound_col && val == pl->bound_val, HNM_EINVAL,
                "spmm: this plan is bound to the col / val of its first use (it snapshots the "
                "graph's values); create a new plan for other values");
    return HNM_OK;
  }
  if (pl->walk) {
    const int64_t T = pl->nnz;
    const std::vector<int64_t>& rp = pl->h_rowptr;
    std::vector<int32_t> c0((size_t)T);
    std::vector<float> v0((size_t)T);
    HNM_HIP_CHECK(hipMemcpyAsync(c0.data(), col, T * 4, hipMemcpyDeviceToHost, ctx->stream));
    HNM_HIP_CHECK(hipMemcpyAsync(v0.data(), val, T * 4, hipMemcpyDeviceToHost, ctx->stream));
    HNM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    // all-or-nothing: the host copies and device uploads are locals, moved into the plan only
    // when every step succeeded, so a failed bind leaves the plan unbound and a retry starts clean
    std::vector<int32_t> hc((size_t)T);
    std::vector<float> hv((size_t)T);
    const int64_t nchunk = hnm_cdiv(pl->N, 4096);
    parallel_for(nchunk, [&](int64_t ch) {
      std::vector<int32_t> ix;
      const int64_t r1 = std::min<int64_t>(pl->N, (ch + 1) * 4096);
      for (int64_t r = ch * 4096; r < r1; ++r) {
        const int64_t a = rp[r], L = rp[r + 1] - a;
        ix.resize((size_t)L);
        for (int64_t q = 0; q < L; ++q) ix[q] = (int32_t)q;
        std::stable_sort(ix.begin(), ix.end(),
                         [&](int32_t x, int32_t y) { return c0[a + x] < c0[a + y]; });
        for (int64_t q = 0; q < L; ++q) {
          hc[a + q] = c0[a + ix[q]];
          hv[a + q] = v0[a + ix[q]];
        }
      }
    });
    DevBuf<int32_t> dcol;
    DevBuf<float> dval;
    hnm_status st;
    if ((st = dcol.upload(hc.data(), (size_t)T)) || (st = dval.upload(hv.data(), (size_t)T))) return st;
    pl->scol = std::move(dcol);
    pl->sval = std::move(dval);
    pl->h_scol = std::move(hc);
    pl->h_sval = std::move(hv);
    if (pl->swalk) plan_bipartite_sides(pl);
  }
  pl->bound_col = col;
  pl->bound_val = val;
  return HNM_OK;
}

// ---------------------------------------------------------------- walk schedules
// The two steps both schedule builders share.  Placement only moves work between lanes; the
// order inside each piece / row (and so every result) is fixed by the sorted copy.

// Deals items 0 .. n-1, in that order, to ng groups: each goes to the group of the least load so
// far (the first of equals), whose load grows by len(i).  Returns the items of every group.
template <typename Len>
static std::vector<std::vector<int32_t>> deal_least_loaded(int64_t n, int ng, Len len) {
  std::vector<std::vector<int32_t>> groups((size_t)ng);
  std::vector<int64_t> load((size_t)ng, 0);
  for (int64_t i = 0; i < n; ++i) {
    const int g = (int)(std::min_element(load.begin(), load.end()) - load.begin());
    groups[g].push_back((int32_t)i);
    load[g] += len(i);
  }
  return groups;
}

// One lane group's list: the entries first, first + stride, ... < end of the sorted copy
// accumulate into LDS slot `slot`.
struct SlotRun {
  int32_t slot;
  int64_t first, stride, end;
};
using WalkRecord = std::pair<uint64_t, float>;  // (col << 10 | slot, weight)

// Gathers the runs' records into rec in run order and stable-sorts them by column, so a slot's
// entries keep their (col, CSR position) order.  put_records then writes rec[i0, i1) to ent / wt
// from offset o on and returns the offset past the last one (where a list is cut into windows or
// padded is the builder's business).
static void merge_runs_by_column(const std::vector<SlotRun>& runs, const std::vector<int32_t>& hc,
                                 const std::vector<float>& hv, std::vector<WalkRecord>& rec) {
  rec.clear();
  for (const SlotRun& r : runs)
    for (int64_t q = r.first; q < r.end; q += r.stride)
      rec.push_back({((uint64_t)(uint32_t)hc[q] << 10) | (uint64_t)r.slot, hv[q]});
  std::stable_sort(rec.begin(), rec.end(),
                   [](const auto& x, const auto& y) { return (x.first >> 10) < (y.first >> 10); });
}
static int64_t put_records(const std::vector<WalkRecord>& rec, size_t i0, size_t i1,
                           std::vector<uint32_t>& ent, std::vector<float>& wt, int64_t o) {
  for (size_t i = i0; i < i1; ++i) {
    ent[o] = (uint32_t)rec[i].first;
    wt[o++] = rec[i].second;
  }
  return o;
}

// Schedule for d (LPR = d / 4 lanes per row): pieces to workgroups (greedy, longest first,
// least-loaded workgroup with a free slot), then to the workgroup's groups (least-loaded), then
// each group's pieces merged by column.
static hnm_status walk_build(const hnm_spmm_plan* pl, int d, std::unique_ptr<WalkSched>* out) {
  const int lpr = d / 4, ng = WALK_THREADS / lpr;
  // slot maxloc absorbs the windows' padding entries (never stored)
  const int maxloc = std::min(1022, WALK_LDS_F4 / lpr - 1);
  const std::vector<int64_t>& rp = pl->h_rowptr;
  const std::vector<int32_t>& wr = pl->h_walk_rows;
  const int64_t cap = pl->walk_cap, T = pl->walk_nnz;
  struct Piece {
    int32_t k;     // walk row
    int32_t j, n;  // piece j of n
    int64_t len;
  };
  std::vector<Piece> pcs;
  for (int64_t k = 0; k < pl->n_walk; ++k) {
    const int64_t L = rp[wr[k] + 1] - rp[wr[k]];
    const int n = (int)hnm_cdiv(L, cap);
    for (int j = 0; j < n; ++j) pcs.push_back({(int32_t)k, j, n, (L - j + n - 1) / n});
  }
  std::stable_sort(pcs.begin(), pcs.end(), [](const Piece& a, const Piece& b) { return a.len > b.len; });
  int64_t nwg = std::max<int64_t>(1, std::min<int64_t>(hnm_cdiv(WALK_GROUPS_TARGET, ng),
                                                        hnm_cdiv(T, (int64_t)ng * 256)));
  while ((int64_t)pcs.size() > nwg * maxloc * 7 / 8) nwg *= 2;
  // a walk of a few entries a group (a restricted plan's item shard: ~260 entries a group at
  // d = 128 for 1/8 of the H&M items) is bound by the per-window latency, not by its gathers:
  // one round of workgroups (one per CU) instead of a second partial round, when the slots hold
  // every piece (placement only moves pieces between lanes; every result is unchanged)
  const int64_t cus = std::max(1, pl->num_cus);
  if (nwg > cus && (int64_t)pcs.size() <= cus * maxloc * 7 / 8 && T <= cus * ng * 1024) nwg = cus;
  std::vector<std::vector<int32_t>> wgp((size_t)nwg);
  {
    using E = std::pair<int64_t, int64_t>;
    std::priority_queue<E, std::vector<E>, std::greater<E>> q;
    for (int64_t w = 0; w < nwg; ++w) q.push({0, w});
    for (int32_t pi = 0; pi < (int32_t)pcs.size(); ++pi) {
      E t = q.top();
      q.pop();
      while ((int64_t)wgp[t.second].size() >= maxloc) {  // full: drop it from the heap
        t = q.top();
        q.pop();
      }
      wgp[t.second].push_back(pi);
      q.push({t.first + pcs[pi].len, t.second});
    }
  }
  // partial indices of split rows: row k's pieces j = 0..n-1 at split_ptr[si] + j
  std::vector<int32_t> srows;
  std::vector<int64_t> sptr{0}, kpart((size_t)pl->n_walk, -1);
  for (int64_t k = 0; k < pl->n_walk; ++k) {
    const int n = (int)hnm_cdiv(rp[wr[k] + 1] - rp[wr[k]], cap);
    if (n <= 1) continue;
    kpart[k] = sptr.back();
    srows.push_back(wr[k]);
    sptr.push_back(sptr.back() + n);
  }
  std::vector<int32_t> slot_out((size_t)(nwg * maxloc), 0), nslot((size_t)nwg);
  std::vector<std::vector<std::vector<int32_t>>> gslots((size_t)nwg);  // per workgroup, per group
  for (int64_t w = 0; w < nwg; ++w) {
    nslot[w] = (int32_t)wgp[w].size();
    gslots[w] = deal_least_loaded(nslot[w], ng, [&](int64_t sl) { return pcs[wgp[w][sl]].len; });
    for (int sl = 0; sl < nslot[w]; ++sl) {
      const Piece& pc = pcs[wgp[w][sl]];
      slot_out[w * maxloc + sl] = pc.n == 1 ? wr[pc.k] : (int32_t)(-(kpart[pc.k] + pc.j) - 1);
    }
  }
  // each group's list is cut at K column bounds (k + 1) * cdiv(N, K), each window padded to a
  // multiple of 4 entries; the kernel syncs its groups after every window
  const int K = walk_windows(d);
  const int64_t wlen = hnm_cdiv(pl->N, K);
  const std::vector<int32_t>& hc = pl->h_scol;
  const std::vector<float>& hv = pl->h_sval;
  std::vector<int64_t> wcnt((size_t)(nwg * ng * K), 0);
  parallel_for(nwg, [&](int64_t w) {
    for (int g = 0; g < ng; ++g)
      for (int sl : gslots[w][g]) {
        const Piece& pc = pcs[wgp[w][sl]];
        const int64_t a = rp[wr[pc.k]], L = rp[wr[pc.k] + 1] - a;
        for (int64_t q = pc.j; q < L; q += pc.n) ++wcnt[(w * ng + g) * K + hc[a + q] / wlen];
      }
  });
  std::vector<int64_t> gptr((size_t)(nwg * ng * K + 1), 0);
  for (int64_t i = 0; i < nwg * ng * K; ++i)
    gptr[i + 1] = gptr[i] + (K > 1 ? hnm_cdiv(wcnt[i], WALK_STEP) * WALK_STEP : wcnt[i]);
  const int64_t Tp = gptr.back();
  std::vector<uint32_t> ent((size_t)Tp, (uint32_t)maxloc);  // padding: col 0, spare slot, 0.0
  std::vector<float> wt((size_t)Tp, 0.f);
  parallel_for(nwg, [&](int64_t w) {
    std::vector<SlotRun> runs;
    std::vector<WalkRecord> rec;
    for (int g = 0; g < ng; ++g) {
      runs.clear();
      for (int sl : gslots[w][g]) {
        const Piece& pc = pcs[wgp[w][sl]];
        const int64_t a = rp[wr[pc.k]];
        runs.push_back({sl, a + pc.j, pc.n, rp[wr[pc.k] + 1]});
      }
      merge_runs_by_column(runs, hc, hv, rec);
      size_t i = 0;
      for (int k = 0; k < K; ++k) {
        size_t i1 = i;
        while (i1 < rec.size() && (int64_t)(rec[i1].first >> 10) / wlen == k) ++i1;
        put_records(rec, i, i1, ent, wt, gptr[(w * ng + g) * K + k]);
        i = i1;
      }
    }
  });
  std::unique_ptr<WalkSched> ws(new WalkSched());
  ws->lpr = lpr;
  ws->ng = ng;
  ws->nwg = (int)nwg;
  ws->maxloc = maxloc;
  ws->nwin = K;
  ws->n_split = (int64_t)srows.size();
  ws->n_part = sptr.back();
  hnm_status st;
  if ((st = ws->gptr.upload(gptr.data(), gptr.size())) || (st = ws->ent.upload(ent.data(), ent.size())) ||
      (st = ws->wt.upload(wt.data(), wt.size())) ||
      (st = ws->slot_out.upload(slot_out.data(), slot_out.size())) ||
      (st = ws->nslot.upload(nslot.data(), nslot.size())) ||
      (st = ws->split_rows.upload(srows.data(), srows.size())) ||
      (st = ws->split_ptr.upload(sptr.data(), sptr.size())))
    return st;
  *out = std::move(ws);
  return HNM_OK;
}

// Short-walk schedule for d: the short rows cut into nb blocks of consecutive rows at equal
// shares of their entries (at most S rows a block; nb a multiple of the persistent grid once the
// graph fills it), each block's rows dealt to its ng lane groups (longest first, least-loaded
// group), each group's rows' entries merged by column and padded to multiples of swalk_step with
// weight-0 entries into the spare slot S.
static hnm_status swalk_build(const hnm_spmm_plan* pl, int d, std::unique_ptr<ShortSched>* out) {
  const int lpr = d / 4, ng = SWALK_THREADS / lpr;
  const int S = std::min(1022, SWALK_LDS_F4 / lpr - 1);
  const std::vector<int64_t>& rp = pl->h_rowptr;
  const std::vector<int32_t>& sr = pl->h_short_rows;
  const std::vector<int32_t>& hc = pl->h_scol;
  const std::vector<float>& hv = pl->h_sval;
  const int64_t ns = (int64_t)sr.size();
  const int64_t nwg_full = (int64_t)std::max(1, pl->num_cus) * SWALK_WG_PER_CU;
  std::vector<int64_t> cum((size_t)ns + 1, 0);
  for (int64_t i = 0; i < ns; ++i) cum[i + 1] = cum[i] + (rp[sr[i] + 1] - rp[sr[i]]);
  const int64_t total = cum[ns];
  int64_t nb0 = std::max<int64_t>(1, hnm_cdiv(ns, S));
  int64_t nb = nb0 >= nwg_full ? hnm_cdiv(nb0, nwg_full) * nwg_full : nb0;
  std::vector<int64_t> bstart;  // first short-row index of each block (+ end)
  for (;;) {
    bstart.assign(1, 0);
    int64_t i = 0;
    for (int64_t b = 0; b < nb; ++b) {
      const int64_t target = total * (b + 1) / nb;
      int64_t j = i;
      while (j < ns && j - i < S && (b == nb - 1 || cum[j + 1] <= target || j == i)) ++j;
      i = j;
      bstart.push_back(i);
    }
    if (i >= ns) break;
    nb += nb >= nwg_full ? nwg_full : 1;  // the last block overflowed S rows
  }
  std::vector<int32_t> srow((size_t)(nb * S), -1), nslot((size_t)nb, 0);
  std::vector<int64_t> wcnt((size_t)(nb * ng), 0);
  std::vector<std::vector<std::vector<int32_t>>> gslot((size_t)nb);  // per block, per group: slots
  parallel_for(nb, [&](int64_t b) {
    const int64_t i0 = bstart[b], n = bstart[b + 1] - i0;
    nslot[b] = (int32_t)n;
    std::vector<int32_t> ord((size_t)n);
    for (int64_t s = 0; s < n; ++s) {
      srow[b * S + s] = sr[i0 + s];
      ord[s] = (int32_t)s;
    }
    auto len = [&](int64_t s) { return cum[i0 + s + 1] - cum[i0 + s]; };
    std::stable_sort(ord.begin(), ord.end(), [&](int32_t x, int32_t y) { return len(x) > len(y); });
    gslot[b] = deal_least_loaded(n, ng, [&](int64_t i) { return len(ord[i]); });
    for (int g = 0; g < ng; ++g)
      for (int32_t& s : gslot[b][g]) {
        s = ord[s];  // dealt position -> slot
        wcnt[b * ng + g] += len(s);
      }
  });
  std::vector<int64_t> gptr((size_t)(nb * ng + 1), 0);
  for (int64_t i = 0; i < nb * ng; ++i)
    gptr[i + 1] = gptr[i] + hnm_cdiv(wcnt[i], swalk_step(lpr)) * swalk_step(lpr);
  const int64_t Tp = gptr.back();
  std::vector<uint32_t> ent((size_t)Tp, (uint32_t)S);
  std::vector<float> wt((size_t)Tp, 0.f);
  parallel_for(nb, [&](int64_t b) {
    const int64_t i0 = bstart[b];
    std::vector<SlotRun> runs;
    std::vector<WalkRecord> rec;
    for (int g = 0; g < ng; ++g) {
      std::vector<int32_t> sl = gslot[b][g];
      std::sort(sl.begin(), sl.end());
      runs.clear();
      for (int32_t s : sl) runs.push_back({s, rp[sr[i0 + s]], 1, rp[sr[i0 + s] + 1]});
      merge_runs_by_column(runs, hc, hv, rec);
      int64_t o = put_records(rec, 0, rec.size(), ent, wt, gptr[b * ng + g]);
      // padding re-gathers the list's last column (a cached row) into the spare slot
      const uint32_t pad = rec.empty() ? (uint32_t)S
                                       : (uint32_t)((rec.back().first >> 10) << 10) | (uint32_t)S;
      for (const int64_t e = gptr[b * ng + g + 1]; o < e; ++o) ent[o] = pad;
    }
  });
  std::unique_ptr<ShortSched> ws(new ShortSched());
  ws->lpr = lpr;
  ws->ng = ng;
  ws->S = S;
  ws->nb = nb;
  ws->nwg = (int)std::min<int64_t>(nb, nwg_full);
  ws->first.resize((size_t)nb);
  ws->last.resize((size_t)nb);
  for (int64_t b = 0; b < nb; ++b) {
    const int64_t n = bstart[b + 1] - bstart[b];
    ws->first[b] = n ? sr[bstart[b]] : (b ? ws->last[b - 1] : 0);
    ws->last[b] = n ? sr[bstart[b + 1] - 1] : ws->first[b];
  }
  hnm_status st;
  if ((st = ws->gptr.upload(gptr.data(), gptr.size())) || (st = ws->ent.upload(ent.data(), ent.size())) ||
      (st = ws->wt.upload(wt.data(), wt.size())) || (st = ws->srow.upload(srow.data(), srow.size())) ||
      (st = ws->nslot.upload(nslot.data(), nslot.size())))
    return st;
  *out = std::move(ws);
  return HNM_OK;
}

static int walk_index(int d) {
  int i = 0;
  while ((4 << i) < d) ++i;
  return i;
}

static bool spmm_d_ok(int d) {
  for (int i = 0; i < 7; ++i)
    if (d == (4 << i)) return true;
  return false;
}

// The plan is const to its callers (the C ABI's SpMM entry points take a const plan); binding and
// the per-d schedules are its lazily built cache, guarded by pl->mu.
hnm_status walk_get(hnm_ctx* ctx, const hnm_spmm_plan* cpl, const int32_t* col, const float* val,
                    int d, const WalkSched** out, const ShortSched** sout) {
  hnm_spmm_plan* pl = const_cast<hnm_spmm_plan*>(cpl);
  std::lock_guard<std::mutex> lk(pl->mu);
  hnm_status s = plan_bind(ctx, pl, col, val);
  if (s) return s;
  if (!pl->walk || d <= 0) return HNM_OK;
  const int i = walk_index(d);
  if (!pl->sched[i] && (s = walk_build(pl, d, &pl->sched[i]))) return s;
  if (pl->swalk && !pl->ssched[i] && (s = swalk_build(pl, d, &pl->ssched[i]))) return s;
  if (out) *out = pl->sched[i].get();
  if (sout) *sout = pl->ssched[i].get();
  return HNM_OK;
}

extern "C" hnm_status hnm_spmm_plan_create(hnm_ctx* ctx, int64_t N, const int64_t* rowptr,
                                           hnm_spmm_plan** out) {
  HNM_CTX_DEVICE(ctx);
  HNM_REQUIRE(ctx && rowptr && out && N > 0, HNM_EINVAL, "spmm_plan: bad argument");
  std::vector<int64_t> rp((size_t)N + 1);
  HNM_HIP_CHECK(hipMemcpyAsync(rp.data(), rowptr, (N + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
  HNM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  std::unique_ptr<hnm_spmm_plan> pl(new hnm_spmm_plan());
  std::vector<int32_t> shrow;
  std::vector<int64_t> sstart, send;
  pl->h_seg_ptr.assign(1, 0);
  for (int64_t r = 0; r < N; ++r) {
    const int64_t s = rp[r], e = rp[r + 1];
    HNM_REQUIRE(e >= s, HNM_EINVAL, "spmm_plan: rowptr decreases at row %lld", (long long)r);
    if (e - s > SPMM_SHORT && e - s <= HEAVY) pl->h_long.push_back((int32_t)r);
    if (e - s <= HEAVY) continue;
    const int32_t hi = (int32_t)pl->h_heavy.size();
    pl->h_heavy.push_back((int32_t)r);
    for (int64_t q = s; q < e; q += SEG) {
      shrow.push_back(hi);
      sstart.push_back(q);
      send.push_back(std::min<int64_t>(q + SEG, e));
    }
    pl->h_seg_ptr.push_back((int64_t)sstart.size());
  }
  pl->device = ctx->device;
  pl->num_cus = ctx->num_cus;
  pl->N = N;
  pl->nnz = rp[N] - rp[0];
  pl->n_heavy = (int64_t)pl->h_heavy.size();
  pl->n_seg = (int64_t)sstart.size();
  pl->n_long = (int64_t)pl->h_long.size();
  // walk rows: every row of more than SPMM_SHORT entries (col << 10 must fit 32 bits)
  pl->walk = N <= (int64_t)1 << 22 && rp[0] == 0 &&
             rp[N] < ((int64_t)1 << 32);
  if (pl->walk) {
    for (int64_t r = 0; r < N; ++r) {
      const int64_t L = rp[r + 1] - rp[r];
      if (L <= SPMM_SHORT) {
        pl->h_short_rows.push_back((int32_t)r);
        continue;
      }
      pl->h_walk_rows.push_back((int32_t)r);
      pl->walk_nnz += L;
    }
    pl->n_walk = (int64_t)pl->h_walk_rows.size();
    // pieces of at most cap entries: half a group's share of a big graph's walk (so the
    // longest list is ~2x the mean), never below 512
    pl->walk_cap = std::max<int64_t>(512, hnm_cdiv(pl->walk_nnz, 2 * WALK_GROUPS_TARGET));
    pl->h_rowptr = std::move(rp);
    pl->swalk = !pl->h_short_rows.empty();
  }
  hnm_status st;
  if (pl->n_long > 0 && (st = pl->long_rows.upload(pl->h_long.data(), (size_t)pl->n_long))) return st;
  if (pl->n_heavy > 0 &&
      ((st = pl->heavy_rows.upload(pl->h_heavy.data(), (size_t)pl->n_heavy)) ||
       (st = pl->seg_ptr.upload(pl->h_seg_ptr.data(), (size_t)pl->n_heavy + 1)) ||
       (st = pl->seg_hrow.upload(shrow.data(), (size_t)pl->n_seg)) ||
       (st = pl->seg_start.upload(sstart.data(), (size_t)pl->n_seg)) ||
       (st = pl->seg_end.upload(send.data(), (size_t)pl->n_seg))))
    return st;
  *out = pl.release();
  return HNM_OK;
}

extern "C" hnm_status hnm_spmm_plan_prepare(hnm_ctx* ctx, hnm_spmm_plan* plan, const int32_t* col,
                                            const float* val, int d) {
  HNM_CTX_DEVICE(ctx);
  HNM_REQUIRE(ctx && plan && col && val, HNM_EINVAL, "spmm_plan_prepare: NULL argument");
  HNM_REQUIRE(d == 0 || spmm_d_ok(d), HNM_EUNSUPPORTED,
              "spmm_plan_prepare: d must be 0 or one of 4, 8, 16, 32, 64, 128, 256 (got %d)", d);
  return walk_get(ctx, plan, col, val, d, nullptr, nullptr);
}

extern "C" hnm_status hnm_spmm_plan_destroy(hnm_spmm_plan* pl) {
  if (!pl) return HNM_OK;
  const HnmDeviceGuard guard(pl->device);
  delete pl;
  return HNM_OK;
}

// Item-sharded propagation: a copy of a bound plan that computes
// only the rows of `ranges` -- e.g. every user row plus this rank's item rows.  A walk plan keeps
// the base's piece length (cap), its bipartite routing and its sorted copy, and filters the walk
// and short-walk row lists, so every kept row is cut into the same pieces and summed in the same
// order as by the base (bitwise equal rows), while the walks' schedules -- built per d on first
// use -- hold only the kept rows' entries (work proportional to them).  A plan without the walks
// runs the kept sub-ranges of each call with its row-class kernels (per-row order independent of
// the range).
extern "C" hnm_status hnm_spmm_plan_restrict(hnm_ctx* ctx, const hnm_spmm_plan* base,
                                             const int64_t* ranges, int n_ranges,
                                             hnm_spmm_plan** out) {
  HNM_CTX_DEVICE(ctx);
  HNM_REQUIRE(ctx && base && out && n_ranges >= 0 && (ranges || n_ranges == 0), HNM_EINVAL,
              "spmm_plan_restrict: bad argument");
  HNM_REQUIRE(!base->restricted, HNM_EINVAL, "spmm_plan_restrict: the base plan is itself restricted");
  for (int j = 0; j < n_ranges; ++j)
    HNM_REQUIRE(ranges[2 * j] >= (j ? ranges[2 * j - 1] : 0) && ranges[2 * j] <= ranges[2 * j + 1] &&
                    ranges[2 * j + 1] <= base->N,
                HNM_EINVAL, "spmm_plan_restrict: ranges must be ascending, disjoint, inside [0, N)");
  std::lock_guard<std::mutex> lk(base->mu);
  HNM_REQUIRE(base->bound_col, HNM_EINVAL,
              "spmm_plan_restrict: bind the base plan first (hnm_spmm_plan_prepare, d = 0)");
  std::unique_ptr<hnm_spmm_plan> pl(new hnm_spmm_plan());
  pl->restricted = true;
  pl->keep.assign(ranges, ranges + 2 * n_ranges);
  const std::vector<int64_t>& kr = pl->keep;
  auto kept = [&](int64_t r) {
    // first range whose end is past r
    int lo = 0, hi = n_ranges;
    while (lo < hi) {
      const int m = (lo + hi) / 2;
      if (kr[2 * m + 1] <= r) lo = m + 1; else hi = m;
    }
    return lo < n_ranges && kr[2 * lo] <= r;
  };
  pl->device = base->device;
  pl->num_cus = base->num_cus;
  pl->N = base->N;
  pl->nnz = base->nnz;
  pl->walk = base->walk;
  pl->swalk = base->swalk;
  pl->walk_cap = base->walk_cap;
  pl->bound_col = base->bound_col;
  pl->bound_val = base->bound_val;
  hnm_status st;
  if (base->walk) {
    const std::vector<int64_t>& rp = base->h_rowptr;
    pl->h_rowptr = rp;
    pl->h_scol = base->h_scol;
    pl->h_sval = base->h_sval;
    for (int32_t r : base->h_walk_rows)
      if (kept(r)) {
        pl->h_walk_rows.push_back(r);
        pl->walk_nnz += rp[r + 1] - rp[r];
      }
    for (int32_t r : base->h_short_rows)
      if (kept(r)) pl->h_short_rows.push_back(r);
    pl->n_walk = (int64_t)pl->h_walk_rows.size();
    pl->h_seg_ptr.assign(1, 0);
    if ((st = pl->scol.dup(base->scol.get(), (size_t)base->nnz)) ||
        (st = pl->sval.dup(base->sval.get(), (size_t)base->nnz)))
      return st;
  } else {
    pl->n_heavy = base->n_heavy;
    pl->n_seg = base->n_seg;
    pl->n_long = base->n_long;
    pl->h_long = base->h_long;
    pl->h_heavy = base->h_heavy;
    pl->h_seg_ptr = base->h_seg_ptr;
    if ((st = pl->long_rows.dup(base->long_rows.get(), (size_t)base->n_long)) ||
        (st = pl->heavy_rows.dup(base->heavy_rows.get(), (size_t)base->n_heavy)) ||
        (st = pl->seg_ptr.dup(base->seg_ptr.get(), (size_t)base->n_heavy + 1)) ||
        (st = pl->seg_hrow.dup(base->seg_hrow.get(), (size_t)base->n_seg)) ||
        (st = pl->seg_start.dup(base->seg_start.get(), (size_t)base->n_seg)) ||
        (st = pl->seg_end.dup(base->seg_end.get(), (size_t)base->n_seg)))
      return st;
  }
  *out = pl.release();
  return HNM_OK;
}
