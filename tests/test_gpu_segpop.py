"""GPU: SegmentPopularity -- hnm_segpop_fit_f64 / hnm_segpop_topk_f32, the module and the
`cold_start="segment"` request path.

The reference has no such model, so the yardsticks are the numpy / Python restatement of the
header's contracts (segpop_oracle.py: the integer table, the ascending-day float64 chain, the
two-phase list comprehension) and the existing PopularityBaseline at its current bits.  Every
comparison is exact: counts, float64 / float32 bit patterns, item ids, seam positions.

The transactions are tests/golden/popularity_small.npz (I ~ 220 items, its users and days);
the users' segments come from a fixed PCG64, about a tenth of them unknown (-1).
"""
import numpy as np
import pytest
import torch

import fuse_oracle as FO
import segpop_oracle as SO
from parity import load_golden
from hnm_recommendation_amd import (Ensemble, NeuralCF, PopularityBaseline, SegmentPopularity,
                                    UserHistory, _lib)
from hnm_recommendation_amd.evaluation import evaluate_recommendations
from hnm_recommendation_amd.serving import Recommender

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
G = load_golden("popularity_small.npz")
I, U = int(G["I"]), int(G["U"])
ITEMS, USERS, DAYS = (G[k].astype(np.int64) for k in ("items", "users", "days"))
NEG_INF = float("-inf")


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype))).to(DEV)


def bits(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else t
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def user_segments(S, seed=77):
    rng = np.random.Generator(np.random.PCG64(seed))
    seg = rng.integers(0, S, size=U).astype(np.int32)
    seg[rng.random(U) < 0.1] = -1
    return seg


def ctx_check():
    return _lib.fn("hnm_ctx_check")(_lib.ctx(DEV))


# ------------------------------------------------------------------ fit
def raw_fit(items, users, useg, days, w, num_items, S, D, slab=0):
    it, us = dev(items, np.int64), dev(users, np.int64)
    sg = dev(useg, np.int32)
    dd = None if days is None else dev(days, np.int32)
    ww = None if w is None else dev(w, np.float64)
    rows = max(S, 0) + 1
    count = torch.full((rows, num_items), -7, dtype=torch.int64, device=DEV)
    pop = torch.full((rows, num_items), -7.0, dtype=torch.float64, device=DEV)
    st = _lib.fn("hnm_segpop_fit_f64")(_lib.ctx(DEV), _lib.ptr(it), _lib.ptr(us), it.numel(),
                                       _lib.ptr(sg), sg.numel(), _lib.ptr(dd), _lib.ptr(ww),
                                       num_items, S, D, slab, _lib.ptr(count), _lib.ptr(pop))
    return st, count, pop


@pytest.mark.parametrize("n", [0, 1, 20_000])
@pytest.mark.parametrize("slab", [0, 8])
@pytest.mark.parametrize("with_days", [False, True])
@pytest.mark.parametrize("decay", [0.0, 0.02])
@pytest.mark.parametrize("S", [1, 3])
def test_fit_is_bitwise_the_oracle_and_the_baseline(S, decay, with_days, slab, n):
    items, users = ITEMS[:n], USERS[:n]
    days = DAYS[:n] if with_days else None
    useg = user_segments(S)
    assert 0.03 < (useg < 0).mean() < 0.25 and set(useg.tolist()) == set(range(-1, S))
    if with_days:
        D = int(days.max()) + 1 if n else 1
        w = np.exp(-decay * np.arange(D))
    else:
        D, w = 1, np.ones(1)
    if n == 20_000 and with_days:
        assert D == 90 and (slab == 0 or -(-D // slab) == 12)     # slab = 8: 12 ascending slabs
    ref_count, ref_pop, skipped = SO.fit(items, users, useg, days, w, I, S, D)
    assert skipped == 0
    for min_count in (1, 3):
        m = SegmentPopularity(I, S, time_decay=decay, min_count=min_count).to(DEV)
        m.fit_interactions(items, users, useg, days_ago=days, _slab=slab)
        assert m.count.shape == (S + 1, I) and m.count.dtype == torch.int64
        assert np.array_equal(m.count.cpu().numpy(), ref_count)
        assert np.array_equal(bits(m.pop), ref_pop.view(np.int64))
        ol, vl, rank = SO.orders(ref_count, ref_pop, min_count)
        ptr = m.order_ptr.cpu().numpy()
        assert ptr.tolist() == np.concatenate([[0], np.cumsum([len(o) for o in ol])]).tolist()
        order, val = m.order.cpu().numpy(), m.order_val.cpu().numpy()
        for s in range(S + 1):
            assert np.array_equal(order[ptr[s]:ptr[s + 1]], ol[s]), (s, min_count)
            assert np.array_equal(bits(val[ptr[s]:ptr[s + 1]]), bits(vl[s])), (s, min_count)
        assert m.rank.dtype == torch.int32 and np.array_equal(m.rank.cpu().numpy(), rank)
    # row S is the existing baseline, bit for bit; so is global_baseline()
    base = PopularityBaseline(I, time_decay=decay).to(DEV)
    base.fit_interactions(items, days_ago=days, _slab=slab)
    assert torch.equal(m.count[S], base.count)
    assert np.array_equal(bits(m.pop[S]), bits(base.pop))
    gb = m.global_baseline()
    for name in ("count", "pop", "order", "order_val", "rank"):
        a, b = getattr(gb, name), getattr(base, name)
        assert a.dtype == b.dtype and torch.equal(a, b), name
    # the segment rows and the transactions of the users without a segment add up to row S
    unknown = np.bincount(items[useg[users] < 0], minlength=I)
    assert np.array_equal(ref_count[:S].sum(0) + unknown, ref_count[S])
    assert np.array_equal(m.count[:S].sum(0).cpu().numpy() + unknown, m.count[S].cpu().numpy())
    sizes = np.bincount(useg[useg >= 0], minlength=S)
    assert m.segment_sizes.cpu().tolist() == sizes.tolist()
    assert torch.equal(m.user_segment.cpu(), torch.from_numpy(useg))


def test_one_segment_holding_every_user_equals_the_global_row():
    w = np.exp(-0.02 * np.arange(90))
    st, count, pop = raw_fit(ITEMS, USERS, np.zeros(U, np.int32), DAYS, w, I, 1, 90)
    assert st == _lib.HNM_OK and ctx_check() == _lib.HNM_OK
    assert torch.equal(count[0], count[1]) and np.array_equal(bits(pop[0]), bits(pop[1]))
    assert int(count[1].sum()) == len(ITEMS)


def test_fit_same_bits_on_every_run_and_slab():
    useg = user_segments(3)
    w = np.exp(-0.02 * np.arange(90))
    a = raw_fit(ITEMS, USERS, useg, DAYS, w, I, 3, 90)
    b = raw_fit(ITEMS, USERS, useg, DAYS, w, I, 3, 90)
    c = raw_fit(ITEMS, USERS, useg, DAYS, w, I, 3, 90, slab=8)
    d = raw_fit(ITEMS, USERS, useg, DAYS, w, I, 3, 90, slab=1)
    assert a[0] == b[0] == c[0] == d[0] == _lib.HNM_OK
    for x in (b, c, d):
        assert torch.equal(a[1], x[1]) and np.array_equal(bits(a[2]), bits(x[2]))
    assert ctx_check() == _lib.HNM_OK
    # NULL day weights: all 1.0 (the windowed count); days past the window are ignored
    st, count, pop = raw_fit(ITEMS, USERS, useg, DAYS, None, I, 3, 30)
    rc, rp, _ = SO.fit(ITEMS, USERS, useg, DAYS, np.ones(30), I, 3, 30)
    assert st == _lib.HNM_OK and np.array_equal(count.cpu().numpy(), rc)
    assert np.array_equal(bits(pop), rp.view(np.int64)) and rc[3].sum() == (DAYS < 30).sum()


def test_fit_out_of_range_ids_and_bad_arguments():
    S = 3
    w = np.exp(-0.02 * np.arange(90))
    items, users, days = ITEMS[:500].copy(), USERS[:500].copy(), DAYS[:500]
    useg = user_segments(S)
    cases = []
    bad_seg = useg.copy()
    bad_seg[users[11]] = S                                           # a segment of S
    cases.append((items, users, bad_seg, int((users == users[11]).sum())))
    bad_users = users.copy()
    bad_users[[3, 77]] = [U, -1]                                     # a user id of num_users
    cases.append((items, bad_users, useg, 2))
    bad_items = items.copy()
    bad_items[[5, 400]] = [I, -1]                                    # an item of I
    cases.append((bad_items, users, useg, 2))
    for it, us, sg, n_bad in cases:
        st, count, pop = raw_fit(it, us, sg, days, w, I, S, 90)
        assert st == _lib.HNM_OK
        assert ctx_check() == _lib.HNM_EOOB
        assert ctx_check() == _lib.HNM_OK                            # the word was cleared
        rc, rp, skipped = SO.fit(it, us, sg, days, w, I, S, 90)      # skips them entirely
        assert skipped == n_bad and rc[S].sum() == 500 - n_bad
        assert np.array_equal(count.cpu().numpy(), rc)
        assert np.array_equal(bits(pop), rp.view(np.int64))
        m = SegmentPopularity(I, S).to(DEV)
        with pytest.raises(IndexError):
            m.fit_interactions(it, us, sg)
    # a bad id is reported whatever its row's day: outside the window, and with several slabs
    late = int(np.nonzero(days >= 30)[0][0])
    for it, us in ((np.where(np.arange(500) == late, I, items), users),
                   (items, np.where(np.arange(500) == late, U, users))):
        st, count, pop = raw_fit(it, us, useg, days, w[:30], I, S, 30, slab=8)
        assert st == _lib.HNM_OK and ctx_check() == _lib.HNM_EOOB and ctx_check() == _lib.HNM_OK
        rc, rp, skipped = SO.fit(it, us, useg, days, w[:30], I, S, 30)
        assert skipped == 1 and np.array_equal(count.cpu().numpy(), rc)
        assert np.array_equal(bits(pop), rp.view(np.int64))
    assert raw_fit(items, users, useg, days, w, I, 0, 90)[0] == _lib.HNM_EINVAL
    assert raw_fit(items, users, useg, days, w, I, -1, 90)[0] == _lib.HNM_EINVAL
    big = np.ones(65_537)
    assert raw_fit(items[:10], users[:10], useg, days[:10], big, I, S, 65_537)[0] == \
        _lib.HNM_EUNSUPPORTED
    assert raw_fit(items[:10], users[:10], np.zeros(U, np.int32), days[:10], big[:-1], I, 1,
                   65_536)[0] == _lib.HNM_OK
    # one day's [S + 1, I] int32 table above the 256 MiB cap: refused before any allocation
    S_big = (256 << 20) // (I * 4)
    st = _lib.fn("hnm_segpop_fit_f64")(_lib.ctx(DEV), None, None, 0, _lib.ptr(dev(useg, np.int32)),
                                       U, None, None, I, S_big, 1, 0, _lib.ptr(dev([0], np.int64)),
                                       _lib.ptr(dev([0], np.float64)))
    assert st == _lib.HNM_EUNSUPPORTED
    assert ctx_check() == _lib.HNM_OK


# ------------------------------------------------------------------ top-K
NUM_ITEMS, R_GLOBAL, S_TOPK = 400, 330, 3


class Catalogue:
    """Installed orders: a global order of 330 of 400 items, and segment orders of 0, 5 and 200
    items as other permutations.  Segment 1's five items are the global ranks 0..4 (reversed:
    phase 2 has to skip exactly what phase 1 emitted); segment 2 mixes ranked and globally
    unranked items."""

    def __init__(self, seed=5, global_len=R_GLOBAL):
        rng = np.random.Generator(np.random.PCG64(seed))
        glob = rng.permutation(NUM_ITEMS)[:R_GLOBAL].astype(np.int64)
        self.unranked = np.setdiff1d(np.arange(NUM_ITEMS), glob)
        seg2 = rng.permutation(NUM_ITEMS)[:200].astype(np.int64)
        assert np.isin(seg2, self.unranked).any() and np.isin(seg2, glob).any()
        self.orders = [np.zeros(0, np.int64), glob[:5][::-1].copy(), seg2, glob[:global_len]]
        self.vals = [np.sort(rng.random(len(o)).astype(np.float32))[::-1].copy()
                     for o in self.orders]
        self.ptr = np.concatenate([[0], np.cumsum([len(o) for o in self.orders])])
        self.rank = np.full((S_TOPK + 1, NUM_ITEMS), -1, np.int32)
        for s, o in enumerate(self.orders):
            self.rank[s, o] = np.arange(len(o))
        self._dev = None

    @property
    def dev(self):
        """(order, order_val, order_ptr, rank) on the device, uploaded on first use."""
        if self._dev is None:
            self._dev = (dev(np.concatenate(self.orders), np.int64),
                         dev(np.concatenate(self.vals), np.float32), dev(self.ptr, np.int64),
                         dev(self.rank, np.int32))
        return self._dev

    def history(self, s, L):
        """L entries: the head of the row's segment order (up to half), then the head of the
        global order; ranks 2 and 7 swapped for globally unranked ids, two duplicates, and the
        whole list reversed (the raw ABI promises no sorting)."""
        seg = self.orders[s] if s >= 0 else self.orders[S_TOPK][:0]
        h = seg[:min(len(seg), L // 2)].tolist()
        have = set(h)
        h += [x for x in self.orders[S_TOPK].tolist() if x not in have][:L - len(h)]
        for j, pos in enumerate((2, 7)):
            if pos < L:
                h[pos] = int(self.unranked[j])
        if L >= 12:
            h[10], h[11] = h[0], h[1]
        assert len(h) == L
        return h[::-1]


CAT = Catalogue()
LENGTHS = (0, 1, 63, 64, 65, 300)
WAVE_SEGS = [s for s in (-1, 0, 1, 2) for _ in LENGTHS]
WAVE_ROWS = [CAT.history(s, L) for s in (-1, 0, 1, 2) for L in LENGTHS]
_oracle = {}


def oracle(k):
    """The wave rows' expected result, computed once per k and shared by every chunk."""
    if k not in _oracle:
        _oracle[k] = SO.topk(CAT.orders, CAT.vals, WAVE_SEGS, WAVE_ROWS, k)
    return _oracle[k]


def raw_topk(segs, rows, k, chunk=0, B=None, cat=None):
    """The raw ABI with an unsorted, possibly duplicated CSR built from `rows` (None: NULL)."""
    o, v, p, r = (cat or CAT).dev
    B = len(segs) if B is None else B
    sg = None if segs is None else dev(segs if len(segs) else [0], np.int32)
    mp = mi = None
    if rows is not None:
        mp = dev(np.concatenate([[0], np.cumsum([len(x) for x in rows])]), np.int64)
        flat = [x for row in rows for x in row]
        mi = dev(flat if flat else [0], np.int32)
    out_v = torch.full((B, k), 123.0, dtype=torch.float32, device=DEV)
    out_i = torch.full((B, k), 123, dtype=torch.int64, device=DEV)
    out_n = torch.full((B,), 123, dtype=torch.int32, device=DEV)
    st = _lib.fn("hnm_segpop_topk_f32")(_lib.ctx(DEV), _lib.ptr(o), _lib.ptr(v), _lib.ptr(p),
                                        _lib.ptr(r), NUM_ITEMS, S_TOPK, _lib.ptr(sg), _lib.ptr(mp),
                                        _lib.ptr(mi), B, k, chunk, _lib.ptr(out_v),
                                        _lib.ptr(out_i), _lib.ptr(out_n))
    return st, out_v, out_i, out_n


def assert_rows(got, want):
    (st, ov, oi, on), (rv, ri, rn) = got, want
    assert st == _lib.HNM_OK
    assert np.array_equal(oi.cpu().numpy(), ri)
    assert np.array_equal(bits(ov), rv.view(np.int32))
    assert np.array_equal(on.cpu().numpy(), rn)


@pytest.mark.parametrize("chunk", [0, 64, 128])
@pytest.mark.parametrize("k", [0, 1, 12, 100, 330])
def test_topk_equals_the_two_phase_restatement(k, chunk):
    got = raw_topk(WAVE_SEGS, WAVE_ROWS, k, chunk)
    if k == 0:
        assert got[0] == _lib.HNM_OK and got[1].shape == (24, 0) and not got[3].any()
        return
    want = oracle(k)
    assert_rows(got, want)
    assert ctx_check() == _lib.HNM_OK
    rv, ri, rn = want
    rows = {(s, L): b for b, (s, L) in enumerate((s, L) for s in (-1, 0, 1, 2) for L in LENGTHS)}
    assert not rn[:12].any()                              # no segment, and the empty segment
    assert rn[rows[(1, 0)]] == min(k, 5) and rn[rows[(1, 1)]] == min(k, 4)
    for L in (63, 64, 65, 300):                           # the history holds segment 1's order
        assert rn[rows[(1, L)]] == 1                      # but for rank 2, swapped out of it
    assert rn[rows[(2, 0)]] == min(k, 200)                # k <= 200: phase 1 fills the row
    if k == 12:
        b = rows[(1, 0)]                                  # the seam: 5 segment items, then the
        assert ri[b, :5].tolist() == CAT.orders[1].tolist()          # global ranks 5..11
        assert ri[b, 5:].tolist() == CAT.orders[3][5:12].tolist()
    if k == 330:
        assert (ri[rows[(-1, 0)]] >= 0).all()
        # segment 2 with nothing filtered: its 200 items, then the 330 global ones it lacks
        b = rows[(2, 0)]
        assert rn[b] == 200 and len(set(ri[b].tolist())) == 330
        n_union = len(set(CAT.orders[2].tolist()) | set(CAT.orders[3].tolist()))
        assert (ri[b] >= 0).sum() == min(330, n_union)


def test_topk_is_the_same_for_every_chunk_and_rejects_a_bad_one():
    """chunk = 64 with a 300-item history: the 312-rank window takes 5 passes in each phase,
    carrying the emitted count through both; the result is that of the single default pass."""
    assert -(-min(R_GLOBAL, 12 + 300) // 64) >= 5
    for k in (12, 100):
        a = raw_topk(WAVE_SEGS, WAVE_ROWS, k, chunk=64)
        for chunk in (0, 128, 8192):
            x = raw_topk(WAVE_SEGS, WAVE_ROWS, k, chunk=chunk)
            assert x[0] == _lib.HNM_OK and torch.equal(a[2], x[2]) and torch.equal(a[3], x[3])
            assert np.array_equal(bits(a[1]), bits(x[1]))
    for chunk in (100, 32, 8256, -64):
        assert raw_topk(WAVE_SEGS, WAVE_ROWS, 12, chunk=chunk)[0] == _lib.HNM_EINVAL
    assert ctx_check() == _lib.HNM_OK


def test_topk_batch_sizes_null_mask_and_empty_orders():
    rng = np.random.Generator(np.random.PCG64(9))
    segs65 = rng.integers(-1, S_TOPK, size=65).tolist()
    rows65 = [rng.integers(0, NUM_ITEMS, size=int(rng.integers(0, 81))).tolist()
              for _ in range(65)]
    assert_rows(raw_topk(segs65, rows65, 12), SO.topk(CAT.orders, CAT.vals, segs65, rows65, 12))
    assert_rows(raw_topk(segs65[:1], rows65[:1], 12),
                SO.topk(CAT.orders, CAT.vals, segs65[:1], rows65[:1], 12))
    st, ov, oi, on = raw_topk([], [], 12, B=0)
    assert st == _lib.HNM_OK and ov.shape == (0, 12)
    # NULL mask: the heads of the two orders; a CSR of empty rows gives the same
    segs = [-1, 0, 1, 2, 2]
    want = SO.topk(CAT.orders, CAT.vals, segs, [[]] * 5, 12)
    assert_rows(raw_topk(segs, None, 12), want)
    assert_rows(raw_topk(segs, [[] for _ in segs], 12), want)
    # a history that covers the row's whole segment order: no segment part, and the global
    # list without it
    full = [CAT.orders[1].tolist(), CAT.orders[2].tolist()[::-1]]
    got = raw_topk([1, 2], full, 12)
    assert_rows(got, SO.topk(CAT.orders, CAT.vals, [1, 2], full, 12))
    assert got[3].cpu().tolist() == [0, 0] and got[2][0].cpu().tolist() == CAT.orders[3][5:17].tolist()
    # a global order of no items: a segment row still gets its own list, the others nothing
    empty = Catalogue(global_len=0)
    assert len(empty.orders[S_TOPK]) == 0 and (empty.rank[S_TOPK] == -1).all()
    rows = [[], [int(empty.orders[1][0])], [int(empty.orders[1][0])], []]
    segs = [-1, 0, 1, 2]
    got = raw_topk(segs, rows, 12, cat=empty)
    assert_rows(got, SO.topk(empty.orders, empty.vals, segs, rows, 12))
    assert got[3].cpu().tolist() == [0, 0, 4, 12] and (got[2][:2] == -1).all()
    assert ctx_check() == _lib.HNM_OK


def test_topk_out_of_range_segment_and_mask_id():
    # seg = S: flagged, and the row is answered as a row without a segment
    rows = [CAT.history(2, 65), CAT.history(1, 1), []]
    got = raw_topk([S_TOPK, 1, S_TOPK + 40], rows, 12)
    assert ctx_check() == _lib.HNM_EOOB
    assert ctx_check() == _lib.HNM_OK
    assert_rows(got, SO.topk(CAT.orders, CAT.vals, [-1, 1, -1], rows, 12))
    # a mask id outside [0, num_items): flagged (once: the word is one bit), skipped, and
    # counted in neither phase -- the rows are those of the history without it
    for bad in (NUM_ITEMS, -3):
        for chunk in (0, 64):
            rows = [CAT.history(1, 65) + [bad], [bad] + CAT.history(2, 300), [bad], []]
            segs = [1, 2, -1, 0]
            got = raw_topk(segs, rows, 100, chunk)
            assert ctx_check() == _lib.HNM_EOOB
            assert ctx_check() == _lib.HNM_OK
            clean = [[x for x in r if x != bad] for r in rows]
            assert_rows(got, SO.topk(CAT.orders, CAT.vals, segs, clean, 100))


def test_topk_without_segments_is_the_baseline_kernel():
    """Every row at segment -1 (or seg == NULL): bitwise hnm_popularity_topk_f32 over the
    global order with the same mask."""
    o, v, p, r = CAT.dev
    rows = [CAT.history(-1, L) for L in LENGTHS] + [CAT.history(2, 65)]
    B = len(rows)
    mp = dev(np.concatenate([[0], np.cumsum([len(x) for x in rows])]), np.int64)
    mi = dev([x for row in rows for x in row], np.int32)
    g0 = int(CAT.ptr[S_TOPK])
    for k in (12, 330):
        for chunk in (0, 64):
            bv = torch.empty(B, k, dtype=torch.float32, device=DEV)
            bi = torch.empty(B, k, dtype=torch.int64, device=DEV)
            st = _lib.fn("hnm_popularity_topk_f32")(
                _lib.ctx(DEV), _lib.ptr(o[g0:]), _lib.ptr(v[g0:]), R_GLOBAL,
                _lib.ptr(r[S_TOPK]), NUM_ITEMS, _lib.ptr(mp), _lib.ptr(mi), B, k, chunk,
                _lib.ptr(bv), _lib.ptr(bi))
            assert st == _lib.HNM_OK
            for segs in ([-1] * B, [-5] * B, None):
                st, ov, oi, on = raw_topk(segs, rows, k, chunk, B=B)
                assert st == _lib.HNM_OK and torch.equal(oi, bi) and not on.any()
                assert np.array_equal(bits(ov), bits(bv))
    assert ctx_check() == _lib.HNM_OK


# ------------------------------------------------------------------ module, ensemble, serving
class World:
    """One fit on the golden transactions (S = 3, decayed), its oracle tables, the users'
    histories; built once."""

    S = 3

    def __init__(self):
        self.useg = user_segments(self.S)
        D = int(DAYS.max()) + 1
        count, pop, _ = SO.fit(ITEMS, USERS, self.useg, DAYS, np.exp(-0.02 * np.arange(D)), I,
                               self.S, D)
        self.orders, self.vals, _ = SO.orders(count, pop, 2)
        self.model = SegmentPopularity(I, self.S, time_decay=0.02, min_count=2).to(DEV)
        self.model.fit_interactions(ITEMS, USERS, self.useg, days_ago=DAYS)
        self.h = {int(u): set(ITEMS[USERS == u].tolist()) for u in np.unique(USERS)}
        self.hist = UserHistory(self.h, U, I, DEV)
        self.heavy, self.nohist = int(G["heavy"]), int(G["nohist"])

    def seg_of(self, users):
        return [int(self.useg[u]) if 0 <= u < U else -1 for u in users]

    def want(self, segs, rows, k):
        return SO.topk(self.orders, self.vals, segs, rows, k)


_world = []


@pytest.fixture
def world():
    if not _world:
        _world.append(World())
    return _world[0]


def assert_lists(got, want):
    assert np.array_equal(got[1].cpu().numpy(), want[1])
    assert np.array_equal(bits(got[0]), want[0].view(np.int32))
    if len(got) > 2:
        assert np.array_equal(got[2].cpu().numpy(), want[2])


def test_module_answers_equal_the_oracle(world):
    m = world.model
    users = np.concatenate([G["batch"], G["batch"][:3], [world.heavy, world.nohist]])
    segs = world.seg_of(users)
    assert {-1, 0, 1, 2} <= set(world.seg_of(range(U)))
    rows = [world.h.get(int(u), ()) for u in users]
    a = m.recommend_with_scores(torch.from_numpy(users), filter_items=world.h, k=12)
    b = m.recommend_with_scores(torch.from_numpy(users).to(DEV), filter_items=world.hist, k=12)
    assert torch.equal(a[1], b[1]) and np.array_equal(bits(a[0]), bits(b[0]))
    assert_lists(a, world.want(segs, rows, 12))
    for chunk in (64, 128):
        c = m.recommend_with_scores(torch.from_numpy(users), filter_items=world.h, k=12,
                                    _chunk=chunk)
        assert torch.equal(a[1], c[1]) and np.array_equal(bits(a[0]), bits(c[0]))
    # ids past the segment table: users without a segment (the global list)
    far = np.array([U, U + 5, 10 ** 6, 3])
    got = m.recommend_with_scores(torch.from_numpy(far), filter_items={U + 5: {1, 2, 3}}, k=12)
    assert_lists(got, world.want(world.seg_of(far), [(), (1, 2, 3), (), ()], 12))
    assert torch.equal(got[1][0], got[1][2])
    # unfiltered, forward, recommend; k clamped to num_items; k = 0
    assert_lists(m.recommend_with_scores(torch.from_numpy(users), k=5),
                 world.want(segs, [()] * len(users), 5))
    top = world.want(segs, [()] * len(users), 12)[1]
    assert m.forward(torch.from_numpy(users)).cpu().tolist() == top.tolist()
    assert m(torch.from_numpy(users).to(DEV)).dtype == torch.int64
    rec = m.recommend(users[:6].tolist(), k=12)
    assert [rec[int(u)] for u in users[:6]] == [[x for x in r if x >= 0] for r in top[:6].tolist()]
    v, i = m.recommend_with_scores(torch.from_numpy(users), k=I + 50)
    assert i.shape == (len(users), I) and (i[:, len(world.orders[world.S]):] == -1).all()
    assert m.recommend_with_scores(torch.from_numpy(users), k=0)[1].shape == (len(users), 0)
    assert m.state_dict() == {}


def test_recommend_for_segments(world):
    m = world.model
    segs = [0, None, 2, -1, 1, 2, 0]
    rows = [(), (), tuple(world.orders[2][:9].tolist()), tuple(world.orders[3][:4].tolist()),
            tuple(world.orders[1].tolist()), (), tuple(world.orders[0][:40].tolist())]
    filt = {j: set(r) for j, r in enumerate(rows) if r}
    num = [-1 if s is None else s for s in segs]
    for k in (12, 100):
        got = m.recommend_for_segments(segs, filter_items=filt, k=k, return_nseg=True)
        assert len(got) == 3 and got[2].dtype == torch.int32
        want = world.want(num, rows, k)
        assert_lists(got, want)
        two = m.recommend_for_segments(torch.tensor(num), filter_items=filt, k=k)
        assert len(two) == 2 and torch.equal(two[1], got[1])
    assert want[2][4] == 0 and want[2][1] == 0 and want[2][0] > 0       # the seam positions
    v, i, n = m.recommend_for_segments([], k=12, return_nseg=True)
    assert i.shape == (0, 12) and n.shape == (0,)
    with pytest.raises(ValueError):
        m.recommend_for_segments([world.S])


def test_ensemble_member_equals_the_fuse_oracle(world):
    m, g = world.model, world.model.global_baseline()
    e = Ensemble([("segment_popularity", m), ("popularity_baseline", g)], mode="rrf")
    k = 12
    depth = e._depth(k)
    users = np.concatenate([G["batch"], [world.heavy, world.nohist, U + 3]])
    ids = torch.from_numpy(users)
    lists = [x.recommend_with_scores(ids, world.h, k=depth) for x in (m, g)]
    got = e.recommend_with_scores(ids, filter_items=world.h, k=k)
    vals = np.stack([v.cpu().numpy() for v, _ in lists])
    idxs = np.stack([i.cpu().numpy() for _, i in lists])
    rows, oob = FO.fuse_full(vals, idxs, FO.RANK, e.rank_weights(depth).numpy(), I)
    assert not oob
    sets = [sorted(world.h.get(int(u), ())) for u in users]
    ptr = np.concatenate([[0], np.cumsum([len(s) for s in sets])])
    idx = np.asarray([x for s in sets for x in s], np.int64)
    wv, wi, _ = FO.cut(rows, k, ptr, idx)
    assert np.array_equal(got[1].cpu().numpy(), wi)
    assert np.array_equal(bits(got[0]), wv.view(np.int32))
    assert (got[1] >= 0).all()


def test_lightning_eval_hooks(world):
    m = world.model
    users = G["batch"]
    top = m.forward(torch.from_numpy(users)).cpu().numpy()
    truth = np.full((len(users), 3), -1, np.int64)
    truth[:, 0] = top[:, 2]
    truth[::2, 1] = top[::2, 7]
    m.validation_step({"user_ids": torch.from_numpy(users).to(DEV),
                       "ground_truth": torch.from_numpy(truth).to(DEV)}, 0)
    m.on_validation_epoch_end()
    ref = evaluate_recommendations({int(u): top[r].tolist() for r, u in enumerate(users)},
                                   {int(u): [int(x) for x in truth[r] if x >= 0]
                                    for r, u in enumerate(users)}, k=12, device=DEV)
    assert float(m.logged_metrics["val_map_at_k"]) == pytest.approx(float(ref["map@12"]),
                                                                     rel=2.0 ** -23)
    assert float(m.logged_metrics["val_map_at_k"]) > 0 and m.metrics._n_all == 0


def test_serving_cold_start_segment(world, monkeypatch):
    srv = Recommender(U, I, models={"neural_cf": NeuralCF(U, I)}, user_history=world.h,
                      device=DEV, cold_start="segment")
    with pytest.raises(ValueError, match="add_segment_popularity"):
        srv.get_batch_recommendations([1, 10 ** 6])
    sp = srv.add_segment_popularity(ITEMS, USERS, world.useg, world.S, days_ago=DAYS,
                                    time_decay=0.02, min_count=2)
    assert isinstance(sp, SegmentPopularity) and srv.models["segment_popularity"] is sp
    assert torch.equal(sp.order, world.model.order) and sp.top_k == 100
    assert srv._get_best_model() == "neural_cf"
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    ask = [world.heavy, 10 ** 6, 7, "nobody", 10 ** 6 + 1, "x", world.nohist]
    segments = [2, 2, None, 0, None, -1, 1]               # known users' entries are not read
    out = srv.get_batch_recommendations(ask, model_name="segment_popularity", num_items=12,
                                        include_scores=True, segments=segments)
    assert calls.count("hnm_segpop_topk_f32") == 2          # the known users, the unknown ones
    known = [world.heavy, 7, world.nohist]
    kv, ki, _ = world.want(world.seg_of(known), [world.h.get(u, ()) for u in known], 12)
    cv, ci, _ = world.want([2, 0, -1, -1], [()] * 4, 12)
    for (rv, ri), slots in (((kv, ki), (0, 2, 6)), ((cv, ci), (1, 3, 4, 5))):
        for r, j in enumerate(slots):
            assert out[j]["model_name"] == "segment_popularity" and out[j]["user_id"] == ask[j]
            n = int((ri[r] >= 0).sum())
            assert n == 12
            assert [x["article_id"] for x in out[j]["recommendations"]] == [str(i) for i in ri[r]]
            assert [x["score"] for x in out[j]["recommendations"]] == rv[r].tolist()
    assert [x["article_id"] for x in out[4]["recommendations"]] == \
        [str(i) for i in world.orders[world.S][:12]]
    # another model for the known users: the unknown ones still come from the segment model,
    # all of them from one kernel call
    del calls[:]
    got = srv.get_batch_recommendations(ask, model_name="neural_cf", num_items=12, segments=segments)
    assert calls.count("hnm_segpop_topk_f32") == 1
    for j in (0, 2, 6):
        assert got[j]["model_name"] == "neural_cf" and len(got[j]["recommendations"]) == 12
    for r, j in enumerate((1, 3, 4, 5)):
        assert got[j]["model_name"] == "segment_popularity"
        assert [x["article_id"] for x in got[j]["recommendations"]] == [str(i) for i in ci[r]]
    one = srv.get_recommendations("nobody", num_items=3, include_scores=True, segment=0)
    assert one["model_name"] == "segment_popularity" and one["user_id"] == "nobody"
    assert [x["score"] for x in one["recommendations"]] == cv[1][:3].tolist()
    none = srv.get_recommendations(10 ** 6, num_items=12)
    assert [x["article_id"] for x in none["recommendations"]] == [str(i) for i in ci[2]]
    with pytest.raises(ValueError, match="segment"):
        srv.get_recommendations("nobody", segment=world.S)
    with pytest.raises(ValueError, match="segment"):
        srv.get_batch_recommendations(ask, segments=[None] * 6 + [-2])
    # an ensemble of registered models takes it as a member, unchanged
    srv.add_item_cf(USERS, ITEMS, num_neighbors=4)
    srv.add_popularity_baseline(ITEMS, days_ago=DAYS, time_decay=0.02)
    e = srv.add_ensemble(["item_cf", "segment_popularity"])
    res = srv.get_recommendations(7, model_name="ensemble", num_items=12)
    assert res["model_name"] == "ensemble" and len(res["recommendations"]) == 12
    wv, wi = e.recommend_with_scores(torch.tensor([7]), filter_items=srv._device_history(), k=12)
    assert [x["article_id"] for x in res["recommendations"]] == [str(i) for i in wi[0].tolist()]


def test_serving_cold_start_popularity_is_unchanged(world):
    """The same recommender class with cold_start="popularity": today's answer, whether or not a
    segment model is registered."""
    cold = Recommender(U, I, models={"neural_cf": NeuralCF(U, I)}, user_history=world.h,
                       device=DEV, cold_start="popularity")
    base = cold.add_popularity_baseline(ITEMS, days_ago=DAYS, time_decay=0.02)
    cold.add_segment_popularity(ITEMS, USERS, world.useg, world.S, days_ago=DAYS, time_decay=0.02)
    order, val = base.order.cpu().numpy(), base.order_val.cpu().numpy()
    ask = [world.heavy, 10 ** 6, 7, world.nohist, "nobody"]
    got = cold.get_batch_recommendations(ask, model_name="neural_cf", num_items=12)
    for j in (1, 4):
        assert got[j]["model_name"] == "popularity_baseline" and got[j]["user_id"] == ask[j]
        assert [x["article_id"] for x in got[j]["recommendations"]] == [str(i) for i in order[:12]]
    for j in (0, 2, 3):
        assert got[j]["model_name"] == "neural_cf" and len(got[j]["recommendations"]) == 12
    single = cold.get_recommendations("nobody", num_items=3, include_scores=True)
    assert single["model_name"] == "popularity_baseline"
    assert [x["score"] for x in single["recommendations"]] == val[:3].tolist()
    with pytest.raises(ValueError, match='cold_start="segment"'):
        cold.get_recommendations("nobody", segment=1)
    err = Recommender(U, I, models={"neural_cf": NeuralCF(U, I)}, device=DEV)
    assert err.get_batch_recommendations([10 ** 6])[0] == {"user_id": 10 ** 6,
                                                           "error": "user 1000000 not found"}
