"""GPU: the weighted ItemCF -- hnm_itemcf_fit_weighted_f32 / hnm_itemcf_scores_weighted_f32 /
hnm_itemcf_topk_weighted_f32, `WeightedItemCF`, weighted baskets and the `Recommender`.

Everything is compared BITWISE against the numpy restatement of the contract (include/hnm.h) in
itemcf_oracle.py (the weighted fit and scores; the top-K is the plain selection, here from the
fused route and from the dense one).

The shapes are test_gpu_itemcf.py's with a few hand-made users and items after the synthetic
ones (exact ties, an item whose weights are all zero, the bulk buyer).
"""
import functools

import numpy as np
import pytest
import torch

from hnm_recommendation_amd import ItemCF, UserHistory, WeightedItemCF, _lib
from hnm_recommendation_amd import synthetic as syn
from hnm_recommendation_amd.serving import Recommender, create_model_from_checkpoint
from itemcf_gpu import (BE, BI, BN, BU, DEV, I_X, NI, NU, U_81, U_82, U_BULK, U_EMPTY, U_HELPER,
                        U_ONE, assert_fit_equal, bits, filters, host_back_fill)
from itemcf_oracle import NEG_INF, np_csr, np_fit_w, np_scores_w, np_topk

pytestmark = pytest.mark.gpu


def pair_weights(n, seed):
    """count * exp(-0.01 days) per pair, a fifth of them zero."""
    rng = np.random.default_rng(seed)
    w = (rng.integers(1, 9, n) * np.exp(-0.01 * rng.integers(0, 366, n))).astype(np.float32)
    w[rng.random(n) < 0.2] = 0
    return w


def history(ptr, idx, w, U, I):
    """A UserHistory whose hist_w is exactly w (one transaction per pair)."""
    rows = np.repeat(np.arange(U, dtype=np.int64), np.diff(ptr))
    h = UserHistory.from_interactions(rows, idx.astype(np.int64), U, I, DEV, weights=w)
    assert np.array_equal(h.hist_ptr.cpu().numpy(), ptr)
    assert np.array_equal(h.hist_idx.cpu().numpy()[:len(idx)], idx)
    assert np.array_equal(bits(h.hist_w[:len(idx)]), bits(np.asarray(w, np.float32)))
    return h


def fit_w(hist, N, shrink=0.0, max_history=0, window=0):
    m = WeightedItemCF(hist.num_users, hist.num_items, num_neighbors=N, shrink=shrink,
                       max_history=max_history).to(DEV)
    return m.fit_history(hist, _window=window)


def fit_plain(hist, N, shrink=0.0, max_history=0, window=0):
    m = ItemCF(hist.num_users, hist.num_items, num_neighbors=N, shrink=shrink,
               max_history=max_history).to(DEV)
    return m.fit_history(hist, _window=window)


def assert_same_table(a, b):
    assert torch.equal(a.neighbor_idx, b.neighbor_idx)
    assert np.array_equal(bits(a.neighbor_val), bits(b.neighbor_val))
    assert torch.equal(a.item_count, b.item_count)


# ------------------------------------------------------------------ fit
S1 = (600, 300, 6000)
S2 = (300, 3000, 4000)
# S1 plus two hand-made users and 22 hand-made items: U_TIE holds I_T and 20 more items at one
# weight (20 exactly equal similarities in row I_T: the cut at N = 16 falls inside the tie, j
# ascending decides); U_ZERO holds I_Z at weight 0 and nothing else does (item_count 0).
U1, I1 = S1[0] + 2, S1[1] + 22
U_TIE, U_ZERO = S1[0], S1[0] + 1
I_T, I_Z = S1[1], S1[1] + 21


@functools.lru_cache(maxsize=None)
def small1():
    users, items = syn.interactions(*S1, seed=2)
    users = np.concatenate([users, np.full(21, U_TIE, np.int64), [U_ZERO, U_ZERO]])
    items = np.concatenate([items, np.arange(I_T, I_T + 21), [I_Z, 3]])
    ptr, idx = np_csr(users, items, U1, I1)
    w = pair_weights(len(idx), seed=1)
    w[ptr[U_TIE]:ptr[U_TIE + 1]] = np.float32(2.5)
    zero_at = ptr[U_ZERO] + np.nonzero(idx[ptr[U_ZERO]:ptr[U_ZERO + 1]] == I_Z)[0][0]
    w[zero_at] = 0
    assert (w == 0).mean() > 0.15 and w.max() > 7
    return ptr, idx, w, history(ptr, idx, w, U1, I1)


@functools.lru_cache(maxsize=None)
def small1_ref(N, shrink):
    ptr, idx, w, _ = small1()
    return np_fit_w(ptr, idx, w, U1, I1, N, shrink)


@functools.lru_cache(maxsize=None)
def small2():
    users, items = syn.interactions(*S2, seed=2)
    U, I, _ = S2
    ptr, idx = np_csr(users, items, U, I)
    w = pair_weights(len(idx), seed=3)
    return ptr, idx, w, history(ptr, idx, w, U, I), np_fit_w(ptr, idx, w, U, I, 8)


@pytest.mark.parametrize("shrink", [0.0, 10.0])
@pytest.mark.parametrize("N", [1, 16, 64])
def test_weighted_fit_is_bitwise_the_numpy_restatement(N, shrink):
    ptr, idx, w, hist = small1()
    ref = small1_ref(N, shrink)
    ridx, rval, rn, sim, C = ref
    if N == 16:
        # what the pass relies on: a tie exactly at the N-th place, rows shorter than N, an item
        # whose weights are all zero, and a table that is not the unweighted one
        npos = (C > 0).sum(1)
        srt = -np.sort(-sim, axis=1)
        assert int(((npos > N) & (srt[:, N - 1] == srt[:, N])).sum()) >= 1
        assert srt[I_T, N - 1] == srt[I_T, N] and ridx[I_T].tolist() == list(range(I_T + 1,
                                                                                 I_T + 17))
        assert int((npos < N).sum()) >= 1
        assert rn[I_Z] == 0 and (ridx[I_Z] == -1).all() and not (ridx == I_Z).any()
        plain = fit_plain(hist, N, shrink)
        assert int(plain.item_count[I_Z]) == 1
        assert not np.array_equal(plain.neighbor_idx.cpu().numpy(), ridx)
        assert not np.array_equal(plain.item_count.cpu().numpy(), rn)
        if shrink == 0.0:   # the float64 route of the restatement is the uint64 one
            exact = np_fit_w(ptr, idx, w, U1, I1, N, shrink, exact_uint64=True)
            assert np.array_equal(exact[4], C) and np.array_equal(bits(exact[1]), bits(rval))
    assert_fit_equal(fit_w(hist, N, shrink), ref)


@pytest.mark.parametrize("window", [0, 1024])
def test_weighted_fit_windows(window):
    """I = 3,000 in windows of 1,024 columns: three LDS passes, the last one partial; the default
    window takes the catalogue in one."""
    ptr, idx, w, hist, ref = small2()
    I = S2[1]
    assert -(-I // 1024) == 3 and I % 1024 != 0
    assert int(((ref[4] > 0).sum(1) < 8).sum()) > 1000 and int((ref[2] == 0).sum()) >= 1
    assert_fit_equal(fit_w(hist, 8, window=window), ref)


def test_weighted_fit_large_window_agrees_with_the_small_ones():
    """More than 8,192 columns of 64-bit counters need more than 64 KiB of LDS (one workgroup a
    CU): I = 9,000 at the default window (16,384: the catalogue in one pass of 9,024 counters,
    72 KiB), at 8,192 and at 1,024 gives one table."""
    U, I, E = 300, 9000, 5000
    users, items = syn.interactions(U, I, E, seed=6)
    ptr, idx = np_csr(users, items, U, I)
    hist = history(ptr, idx, pair_weights(len(idx), seed=6), U, I)
    a = fit_w(hist, 8, 1.0)
    assert int((a.neighbor_idx >= 0).sum()) > 1000
    for window in (16384, 8192, 1024):
        assert_same_table(a, fit_w(hist, 8, 1.0, window=window))


def test_weighted_fit_w_max_comes_from_the_kept_users():
    """The bulk buyer (200 items > max_history) carries by far the largest weight: dropped, it
    must not set the scale either."""
    ptr0, idx0, w0, _ = small1()
    U, I = U1 + 1, I1
    ptr = np.concatenate([ptr0, [ptr0[-1] + 200]])
    idx = np.concatenate([idx0, np.arange(200, dtype=np.int32)])
    w = np.concatenate([w0, np.full(200, 1000.0, np.float32)])
    assert np.diff(ptr0).max() <= 64
    hist = history(ptr, idx, w, U, I)
    capped = fit_w(hist, 16, 10.0, max_history=64)
    ref = np_fit_w(ptr, idx, w, U, I, 16, 10.0, max_history=64)
    assert_fit_equal(capped, ref)
    # the same table as without that user (one more empty row in the CSR)
    without = small1_ref(16, 10.0)
    assert np.array_equal(ref[0], without[0]) and np.array_equal(bits(ref[1]), bits(without[1]))
    free = fit_w(hist, 16, 10.0)
    free_ref = np_fit_w(ptr, idx, w, U, I, 16, 10.0)
    assert_fit_equal(free, free_ref)
    assert not np.array_equal(bits(free_ref[1]), bits(ref[1]))


def test_weighted_fit_same_bits_on_every_run():
    _, _, _, hist = small1()
    a = fit_w(hist, 16, 10.0)
    assert_same_table(a, fit_w(hist, 16, 10.0))
    assert_same_table(a, fit_w(hist, 16, 10.0, window=64))


@pytest.mark.parametrize("shrink", [0.0, 10.0])
def test_unit_weights_are_the_unweighted_fit(shrink):
    ptr, idx, _, _ = small1()
    one = history(ptr, idx, np.ones(len(idx), np.float32), U1, I1)
    for mh in (0, 12):
        assert_same_table(fit_w(one, 16, shrink, max_history=mh),
                          fit_plain(one, 16, shrink, max_history=mh))
    if shrink == 0.0:   # any constant, when there is no shrink to scale
        c = history(ptr, idx, np.full(len(idx), 0.3, np.float32), U1, I1)
        assert_same_table(fit_w(c, 16, 0.0), fit_plain(c, 16, 0.0))


def raw_fit(name, p, x, w, U, I, out, N=4, shrink=0.0, max_history=0, window=0):
    extra = () if name == "hnm_itemcf_fit_f32" else (_lib.ptr(w),)
    return _lib.fn(name)(_lib.ctx(DEV), _lib.ptr(p), _lib.ptr(x), *extra, U, I, N, shrink,
                         max_history, window, *map(_lib.ptr, out))


def fit_outputs(I, N):
    return (torch.full((I, N), 7, dtype=torch.int32, device=DEV),
            torch.full((I, N), 7.0, dtype=torch.float32, device=DEV),
            torch.full((I,), 7, dtype=torch.int64, device=DEV))


def test_raw_fit_argument_errors_bad_weights_and_all_zero():
    ptr, idx, w, hist = small1()
    p, x = hist.hist_ptr, hist.hist_idx
    out = fit_outputs(I1, 4)
    for kw in ({"N": 0}, {"N": 65}, {"shrink": -1.0}, {"max_history": -1}, {"window": 100},
               {"window": 32}, {"window": 1 << 20}):
        assert raw_fit("hnm_itemcf_fit_weighted_f32", p, x, hist.hist_w, U1, I1, out,
                       **kw) == _lib.HNM_EINVAL, kw
    torch.cuda.synchronize()
    assert all(bool((o == 7).all()) for o in out)                 # nothing was written
    # a negative and a NaN weight: the error word, and both count as 0 -- also for w_max (the
    # NaN's bit pattern and |-9| would both win an unguarded max)
    bad = w.copy()
    at = [5, 11]
    bad[at[0]], bad[at[1]] = -9.0, np.nan
    wb = torch.from_numpy(bad).to(DEV)
    assert raw_fit("hnm_itemcf_fit_weighted_f32", p, x, wb, U1, I1, out) == _lib.HNM_OK
    assert _lib.fn("hnm_ctx_check")(_lib.ctx(DEV)) == _lib.HNM_EINVAL
    assert _lib.fn("hnm_ctx_check")(_lib.ctx(DEV)) == _lib.HNM_OK
    zeroed = bad.copy()
    zeroed[at] = 0
    ref = np_fit_w(ptr, idx, zeroed, U1, I1, 4)
    assert np.array_equal(out[2].cpu().numpy(), ref[2])
    assert np.array_equal(out[0].cpu().numpy(), ref[0])
    assert np.array_equal(bits(out[1]), bits(ref[1]))
    # an id outside [0, I) and a bad weight on it: skipped, HNM_EOOB is named first
    xb = x.clone()
    xb[5] = I1
    assert raw_fit("hnm_itemcf_fit_weighted_f32", p, xb, wb, U1, I1, out) == _lib.HNM_OK
    assert _lib.fn("hnm_ctx_check")(_lib.ctx(DEV)) == _lib.HNM_EOOB
    assert _lib.fn("hnm_ctx_check")(_lib.ctx(DEV)) == _lib.HNM_OK
    assert int(out[2].sum()) <= int(ref[2].sum())
    # all weights zero: an empty history
    z = torch.zeros_like(hist.hist_w)
    assert raw_fit("hnm_itemcf_fit_weighted_f32", p, x, z, U1, I1, out) == _lib.HNM_OK
    _lib.sync_check(DEV)
    assert bool((out[0] == -1).all()) and bool((out[1] == 0).all()) and bool((out[2] == 0).all())
    m = fit_w(history(ptr, idx, np.zeros(len(idx), np.float32), U1, I1), 4)
    assert bool((m.neighbor_idx == -1).all()) and bool((m.item_count == 0).all())
    # a NULL weight pointer is the unweighted entry, bit for bit
    plain = fit_outputs(I1, 4)
    assert raw_fit("hnm_itemcf_fit_weighted_f32", p, x, None, U1, I1, out,
                   shrink=3.0) == _lib.HNM_OK
    assert raw_fit("hnm_itemcf_fit_f32", p, x, None, U1, I1, plain, shrink=3.0) == _lib.HNM_OK
    _lib.sync_check(DEV)
    assert torch.equal(out[0], plain[0]) and torch.equal(out[2], plain[2])
    assert np.array_equal(bits(out[1]), bits(plain[1])) and int((plain[0] >= 0).sum()) > 0


# ------------------------------------------------------------------ scores and top-K
@functools.lru_cache(maxsize=None)
def big():
    users, items = syn.interactions(BU, BI, BE, seed=2)
    rng = np.random.Generator(np.random.PCG64(11))
    extra = [(U_ONE, [I_X]), (U_HELPER, [I_X, I_X + 1, I_X + 2, I_X + 3]),
             (U_BULK, rng.choice(BI, size=200, replace=False).tolist()),
             (U_81, rng.choice(BI, size=81, replace=False).tolist()),
             (U_82, rng.choice(BI, size=82, replace=False).tolist())]
    for u, its in extra:
        users = np.concatenate([users, np.full(len(its), u, np.int64)])
        items = np.concatenate([items, np.asarray(its, np.int64)])
    ptr, idx = np_csr(users, items, NU, NI)
    w = pair_weights(len(idx), seed=7)
    w[ptr[U_ONE]:ptr[U_HELPER + 1]] = [3.0, 1.5, 0.75, 2.0, 0.5]   # keep the hand-made rows alive
    hist_dev = history(ptr, idx, w, NU, NI)
    ref = np_fit_w(ptr, idx, w, NU, NI, BN)
    model = fit_w(hist_dev, BN)
    assert_fit_equal(model, ref)
    hist = [idx[ptr[u]:ptr[u + 1]].tolist() for u in range(NU)]
    hw = [w[ptr[u]:ptr[u + 1]] for u in range(NU)]
    batch = np.concatenate([syn.user_batch(BU, 249, seed=4),
                            [U_EMPTY, U_ONE, U_BULK, U_81, U_82, U_BULK, 7]]).astype(np.int64)
    batch[3] = batch[0]                                    # a repeated ordinary user
    assert len(batch) == 256
    rows, wrows = [hist[u] for u in batch], [hw[u] for u in batch]
    scores = np_scores_w(ref[0], ref[1], NI, rows, wrows)
    return model, ref, hist, batch, rows, wrows, scores


def test_weighted_rows_are_bitwise_the_ascending_sums_of_rounded_products():
    model, ref, hist, batch, rows, wrows, scores = big()
    got = model.predict_all_items(torch.from_numpy(batch))
    assert got.shape == (256, NI) and np.array_equal(bits(got), bits(scores))
    again = model.predict_all_items(torch.from_numpy(batch).to(DEV))
    assert np.array_equal(bits(again), bits(got))
    assert (scores[np.nonzero(batch == U_EMPTY)[0][0]] == 0).all()
    # the weights matter, and a fused multiply-add would give other bits somewhere
    one = [np.ones(len(r), np.float32) for r in rows]
    assert (bits(np_scores_w(ref[0], ref[1], NI, rows, one)) != bits(scores)).any()
    fma = np.zeros_like(scores, dtype=np.float64)
    for b in (0, 1, 2):
        acc = np.zeros(NI, np.float32)
        for j, wj in zip(rows[b], wrows[b]):
            ok = ref[0][j] >= 0
            t = acc[ref[0][j][ok]].astype(np.float64) + np.float64(wj) * ref[1][j][ok]
            acc[ref[0][j][ok]] = t.astype(np.float32)
        fma[b] = acc
    assert (bits(fma[:3].astype(np.float32)) != bits(scores[:3])).any()


def test_routes_are_those_of_the_unweighted_entry():
    model, ref, hist, batch, rows, wrows, scores = big()
    route = model.scoring_route(torch.from_numpy(batch))
    lens = np.array([len(r) for r in rows])
    assert [r == "dense" for r in route] == (lens * BN > 4096).tolist()
    by_user = dict(zip(batch.tolist(), route))
    assert by_user[U_BULK] == "dense" and by_user[U_82] == "dense"       # 82 * 50 = 4,100
    assert by_user[U_81] == "fused" and by_user[U_EMPTY] == "fused"      # 81 * 50 = 4,050
    assert route.count("dense") == 3


@pytest.mark.parametrize("kind", ["none", "dict", "history"])
@pytest.mark.parametrize("k", [1, 12, 64, 100])
def test_weighted_topk_equals_the_lists_of_the_dense_rows(k, kind):
    """k <= 64: the fused entry (LDS route, and the dense route for the three long rows);
    k = 100: dense rows + the row top-k kernel.  Ids and score bits."""
    model, ref, hist, batch, rows, wrows, scores = big()
    filt, masks = filters(kind, hist, batch)
    rv, ri = np_topk(scores, masks, k)
    u = torch.from_numpy(batch)
    gv, gi = model.recommend_with_scores(u if kind != "history" else u.to(DEV),
                                         filter_items=filt, k=k)
    assert gi.dtype == torch.int64 and gv.dtype == torch.float32
    assert np.array_equal(gi.cpu().numpy(), ri)
    assert np.array_equal(bits(gv), bits(rv))
    where = {int(x): r for r, x in enumerate(batch)}
    assert (ri[where[U_EMPTY]] == -1).all() and (rv[where[U_EMPTY]] == NEG_INF).all()
    if kind == "none":
        r = where[U_ONE]
        assert set(ri[r, :min(k, 3)].tolist()) <= {I_X + 1, I_X + 2, I_X + 3}
        assert (ri[r, 3:] == -1).all()
        assert (ri[where[U_BULK]] >= 0).all()
    if kind == "history":
        for r in (where[U_BULK], where[7]):
            assert not set(ri[r].tolist()) & set(rows[r])


def test_fused_and_dense_routes_agree_and_forward_filters_the_history():
    model, ref, hist, batch, rows, wrows, scores = big()
    u = torch.from_numpy(batch)
    dense = model.predict_all_items(u).cpu().numpy()        # hnm_itemcf_scores_weighted_f32
    for k in (12, 64):
        wv, wi = np_topk(dense, None, k)
        gv, gi = model.recommend_with_scores(u, k=k)         # fused; three rows dense-routed
        assert np.array_equal(gi.cpu().numpy(), wi) and np.array_equal(bits(gv), bits(wv))
    _, want_f = np_topk(scores, rows, 12)
    assert np.array_equal(model.forward(u).cpu().numpy(), want_f)
    assert np.array_equal(model.recommend(u).cpu().numpy(), np_topk(scores, None, 12)[1])


def test_null_weight_pointer_is_the_unweighted_entry_and_plain_histories_serve_unweighted():
    model, ref, hist, batch, rows, wrows, scores = big()
    h = model.history
    ud = torch.from_numpy(batch).to(DEV)
    B = len(batch)
    head = (_lib.ctx(DEV), _lib.ptr(model.neighbor_idx), _lib.ptr(model.neighbor_val), NI, BN,
            _lib.ptr(h.hist_ptr), _lib.ptr(h.hist_idx))
    a = torch.empty(B, NI, dtype=torch.float32, device=DEV)
    b = torch.empty_like(a)
    assert _lib.fn("hnm_itemcf_scores_weighted_f32")(*head, None, NU, _lib.ptr(ud), B, _lib.ptr(a),
                                                     NI) == _lib.HNM_OK
    assert _lib.fn("hnm_itemcf_scores_f32")(*head, NU, _lib.ptr(ud), B, _lib.ptr(b),
                                            NI) == _lib.HNM_OK
    av, bv = (torch.empty(B, 12, dtype=torch.float32, device=DEV) for _ in range(2))
    ai, bi = (torch.empty(B, 12, dtype=torch.int64, device=DEV) for _ in range(2))
    assert _lib.fn("hnm_itemcf_topk_weighted_f32")(*head, None, NU, _lib.ptr(ud), B, None, None,
                                                   12, _lib.ptr(av), _lib.ptr(ai)) == _lib.HNM_OK
    assert _lib.fn("hnm_itemcf_topk_f32")(*head, NU, _lib.ptr(ud), B, None, None, 12,
                                          _lib.ptr(bv), _lib.ptr(bi)) == _lib.HNM_OK
    _lib.sync_check(DEV)
    assert np.array_equal(bits(a), bits(b)) and float(a.abs().sum()) > 0
    assert torch.equal(ai, bi) and np.array_equal(bits(av), bits(bv))
    assert (bits(a) != bits(scores)).any()
    # a weighted model whose history has no weights serves those unweighted sums
    twin = WeightedItemCF(NU, NI, num_neighbors=BN).to(DEV)
    twin.load_state_dict(model.state_dict())
    twin.set_history(UserHistory({u: set(r) for u, r in enumerate(hist) if r}, NU, NI, DEV))
    assert twin.history.hist_w is None
    assert np.array_equal(bits(twin.predict_all_items(ud)), bits(a))
    gv, gi = twin.recommend_with_scores(ud, k=12)
    assert torch.equal(gi, ai) and np.array_equal(bits(gv), bits(av))
    # raw entry: a negative / non-finite weight raises the weight bit and counts as 0
    wbad = h.hist_w.clone()
    p0 = int(h.hist_ptr[7])
    wbad[p0] = -1.0
    wbad[p0 + 1] = float("inf")
    one = torch.tensor([7], dtype=torch.int64, device=DEV)
    assert _lib.fn("hnm_itemcf_scores_weighted_f32")(*head, _lib.ptr(wbad), NU, _lib.ptr(one), 1,
                                                     _lib.ptr(a), NI) == _lib.HNM_OK
    assert _lib.fn("hnm_ctx_check")(_lib.ctx(DEV)) == _lib.HNM_EINVAL
    assert _lib.fn("hnm_ctx_check")(_lib.ctx(DEV)) == _lib.HNM_OK
    w7 = wbad[p0:int(h.hist_ptr[8])].cpu().numpy().copy()
    w7[:2] = 0
    assert np.array_equal(bits(a[:1]), bits(np_scores_w(ref[0], ref[1], NI, [hist[7]], [w7])))


def test_a_zero_weight_item_contributes_nothing():
    model, ref, hist, batch, rows, wrows, scores = big()
    r = hist[7]
    assert len(r) >= 3
    wz = np.ones(len(r), np.float32)
    wz[1] = 0
    for k in (12, 100):
        a = model.recommend_for_items([r], filter_seen=False, k=k, weights=[wz.tolist()])
        b = model.recommend_for_items([r[:1] + r[2:]], filter_seen=False, k=k,
                                      weights=[[1.0] * (len(r) - 1)])
        c = model.recommend_for_items([r], filter_seen=False, k=k, weights=[[1.0] * len(r)])
        assert torch.equal(a[1], b[1]) and np.array_equal(bits(a[0]), bits(b[0]))
        assert not np.array_equal(bits(a[0]), bits(c[0]))


def test_weighted_baskets_equal_users_with_those_weighted_histories():
    model, ref, hist, batch, rows, wrows, scores = big()
    u = torch.from_numpy(batch)
    # unsorted, the first item repeated with its weight split in two exact halves
    baskets = [list(reversed(r)) + r[:1] for r in rows]
    halves = [np.concatenate([w[::-1], w[:1]]).astype(np.float64) for w in wrows]
    for w in halves:
        if len(w):
            w[-1] /= 2
            w[-2] /= 2
    for k in (12, 100):
        for seen in (True, False):
            filt = model.history if seen else None
            wv, wi = model.recommend_with_scores(u.to(DEV), filter_items=filt, k=k)
            gv, gi = model.recommend_for_items(baskets, filter_seen=seen, k=k,
                                               weights=[w.tolist() for w in halves])
            assert torch.equal(gi, wi) and np.array_equal(bits(gv), bits(wv))
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    idx = np.asarray([x for r in rows for x in r], np.int32)
    flat = np.concatenate(wrows).astype(np.float32)
    wv, wi = model.recommend_with_scores(u.to(DEV), filter_items=model.history, k=12)
    gv, gi = model.recommend_for_items((ptr, idx), k=12, weights=flat)
    assert torch.equal(gi, wi) and np.array_equal(bits(gv), bits(wv))
    # without weights a basket is served unweighted, as by the unweighted entry
    pv, pi = model.recommend_for_items([rows[0]], k=12)
    ov, oi = model.recommend_for_items([rows[0]], k=12, weights=[[1.0] * len(rows[0])])
    assert torch.equal(pi, oi) and np.array_equal(bits(pv), bits(ov))
    for bad in ([[1.0]], [[1.0, -2.0]], [[1.0, float("nan")]]):
        with pytest.raises(ValueError):
            model.recommend_for_items([[1, 2]], weights=bad)
    with pytest.raises(ValueError):
        model.recommend_for_items((ptr, idx), weights=flat[:-1])
    with pytest.raises(IndexError):
        model.recommend_for_items([[1, NI]], weights=[[1.0, 1.0]])
    _lib.sync_check(DEV)


# ------------------------------------------------------------------ the module and serving
def transactions(seed=5):
    """S1's transactions (repeated pairs included) with a count and an age each."""
    U, I, E = S1
    users, items = syn.interactions(U, I, E, seed=2)
    rng = np.random.default_rng(seed)
    return users, items, rng.integers(1, 9, E), rng.integers(0, 366, E)


def test_fit_interactions_weights_days_and_the_plain_model():
    U, I, _ = S1
    users, items, counts, days = transactions()
    m = WeightedItemCF(U, I, num_neighbors=16, shrink=2.0).to(DEV)
    m.fit_interactions(torch.from_numpy(users), items, weights=counts, days_ago=days,
                       time_decay=0.01)
    tw = counts * np.exp(-0.01 * days.astype(np.float64))
    want = UserHistory.from_interactions(users, items, U, I, DEV, weights=tw)
    assert np.array_equal(bits(m.history.hist_w), bits(want.hist_w))
    assert len(np.unique(users * I + items)) < len(users)      # pairs were summed
    ptr, idx = m.history.hist_ptr.cpu().numpy(), m.history.hist_idx.cpu().numpy()[:want.nnz]
    w = m.history.hist_w.cpu().numpy()[:want.nnz]
    assert_fit_equal(m, np_fit_w(ptr, idx, w, U, I, 16, 2.0))
    # days alone; and neither: every transaction weighs 1
    d = WeightedItemCF(U, I, num_neighbors=16, shrink=2.0).to(DEV)
    d.fit_interactions(users, items, days_ago=days, time_decay=0.01)
    wd = UserHistory.from_interactions(users, items, U, I, DEV,
                                       weights=np.exp(-0.01 * days.astype(np.float64)))
    assert np.array_equal(bits(d.history.hist_w), bits(wd.hist_w))
    assert not torch.equal(d.neighbor_idx, m.neighbor_idx)
    cnt = WeightedItemCF(U, I, num_neighbors=16, shrink=2.0).to(DEV).fit_interactions(users, items)
    wc = UserHistory.from_interactions(users, items, U, I, DEV, weights=np.ones(len(users)))
    assert np.array_equal(bits(cnt.history.hist_w), bits(wc.hist_w))       # a pair: its count
    assert float(cnt.history.hist_w.max()) > 1
    plain = ItemCF(U, I, num_neighbors=16, shrink=2.0).to(DEV).fit_interactions(users, items)
    uu, ii = np.divmod(np.unique(users * I + items), I)      # each pair once: unit weights
    one = WeightedItemCF(U, I, num_neighbors=16, shrink=2.0).to(DEV).fit_interactions(uu, ii)
    assert_same_table(one, plain)
    assert plain.history.hist_w is None and bool((one.history.hist_w[:want.nnz] == 1).all())
    with pytest.raises(ValueError):
        WeightedItemCF(U, I).to(DEV).fit_history(plain.history)
    with pytest.raises(ValueError):
        plain.fit_interactions(users, items, weights=counts)
    with pytest.raises(ValueError):
        plain.recommend_for_items([[1, 2]], weights=[[1.0, 2.0]])
    # a plain model ignores a history's weights: fit and serving are the unweighted ones
    again = ItemCF(U, I, num_neighbors=16, shrink=2.0).to(DEV).fit_history(m.history)
    assert_same_table(again, plain)
    ids = torch.arange(50)
    a, b = again.recommend_with_scores(ids, k=12), plain.recommend_with_scores(ids, k=12)
    assert torch.equal(a[1], b[1]) and np.array_equal(bits(a[0]), bits(b[0]))


def test_checkpoint_round_trip_keeps_the_weighted_class():
    U, I, _ = S1
    users, items, counts, days = transactions()
    src = WeightedItemCF(U, I, num_neighbors=16, shrink=2.0).to(DEV)
    src.fit_interactions(users, items, weights=counts, days_ago=days, time_decay=0.01)
    assert src.hparams["weighted"] is True
    assert list(src.state_dict()) == ["neighbor_idx", "neighbor_val", "item_count"]
    hp = dict(src.hparams)
    hp["num_users"], hp["num_items"] = 1, 1
    m = create_model_from_checkpoint("runs/item_cf", {"state_dict": src.state_dict(),
                                                      "hyper_parameters": hp}, U, I, DEV)
    assert type(m) is WeightedItemCF and m.weighted and m.shrink == 2.0
    m.set_history(src.history)
    ids = torch.arange(100)
    a, b = m.recommend_with_scores(ids, k=12), src.recommend_with_scores(ids, k=12)
    assert torch.equal(a[1], b[1]) and np.array_equal(bits(a[0]), bits(b[0]))


def test_recommender_weighted_item_cf_item_weights_and_back_fill():
    U, I, _ = S1
    users, items, counts, days = transactions()
    srv = Recommender(U, I, device=DEV)
    m = srv.add_item_cf(users, items, weights=counts, days_ago=days, time_decay=0.01,
                        num_neighbors=2, shrink=1.0)
    assert type(m) is WeightedItemCF and srv.models["item_cf"] is m and m.num_neighbors == 2
    assert srv._device_history() is m.history
    direct = WeightedItemCF(U, I, num_neighbors=2, shrink=1.0).to(DEV)
    direct.fit_interactions(users, items, weights=counts, days_ago=days, time_decay=0.01)
    assert_same_table(m, direct)
    assert type(Recommender(U, I, device=DEV).add_item_cf(users, items, days_ago=days,
                                                          time_decay=0.01)) is WeightedItemCF
    k = 30
    ask = [3, 17]
    wv, wi = m.recommend_with_scores(torch.tensor(ask), filter_items=m.history, k=k)
    wv, wi = wv.cpu().tolist(), wi.cpu().tolist()
    assert all(row[-1] < 0 <= row[0] for row in wi)          # N = 2: every row is short
    out = srv.get_batch_recommendations(ask, model_name="item_cf", num_items=k,
                                        include_scores=True)
    for r in range(2):
        n = sum(i >= 0 for i in wi[r])
        assert [x["article_id"] for x in out[r]["recommendations"]] == [str(i) for i in wi[r][:n]]
        assert [x["score"] for x in out[r]["recommendations"]] == wv[r][:n]
    # a weighted basket with a repeated item: its weights are summed
    ptr, idx = m.history.hist_ptr.cpu().numpy(), m.history.hist_idx.cpu().numpy()
    basket = idx[ptr[17]:ptr[18]].tolist()
    assert len(basket) >= 2
    given = basket + basket[:1]
    bw = [float(j + 1) for j in range(len(basket))] + [0.5]
    summed = list(bw[:len(basket)])
    summed[0] += 0.5
    bv, bi = m.recommend_for_items([basket], k=k, weights=[summed])
    got = srv.get_recommendations_for_items(given, num_items=k, include_scores=True,
                                            item_weights=bw)
    n = int((bi[0] >= 0).sum())
    assert got["model_name"] == "item_cf" and got["user_id"] is None and 0 < n < k
    assert [x["article_id"] for x in got["recommendations"]] == [str(i) for i in bi[0, :n].tolist()]
    assert [x["score"] for x in got["recommendations"]] == bv[0, :n].cpu().tolist()
    flat = srv.get_recommendations_for_items(basket, num_items=k, include_scores=True)
    assert [x["score"] for x in flat["recommendations"]] != \
        [x["score"] for x in got["recommendations"]]
    with pytest.raises(ValueError):
        srv.get_recommendations_for_items(basket, item_weights=[1.0])
    with pytest.raises(ValueError):
        srv.get_recommendations_for_items(basket[:2], item_weights=[1.0, -2.0])
    # with a baseline registered short rows are continued from the popularity list, and trimmed
    base = srv.add_popularity_baseline(items)
    pv, pi = base.recommend_with_scores(torch.tensor(ask), filter_items=m.history, k=k)
    pv, pi = pv.cpu().tolist(), pi.cpu().tolist()
    out = srv.get_batch_recommendations(ask, model_name="item_cf", num_items=k,
                                        include_scores=True)
    for r in range(2):
        ev, ei = host_back_fill(wv[r], wi[r], pv[r], pi[r])
        recs = out[r]["recommendations"]
        assert len(recs) == k == len(set(ei))
        assert [x["article_id"] for x in recs] == [str(i) for i in ei]
        assert [x["score"] for x in recs] == ev
    got = srv.get_recommendations_for_items(given, num_items=k, item_weights=bw)
    assert len(got["recommendations"]) == k
    assert [x["article_id"] for x in got["recommendations"]][:n] == [str(i) for i in
                                                                    bi[0, :n].tolist()]
    assert not {x["article_id"] for x in got["recommendations"]} & {str(i) for i in basket}
    # an unweighted item_cf still refuses item weights
    plain = Recommender(U, I, device=DEV)
    plain.add_item_cf(users, items)
    assert type(plain.models["item_cf"]) is ItemCF
    with pytest.raises(ValueError, match="item weights"):
        plain.get_recommendations_for_items(basket, model_name="item_cf", item_weights=bw)
