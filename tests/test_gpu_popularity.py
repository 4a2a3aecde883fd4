"""GPU: PopularityBaseline -- hnm_popularity_fit_f64 / hnm_popularity_topk_f32, the module and
its serving fallback.

* the fit is BITWISE a numpy restatement (integer table, then the ascending-day float64 chain),
  whatever the slab size, and within float64 summation error of the REFERENCE's pandas values
  (tests/golden/popularity_small.npz, made by make_golden_popularity.py);
* the top-K is EXACTLY `[x for x in order if x not in history][:k]` (ids and score bits), and
  equals the reference's `recommend()` lists and the dense route (`dense_topk` over a scattered
  [B, I] matrix with the same mask).
"""
import numpy as np
import pytest
import torch

from parity import load_golden
from hnm_recommendation_amd import NeuralCF, PopularityBaseline, UserHistory, _lib
from hnm_recommendation_amd import synthetic as syn
from hnm_recommendation_amd.evaluation import evaluate_recommendations
from hnm_recommendation_amd.models.base import dense_topk, filter_csr
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
    return t.cpu().numpy().view(np.int64 if t.dtype == torch.float64 else np.int32)


# ------------------------------------------------------------------ fit
def np_fit(items, days, w, num_items, D):
    """The contract: [I, D] integer table by np.add.at, then acc = acc + cnt[:, d] * w[d]."""
    cnt = np.zeros((num_items, D), np.int64)
    d = np.zeros(len(items), np.int64) if days is None else np.asarray(days, np.int64)
    keep = (d >= 0) & (d < D) & (items >= 0) & (items < num_items)
    np.add.at(cnt, (items[keep], d[keep]), 1)
    acc = np.zeros(num_items, np.float64)
    for j in range(D):
        acc = acc + cnt[:, j] * w[j]
    return cnt.sum(1), acc


def raw_fit(items, days, w, num_items, D, slab=0):
    it = dev(items, np.int64)
    dd = None if days is None else dev(days, np.int32)
    ww = None if w is None else dev(w, np.float64)
    count = torch.full((num_items,), -7, dtype=torch.int64, device=DEV)
    pop = torch.full((num_items,), -7.0, dtype=torch.float64, device=DEV)
    st = _lib.fn("hnm_popularity_fit_f64")(_lib.ctx(DEV), _lib.ptr(it), it.numel(), _lib.ptr(dd),
                                           _lib.ptr(ww), num_items, D, slab, _lib.ptr(count),
                                           _lib.ptr(pop))
    return st, count, pop


@pytest.mark.parametrize("n", [0, 1, 20_000])
@pytest.mark.parametrize("slab", [0, 8])
@pytest.mark.parametrize("window", [None, 7])
@pytest.mark.parametrize("decay", [0.0, 0.02])
@pytest.mark.parametrize("with_days", [False, True])
def test_fit_is_bitwise_the_numpy_restatement(with_days, decay, window, slab, n):
    items, days = ITEMS[:n], (DAYS[:n] if with_days else None)
    if with_days:
        D = window if window is not None else (int(days.max()) + 1 if n else 1)
        w = np.exp(-decay * np.arange(D))
    else:
        D, w = 1, np.ones(1)
    if n == 20_000 and with_days and window is None:
        assert D == 90 and (slab == 0 or -(-D // slab) == 12)   # slab = 8: 12 ascending slabs
    ref_count, ref_pop = np_fit(items, days, w, I, D)
    m = PopularityBaseline(I, time_decay=decay).to(DEV)
    m.fit_interactions(items, days_ago=days, window_days=window, _slab=slab)
    assert np.array_equal(m.count.cpu().numpy(), ref_count)
    assert np.array_equal(bits(m.pop), ref_pop.view(np.int64))
    if not with_days:
        assert np.array_equal(m.pop.cpu().numpy(), ref_count.astype(np.float64))
    # the order: items bought at least once (inside the window), (pop desc, id asc)
    ids = np.nonzero(ref_count > 0)[0]
    want = ids[np.lexsort((ids, -ref_pop[ids]))]
    assert np.array_equal(m.order.cpu().numpy(), want)
    assert np.array_equal(m.order_val.cpu().numpy(), ref_pop[want].astype(np.float32))
    rank = np.full(I, -1, np.int32)
    rank[want] = np.arange(len(want))
    assert np.array_equal(m.rank.cpu().numpy(), rank)


def test_fit_same_bits_on_every_run():
    w = np.exp(-0.02 * np.arange(90))
    a = raw_fit(ITEMS, DAYS, w, I, 90)
    b = raw_fit(ITEMS, DAYS, w, I, 90)
    c = raw_fit(ITEMS, DAYS, w, I, 90, slab=8)
    assert a[0] == b[0] == c[0] == _lib.HNM_OK
    for x in (b, c):
        assert torch.equal(a[1], x[1]) and np.array_equal(bits(a[2]), bits(x[2]))
    _lib.sync_check(DEV)
    # NULL day weights: all 1.0 (the windowed count)
    st, count, pop = raw_fit(ITEMS, DAYS, None, I, 30)
    rc, rp = np_fit(ITEMS, DAYS, np.ones(30), I, 30)
    assert st == _lib.HNM_OK and np.array_equal(count.cpu().numpy(), rc)
    assert np.array_equal(bits(pop), rp.view(np.int64)) and rc.sum() == (DAYS < 30).sum()


def test_fit_out_of_range_item_and_unsupported_days():
    items = ITEMS[:500].copy()
    items[[3, 77]] = [I, -1]
    w = np.exp(-0.02 * np.arange(90))
    st, count, pop = raw_fit(items, DAYS[:500], w, I, 90)
    assert st == _lib.HNM_OK
    assert _lib.fn("hnm_ctx_check")(_lib.ctx(DEV)) == _lib.HNM_EOOB
    assert _lib.fn("hnm_ctx_check")(_lib.ctx(DEV)) == _lib.HNM_OK     # the word was cleared
    rc, rp = np_fit(items, DAYS[:500], w, I, 90)                       # skips the two bad rows
    assert rc.sum() == 498 and np.array_equal(count.cpu().numpy(), rc)
    assert np.array_equal(bits(pop), rp.view(np.int64))
    m = PopularityBaseline(I).to(DEV)
    with pytest.raises(IndexError):
        m.fit_interactions(items)
    big = np.ones(65_537)
    assert raw_fit(ITEMS[:10], DAYS[:10], big, I, 65_537)[0] == _lib.HNM_EUNSUPPORTED
    assert raw_fit(ITEMS[:10], DAYS[:10], big[:-1], I, 65_536)[0] == _lib.HNM_OK
    _lib.sync_check(DEV)


@pytest.mark.parametrize("tag", ["d0", "d1"])
def test_fit_matches_reference(tag):
    """pop within rtol 1e-11 of the reference's pandas sums: both are float64 sums of at most
    2e4 positive terms in different orders, each within n * 2^-53 ~ 2.2e-12 of exact."""
    decay = float(G[f"decay_{tag}"])
    m = PopularityBaseline(I, time_decay=decay).to(DEV)
    m.fit_interactions(ITEMS, days_ago=DAYS if decay > 0 else None)
    pop = m.pop.cpu().numpy()
    np.testing.assert_allclose(pop, G[f"pop_{tag}"], rtol=1e-11, atol=0.0)
    ref_order = G[f"order_{tag}"]
    ours = m.order.cpu().numpy()
    assert set(ours.tolist()) == set(ref_order.tolist()) and len(ours) == len(ref_order) <= 220
    p = pop[ref_order]
    assert (p[1:] <= p[:-1] * (1 + 1e-11)).all()       # the reference's order under our pop
    ids = np.nonzero(m.count.cpu().numpy() > 0)[0]
    assert np.array_equal(ours, ids[np.lexsort((ids, -pop[ids]))])


class Frame:
    """A duck-typed frame: `columns` and `frame[col]` -> array (no pandas)."""

    def __init__(self, **cols):
        self.cols = cols
        self.columns = list(cols)

    def __getitem__(self, c):
        return self.cols[c]


def test_fit_popularity_takes_a_duck_typed_frame():
    dates = np.datetime64("2020-09-22") - DAYS.astype("timedelta64[D]")
    f = Frame(customer_idx=USERS, article_idx=ITEMS, t_dat=dates.astype("datetime64[ns]"))
    a = PopularityBaseline(I, time_decay=0.02, personalized=True).to(DEV)
    a.fit_popularity(f)
    b = PopularityBaseline(I, time_decay=0.02, personalized=True).to(DEV)
    b.fit_interactions(ITEMS, USERS, DAYS)
    assert np.array_equal(bits(a.pop), bits(b.pop)) and torch.equal(a.order, b.order)
    assert torch.equal(a.history.hist_idx, b.history.hist_idx)
    assert f.columns == ["customer_idx", "article_idx", "t_dat"]        # nothing added
    c = PopularityBaseline(I).to(DEV).fit_popularity(Frame(customer_idx=USERS, article_idx=ITEMS))
    assert np.array_equal(c.pop.cpu().numpy(), np.bincount(ITEMS, minlength=I).astype(float))
    assert c.history is None and c.state_dict() == {}


# ------------------------------------------------------------------ top-K
def py_topk(order, val, rows, k):
    """[x for x in order if x not in hist][:k], padded with (-inf, -1)."""
    ids = np.full((len(rows), k), -1, np.int64)
    vals = np.full((len(rows), k), NEG_INF, np.float32)
    score = dict(zip(order.tolist(), val.tolist()))
    for b, hist in enumerate(rows):
        hist = set(hist)
        got = [x for x in order.tolist() if x not in hist][:k]
        ids[b, :len(got)] = got
        vals[b, :len(got)] = [score[x] for x in got]
    return vals, ids


def raw_topk(order, val, num_items, rows, k, chunk=0, B=None):
    """The raw ABI with an unsorted, possibly duplicated CSR built from `rows` (None: NULL)."""
    R = len(order)
    rank = np.full(num_items, -1, np.int32)
    rank[order] = np.arange(R)
    B = len(rows) if B is None else B
    o, v, r = dev(order, np.int64), dev(val, np.float32), dev(rank, np.int32)
    mp = mi = None
    if rows is not None:
        mp = dev(np.concatenate([[0], np.cumsum([len(x) for x in rows])]), np.int64)
        flat = [x for row in rows for x in row]
        mi = dev(flat if flat else [0], np.int32)
    out_v = torch.full((B, k), 123.0, dtype=torch.float32, device=DEV)
    out_i = torch.full((B, k), 123, dtype=torch.int64, device=DEV)
    st = _lib.fn("hnm_popularity_topk_f32")(_lib.ctx(DEV), _lib.ptr(o), _lib.ptr(v), R, _lib.ptr(r),
                                            num_items, _lib.ptr(mp), _lib.ptr(mi), B, k, chunk,
                                            _lib.ptr(out_v), _lib.ptr(out_i))
    return st, out_v, out_i


def check_topk(order, val, num_items, rows, k, chunk=0, B=None):
    st, ov, oi = raw_topk(order, val, num_items, rows, k, chunk, B)
    assert st == _lib.HNM_OK
    rv, ri = py_topk(order, val, rows if rows is not None else [[]] * ov.shape[0], k)
    assert np.array_equal(oi.cpu().numpy(), ri), (k, chunk)
    assert np.array_equal(bits(ov), rv.view(np.int32)), (k, chunk)
    _lib.sync_check(DEV)
    return ov, oi


def ranked_catalogue(num_items=400, R=330, seed=5):
    rng = np.random.Generator(np.random.PCG64(seed))
    order = rng.permutation(num_items)[:R].astype(np.int64)
    val = np.sort(rng.random(R).astype(np.float32))[::-1].copy()
    unranked = np.setdiff1d(np.arange(num_items), order)
    return order, val, unranked


def wave_rows(order, unranked):
    """Histories of 0, 1, 63, 64, 65 and 300 entries: the head of the order, so every window
    extends past k, with ranks 2 and 7 swapped for unranked items (rank -1)."""
    rows = []
    for L in (0, 1, 63, 64, 65, 300):
        h = order[:L].tolist()
        for j, pos in enumerate((2, 7)):
            if pos < L:
                h[pos] = int(unranked[j])
        rows.append(h[::-1])                                 # the raw ABI promises no sorting
    return rows


@pytest.mark.parametrize("k", [0, 1, 12, 100, 330])
def test_topk_equals_python_restatement(k):
    order, val, unranked = ranked_catalogue()
    rows = wave_rows(order, unranked)
    if k == 0:
        st, ov, oi = raw_topk(order, val, 400, rows, 0)
        assert st == _lib.HNM_OK and ov.shape == (6, 0)
        return
    check_topk(order, val, 400, rows, k)
    check_topk(order, val, 400, None, k, B=6)                   # NULL mask: the head of the order
    check_topk(order, val, 400, [[] for _ in rows], k)       # a CSR of empty rows


def test_topk_duplicates_short_orders_and_batch_sizes():
    order, val, unranked = ranked_catalogue()
    top = order.tolist()
    # duplicate entries do nothing twice; only-unranked histories do nothing at all
    rows = [[top[0]] * 5 + [top[1], top[1]], [int(unranked[0])] * 3, top[:20] * 3,
            [top[3], int(unranked[1]), top[3], top[0], int(unranked[1])]]
    check_topk(order, val, 400, rows, 12)
    # R < k: the row ends in (-inf, -1); with the whole order masked, nothing is left
    ov, oi = check_topk(order[:5], val[:5], 400, [[], top[1:3], top[:5]], 12)
    assert oi[2].tolist() == [-1] * 12 and (ov[2] == NEG_INF).all()
    assert oi[0, :5].tolist() == top[:5] and oi[1, :3].tolist() == [top[0], top[3], top[4]]
    check_topk(order[:0], val[:0], 400, [[], top[:3]], 4)    # an empty order
    # B = 1, 65 (random histories of 0..80 items over ranked and unranked ids), 0
    rng = np.random.Generator(np.random.PCG64(9))
    rows65 = [rng.integers(0, 400, size=int(rng.integers(0, 81))).tolist() for _ in range(65)]
    check_topk(order, val, 400, rows65, 12)
    check_topk(order, val, 400, rows65[:1], 12)
    st, ov, oi = raw_topk(order, val, 400, [], 12, B=0)
    assert st == _lib.HNM_OK and ov.shape == (0, 12)


def test_topk_chunked_passes_equal_one_pass():
    """chunk = 64 with a 300-item history: the 312-rank window takes 5 passes, carrying the
    emitted count; the result is that of the single default pass."""
    order, val, unranked = ranked_catalogue()
    rows = wave_rows(order, unranked)
    assert -(-min(len(order), 12 + len(rows[-1])) // 64) >= 5
    for k in (12, 100):
        a = check_topk(order, val, 400, rows, k, chunk=64)
        b = check_topk(order, val, 400, rows, k, chunk=0)
        c = check_topk(order, val, 400, rows, k, chunk=128)
        for x in (b, c):
            assert torch.equal(a[1], x[1]) and np.array_equal(bits(a[0]), bits(x[0]))
    assert raw_topk(order, val, 400, rows, 12, chunk=100)[0] == _lib.HNM_EINVAL


def test_topk_out_of_range_mask_id():
    order, val, _ = ranked_catalogue()
    for bad in (400, -3):
        st, ov, oi = raw_topk(order, val, 400, [[int(order[0])], [int(order[1]), bad]], 4)
        assert st == _lib.HNM_OK
        assert _lib.fn("hnm_ctx_check")(_lib.ctx(DEV)) == _lib.HNM_EOOB
        assert oi[0].tolist() == order[1:5].tolist()          # the other rows are answered
    _lib.sync_check(DEV)


@pytest.mark.parametrize("tag", ["d0", "d1"])
@pytest.mark.parametrize("pers", [False, True])
@pytest.mark.parametrize("k", [5, 12])
def test_recommend_equals_reference_lists(tag, pers, k):
    """The reference's order installed, its recommend() lists reproduced exactly -- the user
    who bought the entire top 40 (the window extends) and the user without history included."""
    batch = G["batch"]
    assert batch[0] == G["heavy"] and batch[1] == G["nohist"]
    want = G[f"rec_{tag}_{'p' if pers else 'np'}_k{k}"]
    m = PopularityBaseline(I, k=k, time_decay=float(G[f"decay_{tag}"]), personalized=pers).to(DEV)
    m.fit_interactions(ITEMS, USERS, DAYS)
    assert (m.history is not None) == pers
    m.set_popular_items(G[f"order_{tag}"])
    rec = m.recommend(batch.tolist(), k=k)
    assert list(rec) == batch.tolist()
    assert [rec[int(u)] for u in batch] == want.tolist()
    assert m.forward(torch.from_numpy(batch)).cpu().tolist() == want.tolist()
    assert m(torch.from_numpy(batch).to(DEV)).dtype == torch.int64
    if pers:
        top40 = set(G[f"order_{tag}"][:40].tolist())
        assert not top40 & set(want[0].tolist()) and top40 >= set(want[1].tolist())
    else:
        assert (want == G[f"order_{tag}"][:k]).all()


def test_filter_dict_and_user_history_agree():
    m = PopularityBaseline(I, time_decay=0.02).to(DEV).fit_interactions(ITEMS, days_ago=DAYS)
    users = np.concatenate([G["batch"], G["batch"][:3]])
    h = {int(u): set(ITEMS[USERS == u].tolist()) for u in np.unique(USERS)}
    hist = UserHistory(h, U, I, DEV)
    a = m.recommend_with_scores(torch.from_numpy(users), filter_items=h, k=12)
    b = m.recommend_with_scores(torch.from_numpy(users).to(DEV), filter_items=hist, k=12)
    assert torch.equal(a[1], b[1]) and np.array_equal(bits(a[0]), bits(b[0]))
    order, val = m.order.cpu().numpy(), m.order_val.cpu().numpy()
    rv, ri = py_topk(order, val, [h.get(int(u), ()) for u in users], 12)
    assert np.array_equal(a[1].cpu().numpy(), ri) and np.array_equal(bits(a[0]), rv.view(np.int32))
    # k is clamped to num_items; k = 0 is torch.topk's empty result
    v, i = m.recommend_with_scores(torch.from_numpy(users), k=I + 50)
    assert i.shape == (len(users), I) and (i[:, len(order):] == -1).all()
    assert m.recommend_with_scores(torch.from_numpy(users), k=0)[1].shape == (len(users), 0)


def test_equals_dense_route():
    """I = 20,000, B = 64, k = 12: ids and scores equal dense_topk over the [B, I] matrix that
    holds order_val at the ranked items and -inf elsewhere, with the same mask.  Weights are
    distinct, so the order is unambiguous."""
    n_items, B, R = 20_000, 64, 15_000
    rng = np.random.Generator(np.random.PCG64(21))
    order = rng.permutation(n_items)[:R].astype(np.int64)
    weights = np.arange(R, 0, -1).astype(np.float32) * np.float32(0.25)
    m = PopularityBaseline(n_items).to(DEV).set_popular_items(order, weights)
    users = syn.user_batch(5000, B, seed=4)
    h = syn.filter_dict(users, n_items, per_user=23, seed=8)
    for j, u in enumerate(users[:20]):                       # histories that reach into the top
        h[int(u)] |= set(order[:3 * j + 1].tolist())
    u = torch.from_numpy(users).to(DEV)
    scores = torch.full((B, n_items), NEG_INF, dtype=torch.float32, device=DEV)
    scores[:, m.order] = m.order_val
    mptr, midx = filter_csr(u, h, n_items, DEV)
    dv, di = dense_topk(scores, 12, mptr, midx)
    pv, pi = m.recommend_with_scores(u, filter_items=h, k=12)
    assert torch.equal(pi, di) and np.array_equal(bits(pv), bits(dv))
    assert (pi[19] != pi[0]).any()


# ------------------------------------------------------------------ hooks, serving
def test_lightning_eval_hooks():
    """validation_step + on_validation_epoch_end log what evaluate_recommendations gives for
    the same lists (every user has truth, so both average every metric over all rows; the
    logged values are float32 tensors: 2^-23 relative)."""
    m = PopularityBaseline(I, personalized=True).to(DEV).fit_interactions(ITEMS, USERS, DAYS)
    users = G["batch"]
    top = m.forward(torch.from_numpy(users)).cpu().numpy()
    rng = np.random.Generator(np.random.PCG64(3))
    truth = np.full((len(users), 6), -1, np.int64)
    for r in range(len(users)):
        n = int(rng.integers(1, 7))
        truth[r, :n] = rng.choice(I, size=n, replace=False)
    truth[::2, 0] = top[::2, 3]
    half = len(users) // 2
    for j, sl in enumerate((slice(0, half), slice(half, len(users)))):
        m.validation_step({"user_ids": torch.from_numpy(users[sl]).to(DEV),
                           "ground_truth": torch.from_numpy(truth[sl]).to(DEV)}, j)
    m.on_validation_epoch_end()
    ref = evaluate_recommendations({int(u): top[r].tolist() for r, u in enumerate(users)},
                                   {int(u): [int(x) for x in truth[r] if x >= 0]
                                    for r, u in enumerate(users)}, k=12, device=DEV)
    for ours, theirs in (("map_at_k", "map@12"), ("recall_at_k", "recall@12"),
                         ("precision_at_k", "precision@12"), ("ndcg_at_k", "ndcg@12")):
        assert float(m.logged_metrics[f"val_{ours}"]) == pytest.approx(float(ref[theirs]),
                                                                       rel=2.0 ** -23)
    assert float(m.logged_metrics["val_map_at_k"]) > 0 and m.metrics._n_all == 0


def test_serving_fallback_and_cold_start():
    h = {int(u): set(ITEMS[USERS == u].tolist()) for u in np.unique(USERS)}
    srv = Recommender(U, I, models={"neural_cf": NeuralCF(U, I)}, user_history=h, device=DEV)
    assert srv._get_best_model() == "neural_cf"
    base = srv.add_popularity_baseline(ITEMS, days_ago=DAYS, time_decay=0.02)
    assert isinstance(base, PopularityBaseline) and not base.personalized
    assert srv._get_best_model() == "popularity_baseline"      # serve.py:421
    order, val = base.order.cpu().numpy(), base.order_val.cpu().numpy()
    heavy, nohist = int(G["heavy"]), int(G["nohist"])
    ask = [heavy, 10 ** 6, 7, nohist, "nobody"]
    out = srv.get_batch_recommendations(ask, num_items=12, include_scores=True)
    assert out[1] == {"user_id": 10 ** 6, "error": "user 1000000 not found"}
    assert out[4] == {"user_id": "nobody", "error": "user nobody not found"}
    rv, ri = py_topk(order, val, [h[heavy], h[7], ()], 12)
    for r, j in enumerate((0, 2, 3)):
        assert out[j]["model_name"] == "popularity_baseline" and out[j]["user_id"] == ask[j]
        assert [x["article_id"] for x in out[j]["recommendations"]] == [str(i) for i in ri[r]]
        assert [x["score"] for x in out[j]["recommendations"]] == rv[r].tolist()
        assert not {int(x["article_id"]) for x in out[j]["recommendations"]} & set(h.get(ask[j], ()))
    one = srv.get_recommendations(heavy, num_items=5, filter_purchased=False)
    assert [x["article_id"] for x in one["recommendations"]] == [str(i) for i in order[:5]]
    with pytest.raises(ValueError):
        srv.get_recommendations(10 ** 6)
    # opt-in cold start: the unfiltered popular list in the unknown user's slot
    cold = Recommender(U, I, models={"neural_cf": NeuralCF(U, I)}, user_history=h, device=DEV,
                       cold_start="popularity")
    with pytest.raises(ValueError, match="popularity_baseline"):
        cold.get_batch_recommendations(ask)
    cold.add_popularity_baseline(ITEMS, days_ago=DAYS, time_decay=0.02)
    got = cold.get_batch_recommendations(ask, model_name="neural_cf", num_items=12)
    for j in (1, 4):
        assert got[j]["model_name"] == "popularity_baseline" and got[j]["user_id"] == ask[j]
        assert [x["article_id"] for x in got[j]["recommendations"]] == [str(i) for i in order[:12]]
    for j in (0, 2, 3):
        assert got[j]["model_name"] == "neural_cf" and len(got[j]["recommendations"]) == 12
    single = cold.get_recommendations("nobody", num_items=3, include_scores=True)
    assert single["model_name"] == "popularity_baseline"
    assert [x["score"] for x in single["recommendations"]] == val[:3].tolist()
