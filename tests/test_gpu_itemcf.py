"""GPU: ItemCF -- hnm_itemcf_fit_f32 / hnm_itemcf_scores_f32 / hnm_itemcf_topk_f32, the module,
basket serving and the popularity back-fill.

There is no reference implementation, so everything is compared BITWISE against the numpy
restatement of the contract (include/hnm.h) in itemcf_oracle.py (fit, scores, and the top-K
selection -- here from the fused route and from the dense one).
"""
import functools

import numpy as np
import pytest
import torch

from hnm_recommendation_amd import ItemCF, PopularityBaseline, _lib
from hnm_recommendation_amd import synthetic as syn
from hnm_recommendation_amd.evaluation import (evaluate_model, evaluate_recommendations,
                                               truth_csr)
from hnm_recommendation_amd.serving import Recommender, create_model_from_checkpoint
from itemcf_gpu import (BE, BI, BN, BU, DEV, I_X, NI, NU, U_81, U_82, U_BULK, U_EMPTY, U_HELPER,
                        U_ONE, assert_fit_equal, bits, filters, host_back_fill)
from itemcf_oracle import NEG_INF, np_csr, np_fit, np_scores, np_topk

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ fit
@functools.lru_cache(maxsize=None)
def small(shape):
    U, I, E = shape
    users, items = syn.interactions(U, I, E, seed=2)
    assert len(np.unique(users * I + items)) < E          # duplicates kept: the CSR drops them
    return users, items, np_csr(users, items, U, I)


@functools.lru_cache(maxsize=None)
def small_ref(shape, N, shrink):
    U, I, _ = shape
    _, _, (ptr, idx) = small(shape)
    return np_fit(ptr, idx, U, I, N, shrink)


def fit_model(users, items, U, I, N, shrink=0.0, max_history=0, window=0):
    m = ItemCF(U, I, num_neighbors=N, shrink=shrink, max_history=max_history).to(DEV)
    return m.fit_interactions(users, items, _window=window)


S1 = (600, 300, 6000)
S2 = (300, 3000, 4000)


@pytest.mark.parametrize("shrink", [0.0, 10.0])
@pytest.mark.parametrize("N", [1, 16, 64])
def test_fit_is_bitwise_the_numpy_restatement(N, shrink):
    U, I, _ = S1
    users, items, _ = small(S1)
    ref = small_ref(S1, N, shrink)
    ridx, rval, rn, sim, C = ref
    if N == 16:
        # what the pass relies on: rows with a tie exactly at the N-th place (j ascending
        # decides) and rows shorter than N (padding)
        npos = (C > 0).sum(1)
        srt = -np.sort(-sim, axis=1)
        ties = int(((npos > N) & (srt[:, N - 1] == srt[:, N])).sum())
        assert ties >= 1 and int((npos < N).sum()) >= 1
        if shrink == 0.0:
            assert ties == 99 and int((npos < N).sum()) == 6
    assert_fit_equal(fit_model(users, items, U, I, N, shrink), ref)


@pytest.mark.parametrize("window", [0, 1024])
def test_fit_windows(window):
    """I = 3,000 in windows of 1,024 columns: three LDS passes, the last one partial; the default
    window takes the catalogue in one.  Most rows are short, never-bought items included."""
    U, I, _ = S2
    users, items, _ = small(S2)
    ref = small_ref(S2, 8, 0.0)
    assert -(-I // 1024) == 3 and I % 1024 != 0
    assert int(((ref[4] > 0).sum(1) < 8).sum()) == 1714 and int((ref[2] == 0).sum()) >= 1
    assert_fit_equal(fit_model(users, items, U, I, 8, window=window), ref)


def test_fit_max_history_drops_the_bulk_buyer():
    U, I, _ = S1
    users, items, _ = small(S1)
    bulk = np.arange(0, 200, dtype=np.int64)
    u2 = np.concatenate([users, np.full(200, U, np.int64)])
    i2 = np.concatenate([items, bulk])
    assert np.diff(np_csr(users, items, U, I)[0]).max() <= 64
    without = small_ref(S1, 16, 0.0)
    capped = fit_model(u2, i2, U + 1, I, 16, max_history=64)
    assert_fit_equal(capped, without)
    free = fit_model(u2, i2, U + 1, I, 16, max_history=0)
    ptr, idx = np_csr(u2, i2, U + 1, I)
    assert_fit_equal(free, np_fit(ptr, idx, U + 1, I, 16))
    assert not np.array_equal(free.item_count.cpu().numpy(), without[2])
    assert not np.array_equal(bits(free.neighbor_val), bits(without[1]))


def test_fit_out_of_range_ids_and_bad_arguments():
    U, I, _ = S1
    users, items, (ptr, idx) = small(S1)
    for bad_u, bad_i in ((U, 0), (0, I), (-1, 0), (0, -1)):
        m = ItemCF(U, I, num_neighbors=4).to(DEV)
        with pytest.raises(IndexError):
            m.fit_interactions(np.append(users, bad_u), np.append(items, bad_i))
    # the raw entry: a CSR that holds an id outside [0, I) raises the error word, writes nothing
    # out of bounds and skips the entry
    bad = idx.copy()
    bad[5], bad[-1] = I, -3
    out = (torch.empty(I, 4, dtype=torch.int32, device=DEV),
           torch.empty(I, 4, dtype=torch.float32, device=DEV),
           torch.empty(I, dtype=torch.int64, device=DEV))
    p, x = torch.from_numpy(ptr).to(DEV), torch.from_numpy(bad).to(DEV)

    def raw(N=4, shrink=0.0, max_history=0, window=0):
        return _lib.fn("hnm_itemcf_fit_f32")(_lib.ctx(DEV), _lib.ptr(p), _lib.ptr(x), U, I, N,
                                             shrink, max_history, window, *map(_lib.ptr, out))
    assert raw() == _lib.HNM_OK
    assert _lib.fn("hnm_ctx_check")(_lib.ctx(DEV)) == _lib.HNM_EOOB
    assert _lib.fn("hnm_ctx_check")(_lib.ctx(DEV)) == _lib.HNM_OK
    assert int(out[2].sum()) == len(idx) - 2
    for kw in ({"N": 0}, {"N": 65}, {"shrink": -1.0}, {"max_history": -1}, {"window": 100},
               {"window": 32}, {"window": 1 << 20}):
        assert raw(**kw) == _lib.HNM_EINVAL, kw
    _lib.sync_check(DEV)


def test_fit_same_bits_on_every_run():
    U, I, _ = S1
    users, items, _ = small(S1)
    a = fit_model(users, items, U, I, 16, 10.0)
    b = fit_model(users, items, U, I, 16, 10.0)
    c = fit_model(users, items, U, I, 16, 10.0, window=64)
    for x in (b, c):
        assert torch.equal(a.neighbor_idx, x.neighbor_idx)
        assert np.array_equal(bits(a.neighbor_val), bits(x.neighbor_val))
        assert torch.equal(a.item_count, x.item_count)


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
    ref = np_fit(ptr, idx, NU, NI, BN)
    model = fit_model(users, items, NU, NI, BN)
    assert_fit_equal(model, ref)
    hist = [idx[ptr[u]:ptr[u + 1]].tolist() for u in range(NU)]
    batch = np.concatenate([syn.user_batch(BU, 249, seed=4),
                            [U_EMPTY, U_ONE, U_BULK, U_81, U_82, U_BULK, 7]]).astype(np.int64)
    batch[3] = batch[0]                                    # a repeated ordinary user
    assert len(batch) == 256
    rows = [hist[u] for u in batch]
    scores = np_scores(ref[0], ref[1], NI, rows)
    return model, ref, hist, batch, rows, scores


def test_predict_all_items_is_bitwise_the_ascending_sums():
    model, ref, hist, batch, rows, scores = big()
    got = model.predict_all_items(torch.from_numpy(batch))
    assert got.shape == (256, NI) and np.array_equal(bits(got), bits(scores))
    again = model.predict_all_items(torch.from_numpy(batch).to(DEV))
    assert np.array_equal(bits(again), bits(got))
    assert (scores[np.nonzero(batch == U_EMPTY)[0][0]] == 0).all()


def test_routes():
    model, ref, hist, batch, rows, scores = big()
    route = model.scoring_route(torch.from_numpy(batch))
    lens = np.array([len(r) for r in rows])
    assert [r == "dense" for r in route] == (lens * BN > 4096).tolist()
    by_user = dict(zip(batch.tolist(), route))
    assert by_user[U_BULK] == "dense" and by_user[U_82] == "dense"       # 82 * 50 = 4,100
    assert by_user[U_81] == "fused" and by_user[U_EMPTY] == "fused"      # 81 * 50 = 4,050
    assert route.count("dense") == 3


@pytest.mark.parametrize("kind", ["none", "dict", "history"])
@pytest.mark.parametrize("k", [1, 12, 64, 100])
def test_topk_equals_the_lists_of_the_dense_rows(k, kind):
    """k <= 64: the fused entry (LDS route, and the dense route for the three long rows);
    k = 100: dense rows + the row top-k kernel.  Ids and score bits."""
    model, ref, hist, batch, rows, scores = big()
    filt, masks = filters(kind, hist, batch)
    rv, ri = np_topk(scores, masks, k)
    u = torch.from_numpy(batch)
    gv, gi = model.recommend_with_scores(u if kind != "history" else u.to(DEV),
                                         filter_items=filt, k=k)
    assert gi.dtype == torch.int64 and gv.dtype == torch.float32
    assert np.array_equal(gi.cpu().numpy(), ri)
    assert np.array_equal(bits(gv), bits(rv))
    v2, i2 = model.recommend_with_scores(u, filter_items=filt, k=k)    # a second call
    assert torch.equal(i2, gi) and np.array_equal(bits(v2), bits(gv))
    where = {int(x): r for r, x in enumerate(batch)}
    assert (ri[where[U_EMPTY]] == -1).all() and (rv[where[U_EMPTY]] == NEG_INF).all()
    if kind == "none":
        # the one-item history: its item has exactly three neighbours, then padding
        r = where[U_ONE]
        assert ri[r, :3].tolist()[:k] == [I_X + 1, I_X + 2, I_X + 3][:k]
        assert (ri[r, 3:] == -1).all()
        assert (ri[where[U_BULK]] >= 0).all()
    if kind == "history":
        for r in (where[U_BULK], where[7]):
            assert not set(ri[r].tolist()) & set(rows[r])
    if k == 12:
        # the summation order is part of the contract: descending order gives other bits
        dv, _ = np_topk(np_scores(ref[0], ref[1], NI, rows, descending=True), masks, k)
        assert (bits(dv) != bits(rv)).any()


def test_recommend_and_edge_calls():
    model, ref, hist, batch, rows, scores = big()
    u = torch.from_numpy(batch)
    _, want = np_topk(scores, None, 12)
    assert np.array_equal(model.recommend(u).cpu().numpy(), want)
    _, want_f = np_topk(scores, rows, 12)
    assert np.array_equal(model.forward(u).cpu().numpy(), want_f)       # own history filtered
    v, i = model.recommend_with_scores(u[:0], k=12)
    assert v.shape == (0, 12) and i.shape == (0, 12)
    v, i = model.recommend_with_scores(u, k=0)
    assert v.shape == (256, 0) and i.shape == (256, 0)
    v, i = model.recommend_with_scores(u[:0], k=100)
    assert v.shape == (0, 100)
    for bad in (NU, -1):
        with pytest.raises(IndexError):
            model.recommend_with_scores(torch.tensor([3, bad]), k=12)
        with pytest.raises(IndexError):
            model.recommend_with_scores(torch.tensor([3, bad], device=DEV), k=12)
        with pytest.raises(IndexError):
            model.predict_all_items(torch.tensor([bad], device=DEV))
    _lib.sync_check(DEV)
    # raw entry: k out of range, B = 0 and k = 0 launch nothing and touch nothing
    h = model.history
    out_v = torch.full((4, 12), 5.0, dtype=torch.float32, device=DEV)
    out_i = torch.full((4, 12), 5, dtype=torch.int64, device=DEV)
    ud = u[:4].to(DEV)

    def raw(B, k):
        return _lib.fn("hnm_itemcf_topk_f32")(
            _lib.ctx(DEV), _lib.ptr(model.neighbor_idx), _lib.ptr(model.neighbor_val), NI, BN,
            _lib.ptr(h.hist_ptr), _lib.ptr(h.hist_idx), NU, _lib.ptr(ud), B, None, None, k,
            _lib.ptr(out_v), _lib.ptr(out_i))
    assert raw(0, 12) == _lib.HNM_OK and raw(4, 0) == _lib.HNM_OK
    assert raw(4, 65) == _lib.HNM_EINVAL and raw(4, -1) == _lib.HNM_EINVAL
    torch.cuda.synchronize()
    assert (out_v == 5.0).all() and (out_i == 5).all()
    assert raw(4, 12) == _lib.HNM_OK
    assert np.array_equal(out_i.cpu().numpy(), want[:4])


def test_recommend_for_items_equals_users_with_those_histories():
    model, ref, hist, batch, rows, scores = big()
    u = torch.from_numpy(batch)
    for k in (12, 100):
        for seen in (True, False):
            filt = model.history if seen else None
            wv, wi = model.recommend_with_scores(u.to(DEV), filter_items=filt, k=k)
            gv, gi = model.recommend_for_items([list(reversed(r)) + r[:1] for r in rows],
                                               filter_seen=seen, k=k)       # unsorted, repeated
            assert torch.equal(gi, wi) and np.array_equal(bits(gv), bits(wv))
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    idx = np.asarray([x for r in rows for x in r], np.int32)
    wv, wi = model.recommend_with_scores(u.to(DEV), filter_items=model.history, k=12)
    gv, gi = model.recommend_for_items((ptr, idx), k=12)
    assert torch.equal(gi, wi) and np.array_equal(bits(gv), bits(wv))
    with pytest.raises(IndexError):
        model.recommend_for_items([[1, NI]])
    with pytest.raises(IndexError):
        model.recommend_for_items((np.array([0, 2]), np.array([1, NI], np.int32)))
    _lib.sync_check(DEV)
    v, i = model.recommend_for_items([], k=5)
    assert v.shape == (0, 5)


def test_similar_items_are_the_table_rows():
    model, ref = big()[:2]
    ids = [0, 5, I_X, NI - 1]
    v, i = model.similar_items(ids, k=7)
    assert i.dtype == torch.int64
    assert np.array_equal(i.cpu().numpy(), ref[0][ids, :7])
    assert np.array_equal(bits(v), bits(ref[1][ids, :7]))
    assert i[2].tolist() == [I_X + 1, I_X + 2, I_X + 3, -1, -1, -1, -1]
    assert model.similar_items(torch.tensor(ids))[1].shape == (4, BN)
    with pytest.raises(ValueError):
        model.similar_items(ids, k=BN + 1)
    with pytest.raises(IndexError):
        model.similar_items([NI])


def test_state_dict_round_trip_keeps_the_answers():
    model, ref, hist, batch, rows, scores = big()
    twin = ItemCF(NU, NI, num_neighbors=BN).to(DEV)
    with pytest.raises(RuntimeError, match="not fitted"):
        twin.recommend(torch.from_numpy(batch))
    twin.load_state_dict(model.state_dict())
    with pytest.raises(RuntimeError, match="no history"):
        twin.recommend(torch.from_numpy(batch))
    twin.set_history(model.history)
    a = model.recommend_with_scores(torch.from_numpy(batch), k=12)
    b = twin.recommend_with_scores(torch.from_numpy(batch), k=12)
    assert torch.equal(a[1], b[1]) and np.array_equal(bits(a[0]), bits(b[0]))


# ------------------------------------------------------------------ serving, evaluation
def test_serving_item_cf_baskets_and_back_fill():
    U, I, _ = S1
    users, items, (ptr, idx) = small(S1)
    hist = {u: set(idx[ptr[u]:ptr[u + 1]].tolist()) for u in range(U) if ptr[u + 1] > ptr[u]}
    srv = Recommender(U, I, device=DEV)
    m = srv.add_item_cf(users, items, num_neighbors=2, shrink=1.0)
    assert isinstance(m, ItemCF) and srv.models["item_cf"] is m and m.num_neighbors == 2
    assert srv._device_history() is m.history               # none was set: the model's own
    ask = [3, 10 ** 6, 17, 3]
    k = 30
    wv, wi = m.recommend_with_scores(torch.tensor([3, 17, 3]), filter_items=m.history, k=k)
    wv, wi = wv.cpu().tolist(), wi.cpu().tolist()
    assert all(row[-1] < 0 <= row[0] for row in wi)          # N = 2: every row is short
    out = srv.get_batch_recommendations(ask, model_name="item_cf", num_items=k,
                                        include_scores=True)
    assert out[1] == {"user_id": 10 ** 6, "error": "user 1000000 not found"}
    for r, j in enumerate((0, 2, 3)):                        # no baseline: no back-fill
        n = sum(i >= 0 for i in wi[r])
        assert out[j]["model_name"] == "item_cf" and out[j]["user_id"] == ask[j]
        assert [x["article_id"] for x in out[j]["recommendations"]] == [str(i) for i in wi[r][:n]]
        assert [x["score"] for x in out[j]["recommendations"]] == wv[r][:n]
    one = srv.get_recommendations(17, model_name="item_cf", num_items=k, include_scores=True)
    assert [x["article_id"] for x in one["recommendations"]] == \
        [x["article_id"] for x in out[2]["recommendations"]]
    # a basket: the visitor without a user index
    basket = sorted(hist[17])
    bv, bi = m.recommend_for_items([basket], k=k)
    got = srv.get_recommendations_for_items(reversed(basket), num_items=k, include_scores=True)
    n = int((bi[0] >= 0).sum())
    assert got["model_name"] == "item_cf" and got["user_id"] is None and 0 < n < k
    assert [x["article_id"] for x in got["recommendations"]] == [str(i) for i in bi[0, :n].tolist()]
    assert [x["article_id"] for x in got["recommendations"]] == \
        [x["article_id"] for x in one["recommendations"]]    # the user's history as a basket
    with pytest.raises(ValueError):
        srv.get_recommendations_for_items([I])
    with pytest.raises(ValueError):
        srv.get_recommendations_for_items([1], num_items=0)
    with pytest.raises(ValueError):
        srv.get_recommendations_for_items([1], model_name="nope")
    # with a baseline registered short rows are continued from the popularity list
    base = srv.add_popularity_baseline(items)
    pv, pi = base.recommend_with_scores(torch.tensor([3, 17, 3]), filter_items=m.history, k=k)
    pv, pi = pv.cpu().tolist(), pi.cpu().tolist()
    out = srv.get_batch_recommendations(ask, model_name="item_cf", num_items=k,
                                        include_scores=True)
    filled = 0
    for r, j in enumerate((0, 2, 3)):
        ev, ei = host_back_fill(wv[r], wi[r], pv[r], pi[r])
        recs = out[j]["recommendations"]
        assert out[j]["model_name"] == "item_cf" and len(recs) == k == len(set(ei))
        assert [x["article_id"] for x in recs] == [str(i) for i in ei]
        assert [x["score"] for x in recs] == ev
        assert not set(ei) & hist[ask[j]]
        filled += k - sum(i >= 0 for i in wi[r])
    assert filled > 0
    got = srv.get_recommendations_for_items(basket, num_items=k)
    assert len(got["recommendations"]) == k and got["recommendations"][0]["score"] is None
    assert [x["article_id"] for x in got["recommendations"]] == \
        [x["article_id"] for x in out[2]["recommendations"]]
    with pytest.raises(ValueError, match="basket"):
        srv.get_recommendations_for_items([1], model_name="popularity_baseline")


def test_checkpoint_dispatch_builds_item_cf():
    U, I, _ = S1
    users, items, (ptr, idx) = small(S1)
    src = fit_model(users, items, U, I, 16, 10.0)
    hp = dict(src.hparams)
    hp["num_users"], hp["num_items"] = 1, 1
    ck = {"state_dict": src.state_dict(), "hyper_parameters": hp}
    m = create_model_from_checkpoint("runs/item_cf", ck, U, I, DEV)
    assert type(m) is ItemCF and m.num_neighbors == 16 and m.shrink == 10.0 and not m.training
    assert torch.equal(m.neighbor_idx, src.neighbor_idx)
    hist = {u: set(idx[ptr[u]:ptr[u + 1]].tolist()) for u in range(U) if ptr[u + 1] > ptr[u]}
    srv = Recommender(U, I, models={"item_cf": m}, device=DEV, user_history=hist)
    assert m.history is None                                 # set from the recommender's
    got = srv.get_recommendations(5, model_name="item_cf", num_items=12)
    want = src.recommend_with_scores(torch.tensor([5]), filter_items=src.history, k=12)[1][0]
    want = [str(i) for i in want.tolist() if i >= 0]
    assert [x["article_id"] for x in got["recommendations"]] == want and len(want) > 0


def test_evaluate_model_and_validation_hooks():
    model, ref, hist, batch, rows, scores = big()
    users = np.unique(batch)
    rng = np.random.Generator(np.random.PCG64(5))
    top = model.recommend_with_scores(torch.from_numpy(users), filter_items=model.history,
                                      k=12)[1].cpu().numpy()
    truth = {}
    for r, u in enumerate(users):
        t = set(rng.choice(NI, size=int(rng.integers(1, 6)), replace=False).tolist())
        if r % 2 == 0 and top[r, 2] >= 0:
            t.add(int(top[r, 2]))
        truth[int(u)] = sorted(t)
    assert (top < 0).any()                                   # short lists are part of the case
    want = evaluate_recommendations({int(u): top[r].tolist() for r, u in enumerate(users)},
                                    truth, k=12, device=DEV)
    tp, ti = truth_csr(users.tolist(), truth, DEV)
    got = evaluate_model(model, torch.from_numpy(users), tp, ti, k=12, batch_size=100,
                         filter_items=model.history)
    for name in ("map@12", "recall@12", "precision@12", "ndcg@12"):
        assert got[name] == pytest.approx(float(want[name]), rel=1e-12), name
    assert got["map@12"] > 0
    pad = max(len(t) for t in truth.values())
    gt = np.full((len(users), pad), -1, np.int64)
    for r, u in enumerate(users):
        gt[r, :len(truth[int(u)])] = truth[int(u)]
    model.validation_step({"user_ids": torch.from_numpy(users).to(DEV),
                           "ground_truth": torch.from_numpy(gt).to(DEV)}, 0)
    model.on_validation_epoch_end()
    assert float(model.logged_metrics["val_map_at_k"]) == pytest.approx(float(want["map@12"]),
                                                                        rel=2.0 ** -22)
