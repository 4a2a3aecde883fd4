"""Ensemble without a GPU: the oracle of hnm_fuse_topk_f32 (fuse_oracle.py) on a hand-worked
example, the rank table, the constructor's validation and the host side of
`Recommender.add_ensemble`."""
import numpy as np
import pytest
import torch

import fuse_oracle as FO
from hnm_recommendation_amd import (Ensemble, ItemCF, MatrixFactorization, NeuralCF,
                                    PopularityBaseline)
from hnm_recommendation_amd.serving import Recommender

INF, NAN = float("inf"), float("nan")

# one row, G = 2 lists of kc = 5 entries over 10 items.  List 0 ends in an idx = -1 entry and an
# entry whose val is -inf; list 1 holds an entry whose val is nan (item 9: empty) and one whose
# id is out of range (10: raises the error word, skipped).  Items 3 and 5 stand in both lists.
IDX = np.array([[[3, 5, 7, -1, 2]], [[5, 3, 8, 9, 10]]], np.int64)            # [G, B = 1, kc]
VAL = np.array([[[0.75, 0.5, 0.125, -INF, -INF]], [[2.0, 1.0, -1.0, NAN, 0.25]]], np.float32)


def _lists(out):
    v, i, full, oob = out
    return [(float(a), int(b)) for a, b in zip(v[0], i[0])], oob


def test_oracle_rank_hand_example():
    coef = np.array([[4, 2, 1, 0.5, 0.25]] * 2, np.float32)     # a made-up rank discount
    # 3: 4 (rank 1 of list 0) + 2 (rank 2 of list 1) = 6;  5: 2 + 4 = 6: a tie, item 3 first;
    # 7: 1 (list 0), 8: 1 (list 1): a tie, item 7 first; 2, 9, -1 are empty, 10 out of range
    got, oob = _lists(FO.fuse(VAL, IDX, FO.RANK, coef, 10, 6))
    assert got == [(6.0, 3), (6.0, 5), (1.0, 7), (1.0, 8), (-INF, -1), (-INF, -1)]
    assert oob
    # the cut at k takes the order's head
    assert _lists(FO.fuse(VAL, IDX, FO.RANK, coef, 10, 3))[0] == [(6.0, 3), (6.0, 5), (1.0, 7)]
    # with 11 items the last entry of list 1 is item 10 at rank 5: 0.25
    got, oob = _lists(FO.fuse(VAL, IDX, FO.RANK, coef, 11, 5))
    assert got == [(6.0, 3), (6.0, 5), (1.0, 7), (1.0, 8), (0.25, 10)] and not oob


def test_oracle_score_hand_example():
    coef = np.array([1.0, 0.5], np.float32)
    # 3: 0.75 + 0.5 * 1.0 = 1.25;  5: 0.5 + 0.5 * 2.0 = 1.5;  7: 0.125;  8: 0.5 * -1.0 = -0.5
    # (negative scores are listed: there is no score > 0 condition)
    got, _ = _lists(FO.fuse(VAL, IDX, FO.SCORE, coef, 10, 5))
    assert got == [(1.5, 5), (1.25, 3), (0.125, 7), (-0.5, 8), (-INF, -1)]
    # the CSR mask of the row removes item 5
    mptr, midx = np.array([0, 2], np.int64), np.array([5, 6], np.int32)
    got, _ = _lists(FO.fuse(VAL, IDX, FO.SCORE, coef, 10, 5, mptr, midx))
    assert got == [(1.25, 3), (0.125, 7), (-0.5, 8), (-INF, -1), (-INF, -1)]


def test_oracle_score_sums_in_ascending_g_from_the_first_term():
    """fp32, ascending g, from the first contribution: (1e8 + 1) - 1e8 is 0 in that order (1e8 +
    1 rounds to 1e8) and would be 1 in any other; and a single contribution of -0.0 stays -0.0
    (a sum started from 0.0f would give +0.0)."""
    idx = np.array([[[4, 6]], [[4, -1]], [[4, -1]]], np.int64)
    val = np.array([[[1e8, -0.0]], [[1.0, 0.0]], [[-1e8, 0.0]]], np.float32)
    v, i, _, _ = FO.fuse(val, idx, FO.SCORE, np.ones(3, np.float32), 10, 2)
    assert i[0].tolist() == [4, 6]
    assert v[0, 0] == 0.0 and not np.signbit(v[0, 0])
    assert v[0, 1] == 0.0 and np.signbit(v[0, 1])


def test_oracle_cascade_hand_example():
    # list 0 in its order (3, 5, 7), then what list 1 adds (8), each with the val of its first
    # occurrence: 5 and 3 keep list 0's values
    got, oob = _lists(FO.fuse(VAL, IDX, FO.CASCADE, None, 10, 5))
    assert got == [(0.75, 3), (0.5, 5), (0.125, 7), (-1.0, 8), (-INF, -1)] and oob
    mptr, midx = np.array([0, 1], np.int64), np.array([3], np.int32)
    got, _ = _lists(FO.fuse(VAL, IDX, FO.CASCADE, None, 10, 2, mptr, midx))
    assert got == [(0.5, 5), (0.125, 7)]


def _members(I=40):
    return [("mf", MatrixFactorization(30, I)), ("popularity", PopularityBaseline(n_items=I))]


def test_rank_weights_hand_values():
    e = Ensemble(_members(), weights=[1.0, 2.0], rank_constant=60.0, depth=3)
    w = e.rank_weights().numpy()
    assert w.dtype == np.float32 and w.shape == (2, 3)
    f = np.float32
    assert w.tolist() == [[f(1) / f(61), f(1) / f(62), f(1) / f(63)],
                          [f(2) / f(61), f(2) / f(62), f(2) / f(63)]]
    np.testing.assert_allclose(w[0], [0.01639344, 0.01612903, 0.01587302], rtol=1e-6)
    assert np.array_equal(w, FO.rank_table([1.0, 2.0], 60.0, 3))
    # the default depth: max(k, 4 * top_k) clamped to num_items; rank_weights(depth) any depth
    assert Ensemble(_members(), top_k=12).rank_weights().shape == (2, 40)
    assert Ensemble(_members(), top_k=5).rank_weights().shape == (2, 20)
    assert e.rank_weights(7).shape == (2, 7)
    assert Ensemble(_members(), rank_constant=0.0).rank_weights(2).tolist() == [[1.0, 0.5]] * 2


def test_constructor_validation():
    with pytest.raises(ValueError, match="mode"):
        Ensemble(_members(), mode="borda")
    for bad in ([1.0], [1.0, 2.0, 3.0], [1.0, 0.0], [1.0, -2.0], [1.0, float("nan")],
                [float("inf"), 1.0]):
        with pytest.raises(ValueError, match="weights"):
            Ensemble(_members(), weights=bad)
    with pytest.raises(ValueError, match="distinct"):
        Ensemble([("a", MatrixFactorization(30, 40)), ("a", PopularityBaseline(n_items=40))])
    with pytest.raises(ValueError, match="num_items"):
        Ensemble([("a", MatrixFactorization(30, 40)), ("b", PopularityBaseline(n_items=41))])
    for bad in (0, -3):
        with pytest.raises(ValueError, match="depth"):
            Ensemble(_members(), depth=bad)
    with pytest.raises(ValueError, match="depth"):
        Ensemble(_members(), depth=513)
    with pytest.raises(ValueError):
        Ensemble([])
    with pytest.raises(ValueError, match="rank_constant"):
        Ensemble(_members(), rank_constant=-1.0)


def test_surface_from_the_members():
    """An ordered dict or a list of pairs; state_dict keys members.<name>.…; what the
    Recommender asks is derived from the members."""
    mf, icf, pop = MatrixFactorization(30, 40), ItemCF(30, 40), PopularityBaseline(n_items=40)
    e = Ensemble({"mf": mf, "item_cf": icf, "popularity": pop}, mode="score", top_k=7)
    assert list(e.members) == ["mf", "item_cf", "popularity"] and e.members["item_cf"] is icf
    keys = set(e.state_dict())
    assert "members.mf.user_embeddings.weight" in keys and "members.item_cf.neighbor_idx" in keys
    assert e.num_items == 40 and e.num_users == 30 and e.top_k == 7 and e.metrics.top_k == 7
    assert e.hparams["members"] == ["mf", "item_cf", "popularity"] and e.hparams["mode"] == "score"
    assert not e.answers_baskets and e.back_fill_short_rows and not e.takes_basket_weights
    assert Ensemble([("item_cf", icf)]).answers_baskets
    assert not Ensemble([("mf", mf), ("popularity", pop)]).back_fill_short_rows
    with pytest.raises(NotImplementedError, match="basket"):
        e.recommend_for_items([[1, 2]])
    # k > 128 is refused before any launch (so also without a GPU), top_k > num_items too
    with pytest.raises(ValueError, match="128"):
        Ensemble([("mf", MatrixFactorization(30, 400))]).recommend_with_scores(
            torch.tensor([0]), k=129)
    with pytest.raises(RuntimeError, match="out of range"):
        Ensemble(_members(), top_k=41).recommend(torch.tensor([0]))
    with pytest.raises(RuntimeError, match="no CPU path|GPU"):
        e.recommend_with_scores(torch.tensor([0]))


def test_predict_all_items_raises():
    with pytest.raises(NotImplementedError, match="dense"):
        Ensemble(_members()).predict_all_items(torch.tensor([0]))


def test_history_is_the_first_members_and_set_history_fills_the_empty_ones():
    from hnm_recommendation_amd import UserHistory
    icf_a, icf_b, pop = ItemCF(6, 10), ItemCF(6, 10), PopularityBaseline(n_items=10)
    e = Ensemble([("popularity", pop), ("a", icf_a), ("b", icf_b)])
    assert e.history is None
    h1, h2 = UserHistory({1: {2}}, 6, 10, "cpu"), UserHistory({2: {3}}, 6, 10, "cpu")
    icf_b.set_history(h1)
    assert e.history is h1
    e.set_history(h2)                      # a has none and takes it; b keeps its own; pop has no
    assert icf_a.history is h2 and icf_b.history is h1 and pop.history is None   # set_history
    assert e.history is h2


def test_add_ensemble_host_logic():
    srv = Recommender(100, 50, device="cpu")
    srv.add_model("neural_cf", NeuralCF(100, 50), {"test_map": 0.2})
    srv.add_model("mf", MatrixFactorization(100, 50))
    with pytest.raises(ValueError, match="nope"):
        srv.add_ensemble(["mf", "nope"])
    assert "ensemble" not in srv.models
    best = srv._get_best_model()
    e = srv.add_ensemble(["mf", "neural_cf"], weights=[2.0, 1.0], mode="score", depth=20)
    assert srv.models["ensemble"] is e and list(e.members) == ["mf", "neural_cf"]
    assert e.weights == [2.0, 1.0] and e.mode == "score" and e.depth == 20
    assert srv.model_metrics["ensemble"] == {} and srv._get_best_model() == best
    srv.add_ensemble(["mf"], name="solo")
    assert list(srv.models["solo"].members) == ["mf"]
    with pytest.raises(ValueError, match="basket"):
        srv.get_recommendations_for_items([1, 2], model_name="ensemble")


@pytest.mark.parametrize("num_items", [300, 50_000])
def test_seeded_gpu_cases_provide_what_the_gpu_test_asserts(num_items):
    """The smallest tie-bearing case of test_gpu_ensemble.py, counted with the oracle alone: exact
    ties among the first k + 1 places in RANK mode, short and full rows, a negative selected
    score in SCORE mode, fully empty rows, rows of identical lists, empty mask rows."""
    import fuse_cases as FC
    G, kc, k = 2, 12, 12
    vals, idxs = FC.lists(G, kc, num_items)
    assert all((idxs[:, b] < 0).all() for b in FC.EMPTY_ROWS)
    assert all((idxs[:, b] == idxs[0, b]).all() for b in FC.SAME_ROWS)
    assert (idxs == -1).any() and np.isnan(vals).any() and np.isneginf(vals[idxs >= 0]).any()
    rank = FC.reference(FO.RANK, G, kc, num_items)
    assert FC.tie_rows(rank, k) >= 50
    count = FO.cut(rank, k)[2]
    assert (count < k).any() and (count >= k).any()
    score = FO.cut(FC.reference(FO.SCORE, G, kc, num_items), k)[0]
    assert (score[np.isfinite(score)] < 0).any()
    mp, mi = FC.mask(G, kc, num_items)
    assert (np.diff(mp) == 0).any()
    for b in range(FC.B):                                  # mask rows ascending and unique
        row = mi[mp[b]:mp[b + 1]]
        assert (np.diff(row) > 0).all()
    assert (FO.cut(rank, k, mp, mi)[1] != FO.cut(rank, k)[1]).any()
