"""CPU-side checks of the weighted ImplicitALS (no GPU): the declared entry, UserHistory's pair
weights, the validation of weights / days_ago / time_decay, no CPU path for the new keywords,
serving's refusal of item weights for another model, and the sanity of the weighted float64
oracle the GPU tests compare against."""
import numpy as np
import pytest
import torch

import wals_oracle as WO
from hnm_recommendation_amd import ImplicitALS, NeuralCF, UserHistory, _lib
from hnm_recommendation_amd import synthetic as syn
from hnm_recommendation_amd.serving import Recommender


def test_weighted_entry_is_declared_and_exported():
    assert "hnm_als_solve_rows_weighted_f32" in _lib.declared_symbols()
    assert hasattr(_lib.load(), "hnm_als_solve_rows_weighted_f32")
    # the arguments of hnm_als_solve_rows_f32 plus one pointer (w, after idx)
    plain = _lib._SIGS["hnm_als_solve_rows_f32"][1]
    weighted = _lib._SIGS["hnm_als_solve_rows_weighted_f32"][1]
    assert weighted == plain[:3] + [_lib._p] + plain[3:]


def interactions_with_weights(seed=3):
    U, I = 40, 30
    users, items = syn.interactions(U, I, 400, seed=seed)      # many repeated pairs
    rng = np.random.default_rng(seed)
    w = rng.integers(1, 9, len(users)) * np.exp(-0.01 * rng.integers(0, 366, len(users)))
    return U, I, users, items, w


def test_pair_weights_are_the_float64_grouped_sums():
    U, I, users, items, w = interactions_with_weights()
    ptr, idx, w64 = WO.pair_weights(users, items, w, U, I)
    assert len(idx) < len(users)                               # duplicates were merged
    h = UserHistory.from_interactions(users, items, U, I, "cpu", weights=w)
    assert h.hist_w.dtype == torch.float32 and h.hist_w.shape == h.hist_idx.shape
    assert np.array_equal(h.hist_ptr.numpy(), ptr) and np.array_equal(h.hist_idx.numpy(), idx)
    assert np.array_equal(h.hist_w.numpy(), w64.astype(np.float32))
    # everything else is what the unweighted constructor builds
    plain = UserHistory.from_interactions(users, items, U, I, "cpu")
    assert plain.hist_w is None
    assert torch.equal(plain.hist_ptr, h.hist_ptr) and torch.equal(plain.hist_idx, h.hist_idx)
    assert (plain.nnz, plain.max_len) == (h.nnz, h.max_len)
    assert UserHistory({0: {1, 2}}, U, I, "cpu").hist_w is None
    # a torch tensor of weights is taken too
    ht = UserHistory.from_interactions(users, items, U, I, "cpu", weights=torch.from_numpy(w))
    assert torch.equal(ht.hist_w, h.hist_w)


def test_pair_weights_do_not_depend_on_the_order_of_the_transactions():
    U, I, users, items, w = interactions_with_weights(seed=5)
    # weights whose float64 sum depends on the order they are added in
    w = w * np.random.default_rng(1).choice([1e-9, 1.0, 1e9], len(w))
    a = UserHistory.from_interactions(users, items, U, I, "cpu", weights=w)
    for seed in range(3):
        p = np.random.default_rng(seed).permutation(len(users))
        b = UserHistory.from_interactions(users[p], items[p], U, I, "cpu", weights=w[p])
        assert torch.equal(a.hist_idx, b.hist_idx)
        assert np.array_equal(a.hist_w.numpy().view(np.int32), b.hist_w.numpy().view(np.int32))


def test_bad_weights_raise():
    u, i = np.array([0, 1, 1]), np.array([2, 3, 3])
    for w in ([1.0, -0.5, 1.0], [1.0, float("nan"), 1.0], [1.0, float("inf"), 1.0],
              [1.0, 1.0], [[1.0, 1.0, 1.0]]):
        with pytest.raises(ValueError):
            UserHistory.from_interactions(u, i, 4, 5, "cpu", weights=w)
    h = UserHistory.from_interactions(u, i, 4, 5, "cpu", weights=[0.0, 0.0, 2.5])   # 0 is legal
    assert h.hist_w.tolist() == [0.0, 2.5]
    e = UserHistory.from_interactions(u[:0], i[:0], 4, 5, "cpu", weights=[])
    assert e.nnz == 0 and e.hist_w is not None


def test_days_ago_and_time_decay_validation():
    f = ImplicitALS._interaction_weights
    assert f(3, None, None, 0.0) is None and f(3, None, None, 0.5) is None
    days = np.array([0, 10, 365])
    assert np.array_equal(f(3, None, days, 0.01), np.exp(-0.01 * days.astype(np.float64)))
    assert np.array_equal(f(3, [2, 1, 3], days, 0.01),
                          np.array([2.0, 1.0, 3.0]) * np.exp(-0.01 * days.astype(np.float64)))
    assert np.array_equal(f(3, [2, 1, 3], None, 0.01), np.array([2.0, 1.0, 3.0]))
    assert np.array_equal(f(3, None, torch.tensor([0.0, 10.0, 365.0]), 0.01),
                          np.exp(-0.01 * days.astype(np.float64)))     # whole days as floats
    for kw in ({"days_ago": days, "time_decay": -0.1},
               {"days_ago": days, "time_decay": float("nan")},
               {"days_ago": np.array([0, -1, 3]), "time_decay": 0.1},
               {"days_ago": np.array([0.0, 1.5, 3.0]), "time_decay": 0.1},
               {"days_ago": np.array([0.0, float("nan"), 3.0]), "time_decay": 0.1},
               {"days_ago": np.array([0, 1]), "time_decay": 0.1},
               {"weights": [1.0, 2.0], "time_decay": 0.0}):
        with pytest.raises(ValueError):
            f(3, kw.get("weights"), kw.get("days_ago"), kw["time_decay"])


def test_no_cpu_path_for_the_new_keywords():
    m = ImplicitALS(30, 20, embedding_dim=16)
    u, i = syn.interactions(30, 20, 100, seed=1)
    w = np.ones(len(u))
    with pytest.raises(RuntimeError, match="no CPU path|GPU"):
        m.fit_interactions(u, i, weights=w)
    with pytest.raises(RuntimeError, match="no CPU path|GPU"):
        m.fit_interactions(u, i, days_ago=np.zeros(len(u), np.int64), time_decay=0.01)
    with pytest.raises(RuntimeError, match="no CPU path|GPU"):
        m.fit_history(UserHistory.from_interactions(u, i, 30, 20, "cpu", weights=w))
    with pytest.raises(RuntimeError, match="no CPU path|GPU"):
        m.user_factors([[1, 2]], [[1.0, 3.0]])
    with pytest.raises(RuntimeError, match="no CPU path|GPU"):
        m.recommend_for_items([[1, 2]], weights=[[1.0, 3.0]])
    srv = Recommender(30, 20, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU path|GPU"):
        srv.add_als(u, i, weights=w, embedding_dim=16)
    with pytest.raises(RuntimeError, match="no CPU path|GPU"):
        srv.add_als(u, i, days_ago=np.zeros(len(u), np.int64), time_decay=0.01, embedding_dim=16)


def test_serving_refuses_item_weights_for_another_model():
    srv = Recommender(30, 20, device="cpu")
    srv.add_model("neural_cf", NeuralCF(30, 20))
    with pytest.raises(ValueError):
        srv.get_recommendations_for_items([1, 2], model_name="neural_cf", item_weights=[1.0, 2.0])
    from hnm_recommendation_amd import ItemCF
    srv.add_model("item_cf", ItemCF(30, 20))
    with pytest.raises(ValueError, match="item weights"):
        srv.get_recommendations_for_items([1, 2], model_name="item_cf", item_weights=[1.0, 2.0])


@pytest.mark.parametrize("alpha,reg", [(10.0, 0.1), (40.0, 0.01)])
def test_weighted_oracle_half_step_zeroes_the_weighted_gradient(alpha, reg):
    """The weighted oracle's half-steps are the exact minimisers of the weighted L in their own
    block: dL/dX = 0 after the user step, dL/dY = 0 after the item step (float64, relative to
    the gradient before); with unit weights the oracle is the unweighted one."""
    import als_oracle as AO
    U, I, d = 40, 30, 8
    users, items = syn.interactions(U, I, 300, seed=4)
    keep = (users % 7 != 0) & (items % 11 != 0)                # empty users and empty items
    users, items = users[keep], items[keep]
    rng = np.random.default_rng(0)
    tw = rng.integers(1, 9, len(users)) * np.exp(-0.01 * rng.integers(0, 366, len(users)))
    tw[::9] = 0.0                                              # some zero-weight transactions
    ptr, idx, w = WO.pair_weights(users, items, tw, U, I)
    assert (w == 0).any() and w.max() > 4
    tptr, tidx, twt = WO.transpose(ptr, idx, w, U, I)
    Y = rng.normal(0, 0.1, (I, d))
    X0 = rng.normal(0, 0.1, (U, d))
    g0 = np.abs(WO.grad_users(X0, Y, ptr, idx, w, alpha, reg)).max()
    X = WO.half_step(ptr, idx, w, Y, alpha, reg)
    g = WO.grad_users(X, Y, ptr, idx, w, alpha, reg)
    nonempty = np.diff(ptr) > 0
    assert np.abs(g[nonempty]).max() <= 1e-10 * g0
    assert not X[~nonempty].any() and (~nonempty).sum() >= 5
    # it is not the unweighted minimiser
    assert np.abs(AO.grad_users(X, Y, ptr, idx, alpha, reg)[nonempty]).max() > 1e-3 * g0
    Y1 = WO.half_step(tptr, tidx, twt, X, alpha, reg)
    gy = WO.grad_users(Y1, X, tptr, tidx, twt, alpha, reg)
    assert np.abs(gy[np.diff(tptr) > 0]).max() <= 1e-10 * g0
    l0 = WO.loss_dense(X0, Y, ptr, idx, w, alpha, reg)
    l1 = WO.loss_dense(X, Y, ptr, idx, w, alpha, reg)
    l2 = WO.loss_dense(X, Y1, ptr, idx, w, alpha, reg)
    assert l2 < l1 < l0
    # unit weights: the unweighted oracle
    one = np.ones(len(idx))
    assert np.allclose(WO.half_step(ptr, idx, one, Y, alpha, reg),
                       AO.half_step(ptr, idx, Y, alpha, reg), rtol=1e-12, atol=1e-14)
    assert WO.loss_dense(X, Y, ptr, idx, one, alpha, reg) == pytest.approx(
        AO.loss_dense(X, Y, ptr, idx, alpha, reg), rel=1e-13)
