"""GPU: ImplicitALS -- hnm_als_gram_f32 / hnm_als_solve_rows_f32, the fit, fold-in and serving.

There is no reference implementation: everything is compared with the float64 numpy restatement
of the contract (include/hnm.h) in als_oracle.py.

* Gram: entrywise |G - G64| <= gamma_n (|T|^T |T|), gamma_n = n u / (1 - n u), u = 2^-24, n = rows
  -- the standard dot-product bound, valid for any summation order.
* Solve: err = max_rows |x - x64|_inf / |x64|_inf against the float64 oracle; the yardstick is
  scipy.linalg.solve(A32, b32, assume_a="pos") (LAPACK's fp32 Cholesky, on the CPU) on the
  fp32-formed system: err_kernel <= 4 * err_lapack32.  Why 4x: an independent plain fp32
  Cholesky with another summation order lands at 0.90-1.16x of LAPACK's error on these inputs;
  4x leaves room for the MFMA update order and the factorisation order without admitting a
  wrong solve.  Measured ratios: profiles/als_accuracy.txt.
* Fit: X and Y after each of 3 sweeps against the float64 oracle run from the same initial Y, at
  the project's 1e-4-of-row-scale bar (parity.assert_scores_close).
"""
import functools

import numpy as np
import pytest
import scipy.linalg
import torch

import als_oracle as AO
from als_raw import (ALPHA, DEV, FI, FU, REG, bits, dev, new_model, raw_solve, rel_err, strided,
                     tables)
from hnm_recommendation_amd import (ImplicitALS, MatrixFactorization, NeuralCF, UserHistory,
                                    _lib)
from hnm_recommendation_amd import synthetic as syn
from hnm_recommendation_amd.evaluation import evaluate_model, truth_csr
from hnm_recommendation_amd.serving import (Recommender, create_model_from_checkpoint,
                                            load_checkpoint)
from parity import assert_scores_close

pytestmark = pytest.mark.gpu
GRAM_ROWS = 2048          # hnm.h: rows per Gram partial


def raw_gram(buf, rows, d):
    out = torch.full((d, d), float("nan"), dtype=torch.float32, device=DEV)
    st = _lib.fn("hnm_als_gram_f32")(_lib.ctx(DEV), _lib.ptr(buf), rows, buf.stride(0), d,
                                     _lib.ptr(out))
    return st, out


# ------------------------------------------------------------------ Gram
@pytest.mark.parametrize("d", [16, 64, 128])
@pytest.mark.parametrize("rows", [1, 63, 2 * GRAM_ROWS + 1])
def test_gram_within_the_dot_product_bound(rows, d):
    rng = np.random.default_rng(rows * 1000 + d)
    T = rng.normal(0, 1.0, (rows, d)).astype(np.float32)
    buf = strided(T, d + 5)
    st, G = raw_gram(buf, rows, d)
    assert st == _lib.HNM_OK
    _lib.sync_check(DEV)
    G = G.cpu().numpy()
    T64 = T.astype(np.float64)
    G64 = T64.T @ T64
    u = 2.0 ** -24
    gamma = rows * u / (1 - rows * u)
    err = np.abs(G - G64)
    bound = gamma * (np.abs(T64).T @ np.abs(T64))
    print(f"gram rows={rows} d={d}: max err/bound = {(err / bound).max():.3f}")
    assert (err <= bound).all()
    assert np.array_equal(bits(G), bits(G.T))                # exactly symmetric
    st, G2 = raw_gram(buf, rows, d)
    assert np.array_equal(bits(G2), bits(G))                 # the same bits on a second run


def test_gram_of_no_rows_is_zero_and_bad_d_is_refused():
    buf = torch.zeros(4, 64, device=DEV)
    st, G = raw_gram(buf, 0, 64)
    assert st == _lib.HNM_OK and not G.cpu().numpy().any()
    for d in (8, 24, 144):
        assert raw_gram(torch.zeros(4, 256, device=DEV), 4, d)[0] == _lib.HNM_EUNSUPPORTED
    out = torch.zeros(64, 64, device=DEV)
    assert _lib.fn("hnm_als_gram_f32")(_lib.ctx(DEV), _lib.ptr(buf), 4, 32, 64,
                                       _lib.ptr(out)) == _lib.HNM_EINVAL   # ld < d


# ------------------------------------------------------------------ solve
NI = 193
LENGTHS = [0, 1, 2, 5, 17, 64, 150, 193]


@functools.lru_cache(maxsize=None)
def solve_rows():
    """(ptr, idx): rows of the fixed lengths plus a dozen random ones below 40; each row is a
    random subset of the table in random (unsorted) order -- the stored order is the caller's."""
    rng = np.random.default_rng(11)
    lens = LENGTHS + rng.integers(0, 40, 12).tolist()
    rows = [rng.permutation(NI)[:n].astype(np.int32) for n in lens]
    ptr = np.zeros(len(rows) + 1, np.int64)
    np.cumsum(lens, out=ptr[1:])
    return ptr, np.concatenate(rows)


@functools.lru_cache(maxsize=None)
def solve_case(d, std, alpha, reg):
    """(T f32, x64 [rows, d], err_lapack32): the float64 oracle and the LAPACK fp32 yardstick,
    computed once on the CPU."""
    ptr, idx = solve_rows()
    rng = np.random.default_rng(d * 7 + int(std * 10))
    T = rng.normal(0, std, (NI, d)).astype(np.float32)
    x64 = AO.half_step(ptr, idx, T, alpha, reg)
    G32 = T.T @ T
    x32 = np.zeros_like(x64)
    for r in range(len(ptr) - 1):
        if ptr[r + 1] > ptr[r]:
            A, b = AO.system32(idx[ptr[r]:ptr[r + 1]], T, G32, alpha, reg)
            x32[r] = scipy.linalg.solve(A, b, assume_a="pos")
    return T, x64, rel_err(x32, x64)


def device_case(d, std, alpha, reg):
    ptr, idx = solve_rows()
    T, x64, e32 = solve_case(d, std, alpha, reg)
    buf = strided(T, d + 4)
    st, G = raw_gram(buf, NI, d)
    assert st == _lib.HNM_OK
    return dev(ptr), dev(idx), len(ptr) - 1, buf, G, x64, e32


@pytest.mark.parametrize("with_ids", [False, True])
@pytest.mark.parametrize("alpha,reg", [(10.0, 0.1), (40.0, 0.01)])
@pytest.mark.parametrize("std", [0.1, 1.0])
@pytest.mark.parametrize("d", [16, 64, 128])
def test_solve_is_as_accurate_as_lapack_fp32(d, std, alpha, reg, with_ids):
    ptr, idx, n, buf, G, x64, e32 = device_case(d, std, alpha, reg)
    if with_ids:   # permuted, with repeats
        rows = np.random.default_rng(5).permutation(np.r_[np.arange(n), [3, 3, 7, 0]])
        ids, B = dev(rows.astype(np.int64)), len(rows)
    else:
        rows, ids, B = np.arange(n), None, n
    ldo = d + 3
    st, out = raw_solve(ptr, idx, n, buf, NI, d, G, alpha, reg, ids, B, ldo)
    assert st == _lib.HNM_OK
    _lib.sync_check(DEV)
    full = out.cpu().numpy()
    assert (full[:, d:] == 7.0).all()                        # nothing written past d
    x = full[:, :d]
    assert np.isfinite(x).all()
    err = rel_err(x, x64[rows])
    print(f"solve d={d} std={std} alpha={alpha} reg={reg} ids={with_ids}: err_kernel={err:.3e} "
          f"err_lapack32={e32:.3e} ratio={err / e32:.2f}")
    assert err <= 4 * e32
    empty = np.diff(solve_rows()[0])[rows] == 0
    assert empty.any() and not bits(x[empty]).any()          # exact +0.0
    st, again = raw_solve(ptr, idx, n, buf, NI, d, G, alpha, reg, ids, B, ldo)
    assert np.array_equal(bits(again), bits(out))            # the same bits on a second run
    if with_ids:   # repeated rows agree, and a row's bits do not depend on the batch
        for r in (3, 7, 0):
            where = np.nonzero(rows == r)[0]
            assert len(where) >= 2
            assert all(np.array_equal(bits(x[w]), bits(x[where[0]])) for w in where)
        c = int(rows[2])
        st, alone = raw_solve(ptr, idx, n, buf, NI, d, G, alpha, reg,
                              dev(np.array([c], np.int64)), 1)
        assert np.array_equal(bits(alone[0, :d]), bits(x[2]))
        st, plain = raw_solve(ptr, idx, n, buf, NI, d, G, alpha, reg, None, n)
        assert np.array_equal(bits(plain[:, :d].cpu().numpy()[rows]), bits(x))


@pytest.mark.parametrize("d", [16, 128])
def test_solve_out_of_range_ids_give_nan_rows_and_eoob(d):
    alpha, reg = 10.0, 0.1
    ptr, idx, n, buf, G, x64, _ = device_case(d, 1.0, alpha, reg)
    st, clean = raw_solve(ptr, idx, n, buf, NI, d, G, alpha, reg, None, n)
    _lib.sync_check(DEV)
    clean = clean.cpu().numpy()
    hptr = solve_rows()[0]
    for victim, value in ((4, NI), (6, -1)):                 # rows of 17 and 150 entries
        bad = idx.clone()
        bad[int(hptr[victim]) + 3] = value
        st, out = raw_solve(ptr, bad, n, buf, NI, d, G, alpha, reg, None, n)
        assert st == _lib.HNM_OK
        with pytest.raises(IndexError):
            _lib.sync_check(DEV)
        out = out.cpu().numpy()
        assert np.isnan(out[victim]).all()
        others = np.arange(n) != victim
        assert np.array_equal(bits(out[others]), bits(clean[others]))
    ids = dev(np.array([0, n, 5, -1, 7], np.int64))
    st, out = raw_solve(ptr, idx, n, buf, NI, d, G, alpha, reg, ids, 5)
    assert st == _lib.HNM_OK
    with pytest.raises(IndexError):
        _lib.sync_check(DEV)
    out = out.cpu().numpy()
    assert np.isnan(out[[1, 3]]).all()
    assert np.array_equal(bits(out[[0, 2, 4]]), bits(clean[[0, 5, 7]]))
    _lib.sync_check(DEV)                                     # the error word was cleared


def test_solve_statuses():
    ptr, idx, n, buf, G, _, _ = device_case(64, 1.0, 10.0, 0.1)
    wide = torch.zeros(NI, 256, device=DEV)
    G2 = torch.zeros(256, 256, device=DEV)
    for d in (8, 24, 144):
        assert raw_solve(ptr, idx, n, wide, NI, d, G2, 10.0, 0.1, None, n)[0] \
            == _lib.HNM_EUNSUPPORTED
    nan, inf = float("nan"), float("inf")
    for alpha, reg in ((10.0, 0.0), (10.0, -1.0), (-1.0, 0.1), (nan, 0.1), (10.0, nan),
                       (inf, 0.1), (10.0, inf)):
        assert raw_solve(ptr, idx, n, buf, NI, 64, G, alpha, reg, None, n)[0] == _lib.HNM_EINVAL
    st, out = raw_solve(ptr, idx, n, buf, NI, 64, G, 10.0, 0.1, None, 0)
    assert st == _lib.HNM_OK and (out.cpu().numpy() == 7.0).all()
    st, out = raw_solve(ptr, idx, 0, buf, NI, 64, G, 10.0, 0.1, dev(np.zeros(2, np.int64)), 2)
    assert st == _lib.HNM_OK and (out.cpu().numpy() == 7.0).all()   # nothing launched
    assert raw_solve(ptr, idx, n, buf, NI, 64, G, 0.0, 0.1, None, n)[0] == _lib.HNM_OK
    _lib.sync_check(DEV)


# ------------------------------------------------------------------ fit
@functools.lru_cache(maxsize=None)
def fit_data():
    """Zipf-0.9 items, 0-30 items a user; users u % 17 == 0 and items i % 23 == 0 stay empty."""
    users, items = syn.interactions(FU, FI, 4500, seed=2)
    keep = (users % 17 != 0) & (items % 23 != 0)
    users, items = users[keep], items[keep]
    ptr, idx = AO.csr(users, items, FU, FI)
    lens = np.diff(ptr)
    tlens = np.diff(AO.transpose(ptr, idx, FU, FI)[0])
    assert lens.max() <= 30 and (lens == 0).sum() >= 18 and (tlens == 0).sum() >= 9
    assert tlens.max() > 4 * 32                              # a row of several gather images
    return users, items, ptr, idx


@functools.lru_cache(maxsize=None)
def fit_reference(d):
    _, _, ptr, idx = fit_data()
    Y0 = new_model(d).item_embeddings.weight.detach().cpu().numpy()
    return AO.sweeps(ptr, idx, FU, FI, Y0, ALPHA, REG, 3)


@functools.lru_cache(maxsize=None)
def fitted(d, iterations=3, seed=0):
    users, items, _, _ = fit_data()
    return new_model(d, seed).fit_interactions(users, items, iterations=iterations)


@pytest.mark.parametrize("d", [16, 64])
def test_fit_follows_the_float64_oracle_sweep_by_sweep(d):
    users, items, ptr, idx = fit_data()
    ref = fit_reference(d)
    for s in range(3):
        m = fitted(d, s + 1)
        X, Y = tables(m)
        assert_scores_close(X, ref[s][0], f"X after sweep {s + 1}")
        assert_scores_close(Y, ref[s][1], f"Y after sweep {s + 1}")
        assert np.abs(ref[s][0]).max() > 1.0 and np.abs(ref[s][1]).max() > 0.01
    # rows of empty users and items are exactly zero
    assert not bits(X[np.diff(ptr) == 0]).any()
    assert not bits(Y[np.arange(FI) % 23 == 0]).any()
    for k in ("user_bias.weight", "item_bias.weight", "global_bias"):
        assert not m.state_dict()[k].any()
    assert m.history is not None and m.history.nnz == ptr[-1]


@pytest.mark.parametrize("d", [16, 64])
def test_loss_is_the_dense_float64_loss_and_decreases(d):
    users, items, ptr, idx = fit_data()
    m = new_model(d).fit_interactions(users, items, iterations=4, track_loss=True)
    X, Y = tables(m)
    want = AO.loss_dense(X, Y, ptr, idx, ALPHA, REG)
    assert m.loss() == pytest.approx(want, rel=1e-9)
    h = m.loss_history
    print(f"loss history d={d}: {h}")
    assert len(h) == 4 and h[-1] == pytest.approx(want, rel=1e-9)
    assert all(b < a for a, b in zip(h, h[1:]))
    assert fitted(d, 3).loss_history == []                   # not tracked unless asked


def test_fit_is_reproducible_and_seeded():
    users, items, _, _ = fit_data()
    a = tables(fitted(64, 3))
    b = tables(new_model(64).fit_interactions(users, items, iterations=3))
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))
    c = tables(fitted(64, 3, seed=1))
    assert not np.array_equal(bits(a[0]), bits(c[0]))
    assert not np.array_equal(bits(a[1]), bits(c[1]))
    # a refit of the same module starts again from its seed
    m = new_model(64).fit_interactions(users, items, iterations=1)
    m.fit_interactions(users, items, iterations=3)
    assert np.array_equal(bits(tables(m)[1]), bits(a[1]))


# ------------------------------------------------------------------ module and serving
def test_recommend_equals_matrix_factorization_with_the_same_state():
    m = fitted(64)
    mf = MatrixFactorization(FU, FI, embedding_dim=64, sparse=False)
    mf.load_state_dict(m.state_dict())
    mf = mf.to(DEV).eval()
    users = torch.from_numpy(syn.user_batch(FU, 100, seed=3))
    for filt in (None, m.history):
        gv, gi = m.recommend_with_scores(users, filter_items=filt, k=12)
        wv, wi = mf.recommend_with_scores(users, filter_items=filt, k=12)
        assert torch.equal(gi, wi) and np.array_equal(bits(gv), bits(wv))
        assert (gi >= 0).all()
    assert torch.equal(m.recommend(users), gi_plain(m, users))
    assert np.array_equal(bits(m.predict_all_items(users[:8])), bits(mf.predict_all_items(users[:8])))


def gi_plain(m, users):
    return m.recommend_with_scores(users, k=m.top_k)[1]


def test_fold_in_equals_the_user_step_bitwise():
    users, items, ptr, idx = fit_data()
    m = new_model(64).fit_interactions(users, items, iterations=3)
    us = [1, 2, 17, 40, 123, 299]                            # 17: an empty user
    baskets = [idx[ptr[u]:ptr[u + 1]].tolist() for u in us]
    F = m.user_factors(baskets)
    assert F.shape == (len(us), 64)
    csr = (np.cumsum([0] + [len(b) for b in baskets]), np.concatenate(baskets).astype(np.int32))
    assert np.array_equal(bits(m.user_factors(csr)), bits(F))
    before = tables(m)[0]
    m.refresh_users(torch.tensor(us))                        # a fresh user step for those users
    after = tables(m)[0]
    assert np.array_equal(bits(after[us]), bits(F))
    assert not bits(F[2]).any()
    others = np.setdiff1d(np.arange(FU), us)
    assert np.array_equal(bits(after[others]), bits(before[others]))
    # the oracle's user step against the fitted Y
    want = AO.half_step(ptr, idx, tables(m)[1], ALPHA, REG, rows=us)
    assert_scores_close(F.cpu().numpy(), want, "fold-in")
    with pytest.raises(IndexError):
        m.user_factors([[FI]])
    with pytest.raises(IndexError):
        m.user_factors((np.array([0, 1]), np.array([FI], np.int32)))


def test_recommend_for_items_is_the_dot_topk_of_the_fold_in_vectors():
    m = fitted(64)
    baskets = [[3, 9, 50], [7], list(range(1, 40)), [], [199, 5]]
    F = m.user_factors(baskets)
    mf = MatrixFactorization(len(baskets), FI, embedding_dim=64, sparse=False)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    sd["user_embeddings.weight"] = F
    sd["user_bias.weight"] = torch.zeros(len(baskets), 1)
    mf.load_state_dict(sd)
    mf = mf.to(DEV).eval()
    rows = torch.arange(len(baskets))
    mask = {r: set(b) for r, b in enumerate(baskets)}
    for k in (12, 80):                                       # fused and dense (k > 64)
        for seen in (True, False):
            gv, gi = m.recommend_for_items(baskets, filter_seen=seen, k=k)
            wv, wi = mf.recommend_with_scores(rows, filter_items=mask if seen else None, k=k)
            assert torch.equal(gi, wi) and np.array_equal(bits(gv), bits(wv))
            assert gi.shape == (len(baskets), k) and (gi >= 0).all()
            assert torch.isfinite(gv).all()
            if seen:
                for r, b in enumerate(baskets):
                    assert not set(gi[r].tolist()) & set(b)
    gv, gi = m.recommend_for_items([list(range(FI - 5))], k=12)   # the mask leaves 5 items
    assert (gi[0, :5] >= FI - 5).all() and torch.isfinite(gv[0, :5]).all()
    assert (gv[0, 5:] == float("-inf")).all()                # the dot top-K's own convention
    assert m.recommend_for_items([], k=12)[1].shape == (0, 12)


def test_refresh_users_after_a_new_purchase_changes_exactly_those_users():
    users, items, ptr, idx = fit_data()
    m = new_model(64).fit_interactions(users, items, iterations=3)
    before = tables(m)[0]
    changed = [5, 17]                                        # 17 had no history
    new_items = []
    for u in changed:
        have = set(idx[ptr[u]:ptr[u + 1]].tolist())
        new_items.append(next(i for i in range(1, FI) if i not in have))
    h2 = UserHistory.from_interactions(np.r_[users, changed], np.r_[items, new_items], FU, FI, DEV)
    m.refresh_users(changed, history=h2)
    after = tables(m)[0]
    diff = np.nonzero((bits(after) != bits(before)).any(1))[0]
    assert diff.tolist() == changed
    want = AO.half_step(h2.hist_ptr.cpu().numpy(), h2.hist_idx.cpu().numpy(), tables(m)[1],
                        ALPHA, REG, rows=changed)
    assert_scores_close(after[changed], want, "refreshed users")
    with pytest.raises(IndexError):
        m.refresh_users([FU])


def test_checkpoint_round_trip_serves_the_same_lists(tmp_path):
    m = fitted(64)
    path = tmp_path / "implicit_als.ckpt"
    torch.save({"state_dict": m.state_dict(), "hyper_parameters": dict(m.hparams)}, path)
    got = create_model_from_checkpoint("runs/implicit_als", load_checkpoint(str(path)), FU, FI,
                                       DEV)
    assert type(got) is ImplicitALS and got.alpha == ALPHA and not got.training
    users = torch.arange(0, FU, 7)
    assert torch.equal(got.recommend(users), m.recommend(users))
    baskets = [[3, 9, 50], [7]]
    a, b = got.recommend_for_items(baskets), m.recommend_for_items(baskets)
    assert torch.equal(a[1], b[1]) and np.array_equal(bits(a[0]), bits(b[0]))
    # the fold-in cache follows a load
    m2 = new_model(64)
    m2.user_factors(baskets)
    m2.load_state_dict(m.state_dict())
    assert np.array_equal(bits(m2.user_factors(baskets)), bits(m.user_factors(baskets)))


def test_recommender_add_als_and_basket_requests():
    users, items, ptr, idx = fit_data()
    srv = Recommender(FU, FI, device=DEV)
    model = srv.add_als(users, items, embedding_dim=16, regularization=REG, alpha=ALPHA,
                        iterations=3)
    assert srv.models["implicit_als"] is model and srv._device_history() is model.history
    out = srv.get_batch_recommendations([1, 2, FU + 5], model_name="implicit_als", num_items=12,
                                        include_scores=True)
    assert "error" in out[2]
    for u, r in zip((1, 2), out):
        assert r["user_id"] == u and r["model_name"] == "implicit_als"
        ids = [int(x["article_id"]) for x in r["recommendations"]]
        assert len(ids) == 12 and not set(ids) & set(idx[ptr[u]:ptr[u + 1]].tolist())
        want = model.recommend_with_scores(torch.tensor([u]), filter_items=model.history, k=12)
        assert ids == want[1][0].tolist()
        assert [x["score"] for x in r["recommendations"]] == want[0][0].tolist()
    basket = [3, 9, 50]
    r = srv.get_recommendations_for_items(basket, num_items=10, model_name="implicit_als",
                                          include_scores=True)
    assert r["user_id"] is None and r["model_name"] == "implicit_als"
    ids = [int(x["article_id"]) for x in r["recommendations"]]
    assert len(ids) == 10 and not set(ids) & set(basket)
    assert ids == model.recommend_for_items([basket], k=10)[1][0].tolist()
    assert set(r["recommendations"][0]) == {"article_id", "product_name", "product_type_name",
                                            "product_group_name", "colour_group_name",
                                            "department_name", "score"}
    srv.add_model("neural_cf", NeuralCF(FU, FI))
    with pytest.raises(ValueError, match="cannot answer from a basket"):
        srv.get_recommendations_for_items(basket, model_name="neural_cf")
    with pytest.raises(ValueError):
        srv.get_recommendations_for_items([FI], model_name="implicit_als")


def test_evaluate_model_runs_on_the_fitted_model():
    users, items, ptr, idx = fit_data()
    m = fitted(64)
    rng = np.random.default_rng(5)
    us = np.array([u for u in range(0, FU, 3) if ptr[u + 1] > ptr[u]])
    truth = {int(u): sorted(set(rng.choice(FI, size=4, replace=False).tolist())) for u in us}
    tp, ti = truth_csr(us.tolist(), truth, DEV)
    got = evaluate_model(m, torch.from_numpy(us), tp, ti, k=12, batch_size=64,
                         filter_items=m.history)
    assert set(got) == {"map@12", "recall@12", "precision@12", "ndcg@12"}
    assert all(np.isfinite(v) and 0.0 <= v <= 1.0 for v in got.values())
    # fitted on the truth itself the model ranks it: far above a random list's precision
    seen = evaluate_model(m, torch.from_numpy(us), *truth_csr(
        us.tolist(), {int(u): idx[ptr[u]:ptr[u + 1]].tolist() for u in us}, DEV), k=12)
    assert seen["precision@12"] > 5 * 12 / FI * np.diff(ptr)[us].mean() / 12
