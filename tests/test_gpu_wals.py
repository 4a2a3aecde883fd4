"""GPU: the weighted ImplicitALS -- hnm_als_solve_rows_weighted_f32, the weighted fit, fold-in
and serving.

There is no reference implementation: everything is compared with the float64 numpy restatement
of the contract (include/hnm.h) in wals_oracle.py, or bit for bit with the unweighted entry.

* Identities: every weight 1 is hnm_als_solve_rows_f32's bits; every weight 2 (0.5) is its bits
  at twice (half) the alpha -- no tolerance.
* Accuracy: err = max_rows |x - x64|_inf / |x64|_inf against the float64 oracle; the yardstick
  is scipy.linalg.solve(A32, b32, assume_a="pos") on the fp32-formed system of the same row:
  err_kernel <= 4 * err_lapack32, test_gpu_als.py's bar.  Measured ratios:
  profiles/wals_accuracy.txt.
* Fit: X and Y after each of 3 sweeps against the float64 weighted oracle run from the same
  initial Y and the same fp32 pair weights, at the project's 1e-4-of-row-scale bar
  (parity.assert_scores_close).
"""
import functools

import numpy as np
import pytest
import scipy.linalg
import torch

import als_oracle as AO
import wals_oracle as WO
from als_raw import (ALPHA, DEV, FI, FU, REG, bits, dev, new_model, raw_solve, rel_err, strided,
                     tables)
from hnm_recommendation_amd import MatrixFactorization, UserHistory, _lib
from hnm_recommendation_amd import synthetic as syn
from hnm_recommendation_amd.serving import Recommender
from parity import assert_scores_close

pytestmark = pytest.mark.gpu


def raw_gram(buf, rows, d):
    out = torch.full((d, d), float("nan"), dtype=torch.float32, device=DEV)
    st = _lib.fn("hnm_als_gram_f32")(_lib.ctx(DEV), _lib.ptr(buf), rows, buf.stride(0), d,
                                     _lib.ptr(out))
    assert st == _lib.HNM_OK
    return out


def raw_wsolve(ptr, idx, w, n_rows, buf, tab_rows, d, gram, alpha, reg, row_ids, B, ldo=None):
    ldo = d if ldo is None else ldo
    out = torch.full((max(B, 1), ldo), 7.0, dtype=torch.float32, device=DEV)
    st = _lib.fn("hnm_als_solve_rows_weighted_f32")(
        _lib.ctx(DEV), _lib.ptr(ptr), _lib.ptr(idx), _lib.ptr(w), n_rows, _lib.ptr(buf), tab_rows,
        buf.stride(0), d, _lib.ptr(gram), alpha, reg, _lib.ptr(row_ids), B, _lib.ptr(out), ldo)
    return st, out


# ------------------------------------------------------------------ the raw entry
NI = 193
LENGTHS = [0, 1, 2, 5, 17, 31, 32, 33, 64, 65, 150, 193]     # 31 .. 33, 65: around the 32-row image
DIMS = [16, 48, 64, 128]                                      # 48: a padded tile


@functools.lru_cache(maxsize=None)
def solve_rows():
    """(ptr, idx, w f32): rows of the fixed lengths plus a dozen random ones below 40, each a
    random subset of the table in random (unsorted) order; weights count * exp(-0.01 * days),
    count in 1..8, days in 0..365."""
    rng = np.random.default_rng(12)
    lens = LENGTHS + rng.integers(0, 40, 12).tolist()
    rows = [rng.permutation(NI)[:n].astype(np.int32) for n in lens]
    ptr = np.zeros(len(rows) + 1, np.int64)
    np.cumsum(lens, out=ptr[1:])
    nnz = int(ptr[-1])
    w = rng.integers(1, 9, nnz) * np.exp(-0.01 * rng.integers(0, 366, nnz))
    return ptr, np.concatenate(rows), w.astype(np.float32)


@functools.lru_cache(maxsize=None)
def table(d, std):
    rng = np.random.default_rng(d * 7 + int(std * 10))
    return rng.normal(0, std, (NI, d)).astype(np.float32)


def oracle_and_yardstick(w, T, alpha, reg):
    """(x64 [rows, d], err_lapack32) for the rows of solve_rows() with the fp32 weights `w`."""
    ptr, idx, _ = solve_rows()
    x64 = WO.half_step(ptr, idx, w, T, alpha, reg)
    G32 = T.T @ T
    x32 = np.zeros_like(x64)
    for r in range(len(ptr) - 1):
        if ptr[r + 1] > ptr[r]:
            s = slice(ptr[r], ptr[r + 1])
            A, b = WO.system32(idx[s], w[s], T, G32, alpha, reg)
            x32[r] = scipy.linalg.solve(A, b, assume_a="pos")
    return x64, rel_err(x32, x64)


@functools.lru_cache(maxsize=None)
def solve_case(d, std, alpha, reg):
    return oracle_and_yardstick(solve_rows()[2], table(d, std), alpha, reg)


@functools.lru_cache(maxsize=None)
def device_table(d, std):
    """(ptr, idx, w, n, buf, G) on the device."""
    ptr, idx, w = solve_rows()
    buf = strided(table(d, std), d + 4)
    return dev(ptr), dev(idx), dev(w), len(ptr) - 1, buf, raw_gram(buf, NI, d)


def id_batch(n):
    """Every row once, permuted, with repeats of rows 3, 7 and 0."""
    rows = np.random.default_rng(5).permutation(np.r_[np.arange(n), [3, 3, 7, 0]])
    return rows, dev(rows.astype(np.int64)), len(rows)


@pytest.mark.parametrize("with_ids", [False, True])
@pytest.mark.parametrize("d", DIMS)
def test_constant_weights_are_the_unweighted_entry_bitwise(d, with_ids):
    """1 + alpha' exact in fp32 (11, 41): w = 1 is the unweighted entry; w = 2^e scales S and bw
    exactly, so it is the unweighted entry at alpha' = 2^e alpha."""
    ptr, idx, _, n, buf, G = device_table(d, 1.0)
    nnz = int(solve_rows()[0][-1])
    rows, ids, B = id_batch(n) if with_ids else (np.arange(n), None, n)
    for wv, alpha_w, alpha_u, reg in ((1.0, 10.0, 10.0, 0.1), (1.0, 40.0, 40.0, 0.01),
                                      (2.0, 20.0, 40.0, 0.01), (0.5, 80.0, 40.0, 0.01)):
        w = torch.full((nnz,), wv, dtype=torch.float32, device=DEV)
        st, got = raw_wsolve(ptr, idx, w, n, buf, NI, d, G, alpha_w, reg, ids, B, d + 3)
        assert st == _lib.HNM_OK
        st, want = raw_solve(ptr, idx, n, buf, NI, d, G, alpha_u, reg, ids, B, d + 3)
        assert st == _lib.HNM_OK
        _lib.sync_check(DEV)
        assert np.isfinite(want.cpu().numpy()).all()
        assert np.array_equal(bits(got), bits(want)), (wv, alpha_w)


@pytest.mark.parametrize("alpha,reg", [(10.0, 0.1), (40.0, 0.01)])
@pytest.mark.parametrize("std", [0.1, 1.0])
@pytest.mark.parametrize("d", DIMS)
def test_weighted_solve_is_as_accurate_as_lapack_fp32(d, std, alpha, reg):
    ptr, idx, w, n, buf, G = device_table(d, std)
    x64, e32 = solve_case(d, std, alpha, reg)
    st, out = raw_wsolve(ptr, idx, w, n, buf, NI, d, G, alpha, reg, None, n)
    assert st == _lib.HNM_OK
    _lib.sync_check(DEV)
    x = out.cpu().numpy()
    assert np.isfinite(x).all()
    err = rel_err(x, x64)
    print(f"weighted solve d={d} std={std} alpha={alpha} reg={reg}: err_kernel={err:.3e} "
          f"err_lapack32={e32:.3e} ratio={err / e32:.2f}")
    assert err <= 4 * e32


@pytest.mark.parametrize("d", [16, 64])
def test_rows_with_zero_weights_match_the_oracle(d):
    """A weight of 0: the entry counts in b0 (its p = 1 at confidence 1) and in nothing else.
    Every third weight is zero, the rows of 5 and 33 entries are zero throughout."""
    alpha, reg = 40.0, 0.01
    hptr, hidx, w = solve_rows()
    w = w.copy()
    w[::3] = 0.0
    for r in (3, 7):
        w[hptr[r]:hptr[r + 1]] = 0.0
    ptr, idx, _, n, buf, G = device_table(d, 1.0)
    T = table(d, 1.0)
    x64, e32 = oracle_and_yardstick(w, T, alpha, reg)
    st, out = raw_wsolve(ptr, idx, dev(w), n, buf, NI, d, G, alpha, reg, None, n)
    assert st == _lib.HNM_OK
    _lib.sync_check(DEV)
    x = out.cpu().numpy()
    err = rel_err(x, x64)
    print(f"zero weights d={d}: err_kernel={err:.3e} err_lapack32={e32:.3e} ratio={err / e32:.2f}")
    assert np.isfinite(x).all() and err <= 4 * e32
    # an all-zero row is (G + reg I)^-1 sum t: no alpha anywhere
    T64 = T.astype(np.float64)
    for r in (3, 7):
        want = np.linalg.solve(T64.T @ T64 + reg * np.eye(d), T64[hidx[hptr[r]:hptr[r + 1]]].sum(0))
        assert np.abs(x64[r] - want).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize("d", DIMS)
def test_weighted_solve_is_deterministic_and_rows_are_independent(d):
    alpha, reg = 40.0, 0.01
    ptr, idx, w, n, buf, G = device_table(d, 1.0)
    rows, ids, B = id_batch(n)
    ldo = d + 3
    st, out = raw_wsolve(ptr, idx, w, n, buf, NI, d, G, alpha, reg, ids, B, ldo)
    assert st == _lib.HNM_OK
    _lib.sync_check(DEV)
    full = out.cpu().numpy()
    assert (full[:, d:] == 7.0).all()                        # nothing written past d
    x = full[:, :d]
    assert np.isfinite(x).all()
    empty = np.diff(solve_rows()[0])[rows] == 0
    assert empty.any() and not bits(x[empty]).any()          # exact +0.0
    st, again = raw_wsolve(ptr, idx, w, n, buf, NI, d, G, alpha, reg, ids, B, ldo)
    assert np.array_equal(bits(again), bits(out))            # the same bits on a second call
    for r in (3, 7, 0):                                      # repeated rows agree
        where = np.nonzero(rows == r)[0]
        assert len(where) >= 2
        assert all(np.array_equal(bits(x[v]), bits(x[where[0]])) for v in where)
    for at in (2, 11):                                       # alone, and in the full batch
        st, alone = raw_wsolve(ptr, idx, w, n, buf, NI, d, G, alpha, reg,
                               dev(np.array([rows[at]], np.int64)), 1)
        assert np.array_equal(bits(alone[0, :d]), bits(x[at]))
    st, plain = raw_wsolve(ptr, idx, w, n, buf, NI, d, G, alpha, reg, None, n)
    assert np.array_equal(bits(plain[:, :d].cpu().numpy()[rows]), bits(x))
    # the weights matter: it is not the unweighted answer
    st, unw = raw_solve(ptr, idx, n, buf, NI, d, G, alpha, reg, None, n)
    assert not np.array_equal(bits(unw), bits(plain))
    _lib.sync_check(DEV)


@pytest.mark.parametrize("d", [16, 128])
def test_bad_weights_give_nan_rows_and_einval(d):
    alpha, reg = 10.0, 0.1
    ptr, idx, w, n, buf, G = device_table(d, 1.0)
    st, clean = raw_wsolve(ptr, idx, w, n, buf, NI, d, G, alpha, reg, None, n)
    _lib.sync_check(DEV)
    clean = clean.cpu().numpy()
    hptr = solve_rows()[0]
    # rows of 17 and 150 entries; of 65; of 64 and 31
    for case in ({4: float("nan"), 10: -1.0}, {9: float("inf")}, {8: -0.0, 5: -1e-30}):
        bad = w.clone()
        hit = []
        for victim, value in case.items():
            bad[int(hptr[victim + 1]) - 2] = value           # in the row's last gather image
            if not value == 0.0:                             # -0.0 is a zero: legal
                hit.append(victim)
        st, out = raw_wsolve(ptr, idx, bad, n, buf, NI, d, G, alpha, reg, None, n)
        assert st == _lib.HNM_OK
        with pytest.raises(ValueError, match="weight"):      # HNM_EINVAL from the ctx check
            _lib.sync_check(DEV)
        out = out.cpu().numpy()
        assert np.isnan(out[hit]).all()
        others = np.setdiff1d(np.arange(n), list(case))
        assert np.array_equal(bits(out[others]), bits(clean[others]))
        assert np.isfinite(out[np.setdiff1d(np.arange(n), hit)]).all()
        _lib.sync_check(DEV)                                 # the error word was cleared
    # an id out of range still reports HNM_EOOB, from idx and from row_ids
    bad_idx = idx.clone()
    bad_idx[int(hptr[4]) + 3] = NI
    st, out = raw_wsolve(ptr, bad_idx, w, n, buf, NI, d, G, alpha, reg, None, n)
    assert st == _lib.HNM_OK
    with pytest.raises(IndexError):
        _lib.sync_check(DEV)
    out = out.cpu().numpy()
    assert np.isnan(out[4]).all()
    others = np.arange(n) != 4
    assert np.array_equal(bits(out[others]), bits(clean[others]))
    ids = dev(np.array([0, n, 5, -1, 7], np.int64))
    st, out = raw_wsolve(ptr, idx, w, n, buf, NI, d, G, alpha, reg, ids, 5)
    assert st == _lib.HNM_OK
    with pytest.raises(IndexError):
        _lib.sync_check(DEV)
    out = out.cpu().numpy()
    assert np.isnan(out[[1, 3]]).all()
    assert np.array_equal(bits(out[[0, 2, 4]]), bits(clean[[0, 5, 7]]))
    _lib.sync_check(DEV)


def test_weighted_solve_statuses():
    ptr, idx, w, n, buf, G = device_table(64, 1.0)
    st, _ = raw_wsolve(ptr, idx, None, n, buf, NI, 64, G, 10.0, 0.1, None, n)
    assert st == _lib.HNM_EINVAL                             # w = NULL with work to do
    wide = torch.zeros(NI, 256, device=DEV)
    G2 = torch.zeros(256, 256, device=DEV)
    for d in (8, 24, 144):
        assert raw_wsolve(ptr, idx, w, n, wide, NI, d, G2, 10.0, 0.1, None, n)[0] \
            == _lib.HNM_EUNSUPPORTED
    nan, inf = float("nan"), float("inf")
    for alpha, reg in ((10.0, 0.0), (10.0, -1.0), (-1.0, 0.1), (nan, 0.1), (10.0, nan),
                       (inf, 0.1), (10.0, inf)):
        assert raw_wsolve(ptr, idx, w, n, buf, NI, 64, G, alpha, reg, None, n)[0] \
            == _lib.HNM_EINVAL
    st, out = raw_wsolve(ptr, idx, w, n, buf, NI, 64, G, 10.0, 0.1, None, 0)
    assert st == _lib.HNM_OK and (out.cpu().numpy() == 7.0).all()
    st, out = raw_wsolve(ptr, idx, None, 0, buf, NI, 64, G, 10.0, 0.1, dev(np.zeros(2, np.int64)), 2)
    assert st == _lib.HNM_OK and (out.cpu().numpy() == 7.0).all()   # nothing launched
    assert raw_wsolve(ptr, idx, w, n, buf, NI, 64, G, 0.0, 0.1, None, n)[0] == _lib.HNM_OK
    _lib.sync_check(DEV)


@pytest.mark.parametrize("alpha,reg", [(10.0, 0.1), (40.0, 0.01)])
def test_score_of_an_item_grows_with_its_weight(alpha, reg):
    """A 5-item basket, d = 16, table std 0.3: as one item's weight runs 0.25 .. 16 (the others
    at 1) its own score x . y_j strictly increases and stays below its preference 1."""
    d = 16
    rng = np.random.default_rng(21)
    T = rng.normal(0, 0.3, (NI, d)).astype(np.float32)
    buf = strided(T, d)
    G = raw_gram(buf, NI, d)
    basket = np.array([7, 150, 31, 99, 4], np.int32)
    ptr, idx = dev(np.array([0, 5], np.int64)), dev(basket)
    scores, scores64 = [], []
    for wj in (0.25, 0.5, 1.0, 2.0, 4.0, 8.0, 16.0):
        w = np.ones(5, np.float32)
        w[2] = wj
        st, out = raw_wsolve(ptr, idx, dev(w), 1, buf, NI, d, G, alpha, reg, None, 1)
        assert st == _lib.HNM_OK
        x = out.cpu().numpy()[0].astype(np.float64)
        scores.append(float(x @ T[basket[2]].astype(np.float64)))
        x64 = WO.half_step(np.array([0, 5]), basket, w, T, alpha, reg)[0]
        scores64.append(float(x64 @ T[basket[2]].astype(np.float64)))
    _lib.sync_check(DEV)
    print(f"monotone alpha={alpha} reg={reg}: scores {np.round(scores, 4).tolist()}, smallest "
          f"step {np.diff(scores).min():.4f} (float64 oracle {np.diff(scores64).min():.4f})")
    assert all(b > a for a, b in zip(scores, scores[1:])) and scores[-1] < 1.0
    assert np.abs(np.array(scores) - np.array(scores64)).max() <= 1e-4


# ------------------------------------------------------------------ the module
@functools.lru_cache(maxsize=None)
def fit_data():
    """test_gpu_als.py's transactions (Zipf-0.9 items; users u % 17 == 0 and items i % 23 == 0
    stay empty) with a quantity in 1..3 and an age in days in 0..365 each.
    -> (users, items, qty, days, ptr, idx, w32): the pair CSR and its fp32 weights, by the
    oracle's plain loop."""
    users, items = syn.interactions(FU, FI, 4500, seed=2)
    keep = (users % 17 != 0) & (items % 23 != 0)
    users, items = users[keep], items[keep]
    rng = np.random.default_rng(8)
    qty = rng.integers(1, 4, len(users))
    days = rng.integers(0, 366, len(users))
    ptr, idx, w64 = WO.pair_weights(users, items, qty * np.exp(-0.01 * days), FU, FI)
    assert len(idx) < len(users)                             # repeat purchases were summed
    tlens = np.diff(WO.transpose(ptr, idx, w64, FU, FI)[0])
    assert (np.diff(ptr) == 0).sum() >= 18 and (tlens == 0).sum() >= 9 and tlens.max() > 4 * 32
    return users, items, qty, days, ptr, idx, w64.astype(np.float32)


@functools.lru_cache(maxsize=None)
def fit_reference(d):
    _, _, _, _, ptr, idx, w = fit_data()
    Y0 = new_model(d).item_embeddings.weight.detach().cpu().numpy()
    return WO.sweeps(ptr, idx, w, FU, FI, Y0, ALPHA, REG, 3)


@functools.lru_cache(maxsize=None)
def fitted(d, iterations=3):
    users, items, qty, days, *_ = fit_data()
    return new_model(d).fit_interactions(users, items, weights=qty, days_ago=days,
                                         time_decay=0.01, iterations=iterations)


@pytest.mark.parametrize("d", [16, 64])
def test_weighted_fit_follows_the_float64_oracle_sweep_by_sweep(d):
    *_, ptr, idx, w = fit_data()
    ref = fit_reference(d)
    for s in range(3):
        m = fitted(d, s + 1)
        X, Y = tables(m)
        assert_scores_close(X, ref[s][0], f"X after sweep {s + 1}")
        assert_scores_close(Y, ref[s][1], f"Y after sweep {s + 1}")
        assert np.abs(ref[s][0]).max() > 1.0 and np.abs(ref[s][1]).max() > 0.01
    assert not bits(X[np.diff(ptr) == 0]).any()              # empty users and items: exact zeros
    assert not bits(Y[np.arange(FI) % 23 == 0]).any()
    h = m.history
    assert h.nnz == ptr[-1] and np.array_equal(h.hist_idx.cpu().numpy(), idx)
    assert np.array_equal(bits(h.hist_w), bits(w))
    # the weights matter at this bar: the unweighted oracle is somewhere else
    unweighted = AO.sweeps(ptr, idx, FU, FI, new_model(d).item_embeddings.weight.detach().cpu()
                           .numpy(), ALPHA, REG, 1)[0][0]
    with pytest.raises(AssertionError):
        assert_scores_close(tables(fitted(d, 1))[0], unweighted, "unweighted")


@pytest.mark.parametrize("d", [16, 64])
def test_weighted_loss_is_the_dense_float64_loss_and_decreases(d):
    users, items, qty, days, ptr, idx, w = fit_data()
    m = new_model(d).fit_interactions(users, items, weights=qty, days_ago=days, time_decay=0.01,
                                      iterations=4, track_loss=True)
    X, Y = tables(m)
    want = WO.loss_dense(X, Y, ptr, idx, w, ALPHA, REG)
    assert m.loss() == pytest.approx(want, rel=1e-9)
    assert m.loss() != pytest.approx(AO.loss_dense(X, Y, ptr, idx, ALPHA, REG), rel=1e-3)
    h = m.loss_history
    print(f"weighted loss history d={d}: {h}")
    assert len(h) == 4 and h[-1] == pytest.approx(want, rel=1e-9)
    assert all(b < a for a, b in zip(h, h[1:]))


def test_weighted_fit_is_reproducible_and_explicit_weights_give_the_same_bits():
    users, items, qty, days, *_ = fit_data()
    a = tables(fitted(64, 3))
    b = tables(new_model(64).fit_interactions(users, items, weights=qty, days_ago=days,
                                              time_decay=0.01, iterations=3))
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))
    # the same float64 products, given as explicit weights (and as a tensor, permuted)
    prod = qty.astype(np.float64) * np.exp(-0.01 * days.astype(np.float64))
    p = np.random.default_rng(0).permutation(len(users))
    c = tables(new_model(64).fit_interactions(torch.from_numpy(users[p]), items[p],
                                              weights=torch.from_numpy(prod[p]), iterations=3))
    assert np.array_equal(bits(a[0]), bits(c[0])) and np.array_equal(bits(a[1]), bits(c[1]))
    # through fit_history of a weighted UserHistory
    h = UserHistory.from_interactions(users, items, FU, FI, DEV, weights=prod)
    e = tables(new_model(64).fit_history(h, iterations=3))
    assert np.array_equal(bits(a[0]), bits(e[0])) and np.array_equal(bits(a[1]), bits(e[1]))


def test_fit_without_weights_is_the_unweighted_fit_bitwise():
    """No weights: the unweighted entry, as before -- the loop of fit_history written out with
    the raw unweighted calls gives the same tables; a history whose pair weights are all 1
    (1 + alpha = 41 is exact) gives them too, through the weighted entry."""
    users, items, *_ = fit_data()
    d = 64
    m = new_model(d).fit_interactions(users, items, iterations=2)
    assert m.history.hist_w is None
    X, Y = tables(m)
    h = UserHistory.from_interactions(users, items, FU, FI, DEV)
    ptr, idx = h.hist_ptr.cpu().numpy(), h.hist_idx.cpu().numpy()
    tptr, tidx = AO.transpose(ptr, idx, FU, FI)
    tptr, tidx = dev(tptr), dev(tidx)
    y = new_model(d).item_embeddings.weight.detach().clone()
    for _ in range(2):
        st, x = raw_solve(h.hist_ptr, h.hist_idx, FU, y, FI, d, raw_gram(y, FI, d), ALPHA, REG,
                          None, FU)
        assert st == _lib.HNM_OK
        st, y = raw_solve(tptr, tidx, FI, x, FU, d, raw_gram(x, FU, d), ALPHA, REG, None, FI)
        assert st == _lib.HNM_OK
    _lib.sync_check(DEV)
    assert np.array_equal(bits(X), bits(x)) and np.array_equal(bits(Y), bits(y))
    hw = UserHistory.from_interactions(users, items, FU, FI, DEV)
    hw.hist_w = torch.ones(hw.hist_idx.shape, dtype=torch.float32, device=DEV)
    one = tables(new_model(d).fit_history(hw, iterations=2))
    assert np.array_equal(bits(one[0]), bits(X)) and np.array_equal(bits(one[1]), bits(Y))


def test_weighted_fold_in_is_the_raw_weighted_entry_bitwise():
    m = fitted(64)
    _, Y = m._tables()
    G = raw_gram(Y, FI, 64)
    baskets = [[3, 9, 50], [7], list(range(1, 40)), [], [199, 5]]
    rng = np.random.default_rng(4)
    ws = [(rng.integers(1, 4, len(b)) * np.exp(-0.01 * rng.integers(0, 30, len(b)))).tolist()
          for b in baskets]
    F = m.user_factors(baskets, ws)
    assert F.shape == (len(baskets), 64) and not bits(F[3]).any()
    ptr = np.cumsum([0] + [len(b) for b in baskets])
    order = [np.argsort(b) for b in baskets]                 # the module sorts a basket's items
    idx = np.concatenate([np.asarray(b, np.int32)[o] for b, o in zip(baskets, order)])
    w = np.concatenate([np.asarray(x, np.float64)[o] for x, o in zip(ws, order)]).astype(np.float32)
    st, want = raw_wsolve(dev(ptr), dev(idx), dev(w), len(baskets), Y, FI, 64, G, ALPHA, REG,
                          None, len(baskets))
    assert st == _lib.HNM_OK
    _lib.sync_check(DEV)
    assert np.array_equal(bits(F), bits(want))
    assert np.array_equal(bits(m.user_factors((ptr, idx), w)), bits(F))      # the CSR form
    # weights=None is the unweighted entry whatever the fit was
    st, plain = raw_solve(dev(ptr), dev(idx), len(baskets), Y, FI, 64, G, ALPHA, REG, None,
                          len(baskets))
    assert np.array_equal(bits(m.user_factors(baskets)), bits(plain))
    assert not np.array_equal(bits(plain), bits(F))
    # against the oracle
    x64 = WO.half_step(ptr, idx, w, Y.cpu().numpy(), ALPHA, REG)
    assert_scores_close(F.cpu().numpy(), x64, "weighted fold-in")
    for bad in ([[1.0]], [[1.0, 2.0, 3.0], [1.0, 1.0]]):
        with pytest.raises(ValueError):
            m.user_factors([[3, 9, 50], [7]], bad)
    with pytest.raises(ValueError):
        m.user_factors([[3, 9]], [[1.0, -1.0]])
    with pytest.raises(ValueError):                          # the kernel's own check (a CSR)
        m.user_factors((np.array([0, 2]), np.array([3, 9], np.int32)), np.array([1.0, np.nan]))
    with pytest.raises(ValueError):
        m.user_factors((np.array([0, 2]), np.array([3, 9], np.int32)), np.array([1.0]))
    with pytest.raises(IndexError):
        m.user_factors([[FI]], [[1.0]])


def test_duplicate_basket_items_sum_their_weights():
    m = fitted(64)
    a = m.user_factors([[9, 3, 9, 50, 9], [7, 7]], [[0.5, 2.0, 0.25, 1.0, 1.5], [1.0, 2.0]])
    b = m.user_factors([[3, 9, 50], [7]], [[2.0, 2.25, 1.0], [3.0]])
    assert np.array_equal(bits(a), bits(b))
    va, ia = m.recommend_for_items([[9, 3, 9, 50, 9]], weights=[[0.5, 2.0, 0.25, 1.0, 1.5]], k=12)
    vb, ib = m.recommend_for_items([[3, 9, 50]], weights=[[2.0, 2.25, 1.0]], k=12)
    assert torch.equal(ia, ib) and np.array_equal(bits(va), bits(vb))


def test_refresh_users_on_a_weighted_history_is_the_user_step_bitwise():
    users, items, qty, days, ptr, idx, w = fit_data()
    m = new_model(64).fit_interactions(users, items, weights=qty, days_ago=days, time_decay=0.01,
                                       iterations=3)
    _, Y = m._tables()
    st, step = raw_wsolve(m.history.hist_ptr, m.history.hist_idx, m.history.hist_w, FU, Y, FI, 64,
                          raw_gram(Y, FI, 64), ALPHA, REG, None, FU)
    assert st == _lib.HNM_OK
    _lib.sync_check(DEV)
    step = step.cpu().numpy()
    us = [1, 2, 17, 40, 123, 299]                            # 17: an empty user
    before = tables(m)[0]
    m.refresh_users(torch.tensor(us))
    after = tables(m)[0]
    assert np.array_equal(bits(after[us]), bits(step[us])) and not bits(after[17]).any()
    others = np.setdiff1d(np.arange(FU), us)
    assert np.array_equal(bits(after[others]), bits(before[others]))
    assert not np.array_equal(bits(after[us]), bits(before[us]))   # X was a step behind Y
    # and the fold-in of the same rows with the same weights
    F = m.user_factors([idx[ptr[u]:ptr[u + 1]].tolist() for u in us],
                       [w[ptr[u]:ptr[u + 1]].tolist() for u in us])
    assert np.array_equal(bits(F), bits(after[us]))


def test_weighted_recommend_for_items_is_the_dot_topk_of_the_fold_in_vectors():
    m = fitted(64)
    baskets = [[3, 9, 50], [7], list(range(1, 40)), [], [199, 5]]
    rng = np.random.default_rng(6)
    ws = [rng.integers(1, 9, len(b)).astype(np.float64).tolist() for b in baskets]
    F = m.user_factors(baskets, ws)
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
            gv, gi = m.recommend_for_items(baskets, filter_seen=seen, k=k, weights=ws)
            wv, wi = mf.recommend_with_scores(rows, filter_items=mask if seen else None, k=k)
            assert torch.equal(gi, wi) and np.array_equal(bits(gv), bits(wv))
            assert gi.shape == (len(baskets), k) and (gi >= 0).all()
    pv, pi = m.recommend_for_items(baskets, k=12)            # unweighted: another answer
    assert not np.array_equal(bits(pv), bits(m.recommend_for_items(baskets, k=12, weights=ws)[0]))


def test_recommender_add_als_with_recency_and_weighted_basket_requests():
    users, items, qty, days, ptr, idx, w = fit_data()
    srv = Recommender(FU, FI, device=DEV)
    model = srv.add_als(users, items, weights=qty, days_ago=days, time_decay=0.01,
                        embedding_dim=16, regularization=REG, alpha=ALPHA, iterations=3)
    assert srv.models["implicit_als"] is model and srv._device_history() is model.history
    assert np.array_equal(bits(model.history.hist_w), bits(w))
    X, Y = tables(model)
    assert np.array_equal(bits(X), bits(tables(fitted(16, 3))[0]))
    assert np.array_equal(bits(Y), bits(tables(fitted(16, 3))[1]))
    out = srv.get_batch_recommendations([1, 2], model_name="implicit_als", num_items=12)
    for u, r in zip((1, 2), out):
        ids = [int(x["article_id"]) for x in r["recommendations"]]
        assert len(ids) == 12 and not set(ids) & set(idx[ptr[u]:ptr[u + 1]].tolist())
    basket, bw = [50, 3, 9, 3], [1.0, 2.0, 0.5, 1.0]         # item 3 twice: 3.0 in all
    r = srv.get_recommendations_for_items(basket, num_items=10, model_name="implicit_als",
                                          include_scores=True, item_weights=bw)
    assert r["user_id"] is None and r["model_name"] == "implicit_als"
    ids = [int(x["article_id"]) for x in r["recommendations"]]
    want = model.recommend_for_items([[3, 9, 50]], k=10, weights=[[3.0, 0.5, 1.0]])
    assert len(ids) == 10 and not set(ids) & set(basket) and ids == want[1][0].tolist()
    assert [x["score"] for x in r["recommendations"]] == want[0][0].tolist()
    plain = srv.get_recommendations_for_items(basket, num_items=10, model_name="implicit_als",
                                              include_scores=True)
    assert [x["score"] for x in plain["recommendations"]] != want[0][0].tolist()
    with pytest.raises(ValueError):
        srv.get_recommendations_for_items(basket, model_name="implicit_als", item_weights=[1.0])
    with pytest.raises(ValueError):
        srv.get_recommendations_for_items(basket, model_name="implicit_als",
                                          item_weights=[1.0, -2.0, 1.0, 1.0])
    srv.add_item_cf(users, items)
    with pytest.raises(ValueError, match="item weights"):
        srv.get_recommendations_for_items(basket, model_name="item_cf", item_weights=bw)
