"""CPU: the lattice inputs (tests/lattice.py) are what the GPU order tests need them to be.

Exactness (every fused-route input passes the oracle's magnitude assertions, so fp32 is exact
in any order), tie pressure (the k-th and (k+1)-th reference scores are equal in most rows),
and which kernel of the sample-threshold path of hnm_dot_topk_f32 answers each input.  These
are properties of the inputs and the numpy references alone: nothing here runs a kernel.
"""
import numpy as np
import pytest

import lattice as L

DOT_IDS = [c.id for c in L.DOT_CASES]
NCF_CASES = [L.NCF_SMALL, *L.NCF_CERT.values(), L.NCF_DEEP, L.NCF_TWO_PHASE]


def _min_tie(k):
    return 0.5 if k >= 12 else 0.1


# ------------------------------------------------------------------ exactness
@pytest.mark.parametrize("case", L.DOT_CASES, ids=DOT_IDS)
def test_dot_inputs_exact(case):
    """dot_scores asserts integer tables, quarter-integer biases, 4 * sum|u||i| < 2^24 and
    equality with fp32 evaluations in two summation orders."""
    s = case.scores
    assert s.dtype == np.float32 and s.shape == (case.B, case.I) and np.isfinite(s).all()
    assert len(np.unique(s)) <= 256  # a lattice: few distinct levels


def test_dot_exactness_assertion_bites():
    """The magnitude assertion is live: a table entry of 2^23 breaks the bound, 0.3 the lattice."""
    t = L.dot_tables(4, 50, 8, seed=1)
    L.dot_scores(t, np.arange(4))
    big = dict(t, it=t["it"].copy())
    big["it"][3, 2] = 2.0 ** 23
    big["ut"] = np.abs(t["ut"]) + 1
    with pytest.raises(AssertionError):
        L.dot_scores(big, np.arange(4))
    frac = dict(t, it=t["it"].copy())
    frac["it"][3, 2] = 0.3
    with pytest.raises(AssertionError):
        L.dot_scores(frac, np.arange(4))


@pytest.mark.parametrize("case", NCF_CASES, ids=[c.id for c in NCF_CASES])
def test_ncf_inputs_exact(case):
    s = case.scores
    assert s.dtype == np.float32 and s.shape == (case.B, case.I)
    assert np.abs(s).max() < 256 and len(np.unique(s)) <= 256
    # pair scores are the same numbers
    items = np.arange(case.B) * 7 % case.I
    assert np.array_equal(L.ncf_scores(case.sd, case.users, items), s[np.arange(case.B), items])


# ------------------------------------------------------------------ tie pressure
@pytest.mark.parametrize("case", L.DOT_CASES, ids=DOT_IDS)
def test_dot_tie_pressure(case):
    f = L.tie_fraction(case.scores, case.k, case.mask_csr)
    assert f >= _min_tie(case.k), (case.id, f)


@pytest.mark.parametrize("case,ks", [(L.NCF_SMALL, L.NCF_SMALL_KS), (L.NCF_DEEP, (12,)),
                                     (L.NCF_TWO_PHASE, (12,)),
                                     *[(c, L.NCF_CERT_KS) for c in L.NCF_CERT.values()]],
                         ids=lambda v: getattr(v, "id", None))
def test_ncf_tie_pressure(case, ks):
    for k in ks:
        f = L.tie_fraction(case.scores, k)
        assert f >= _min_tie(k), (case.id, k, f)


def test_tie_group_mask_leaves_the_last_member():
    """The "tie_group" mask removes every member of the tie group at position k but its last:
    the reference's k-th item is then that last member, the highest id of the group."""
    c = next(c for c in L.DOT_CASES if c.mask == "tie_group")
    ptr, idx = c.mask_csr
    hit = 0
    for b in range(c.B):
        m = idx[ptr[b]:ptr[b + 1]]
        row = c.scores[b]
        kth = -np.sort(-row)[c.k - 1]
        grp = np.nonzero(row == kth)[0]
        assert np.array_equal(m, grp[:-1])
        hit += int(grp[-1] in c.ref[1][b])
    assert hit == c.B


# ------------------------------------------------------------------ threshold path routing
SPARSE_THRESH = [c for c in L.DOT_CASES if c.kind == "sparse" and c.I >= L.THRESH_MIN_ITEMS
                 and c.mask == "none"]
DENSE_THRESH = [c for c in L.DOT_CASES if c.kind == "dense" and c.I >= L.THRESH_MIN_ITEMS]


@pytest.mark.parametrize("case", SPARSE_THRESH, ids=[c.id for c in SPARSE_THRESH])
def test_sparse_tie_rows_reach_the_select_kernel(case):
    """Every row's appends fit the candidate buffer, so thresh_select_kernel answers it on
    tied rows.  If score.hip's constants change, re-tune the inputs."""
    n = L.thresh_counts(case)
    assert (n >= case.k).all() and (n <= L.thresh_cap(case.I, case.k)).all(), (n.min(), n.max())


@pytest.mark.parametrize("case", DENSE_THRESH, ids=[c.id for c in DENSE_THRESH])
def test_dense_tie_rows_overflow_to_the_fallback(case):
    """Every row exceeds the cap, so the overflow fallback (LIST pass over queued rows) answers
    it.  If score.hip's constants change, re-tune the inputs."""
    n = L.thresh_counts(case)
    assert (n > L.thresh_cap(case.I, case.k)).all(), (n.min(), L.thresh_cap(case.I, case.k))


def test_thresh_cases_exist():
    assert len(SPARSE_THRESH) >= 6 and len(DENSE_THRESH) >= 3
    assert any(c.d == 64 and not c.bias for c in SPARSE_THRESH)


# ------------------------------------------------------------------ certified bound width
@pytest.mark.parametrize("case", SPARSE_THRESH, ids=[c.id for c in SPARSE_THRESH])
def test_certified_bound_is_narrower_than_a_level(case):
    """dot_cert.hip: E_u = 3 * 2^-11 ||u|| max||i|| + 2^-22 (|ub_u| + max|ib|) (+ a subnormal
    slack far below 2^-20 here); the scan prunes at (sample k-th) - 2 E_u.  2 E_u stays below 1,
    the spacing of bias-free scores: the certified candidate set of those cases is exactly
    {score >= sample k-th}, so the tie group at the boundary must come through re-scoring and
    selection (with quarter-integer biases it may hold up to three more levels)."""
    t = case.tables
    nu = np.linalg.norm(t["ut"][case.users].astype(np.float64), axis=1)
    ni = np.linalg.norm(t["it"].astype(np.float64), axis=1).max()
    e = L.DCERT_RHO * nu * ni + 2.0 ** -20
    if case.bias:
        e = e + 2.0 ** -22 * (np.abs(t["ub"][case.users]) + np.abs(t["ib"]).max())
    assert (2 * e).max() < 1.0, (2 * e).max()


# ------------------------------------------------------------------ Wide&Deep
WD_IDS = [c.id for c in L.WD_CASES]


def wd_oracle_fp32(case, chunk=500):
    """The fp32 numpy oracle over every (user, item) pair, in the reference's 500-item chunks
    (with item features: forward on the expanded pairs, item_features = table[item])."""
    from oracle import hnm_oracle as O
    if case.Fi == 0:
        return O.widedeep_predict_all_items(case.sd, case.users, case.user_features)
    out = []
    for s in range(0, case.I, chunk):
        e = min(s + chunk, case.I)
        eu, ei = np.repeat(case.users, e - s), np.tile(np.arange(s, e), case.B)
        ef = np.repeat(case.user_features, e - s, axis=0)
        out.append(O.widedeep_forward(case.sd, eu, ei, ef, item_features=case.item_table[ei])
                   .reshape(case.B, e - s))
    return np.concatenate(out, axis=1)


@pytest.mark.parametrize("case", L.WD_CASES, ids=WD_IDS)
def test_wd_inputs_exact_three_ways(case):
    """wd_scores (float64, unfolded, with its own lattice / magnitude / folded-fp32 assertions)
    == the fp32 numpy oracle == the torch CPU reference module, as uint32 bits.  The torch
    module has no item features and always a one-hot wide part (its [pairs, U + I] one-hot
    input: small batches only)."""
    s = case.scores
    assert s.dtype == np.float32 and s.shape == (case.B, case.I) and np.isfinite(s).all()
    assert np.array_equal(s * 8, np.round(s * 8)) and np.abs(s).max() < 2048
    assert np.array_equal(L.bits(wd_oracle_fp32(case)), L.bits(s))
    if case.Fi == 0 and case.wide and case.B <= 16:
        import torch
        from oracle import torch_cpu as T
        uf = None if case.Fu == 0 else torch.from_numpy(case.user_features)
        with torch.no_grad():
            t = T.widedeep_predict_all_items(T.as_torch(case.sd), torch.from_numpy(case.users), uf)
        assert np.array_equal(L.bits(t.numpy()), L.bits(s))


def test_wd_exactness_assertion_bites():
    """The lattice assertions are live: running_var = 1 in place of 1 - eps (sqrt(1 + 1e-5) is
    no lattice point), a weight of 0.3, and an entry of 2^22 are each refused."""
    sd = L.wd_state_dict(12, 60, 8, (16, 8), seed=1)
    users = np.arange(5)
    L.wd_scores(sd, users)
    for key, at, bad in (("deep_network.2.running_var", (3,), 1.0),
                         ("deep_network.4.weight", (2, 5), 0.3),
                         ("deep_item_embedding.weight", (7, 1), 2.0 ** 22)):
        broken = dict(sd, **{key: sd[key].copy()})
        broken[key][at] = bad
        with pytest.raises(AssertionError):
            L.wd_scores(broken, users)
    # and the generator's own check of the BatchNorm construction: 0.25, 1 and 4 are the only
    # squares it uses; each survives the round trip through running_var bit for bit
    for t in (0.25, 1.0, 4.0):
        v = np.float32(t) - L.WD_EPS
        assert L.bits(v + L.WD_EPS) == L.bits(np.float32(t)) and v != np.float32(t)


@pytest.mark.parametrize("case", L.WD_CASES, ids=WD_IDS)
def test_wd_tie_pressure(case):
    """Ties across position k in most rows; in the sparse-tie cases the median tie group at k
    has at most 64 members, so a certified row is answered by the cascade and not by a fallback;
    the best-first case has rows whose tie group alone exceeds the single-phase limit."""
    for k in case.ks:
        f = L.tie_fraction(case.scores, k)
        assert f >= _min_tie(k), (case.id, k, f)
        if case.sparse:
            g = L.tie_group_sizes(case.scores, k)
            assert np.median(g) <= 64, (case.id, k, g)
    if case is L.WD_BEST_FIRST:
        g = L.tie_group_sizes(case.scores, 64)
        assert (g > L.WDC_BF_MIN).sum() >= 3 and g.max() <= 300, g


def test_wd_case_table():
    from test_gpu_widedeep_shapes import CERT_TOWERS
    assert [list(t) for t in L.WD_CERT] == CERT_TOWERS and set(L.WD_CERT_FULL) <= set(L.WD_CERT)
    assert all(c.certified for c in L.WD_CERT.values())
    assert not L.WD_EXACT.certified and not L.WD_FEAT_EXACT.certified
    assert L.WD_FEAT_CERT.certified and L.WD_NOWIDE.certified and L.WD_B70.certified
    assert "wide_user_embedding.weight" not in L.WD_NOWIDE.sd
    assert (L.WD_NOWIDE.ref(64)[0] == 0).any()  # exact zeros reach the top-K: their sign counts


def test_wd_tie_group_mask_leaves_the_last_member():
    """The same check as test_tie_group_mask_leaves_the_last_member on a Wide&Deep case."""
    c, k = L.WD_CERT[(48, 50)], 12
    ptr, idx = c.mask_csr("tie_group", k)
    _, ri = c.ref(k, "tie_group")
    for b in range(c.B):
        row = c.scores[b]
        grp = np.nonzero(row == -np.sort(-row)[k - 1])[0]
        assert np.array_equal(idx[ptr[b]:ptr[b + 1]], grp[:-1])
        assert grp[-1] in ri[b] and not (set(grp[:-1].tolist()) & set(ri[b].tolist()))
