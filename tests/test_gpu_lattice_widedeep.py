"""GPU: every Wide&Deep scoring and top-K route against the lattice oracle, bitwise.

`WideDeep` loaded from lattice.wd_state_dict: ternary embeddings and weights, integer biases,
and BatchNorm statistics whose sqrt(running_var + eps) is 0.5, 1 or 2 exactly in fp32, so every
intermediate of a score is a multiple of 2^-3 below 2^11 and the fp32 score is one number in
any summation order, folded or not, on the matrix pipe or the vector pipe: lattice.wd_scores
is a bitwise oracle (tests/test_cpu_lattice.py proves that three ways on the CPU, and that most
rows tie across position k).  Ids are compared with np.array_equal, values as uint32 bits,
against numpy's (score desc, id asc) order, lattice.ref_topk.

  dense scores / pair scores        widedeep_score_kernel<DENSE>, widedeep_pair_kernel
  exact fused top-K                 widedeep_score_kernel's per-partition lists + merge, masks
  certified cascade                 scan, collect, best-first, refine, filter, re-score, on each
                                    certified tower shape; its second phase; forced fallback
                                    rows and the scatter; segment overflow
  k > 64                            dense scores + hnm_topk_rows_f32
  user / item features              passed and registered tables, a strided item table
  use_wide_user_item=False          the all-zero wide vector, the sign of zero included

Helpers come from test_gpu_prefilter.py (to_module, topk_both; its wd_model draws the random
synthetic weights and cannot load a lattice state dict) and test_gpu_topk_order.py
(assert_bitwise).  Segment overflow (more than WDC_CAP = 4,096 appends in one item partition)
needs a partition wider than 4,096 items, which wd_partition gives only to a batch of at least
8 * (compute units) - 3 rows: the overflow test runs that many rows of nine distinct users.
Every printed line starts with "wd-lattice": profiles/widedeep_lattice_gpu_tests.txt keeps them.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import lattice as L
from hnm_recommendation_amd import WideDeep, _lib
from test_gpu_prefilter import to_module, topk_both
from test_gpu_topk_order import assert_bitwise

pytestmark = pytest.mark.gpu
DEV = "cuda"
# masks after which a certified row may legitimately be short of k candidates (exact fallback)
SHORT_MASKS = ("all_but_few", "all")


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def model(case):
    m = WideDeep(case.U, case.I, num_user_features=case.Fu, num_item_features=case.Fi,
                 embedding_dim=case.d, deep_layers=list(case.tower),
                 use_wide_user_item=case.wide)
    return to_module(m, case.sd)


def with_stats(fn):
    """fn() with the counters on: (result, (rows, candidates, fallback rows, second-phase rows))."""
    d0 = torch.device(DEV)
    _lib.prefilter_stats(d0, reset=True)
    _lib.set_option(d0, _lib.HNM_OPT_STATS, 1)
    try:
        out = fn()
    finally:
        _lib.set_option(d0, _lib.HNM_OPT_STATS, 0)
    s = _lib.prefilter_stats(d0, reset=True, extended="cascade")
    return out, (s[0], s[1], s[2], s[6])


def wd_topk(case, k, mask=(None, None), prefilter=True, users=None, user_features=None,
            item_features=None):
    """hnm_widedeep_topk_ex_f32 with a CSR mask as is (duplicates and ids >= I included)."""
    m = model(case)
    w, keep = m._weights()
    u = dev(case.users if users is None else users)
    if user_features is None and case.Fu and m.user_feature_table is None:
        user_features = dev(case.user_features)
    f = m._features(user_features, u)
    if item_features is None and case.Fi and m.item_feature_table is None:
        item_features = dev(case.item_table)
    itf, tab, ldf = m._item_table(item_features, u.device, keep)
    mptr, midx = dev(mask[0]), dev(mask[1])
    B = u.numel()
    ov = torch.empty(B, k, device=DEV)
    oi = torch.empty(B, k, dtype=torch.int64, device=DEV)
    _lib.set_prefilter(u.device, prefilter)
    try:
        _lib.check(_lib.fn("hnm_widedeep_topk_ex_f32")(
            _lib.ctx(u.device), w, _lib.ptr(u), B, _lib.ptr(f), _lib.ptr(mptr), _lib.ptr(midx), k,
            _lib.ptr(ov), _lib.ptr(oi), None if itf is None else C.byref(itf), _lib.ptr(tab), ldf),
            "hnm_widedeep_topk_ex_f32")
        _lib.sync_check(u.device)
    finally:
        _lib.set_prefilter(u.device, True)
    return ov, oi


def filter_dict(case, mask):
    """The CSR mask as the filter_items dict of the module's API (ids < I)."""
    ptr, idx = mask
    if ptr is None:
        return None
    return {int(u): {int(x) for x in idx[ptr[b]:ptr[b + 1]] if x < case.I}
            for b, u in enumerate(case.users)}


def say(case, k, kind, stats):
    print(f"wd-lattice {case.id} k={k} mask={kind}: rows {stats[0]}, re-scored {stats[1]}, "
          f"fallback rows {stats[2]}, second-phase rows {stats[3]}")


def pairs_of(case, n=64):
    rows = np.arange(n) % case.B  # repeated users
    items = L._rng(17, case.I).integers(0, case.I, n)
    return rows, items


# ------------------------------------------------------------------ dense and pair scores
DENSE_CASES = (L.WD_CERT[(48, 200, 100)], L.WD_CERT[(48, 50)], L.WD_EXACT)


@pytest.mark.parametrize("case", DENSE_CASES, ids=lambda c: c.id)
def test_dense_and_pair_scores(case):
    m = model(case)
    got = m.predict_all_items(dev(case.users)).cpu().numpy()
    assert np.array_equal(L.bits(got), L.bits(case.scores))
    rows, items = pairs_of(case)
    pair = m(dev(case.users[rows]), dev(items)).cpu().numpy()
    assert np.array_equal(L.bits(pair), L.bits(case.scores[rows, items]))


# ------------------------------------------------------------------ exact fused top-K
# the two certified towers with the pre-filter off, and the exact-only towers (40 wide, 1,111
# items) whatever the switch
EXACT_RUNS = [(L.WD_CERT[(48, 200, 100)], False), (L.WD_CERT[(48, 50)], False),
              (L.WD_EXACT, True), (L.WD_EXACT_WIDE, True)]


@pytest.mark.parametrize("k", L.WD_EXACT_KS)
@pytest.mark.parametrize("case,prefilter", EXACT_RUNS, ids=lambda v: getattr(v, "id", str(v)))
def test_exact_topk(case, prefilter, k):
    for kind in L.MASK_KINDS:
        (ov, oi), stats = with_stats(lambda: wd_topk(case, k, case.mask_csr(kind, k), prefilter))
        assert_bitwise(ov, oi, *case.ref(k, kind), f"exact {case.id} k={k} mask={kind}")
        assert stats[0] == 0, stats  # the certified route did not run


# ------------------------------------------------------------------ certified cascade
CERT_RUNS = [(t, k) for t in L.WD_CERT for k in (L.WD_CERT_KS if t in L.WD_CERT_FULL else (12,))]


@pytest.mark.parametrize("tower,k", CERT_RUNS, ids=lambda v: str(v).replace(" ", ""))
def test_certified_cascade(tower, k):
    """Each certified tower shape on the sparse-tie case: the cascade, not a fallback, answers
    (at most half the rows fall back unless the mask leaves fewer than k items)."""
    case = L.WD_CERT[tower]
    for kind in (L.MASK_KINDS if tower in L.WD_CERT_FULL else ("none",)):
        (ov, oi), stats = with_stats(lambda: wd_topk(case, k, case.mask_csr(kind, k)))
        say(case, k, kind, stats)
        assert_bitwise(ov, oi, *case.ref(k, kind), f"certified {case.id} k={k} mask={kind}")
        assert stats[0] == case.B, stats  # the certified route ran
        if kind not in SHORT_MASKS:
            assert stats[2] <= case.B // 2, stats


def test_certified_more_than_one_user_block():
    """70 rows: another partition count and several user blocks; certified and exact."""
    case, k = L.WD_B70, 12
    for kind in ("none", "random"):
        mask, ref = case.mask_csr(kind, k), case.ref(k, kind)
        (ov, oi), stats = with_stats(lambda: wd_topk(case, k, mask))
        say(case, k, kind, stats)
        assert_bitwise(ov, oi, *ref, f"certified {case.id} mask={kind}")
        assert stats[0] == case.B and stats[2] <= case.B // 2, stats
        assert_bitwise(*wd_topk(case, k, mask, prefilter=False), *ref, f"exact {case.id} {kind}")


@pytest.mark.parametrize("k", L.WD_BEST_FIRST.ks)
def test_best_first_second_phase(k):
    """Rows whose tie group at k alone exceeds WDC_BF_MIN have more survivors than the first
    phase refines: they run wdc_filter_kernel and the second refining pass."""
    case = L.WD_BEST_FIRST
    rv, _ = case.ref(k)
    need = int(((case.scores >= rv[:, -1:]).sum(1) > L.WDC_BF_MIN).sum())
    for kind in ("none", "random", "dups_oob"):
        (ov, oi), stats = with_stats(lambda: wd_topk(case, k, case.mask_csr(kind, k)))
        say(case, k, kind, stats)
        assert_bitwise(ov, oi, *case.ref(k, kind), f"best-first k={k} mask={kind}")
        assert stats[0] == case.B and stats[2] <= case.B // 2, stats
        if kind == "none":
            assert stats[3] >= need, (stats, need)
    if k == 64:
        assert need >= 3, need


def test_forced_fallback_rows():
    """Three rows are left with fewer than k unmasked items (9, 0 and 3): they take the exact
    kernel and the scatter, the other rows the cascade; all in numpy's order."""
    case, k = L.WD_CERT[(48, 50)], 12
    rng = L._rng(23)
    left = {1: 9, 4: 0, 7: 3}
    rows = [np.setdiff1d(np.arange(case.I), rng.choice(case.I, left[b], replace=False))
            if b in left else np.zeros(0, np.int64) for b in range(case.B)]
    ptr = np.zeros(case.B + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=ptr[1:])
    mask = (ptr, np.concatenate(rows).astype(np.int32))
    (ov, oi), stats = with_stats(lambda: wd_topk(case, k, mask))
    say(case, k, "three-short-rows", stats)
    assert_bitwise(ov, oi, *L.ref_topk(case.scores, k, mask), "forced fallback rows")
    assert stats[0] == case.B and 3 <= stats[2] <= case.B // 2 + 3, stats
    # the module's API agrees with its exact route on the same filter
    (ev, ei), (pv, pi), st = topk_both(model(case), dev(case.users), filter_dict(case, mask), k=k)
    assert np.array_equal(ei, pi) and np.array_equal(L.bits(ev), L.bits(pv)) and st[2] >= 3
    assert np.array_equal(pi, oi.cpu().numpy())


def test_segment_overflow_falls_back():
    """All-tied rows in one item partition of 4,224 items: every segment overflows WDC_CAP, the
    rows take the exact kernel: the k lowest ids."""
    case, k = L.WD_OVERFLOW, 12
    ncu = C.c_int(0)
    _lib.check(_lib.fn("hnm_ctx_num_cus")(_lib.ctx(torch.device(DEV)), C.byref(ncu)), "num_cus")
    rows = np.arange(8 * ncu.value) % case.B  # wd_partition: one partition from 8 CUs - 3 rows on
    assert case.I > L.WDC_CAP
    (ov, oi), stats = with_stats(lambda: wd_topk(case, k, users=case.users[rows]))
    print(f"wd-lattice {case.id} k={k} rows {len(rows)}: rows {stats[0]}, fallback rows {stats[2]}")
    rv, ri = case.ref(k)
    assert_bitwise(ov, oi, rv[rows], ri[rows], "segment overflow")
    assert (ri == np.arange(k)).all()
    assert stats[0] == len(rows) and stats[2] >= 1, stats


# ------------------------------------------------------------------ k > 64
@pytest.mark.parametrize("case", L.WD_DENSE_K_CASES, ids=lambda c: c.id)
def test_k_above_64(case):
    k, m = L.WD_DENSE_K, model(case)
    for kind in ("none", "tie_group"):
        ov, oi = m.recommend_with_scores(dev(case.users), k=k,
                                         filter_items=filter_dict(case, case.mask_csr(kind, k)))
        assert_bitwise(ov, oi, *case.ref(k, kind), f"k=100 {case.id} mask={kind}")


# ------------------------------------------------------------------ features
@pytest.mark.parametrize("case", (L.WD_FEAT_EXACT, L.WD_FEAT_CERT), ids=lambda c: c.id)
def test_user_and_item_features(case):
    """Integer user features (per call / gathered from the registered table) and an integer
    item table (per call / registered / a strided row view): the fold into Q_i and the wide
    item term, P_u's feature part and the per-user constant -- all the oracle's numbers."""
    m, u = model(case), dev(case.users)
    uf, it = dev(case.user_features), dev(case.item_table)
    wide = torch.full((case.I, case.Fi + 3), 7.0, device=DEV)  # ldf = Fi + 3
    wide[:, :case.Fi] = it
    strided = wide[:, :case.Fi]
    assert strided.stride(0) == case.Fi + 3
    want = L.bits(case.scores)
    try:
        for how in ("passed", "strided", "registered"):
            if how == "registered":
                m.set_user_features(case.user_table)
                m.set_item_features(case.item_table)
            a_uf = None if how == "registered" else uf
            a_it = {"passed": it, "strided": strided, "registered": None}[how]
            got = m.predict_all_items(u, a_uf, a_it).cpu().numpy()
            assert np.array_equal(L.bits(got), want), how
            for k in (case.ks if how == "passed" else (12,)):
                for kind in ("none", "tie_group"):
                    mask = case.mask_csr(kind, k)
                    (ov, oi), stats = with_stats(
                        lambda: wd_topk(case, k, mask, user_features=a_uf, item_features=a_it))
                    say(case, k, f"{kind}/{how}", stats)
                    assert_bitwise(ov, oi, *case.ref(k, kind), f"{case.id} {how} k={k} {kind}")
                    assert stats[0] == (case.B if case.certified else 0), stats
                    if case.certified:
                        assert stats[2] <= case.B // 2, stats
                        assert_bitwise(*wd_topk(case, k, mask, False, None, a_uf, a_it),
                                       *case.ref(k, kind), f"{case.id} {how} exact k={k} {kind}")
            ov, oi = m.recommend_with_scores(u, a_uf, k=L.WD_DENSE_K, item_features=a_it)
            assert_bitwise(ov, oi, *case.ref(L.WD_DENSE_K), f"{case.id} {how} k=100")
    finally:
        m.set_user_features(None)
        m.set_item_features(None)
    rows, items = pairs_of(case)
    pair = m(dev(case.users[rows]), dev(items), dev(case.user_features[rows]),
             dev(case.item_table[items])).cpu().numpy()
    assert np.array_equal(L.bits(pair), L.bits(case.scores[rows, items]))


# ------------------------------------------------------------------ use_wide_user_item=False
def test_no_wide_user_item():
    """The kernels read an all-zero wide vector: scores (an exact zero is +0, as the oracle's),
    pair scores, the certified and the exact top-K."""
    case = L.WD_NOWIDE
    m = model(case)
    got = m.predict_all_items(dev(case.users)).cpu().numpy()
    assert (case.scores == 0).any()  # zeros occur: their sign is compared
    assert np.array_equal(L.bits(got), L.bits(case.scores))
    rows, items = pairs_of(case)
    pair = m(dev(case.users[rows]), dev(items)).cpu().numpy()
    assert np.array_equal(L.bits(pair), L.bits(case.scores[rows, items]))
    for k in case.ks:
        for kind in ("none", "tie_group", "dups_oob"):
            mask = case.mask_csr(kind, k)
            (ov, oi), stats = with_stats(lambda: wd_topk(case, k, mask))
            say(case, k, kind, stats)
            assert_bitwise(ov, oi, *case.ref(k, kind), f"{case.id} certified k={k} {kind}")
            assert stats[0] == case.B and stats[2] <= case.B // 2, stats
            assert_bitwise(*wd_topk(case, k, mask, prefilter=False), *case.ref(k, kind),
                           f"{case.id} exact k={k} {kind}")


# ------------------------------------------------------------------ determinism
def test_certified_is_deterministic():
    case, k = L.WD_CERT[(48, 200, 100)], 12
    mask = case.mask_csr("random", k)
    a = [t.cpu().numpy() for t in wd_topk(case, k, mask)]
    b = [t.cpu().numpy() for t in wd_topk(case, k, mask)]
    assert np.array_equal(L.bits(a[0]), L.bits(b[0])) and np.array_equal(a[1], b[1])
