"""GPU: hnm_dot_topk_f32 and its two-phase form against the integer oracle, bitwise.

Inputs are lattice tables (tests/lattice.py): integer embeddings, quarter-integer biases, so
the fp32 score is one number whatever the summation order and numpy's integer computation is
a bitwise oracle for every route -- LIST lists + partition merge (I < 8,192), the
sample-threshold path with its select kernel and overflow fallback (pre-filter off), the
certified f16 scan with re-scoring and its fallback (pre-filter on).  Scores take ~50 values,
so most rows tie across position k and the (score desc, id asc) order decides the answer.
tests/test_cpu_lattice.py checks those properties of the inputs on the CPU.
"""
import functools

import numpy as np
import pytest
import torch

import lattice as L
from hnm_recommendation_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD_FILL = 1000.0  # in the columns past d of a padded table: a kernel that reads them is off


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def padded(tab, extra):
    t = torch.full((tab.shape[0], tab.shape[1] + extra), PAD_FILL, device=DEV)
    t[:, :tab.shape[1]] = dev(tab)
    return t


@functools.lru_cache(maxsize=None)
def device_case(case):
    t = case.tables
    ut = padded(t["ut"], 4 if case.pad else 0)   # ldu = d + 4
    it = padded(t["it"], 8 if case.pad else 0)   # ldi = d + 8
    mptr, midx = case.mask_csr
    return dict(ut=ut, it=it, ids=dev(case.users), ub=dev(t["ub"]), ib=dev(t["ib"]),
                cb=dev(t["cb"]), mptr=dev(mptr), midx=dev(midx))


def common(case, g, mask=True):
    a = [_lib.ctx(g["ids"].device), _lib.ptr(g["ut"]), g["ut"].shape[0], g["ut"].stride(0),
         _lib.ptr(g["ids"]), case.B, _lib.ptr(g["it"]), case.I, g["it"].stride(0), case.d,
         _lib.ptr(g["ub"]), _lib.ptr(g["ib"]), _lib.ptr(g["cb"])]
    if mask:
        a += [_lib.ptr(g["mptr"]), _lib.ptr(g["midx"])]
    return a


def outputs(case):
    return (torch.empty(case.B, case.k, device=DEV),
            torch.empty(case.B, case.k, dtype=torch.int64, device=DEV))


def dot_topk(case):
    g = device_case(case)
    ov, oi = outputs(case)
    _lib.check(_lib.fn("hnm_dot_topk_f32")(*common(case, g), case.k, _lib.ptr(ov), _lib.ptr(oi)),
               "hnm_dot_topk_f32")
    _lib.sync_check(ov.device)
    return ov.cpu().numpy(), oi.cpu().numpy()


def with_stats(fn):
    dev_ = torch.device(DEV)
    _lib.prefilter_stats(dev_, reset=True)
    _lib.set_option(dev_, _lib.HNM_OPT_STATS, 1)
    try:
        out = fn()
    finally:
        _lib.set_option(dev_, _lib.HNM_OPT_STATS, 0)
    return out, _lib.prefilter_stats(dev_, reset=True)


def assert_is_oracle(case, ov, oi, what):
    rv, ri = case.ref
    if not np.array_equal(oi, ri):
        b = int(np.argwhere((oi != ri).any(1))[0, 0])
        raise AssertionError(f"{what} {case.id}: ids differ in {int((oi != ri).any(1).sum())} rows, "
                             f"first row {b}: got {oi[b]} scores {ov[b]}, want {ri[b]} scores {rv[b]}")
    assert np.array_equal(L.bits(ov), L.bits(rv)), f"{what} {case.id}: score bits differ"


@pytest.mark.parametrize("prefilter", (False, True), ids=("exact", "certified"))
@pytest.mark.parametrize("case", L.DOT_CASES, ids=[c.id for c in L.DOT_CASES])
def test_dot_topk_is_the_oracle(case, prefilter):
    d0 = torch.device(DEV)
    _lib.set_prefilter(d0, prefilter)
    try:
        (ov, oi), stats = with_stats(lambda: dot_topk(case))
    finally:
        _lib.set_prefilter(d0, True)
    assert_is_oracle(case, ov, oi, "certified" if prefilter else "exact")
    if case.mask in ("all", "mixed"):  # a fully masked row: -inf, the lowest ids
        ptr = case.mask_csr[0]
        full = [b for b in range(case.B)
                if len(np.unique(case.mask_csr[1][ptr[b]:ptr[b + 1]])) >= case.I]
        assert full
        for b in full:
            assert oi[b].tolist() == list(range(case.k)) and np.isneginf(ov[b]).all()
    if case.kind == "clustered" and case.mask == "none":
        b = int(np.nonzero(case.users == 0)[0][0])  # the cluster's user: the block's first k
        assert oi[b].tolist() == list(range(2000, 2000 + case.k))
    if not prefilter and case.I >= L.THRESH_MIN_ITEMS and case.mask == "none":
        # the sample-threshold path: which kernel answered is known from the inputs alone
        # (test_cpu_lattice.py): the select kernel for every sparse-tie row, with exactly the
        # items at or above the sample's k-th score appended; the overflow fallback for the rest
        rows, cands, fallback = stats
        n = L.thresh_counts(case)
        over = (n > L.thresh_cap(case.I, case.k)) | (n < case.k)
        print(f"{case.id}: threshold path rows {rows}, appended {cands}, fallback rows {fallback}")
        assert rows == case.B and fallback == int(over.sum()) and cands == int(n[~over].sum())
        assert fallback == (0 if case.kind == "sparse" else case.B) or case.kind == "clustered"
    if prefilter and case.I >= 8192:
        rows, cands, fallback = stats
        print(f"{case.id}: rows {rows}, candidates {cands}, fallback rows {fallback}")
        assert rows == case.B
        if case is L.SPARSE_STATS_CASE:
            # the certified candidate set is ~150 items a row spread over the partitions
            # (test_cpu_lattice.py's bound-width check): the scan, not the fallback, answers
            assert fallback <= case.B // 2, fallback
        if case.kind in ("clustered", "dense"):
            assert fallback >= 1, fallback


@pytest.mark.parametrize("case", L.DOT_CASES, ids=[c.id for c in L.DOT_CASES])
def test_dot_scores_are_the_oracle(case):
    """hnm_dot_scores_f32 == the oracle matrix, bitwise: the exactness claim on the GPU side."""
    g = device_case(case)
    ldo = case.I + (5 if case.pad else 0)
    out = torch.full((case.B, ldo), -7.0, device=DEV)
    _lib.check(_lib.fn("hnm_dot_scores_f32")(*common(case, g, mask=False), _lib.ptr(out), ldo),
               "hnm_dot_scores_f32")
    _lib.sync_check(out.device)
    got = out.cpu().numpy()
    assert np.array_equal(L.bits(got[:, :case.I]), L.bits(case.scores))
    assert (got[:, case.I:] == -7.0).all()


# ------------------------------------------------------------------ two-phase API
def begin(case, g, lists):
    name = "hnm_dot_topk_begin_lists_f32" if lists else "hnm_dot_topk_begin_f32"
    out = torch.empty((case.B, case.k) if lists else (case.B,), device=DEV)
    _lib.check(_lib.fn(name)(*common(case, g), case.k, _lib.ptr(out)), name)
    return out


def finish(case, g, bound, short_ok):
    ov, oi = outputs(case)
    lb = dev(np.asarray(bound, np.float32))
    _lib.check(_lib.fn("hnm_dot_topk_finish_f32")(*common(case, g), case.k, _lib.ptr(lb), short_ok,
                                                  _lib.ptr(ov), _lib.ptr(oi)),
               "hnm_dot_topk_finish_f32")
    _lib.sync_check(ov.device)
    return ov.cpu().numpy(), oi.cpu().numpy()


def test_two_phase_begin_bounds():
    case = L.TWO_PHASE_DOT_CASE
    g = device_case(case)
    rv, _ = case.ref
    try:
        lb = begin(case, g, lists=False)
        lb = lb.cpu().numpy()
        assert np.isfinite(lb).any(), "the certified begin phase must produce bounds here"
        assert (lb <= rv[:, -1]).all(), np.max(lb - rv[:, -1])
        ov, oi = finish(case, g, lb, 0)          # its own bound: the one-shot result
        assert_is_oracle(case, ov, oi, "finish(begin's bound)")
        ll = begin(case, g, lists=True)
        ll = ll.cpu().numpy()
        assert (np.diff(ll, axis=1) <= 0).all(), "begin_lists rows must be descending"
        assert (ll <= rv).all(), "entry j bounds the j-th best from below"
    finally:
        _lib.abort_pending(torch.device(DEV))


def test_two_phase_finish_tightest_bound():
    """lower_bound = the exact k-th score, with tied items sitting on it: nothing on the bound
    may be dropped -- bitwise the one-shot result."""
    case = L.TWO_PHASE_DOT_CASE
    g = device_case(case)
    rv, _ = case.ref
    assert L.tie_fraction(case.scores, case.k) >= 0.5
    try:
        begin(case, g, lists=False)
        ov, oi = finish(case, g, rv[:, -1], 0)
    finally:
        _lib.abort_pending(torch.device(DEV))
    assert_is_oracle(case, ov, oi, "finish(exact k-th)")


@pytest.mark.parametrize("j", (1, 5))
def test_two_phase_finish_bound_above_kth_short_rows(j):
    """lower_bound = the j-th best score (j < k) with short_ok = 1: a prefix of the oracle's
    top-k holding at least every item scoring >= the bound, then only (-inf, -1)."""
    case = L.TWO_PHASE_DOT_CASE
    g = device_case(case)
    rv, ri = case.ref
    bound = rv[:, j - 1].copy()
    try:
        begin(case, g, lists=True)
        ov, oi = finish(case, g, bound, 1)
    finally:
        _lib.abort_pending(torch.device(DEV))
    L.assert_short_rows(ov, oi, rv, ri, bound)
