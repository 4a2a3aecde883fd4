"""GPU: NeuralCF against the integer oracle, bitwise.

`NeuralCF` loaded from lattice.ncf_state_dict: sparse ternary weights and integer biases, so
every intermediate of the score is a small integer and the fp32 score is the same number in
any order -- lattice.ncf_scores is a bitwise oracle for the small-catalogue kernels, the exact
scan, the certified f16 scan in every layout / loop / epilogue variant, the deep tower and the
two-phase API.  Scores take ~70 values: most rows tie across position k, so the
(score desc, id asc) order decides them (tests/test_cpu_lattice.py checks that on the CPU).
Wide&Deep's oracle: tests/test_gpu_lattice_widedeep.py.
"""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest
import torch

import lattice as L
from hnm_recommendation_amd import NeuralCF, _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
DEFAULTS = {_lib.HNM_OPT_PREFILTER: 1, _lib.HNM_OPT_STRIDED: 0, _lib.HNM_OPT_DEEP_MFMA: 1,
            _lib.HNM_OPT_NCF_TABLES: 1, _lib.HNM_OPT_SCAN_SHAPE: 1, _lib.HNM_OPT_SCAN_PIPE: 1,
            _lib.HNM_OPT_SCAN_SPARSE: 1, _lib.HNM_OPT_STATS: 0}


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class options:
    """Set ctx options for a block; every option back at its default afterwards."""

    def __init__(self, **kw):
        self.opts = {getattr(_lib, "HNM_OPT_" + k): v for k, v in kw.items()}

    def __enter__(self):
        for o, v in self.opts.items():
            _lib.set_option(torch.device(DEV), o, v)

    def __exit__(self, *exc):
        for o in self.opts:
            _lib.set_option(torch.device(DEV), o, DEFAULTS[o])


@functools.lru_cache(maxsize=None)
def model(case):
    m = NeuralCF(case.U, case.I, mf_dim=64, mlp_dims=list(case.mlp_dims))
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in case.sd.items()})
    return m.to(DEV).eval()


def ncf_topk(case, k, mask=(None, None), entry="hnm_ncf_topk_f32"):
    """The C entry with a CSR mask as is (duplicates and ids >= I included)."""
    m = model(case)
    w, keep = m._weights() if m._fused() else m._deep_weights()
    u = dev(case.users)
    mptr, midx = dev(mask[0]), dev(mask[1])
    ov = torch.empty(case.B, k, device=DEV)
    oi = torch.empty(case.B, k, dtype=torch.int64, device=DEV)
    _lib.check(_lib.fn(entry)(_lib.ctx(u.device), C.byref(w), _lib.ptr(u), case.B, _lib.ptr(mptr),
                              _lib.ptr(midx), k, _lib.ptr(ov), _lib.ptr(oi)), entry)
    _lib.sync_check(u.device)
    return ov.cpu().numpy(), oi.cpu().numpy()


def assert_is_oracle(ov, oi, ref, what):
    rv, ri = ref
    ov, oi = np.asarray(ov), np.asarray(oi)
    if not np.array_equal(oi, ri):
        b = int(np.argwhere((oi != ri).any(1))[0, 0])
        raise AssertionError(f"{what}: ids differ in {int((oi != ri).any(1).sum())} rows, first "
                             f"row {b}: got {oi[b]} scores {ov[b]}, want {ri[b]} scores {rv[b]}")
    assert np.array_equal(L.bits(ov), L.bits(rv)), f"{what}: score bits differ"


# ------------------------------------------------------------------ small catalogue
def test_small_predict_all_items_and_forward():
    case = L.NCF_SMALL
    m = model(case)
    u = dev(case.users)
    got = m.predict_all_items(u).cpu().numpy()
    assert np.array_equal(L.bits(got), L.bits(case.scores))
    rng = np.random.default_rng(3)
    pu, pi = rng.integers(0, case.U, 777), rng.integers(0, case.I, 777)
    pair = m(dev(pu), dev(pi)).cpu().numpy()
    assert np.array_equal(L.bits(pair), L.bits(L.ncf_scores(case.sd, pu, pi)))


@pytest.mark.parametrize("k", L.NCF_SMALL_KS)
@pytest.mark.parametrize("kind", ("none", "tie_group"))
def test_small_recommend(kind, k):
    """recommend_with_scores at 1,500 items: the fused exact scan (k <= 64) and dense scores +
    the row top-K (k = 100), with and without a filter that removes the tie group at k."""
    case = L.NCF_SMALL
    m = model(case)
    mask = case.mask_csr(kind, k)
    f = None
    if mask[0] is not None:
        f = {int(u): set(mask[1][mask[0][b]:mask[0][b + 1]].tolist())
             for b, u in enumerate(case.users)}
    ov, oi = m.recommend_with_scores(dev(case.users), filter_items=f, k=k)
    assert_is_oracle(ov.cpu().numpy(), oi.cpu().numpy(), case.ref(k, kind), f"small k={k} {kind}")


# ------------------------------------------------------------------ certified route
SCAN_VARIANTS = [dict(SCAN_SHAPE=0)] + [dict(SCAN_SHAPE=1, SCAN_PIPE=p, SCAN_SPARSE=s)
                                        for p in (0, 1) for s in (0, 1)]


@pytest.mark.parametrize("I,B", list(L.NCF_CERT), ids=lambda v: str(v))
def test_certified_route_every_variant(I, B):
    """Exact scan and the certified scan in each layout / loop / epilogue / table-build / sample
    variant: every result is the oracle's (so all are identical).  Batches below 16 rows take the
    exact scan whatever the options: they run the pre-filter switch alone."""
    case = L.NCF_CERT[(I, B)]
    for k in L.NCF_CERT_KS:
        for kind in ("none", "mixed"):
            mask, ref = case.mask_csr(kind, k), case.ref(k, kind)
            with options(PREFILTER=0):
                ov, oi = ncf_topk(case, k, mask)
            assert_is_oracle(ov, oi, ref, f"exact {case.id} k={k} {kind}")
            variants = SCAN_VARIANTS if B >= 16 else [dict()]
            for scan, tables, strided in itertools.product(variants, (0, 1), (0, 1)):
                if B < 16 and (tables, strided) != (1, 0):
                    continue
                with options(NCF_TABLES=tables, STRIDED=strided, **scan):
                    ov, oi = ncf_topk(case, k, mask)
                assert_is_oracle(ov, oi, ref, f"certified {case.id} k={k} {kind} {scan} "
                                              f"tables={tables} strided={strided}")


def test_certified_route_runs_the_scan():
    """The certified cases above are answered by the scan, not only by its fallback."""
    case = L.NCF_CERT[(9001, 130)]
    d0 = torch.device(DEV)
    _lib.prefilter_stats(d0, reset=True)
    with options(STATS=1):
        ov, oi = ncf_topk(case, 12)
    rows, cands, fallback = _lib.prefilter_stats(d0, reset=True)
    print(f"NeuralCF lattice {case.id} k=12: rows {rows}, candidates {cands}, fallback {fallback}")
    assert_is_oracle(ov, oi, case.ref(12), "stats run")
    assert rows == case.B and fallback <= case.B // 2



# ------------------------------------------------------------------ deep tower
@pytest.mark.parametrize("deep_mfma", (0, 1))
@pytest.mark.parametrize("prefilter", (0, 1))
def test_deep_tower(prefilter, deep_mfma):
    """A 3-layer tower (128, 64, 32, 16) at 8,200 items: dense scores and top-12 with the
    certified deep scan (pre-filter on, B >= 16) and both exact kernels."""
    case = L.NCF_DEEP
    m = model(case)
    with options(PREFILTER=prefilter, DEEP_MFMA=deep_mfma):
        got = m.predict_all_items(dev(case.users)).cpu().numpy()
        assert np.array_equal(L.bits(got), L.bits(case.scores))
        for kind in ("none", "mixed"):
            ov, oi = ncf_topk(case, 12, case.mask_csr(kind, 12), entry="hnm_ncf_deep_topk_f32")
            assert_is_oracle(ov, oi, case.ref(12, kind), f"deep {kind} prefilter={prefilter} "
                                                         f"mfma={deep_mfma}")


# ------------------------------------------------------------------ two-phase API
class TwoPhase:
    def __init__(self, case, k):
        self.case, self.k = case, k
        self.m = model(case)
        self.w, self.keep = self.m._weights()
        self.u = dev(case.users)

    def begin(self, lists):
        name = "hnm_ncf_topk_begin_lists_f32" if lists else "hnm_ncf_topk_begin_f32"
        out = torch.empty((self.case.B, self.k) if lists else (self.case.B,), device=DEV)
        _lib.check(_lib.fn(name)(_lib.ctx(self.u.device), C.byref(self.w), _lib.ptr(self.u),
                                 self.case.B, None, None, self.k, _lib.ptr(out)), name)
        return out

    def finish(self, bound, short_ok):
        lb = dev(np.asarray(bound, np.float32))
        ov = torch.empty(self.case.B, self.k, device=DEV)
        oi = torch.empty(self.case.B, self.k, dtype=torch.int64, device=DEV)
        _lib.check(_lib.fn("hnm_ncf_topk_finish_f32")(
            _lib.ctx(self.u.device), C.byref(self.w), _lib.ptr(self.u), self.case.B, None, None,
            self.k, _lib.ptr(lb), short_ok, _lib.ptr(ov), _lib.ptr(oi)), "hnm_ncf_topk_finish_f32")
        _lib.sync_check(self.u.device)
        return ov.cpu().numpy(), oi.cpu().numpy()


def test_two_phase_begin_bounds():
    case, k = L.NCF_TWO_PHASE, 12
    rv, _ = case.ref(k)
    t = TwoPhase(case, k)
    try:
        lb = t.begin(lists=False)
        lb = lb.cpu().numpy()
        assert np.isfinite(lb).any(), "the certified begin phase must produce bounds here"
        assert (lb <= rv[:, -1]).all(), np.max(lb - rv[:, -1])
        ov, oi = t.finish(lb, 0)
        assert_is_oracle(ov, oi, case.ref(k), "finish(begin's bound)")
        ll = t.begin(lists=True)
        ll = ll.cpu().numpy()
        assert (np.diff(ll, axis=1) <= 0).all(), "begin_lists rows must be descending"
        assert (ll <= rv).all(), "entry j bounds the j-th best from below"
    finally:
        _lib.abort_pending(torch.device(DEV))


def test_two_phase_finish_tightest_bound():
    """lower_bound = the exact k-th score with tied items sitting on it, short_ok = 0: bitwise
    the one-shot result."""
    case, k = L.NCF_TWO_PHASE, 12
    rv, _ = case.ref(k)
    t = TwoPhase(case, k)
    try:
        t.begin(lists=False)
        ov, oi = t.finish(rv[:, -1], 0)
    finally:
        _lib.abort_pending(torch.device(DEV))
    assert_is_oracle(ov, oi, case.ref(k), "finish(exact k-th)")


@pytest.mark.parametrize("j", (1, 5))
def test_two_phase_finish_bound_above_kth_short_rows(j):
    case, k = L.NCF_TWO_PHASE, 12
    rv, ri = case.ref(k)
    bound = rv[:, j - 1].copy()
    t = TwoPhase(case, k)
    try:
        t.begin(lists=True)
        ov, oi = t.finish(bound, 1)
    finally:
        _lib.abort_pending(torch.device(DEV))
    L.assert_short_rows(ov, oi, rv, ri, bound)
