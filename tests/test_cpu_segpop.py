"""CPU-side checks of SegmentPopularity (no GPU): the oracle against a brute-force dict
implementation, `age_segments`, the constructor and argument errors, the two ABI entries, and
the host side of `Recommender(cold_start="segment")`."""
import inspect
import os
import re
from collections import defaultdict

import numpy as np
import pytest
import torch

import segpop_oracle as SO
import hnm_recommendation_amd as pkg
from hnm_recommendation_amd import NeuralCF, SegmentPopularity, _lib, age_segments, models
from hnm_recommendation_amd.serving import Recommender

SYMBOLS = ("hnm_segpop_fit_f64", "hnm_segpop_topk_f32")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the oracle itself
def brute_fit(items, users, useg, days, w, I, S, D):
    """Transaction by transaction into dicts keyed (row, item) -> {day: n}; then the chain."""
    cells = defaultdict(lambda: defaultdict(int))
    for r in range(len(items)):
        it, u = int(items[r]), int(users[r])
        if not (0 <= it < I and 0 <= u < len(useg)) or useg[u] >= S:
            continue
        d = 0 if days is None else int(days[r])
        if not 0 <= d < D:
            continue
        cells[(S, it)][d] += 1
        if useg[u] >= 0:
            cells[(int(useg[u]), it)][d] += 1
    count = np.zeros((S + 1, I), np.int64)
    pop = np.zeros((S + 1, I), np.float64)
    for (s, it), per_day in cells.items():
        acc = np.float64(0.0)
        for d in range(D):
            acc = acc + np.float64(per_day.get(d, 0)) * np.float64(w[d])
        count[s, it], pop[s, it] = sum(per_day.values()), acc
    return count, pop


def brute_topk(order_list, val_list, seg, hist, k):
    S = len(order_list) - 1
    out = []
    if 0 <= seg < S:
        for x, v in zip(order_list[seg].tolist(), val_list[seg].tolist()):
            if x not in hist and len(out) < k:
                out.append((v, x))
    nseg = len(out)
    for x, v in zip(order_list[S].tolist(), val_list[S].tolist()):
        if x not in hist and x not in [i for _, i in out] and len(out) < k:
            out.append((v, x))
    return out, nseg


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("S", [1, 4])
def test_oracle_equals_brute_force(seed, S):
    rng = np.random.Generator(np.random.PCG64(seed))
    I, U, D, n = 30, 40, 9, 600
    items = rng.integers(-1, I + 1, size=n)
    users = rng.integers(-1, U + 1, size=n)
    days = rng.integers(-1, D + 2, size=n)
    useg = rng.integers(-1, S + 1, size=U)           # S itself: out of range
    w = np.exp(-0.05 * np.arange(D))
    count, pop, skipped = SO.fit(items, users, useg, days, w, I, S, D)
    bc, bp = brute_fit(items, users, useg, days, w, I, S, D)
    assert skipped > 0 and np.array_equal(count, bc)
    assert np.array_equal(pop.view(np.int64), bp.view(np.int64))
    known = (useg >= 0) & (useg < S)
    assert count[:S].sum() <= count[S].sum() and known.any()
    for mc in (1, 3):
        ol, vl, rank = SO.orders(count, pop, mc)
        for s in range(S + 1):
            want = sorted((i for i in range(I) if count[s, i] >= (mc if s < S else 1)),
                          key=lambda i: (-pop[s, i], i))
            assert ol[s].tolist() == want
            assert [int(rank[s, i]) for i in want] == list(range(len(want)))
            assert (rank[s] >= 0).sum() == len(want)
        segs = rng.integers(-1, S + 1, size=12)      # S: answered as no segment
        rows = [rng.integers(0, I, size=int(rng.integers(0, 25))).tolist() for _ in segs]
        for k in (1, 5, I):
            v, i, ns = SO.topk(ol, vl, segs, rows, k)
            for b in range(len(segs)):
                got, nseg = brute_topk(ol, vl, int(segs[b]), set(rows[b]), k)
                assert i[b, :len(got)].tolist() == [x for _, x in got] and ns[b] == nseg
                assert v[b, :len(got)].tolist() == [np.float32(x) for x, _ in got]
                assert (i[b, len(got):] == -1).all() and np.isneginf(v[b, len(got):]).all()


def test_plain_counts_without_days():
    items, users = np.array([1, 1, 2, 0, 1]), np.array([0, 1, 2, 2, 3])
    count, pop, skipped = SO.fit(items, users, [0, 1, -1, 0], None, np.ones(1), 3, 2, 1)
    assert skipped == 0 and count.tolist() == [[0, 2, 0], [0, 1, 0], [1, 3, 1]]
    assert np.array_equal(pop, count.astype(np.float64))


# ------------------------------------------------------------------ age_segments
def test_age_segments_edges_nan_and_negatives():
    ages = [0, 24, 24.9, 25, 34, 35, 44.5, 45, 54, 55, 64, 65, 99, np.nan, -1, -0.5]
    out = age_segments(ages)
    assert out.dtype == np.int32
    assert out.tolist() == [0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, -1, -1, -1]
    assert age_segments(torch.tensor([30.0, float("nan")]).numpy()).tolist() == [1, -1]
    assert age_segments([17, 18, 70], edges=(18,)).tolist() == [0, 1, 1]
    assert age_segments([5, np.nan], edges=()).tolist() == [0, -1]
    assert age_segments([]).shape == (0,)
    assert age_segments(np.array([20, 40], np.int64)).tolist() == [0, 2]
    with pytest.raises(ValueError):
        age_segments([1], edges=(30, 20))
    with pytest.raises(ValueError):
        age_segments([1], edges=(20, np.nan))


# ------------------------------------------------------------------ module surface
def test_exported_and_constructor():
    assert "SegmentPopularity" in pkg.__all__ and "SegmentPopularity" in models.__all__
    assert "age_segments" in pkg.__all__ and pkg.SegmentPopularity is models.SegmentPopularity
    names = list(inspect.signature(SegmentPopularity.__init__).parameters)
    assert names == ["self", "n_items", "n_segments", "k", "time_decay", "min_count"]
    m = SegmentPopularity(50, 6)
    assert m.hparams == {"n_items": 50, "n_segments": 6, "k": 12, "time_decay": 0.0,
                         "min_count": 1}
    assert (m.num_items, m.num_segments, m.top_k, m.min_count) == (50, 6, 12, 1)
    assert m.metrics.top_k == 12 and not m.back_fill_short_rows and not m.answers_baskets
    assert list(m.parameters()) == [] and m.state_dict() == {}
    assert m.device == torch.device("cpu") and m.order is None and m.user_segment is None
    m.load_state_dict({})
    for bad in (dict(n_segments=0), dict(n_segments=-2), dict(n_segments=3, min_count=0),
                dict(n_segments=3, time_decay=-0.1), dict(n_segments=3, time_decay=float("nan"))):
        with pytest.raises(ValueError):
            SegmentPopularity(10, **bad)
    with pytest.raises(TypeError):
        SegmentPopularity(10)


def test_not_fitted_argument_errors_and_no_cpu_path():
    m = SegmentPopularity(10, 3)
    for call in (lambda: m.recommend([0, 1]), lambda: m.forward(torch.tensor([0])),
                 lambda: m.recommend_with_scores(torch.tensor([0])),
                 lambda: m.recommend_for_segments([0, None, -1]), lambda: m.global_baseline()):
        with pytest.raises(RuntimeError, match="not fitted"):
            call()
    # a request segment outside [-1, S) is a ValueError before anything else is looked at
    for bad in ([3], [0, -2], torch.tensor([1, 7])):
        with pytest.raises(ValueError, match=r"\[-1, 3\)"):
            m.recommend_for_segments(bad)
    with pytest.raises(RuntimeError, match="no CPU path|GPU"):
        m.fit_interactions([1, 2, 3], [0, 1, 2], [0, 1, 2])


def test_abi_entries_declared_in_header_and_lib():
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "hnm.h")).read()
    for s in SYMBOLS:
        assert s in _lib.declared_symbols()
        assert re.search(rf"^hnm_status\s+{s}\s*\(", header, re.M), s
        assert hasattr(lib, s), s
    # one ctypes argument per parameter of the header's declaration
    for s in SYMBOLS:
        decl = re.search(rf"^hnm_status\s+{s}\s*\((.*?)\);", header, re.M | re.S).group(1)
        assert len(decl.split(",")) == len(_lib._SIGS[s][1]), s


# ------------------------------------------------------------------ serving, host side
def test_cold_start_segment_needs_the_model_and_a_valid_segment():
    srv = Recommender(20, 40, device="cpu", cold_start="segment")
    assert srv.cold_start == "segment"
    srv.add_model("neural_cf", NeuralCF(20, 40))
    for call in (lambda: srv.get_recommendations(99, segment=1),
                 lambda: srv.get_recommendations(99),
                 lambda: srv.get_batch_recommendations([1, 99], segments=[None, 2])):
        with pytest.raises(ValueError, match="add_segment_popularity"):
            call()
    srv.add_model("segment_popularity", SegmentPopularity(40, 3))     # registered, not fitted
    # outside [-1, S), or not an integer: ValueError on the host, before the model is asked
    for bad in (3, -2, 1.0, True, "1"):
        with pytest.raises(ValueError, match="segment"):
            srv.get_recommendations(99, segment=bad)
        with pytest.raises(ValueError, match="segment"):
            srv.get_batch_recommendations([99, 1], segments=[0, bad])
    with pytest.raises(ValueError, match="one entry per user"):
        srv.get_batch_recommendations([99, 1], segments=[0])
    # valid segments reach the (unfitted) model
    for seg in (None, -1, 0, 2):
        with pytest.raises(RuntimeError, match="not fitted"):
            srv.get_recommendations(99, segment=seg)
    with pytest.raises(RuntimeError, match="not fitted"):
        srv.get_batch_recommendations([99, "nobody"], segments=[2, None])
    with pytest.raises(ValueError, match="num_items"):
        srv.get_recommendations(99, segment=0, num_items=0)


def test_other_cold_start_modes_are_unchanged():
    with pytest.raises(ValueError):
        Recommender(20, 10, device="cpu", cold_start="segments")
    for mode in ("error", "popularity"):
        srv = Recommender(20, 10, device="cpu", cold_start=mode)
        srv.add_model("neural_cf", NeuralCF(20, 10))
        srv.add_model("segment_popularity", SegmentPopularity(10, 3))
        with pytest.raises(ValueError, match='cold_start="segment"'):
            srv.get_recommendations(99, segment=1)
        with pytest.raises(ValueError, match='cold_start="segment"'):
            srv.get_batch_recommendations([99], segments=[1])
    err = Recommender(20, 10, device="cpu")
    err.add_model("neural_cf", NeuralCF(20, 10))
    with pytest.raises(ValueError, match="user 99 not found"):
        err.get_recommendations(99)
    with pytest.raises(ValueError, match="user 99 not found"):
        err.get_recommendations(99, segment=None)
    pop = Recommender(20, 10, device="cpu", cold_start="popularity")
    pop.add_model("neural_cf", NeuralCF(20, 10))
    with pytest.raises(ValueError, match="popularity_baseline"):
        pop.get_batch_recommendations([1, 99], segments=[None, None])
