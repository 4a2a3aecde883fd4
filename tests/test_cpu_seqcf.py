"""CPU-side checks of SequentialCF (no GPU): exports, the ABI entry, the serving dispatch,
`UserSequence` on the CPU device, the gap table, host-side refusals, and the oracle
(seqcf_oracle.py) against three hand-computed cases."""
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import hnm_recommendation_amd as pkg
from hnm_recommendation_amd import ItemCF, SequentialCF, UserHistory, UserSequence, _lib, build, models
from hnm_recommendation_amd.models.sequential_cf import gap_table
from hnm_recommendation_amd.serving import _DISPATCH, Recommender, create_model_from_checkpoint
from seqcf_oracle import np_gap_table, np_seq_events, np_seqcf_fit

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "hnm_seqcf_fit_f32"
ONE = 32768


def test_exported_built_and_dispatched():
    for name in ("SequentialCF", "UserSequence"):
        assert name in pkg.__all__ and name in models.__all__
        assert getattr(pkg, name) is getattr(models, name)
    assert "seqcf.hip" in build.SOURCES
    assert dict(_DISPATCH)["sequential_cf"] is SequentialCF
    assert dict(_DISPATCH)["item_cf"] is ItemCF
    assert sum(key in "runs/sequential_cf" for key, _ in _DISPATCH) == 1   # no other name matches


def test_header_and_lib_agree_on_the_entry():
    header = open(os.path.join(REPO, "include", "hnm.h")).read()
    assert re.search(r"^hnm_status\s+%s\s*\(" % SYMBOL, header, re.M)
    assert SYMBOL in _lib.declared_symbols()
    params = re.search(r"%s\s*\(([^;]*)\);" % SYMBOL, header).group(1)
    assert len(_lib._SIGS[SYMBOL][1]) == params.count(",") + 1 == 16
    if os.path.exists(_lib.LIB_PATH):
        assert hasattr(_lib.load(), SYMBOL)


# ------------------------------------------------------------------ UserSequence
def seq_arrays(s):
    return (s.seq_ptr.numpy()[:s.num_users + 1], s.seq_item.numpy()[:s.nnz],
            s.seq_day.numpy()[:s.nnz])


def test_user_sequence_sort_order_and_deduplication():
    #     user 1: item 4 twice 9 days ago (one event), item 2 9 days ago, item 7 today, item 4 today
    u = [1, 1, 1, 1, 1, 3, 0]
    i = [4, 4, 2, 7, 4, 5, 6]
    d = [9, 9, 9, 0, 0, 3, 12]
    s = UserSequence.from_interactions(u, i, d, 5, 8, "cpu")
    ptr, item, day = seq_arrays(s)
    assert ptr.tolist() == [0, 1, 5, 5, 6, 6] and ptr.dtype == np.int64
    assert item.tolist() == [6, 2, 4, 4, 7, 5] and item.dtype == np.int32
    assert day.tolist() == [0, 3, 3, 12, 12, 9] and day.dtype == np.int32     # 12 - days_ago
    assert (s.nnz, s.max_len, s.max_days_ago) == (6, 4, 12)
    assert s.device == torch.device("cpu") and (s.num_users, s.num_items) == (5, 8)
    ref = np_seq_events(u, i, d, 5)
    assert all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip((ptr, item, day), ref))
    empty = UserSequence.from_interactions([], [], [], 3, 4, "cpu")
    assert empty.nnz == 0 and empty.max_len == 0 and empty.seq_ptr.tolist() == [0, 0, 0, 0]
    assert empty.seq_item.numel() == 1 and empty.seq_day.numel() == 1        # an address to pass


def test_user_sequence_is_permutation_invariant():
    rng = np.random.Generator(np.random.PCG64(3))
    n, U, I = 500, 40, 30
    u, i, d = rng.integers(0, U, n), rng.integers(0, I, n), rng.integers(0, 60, n)
    a = UserSequence.from_interactions(u, i, d, U, I, "cpu")
    p = rng.permutation(n)
    p = np.concatenate([p, p[:50]])                                # shuffled, 50 given twice
    b = UserSequence.from_interactions(torch.from_numpy(u[p]), torch.from_numpy(i[p]),
                                       torch.from_numpy(d[p]).to(torch.float64), U, I, "cpu")
    assert a.nnz == b.nnz < n
    for x, y in zip(seq_arrays(a), seq_arrays(b)):
        assert np.array_equal(x, y)
    assert all(np.array_equal(x, y) for x, y in zip(seq_arrays(a), np_seq_events(u, i, d, U)))
    ptr, item, day = seq_arrays(a)
    for r in range(U):                                             # (day asc, item asc), distinct
        ev = list(zip(day[ptr[r]:ptr[r + 1]].tolist(), item[ptr[r]:ptr[r + 1]].tolist()))
        assert ev == sorted(set(ev))


def test_user_sequence_refuses_bad_days_and_ids():
    ok = ([0, 1], [1, 2])
    for days in ([0.5, 1.0], [-1, 0], [float("nan"), 0.0], [float("inf"), 0.0], [0, 32768], [1],
                 None):
        with pytest.raises(ValueError):
            UserSequence.from_interactions(*ok, days, 2, 3, "cpu")
    assert UserSequence.from_interactions(*ok, [0.0, 32767.0], 2, 3, "cpu").seq_day.tolist() == \
        [32767, 0]
    for u, i in (([0, 2], [1, 2]), ([0, -1], [1, 2]), ([0, 1], [1, 3]), ([0, 1], [-1, 2])):
        with pytest.raises(IndexError):
            UserSequence.from_interactions(u, i, [0, 0], 2, 3, "cpu")
    with pytest.raises(ValueError):
        UserSequence.from_interactions([0, 1], [1], [0, 0], 2, 3, "cpu")


# ------------------------------------------------------------------ the gap table
def test_gap_table():
    for decay in (0.0, 0.05, 3.0, 700.0):
        t = gap_table(28, decay)
        assert t.dtype == np.uint32 and t.shape == (28,) and t[0] == ONE
        assert np.array_equal(t, np_gap_table(28, decay))
    assert (gap_table(1024, 0.0) == ONE).all()
    t = gap_table(20, 1.0)
    assert t[1] == round(ONE / math.e) and t[10] == 1 and (t[12:] == 0).all()   # 32768 e^-12 = 0.20
    assert (np.diff(t.astype(np.int64)) <= 0).all()
    for bad in ((0, 0.0), (1025, 0.0), (2.5, 0.0), (7, -0.1), (7, float("nan")),
                (7, float("inf"))):
        with pytest.raises(ValueError):
            gap_table(*bad)


# ------------------------------------------------------------------ the module on the host
HPARAMS = ["num_users", "num_items", "num_neighbors", "shrink", "max_history", "max_gap",
           "gap_decay", "repeat_buys", "top_k"]


def test_constructor_state_and_shared_surface():
    assert list(inspect.signature(SequentialCF.__init__).parameters) == ["self"] + HPARAMS
    m = SequentialCF(30, 20)
    assert m.hparams == {"num_users": 30, "num_items": 20, "num_neighbors": 64, "shrink": 0.0,
                         "max_history": 0, "max_gap": 28, "gap_decay": 0.0, "repeat_buys": False,
                         "top_k": 12}
    assert {k: (tuple(v.shape), v.dtype) for k, v in m.state_dict().items()} == {
        "neighbor_idx": ((20, 64), torch.int32), "neighbor_val": ((20, 64), torch.float32),
        "item_count": ((20,), torch.int64)}
    assert m.weighted and m.takes_basket_weights
    assert m.answers_baskets and m.back_fill_short_rows and m.history is None
    for name in ("predict_all_items", "recommend_with_scores", "recommend", "forward",
                 "recommend_for_items", "similar_items", "scoring_route"):
        assert getattr(SequentialCF, name) is getattr(ItemCF, name), name
    for kw in ({"num_neighbors": 0}, {"num_neighbors": 65}, {"shrink": -1.0},
               {"shrink": float("nan")}, {"max_history": -1}, {"max_history": 65536},
               {"max_gap": 0}, {"max_gap": 1025}, {"gap_decay": -0.5},
               {"gap_decay": float("inf")}):
        with pytest.raises(ValueError):
            SequentialCF(30, 20, **kw)
    assert SequentialCF(30, 20, max_history=65535, max_gap=1024).max_history == 65535
    with pytest.raises(RuntimeError, match="not fitted"):
        m.similar_items([1])


def test_fit_refusals_before_a_gpu_is_asked_for():
    m = SequentialCF(3, 5, num_neighbors=2)
    hist = UserHistory.from_interactions([0, 1], [1, 2], 3, 5, "cpu", weights=[1.0, 1.0])
    for call in (lambda: m.fit_history(hist), lambda: m.fit_history()):
        with pytest.raises(TypeError, match="fit_interactions.*fit_sequence"):
            call()
    seq = UserSequence.from_interactions([0, 1], [1, 2], [3, 0], 3, 5, "cpu")
    bare = UserHistory.from_interactions([0, 1], [1, 2], 3, 5, "cpu")
    with pytest.raises(ValueError, match="weights"):
        m.fit_sequence(seq, bare)
    with pytest.raises(TypeError):
        m.fit_sequence(hist, hist)
    with pytest.raises(ValueError, match="sequence built for"):
        m.fit_sequence(UserSequence.from_interactions([0], [1], [0], 4, 5, "cpu"), hist)
    with pytest.raises(ValueError):
        m.fit_interactions([0, 1], [1, 2], [0.5, 1])
    with pytest.raises(ValueError):
        m.fit_interactions([0, 1], [1, 2], [0, 1], recency_decay=-1.0)
    with pytest.raises(IndexError):
        m.fit_interactions([0, 3], [1, 2], [0, 1])
    with pytest.raises(RuntimeError, match="no CPU path|GPU"):
        m.fit_sequence(seq, hist)
    with pytest.raises(RuntimeError, match="no CPU path|GPU"):
        m.fit_interactions([0, 1], [1, 2], [3, 0])
    with pytest.raises(RuntimeError, match="no CPU path|GPU"):
        Recommender(3, 5, device="cpu").add_sequential_cf([0, 1], [1, 2], [3, 0])


def test_hparams_round_trip_through_the_checkpoint_dispatch():
    src = SequentialCF(1, 1, num_neighbors=5, shrink=2.5, max_history=40, max_gap=9,
                       gap_decay=0.25, repeat_buys=True, top_k=7)
    sd = SequentialCF(30, 20, num_neighbors=5).state_dict()
    sd["item_count"][3] = 2
    ck = {"state_dict": sd, "hyper_parameters": dict(src.hparams)}
    m = create_model_from_checkpoint("exp/sequential_cf_v1", ck, 30, 20, "cpu")
    assert type(m) is SequentialCF and (m.num_users, m.num_items) == (30, 20) and not m.training
    want = dict(src.hparams, num_users=30, num_items=20)
    assert m.hparams == want and list(m.hparams) == HPARAMS
    assert (m.num_neighbors, m.shrink, m.max_history, m.max_gap, m.gap_decay, m.repeat_buys,
            m.top_k) == (5, 2.5, 40, 9, 0.25, True, 7)
    assert m.similar_items([3], k=2)[1].tolist() == [[-1, -1]]


# ------------------------------------------------------------------ the oracle, by hand
def f32(x):
    return np.float32(x)


def test_oracle_two_user_chain():
    """User 0: item 0 (day 0), 1 (day 1), 2 (day 3).  User 1: item 0 (day 0), 1 (day 2).
    max_gap 2, gap_q = (32768, 16384).  Pairs: u0 0 -> 1 at gap 1 (32768), 0 -> 2 at gap 3 (too
    far), 1 -> 2 at gap 2 (16384); u1 0 -> 1 at gap 2 (16384)."""
    ptr, item, day = np_seq_events([0, 0, 0, 1, 1], [0, 1, 2, 0, 1], [3, 2, 0, 3, 1], 2)
    assert day.tolist() == [0, 1, 3, 0, 2]
    idx, val, n, sim, T = np_seqcf_fit(ptr, item, day, 3, 2, 0.0, 65535, 2, [ONE, ONE // 2], False)
    assert n.tolist() == [2, 2, 1]
    assert T.tolist() == [[0, ONE + ONE // 2, 0], [0, 0, ONE // 2], [0, 0, 0]]
    assert idx.tolist() == [[1, -1], [2, -1], [-1, -1]]
    assert val.tolist() == [[f32(0.75), 0.0], [f32(0.5 / math.sqrt(2.0)), 0.0], [0.0, 0.0]]
    assert val.dtype == np.float32 and idx.dtype == np.int32
    # shrink enters beside the root: 1.5 T / (sqrt(4) + 2) = 0.375
    assert np_seqcf_fit(ptr, item, day, 3, 2, 2.0, 65535, 2, [ONE, ONE // 2], False)[1][0, 0] == \
        f32(0.375)
    # user 0 holds three events: max_history = 2 drops the user
    idx, val, n, _, T = np_seqcf_fit(ptr, item, day, 3, 2, 0.0, 2, 2, [ONE, ONE // 2], False)
    assert n.tolist() == [1, 1, 0] and T[0, 1] == ONE // 2 and T[1, 2] == 0
    assert idx.tolist() == [[1, -1], [-1, -1], [-1, -1]] and val[0, 0] == f32(0.5)


def test_oracle_gap_exactly_at_and_one_past_max_gap():
    """One user: item 0 (day 0), 1 (day 3), 2 (day 4), max_gap 3: 0 -> 1 is exactly at the limit
    and counts, 0 -> 2 is one past and does not, 1 -> 2 is a day apart."""
    ptr, item, day = np_seq_events([0, 0, 0], [0, 1, 2], [4, 1, 0])
    assert day.tolist() == [0, 3, 4]
    idx, val, n, sim, T = np_seqcf_fit(ptr, item, day, 3, 4, 0.0, 65535, 3, [ONE, 5, 7], False)
    assert T.tolist() == [[0, 7, 0], [0, 0, ONE], [0, 0, 0]]
    assert idx.tolist() == [[1, -1, -1, -1], [2, -1, -1, -1], [-1] * 4]
    assert val[0, 0] == f32(7.0 / 32768.0) and val[1, 0] == f32(1.0)
    # one more day of reach: 0 -> 2 counts too, and at weight 0 a pair is absent
    T4 = np_seqcf_fit(ptr, item, day, 3, 4, 0.0, 65535, 4, [ONE, 5, 0, 9], False)
    assert T4[4].tolist() == [[0, 0, 9], [0, 0, ONE], [0, 0, 0]]
    assert T4[0][0].tolist() == [2, -1, -1, -1]


def test_oracle_repeat_buy_with_and_without_the_flag():
    """One user: item 0 on days 0, 2 and 5, item 1 on day 5; max_gap 5, every weight 1.  0 -> 1:
    from day 0 (gap 5) and day 2 (gap 3), not from day 5 (the same day).  0 -> 0: the three
    ordered pairs of its days, with the flag only."""
    ptr, item, day = np_seq_events([0] * 5, [0, 0, 0, 1, 0], [5, 3, 0, 0, 5])     # one repeated
    assert item.tolist() == [0, 0, 0, 1] and day.tolist() == [0, 2, 5, 5]
    q = [ONE] * 5
    idx, val, n, _, T = np_seqcf_fit(ptr, item, day, 2, 2, 0.0, 65535, 5, q, False)
    assert n.tolist() == [3, 1] and T.tolist() == [[0, 2 * ONE], [0, 0]]
    assert idx.tolist() == [[1, -1], [-1, -1]] and val[0, 0] == f32(2.0 / math.sqrt(3.0))
    idx, val, n, _, T = np_seqcf_fit(ptr, item, day, 2, 2, 0.0, 65535, 5, q, True)
    assert n.tolist() == [3, 1] and T.tolist() == [[3 * ONE, 2 * ONE], [0, 0]]
    assert idx.tolist() == [[1, 0], [-1, -1]]
    assert val[0].tolist() == [f32(2.0 / math.sqrt(3.0)), f32(1.0)]
