"""CPU-side checks of ContentKNN (no GPU): exports, the ABI entry, the serving dispatch, host-side
argument validation, and the oracle (content_oracle.py) against a hand-computed example and its
own invariants."""
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import hnm_recommendation_amd as pkg
from content_oracle import np_content_fit, np_weights
from hnm_recommendation_amd import ContentKNN, ItemCF, _lib, build, models
from hnm_recommendation_amd import synthetic as syn
from hnm_recommendation_amd.models.content_knn import encode_attributes
from hnm_recommendation_amd.serving import _DISPATCH, Recommender, create_model_from_checkpoint

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "hnm_content_fit_f32"
Q1 = 1 << 20


def test_exported_built_and_dispatched():
    assert "ContentKNN" in pkg.__all__ and "ContentKNN" in models.__all__
    assert pkg.ContentKNN is models.ContentKNN
    assert "content.hip" in build.SOURCES
    assert dict(_DISPATCH)["content_knn"] is ContentKNN
    assert dict(_DISPATCH)["item_cf"] is ItemCF


def test_header_lib_and_library_agree_on_the_entry():
    header = open(os.path.join(REPO, "include", "hnm.h")).read()
    assert re.search(r"^hnm_status\s+%s\s*\(" % SYMBOL, header, re.M)
    assert SYMBOL in _lib.declared_symbols() and hasattr(_lib.load(), SYMBOL)
    params = re.search(r"%s\s*\(([^;]*)\);" % SYMBOL, header).group(1)
    assert len(_lib._SIGS[SYMBOL][1]) == params.count(",") + 1 == 11


def test_constructor_state_and_shared_surface():
    names = list(inspect.signature(ContentKNN.__init__).parameters)
    assert names == ["self", "num_users", "num_items", "num_neighbors", "weighting", "top_k"]
    m = ContentKNN(30, 20)
    assert m.hparams == {"num_users": 30, "num_items": 20, "num_neighbors": 64,
                         "weighting": "idf", "top_k": 12}
    assert {k: (tuple(v.shape), v.dtype) for k, v in m.state_dict().items()} == {
        "neighbor_idx": ((20, 64), torch.int32), "neighbor_val": ((20, 64), torch.float32),
        "item_count": ((20,), torch.int64)}
    assert not m.weighted and not m.takes_basket_weights
    assert m.answers_baskets and m.back_fill_short_rows and m.history is None
    for name in ("predict_all_items", "recommend_with_scores", "recommend", "forward",
                 "recommend_for_items", "similar_items", "scoring_route"):
        assert getattr(ContentKNN, name) is getattr(ItemCF, name), name
    for kw in ({"num_neighbors": 0}, {"num_neighbors": 65}, {"weighting": "bm25"}):
        with pytest.raises(ValueError):
            ContentKNN(30, 20, **kw)
    with pytest.raises(RuntimeError, match="not fitted"):
        m.similar_items([1])
    for call in (lambda: m.fit_interactions([0], [1]), lambda: m.fit_history(None)):
        with pytest.raises(TypeError, match="fit_attributes"):
            call()


def test_fit_attributes_validates_before_it_asks_for_a_gpu():
    m = ContentKNN(3, 5, num_neighbors=2)
    ok = np.zeros((5, 3), np.int64)
    for attrs, cw in ((np.zeros((5, 0), np.int64), None),          # F = 0
                      (np.zeros((5, 17), np.int64), None),         # F = 17
                      (np.zeros((4, 3), np.int64), None),          # a wrong row count
                      (ok, [1.0, -1.0, 1.0]),                      # a negative column weight
                      (ok, [0.0, 0.0, 0.0]),                       # all-zero column weights
                      (ok, [1.0, 1.0]), (ok, [1.0, float("nan"), 1.0]),
                      (ok.astype(np.float32), None), (ok[0], None)):
        with pytest.raises(ValueError):
            m.fit_attributes(attrs, column_weights=cw)
    with pytest.raises(RuntimeError, match="no CPU path|GPU"):
        m.fit_attributes(ok)
    with pytest.raises(RuntimeError, match="no CPU path|GPU"):
        Recommender(3, 5, device="cpu").add_content_knn(torch.from_numpy(ok))


def test_checkpoint_dispatch_on_cpu():
    src = ContentKNN(1, 1, num_neighbors=5, weighting="uniform", top_k=9)
    sd = ContentKNN(30, 20, num_neighbors=5).state_dict()
    sd["item_count"][3] = 2
    m = create_model_from_checkpoint("exp/content_knn_v1", {"state_dict": sd,
                                                            "hyper_parameters": dict(src.hparams)},
                                     30, 20, "cpu")
    assert type(m) is ContentKNN and (m.num_users, m.num_items) == (30, 20) and not m.training
    assert (m.num_neighbors, m.weighting, m.top_k) == (5, "uniform", 9)
    assert m.similar_items([3], k=2)[1].tolist() == [[-1, -1]]


# ------------------------------------------------------------------ the oracle
HAND = np.array([[5, 1], [5, 2], [9, 1], [-1, 1]])


def test_the_weighting_rule_on_a_hand_computed_example():
    """I = 4.  Column 0: value 5 (df 2), 9 (df 1), one missing; column 1: value 1 (df 3), 2 (df 1).
    idf = ln(5 / (1 + df)) + 1, g = idf^2, q = rint(g * 2^20 / g_max), g_max at df = 1."""
    codes, ptr, q = np_weights(HAND)
    assert codes.tolist() == [[0, 0], [0, 1], [1, 0], [-1, 0]] and ptr.tolist() == [0, 2, 4]
    idf = {df: math.log(5.0 / (1 + df)) + 1.0 for df in (1, 2, 3)}
    g_max = idf[1] ** 2
    want = [round(idf[2] ** 2 * Q1 / g_max), Q1, round(idf[3] ** 2 * Q1 / g_max), Q1]
    assert q.dtype == np.uint32 and q.tolist() == want == [651787, 1048576, 427201, 1048576]
    # column weights scale idf before the square; uniform: every idf is 1
    assert np_weights(HAND, [1.0, 2.0], "uniform")[2].tolist() == [Q1 // 4, Q1 // 4, Q1, Q1]
    assert np_weights(HAND, [3.0, 0.0], "uniform")[2].tolist() == [Q1, Q1, 0, 0]
    # the module's host encoding is the same rule
    for cw, wt in ((None, "idf"), ([1.0, 2.0], "uniform"), ([0.5, 3.0], "idf")):
        a, b = np_weights(HAND, cw, wt), encode_attributes(HAND, 4, cw, wt)
        assert all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(a, b))
    sparse = np.array([[70, -4], [10 ** 9, 3], [70, 3]])          # arbitrary values: remapped
    assert encode_attributes(sparse, 3)[0].tolist() == [[0, -1], [1, 0], [0, 0]]


def test_the_fit_on_the_hand_computed_example():
    codes, ptr, q = np_weights(HAND)
    idx, val, count, sim, S = np_content_fit(codes, ptr, q, 2)
    a, b, c = 651787, 1048576, 427201                            # q of (0: 5), (0: 9) = (1: 2), (1: 1)
    assert count.tolist() == [2, 2, 2, 1]
    assert S.tolist() == [[0, a, c, c], [a, 0, 0, 0], [c, 0, 0, c], [c, 0, c, 0]]
    n = [a + c, a + b, b + c, c]
    f = lambda s, i, j: np.float32(s / math.sqrt(float(n[i]) * float(n[j])))
    assert idx.tolist() == [[3, 1], [0, -1], [3, 0], [0, 2]]
    assert val[0].tolist() == [f(c, 0, 3), f(a, 0, 1)] and val[1].tolist() == [f(a, 0, 1), 0.0]
    assert f(c, 0, 3) > f(c, 0, 2)                               # item 3's norm is the smaller


def test_the_oracles_invariants_on_a_catalogue_with_duplicates():
    a = syn.item_attributes(400, seed=3, missing=0.02)
    assert a.shape == (400, len(syn.ATTRIBUTE_VOCAB)) and a.dtype == np.int32
    assert (a.max(0) < np.asarray(syn.ATTRIBUTE_VOCAB)).all() and (a < 0).any()
    assert np.array_equal(a, syn.item_attributes(400, seed=3, missing=0.02))
    idx, val, count, sim, S = np_content_fit(*np_weights(a), 8)
    assert np.array_equal(S, S.T)                                # the weight belongs to the code
    assert (sim <= 1.0).all() and (sim >= 0.0).all() and np.array_equal(sim, sim.T)
    same = (a[:, None, :] == a[None, :, :]).all(2) & ~np.eye(400, dtype=bool)
    same &= (a >= 0).any(1)[:, None]
    assert int(same.sum()) > 100                                 # the duplicated rows
    assert (sim[same] == np.float32(1.0)).all()
    assert ((val[:, :-1] >= val[:, 1:]) | (idx[:, 1:] < 0)).all()
    tie = (val[:, :-1] == val[:, 1:]) & (idx[:, 1:] >= 0)
    assert tie.any() and (idx[:, :-1][tie] < idx[:, 1:][tie]).all()
