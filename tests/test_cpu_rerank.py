"""Two-stage serving without a GPU: the oracle of the candidate entries (rerank_oracle.py) on
hand-written rows, the Reranker's host-side validation, the declarations of the three entries,
the depth rule and the host side of `Recommender.add_reranker`."""
import os
import re

import numpy as np
import pytest
import torch

import rerank_oracle as RO
from hnm_recommendation_amd import (Ensemble, ItemCF, MatrixFactorization, NeuralCF,
                                    PopularityBaseline, Reranker, WideDeep, _lib)
from hnm_recommendation_amd.models import reranker as RR
from hnm_recommendation_amd.serving import Recommender

INF, NAN = float("inf"), float("nan")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("hnm_cand_union_i32", "hnm_cand_topk_f32", "hnm_widedeep_cand_topk_ex_f32")

# G = 2 lists of kc = 4 entries over I = 10 items, B = 3 rows.
# row 0: item 5 stands in both lists, item 0 and item I - 1 = 9 are there; list 0 ends in an
#        idx = -1 entry; list 1 holds item 7 with a -inf value (empty) and item 10 (out of range)
# row 1: everything empty (idx < 0, or a NaN / +inf value)
# row 2: two identical lists
IDX = np.array([[[5, 9, 0, -1], [-1, 3, 4, -2], [2, 1, 8, 6]],
                [[7, 5, 10, 0], [6, -1, 2, 2], [2, 1, 8, 6]]], np.int64)
VAL = np.array([[[1.0, 0.5, -2.0, 9.0], [1.0, NAN, INF, 0.0], [4.0, 3.0, 2.0, 1.0]],
                [[-INF, 2.0, 1.0, 0.0], [NAN, 1.0, -INF, INF], [4.0, 3.0, 2.0, 1.0]]],
               np.float32)


def test_oracle_union_hand_rows():
    cand, n, oob = RO.union(VAL, IDX, 10)
    assert cand.dtype == np.int32 and cand.shape == (3, 8) and oob
    assert cand.tolist() == [[0, 5, 9, -1, -1, -1, -1, -1],
                             [-1] * 8,
                             [1, 2, 6, 8, -1, -1, -1, -1]]
    assert n.tolist() == [3, 0, 4]
    # with 11 items the id 10 is an item like any other
    cand, n, oob = RO.union(VAL, IDX, 11)
    assert cand[0].tolist() == [0, 5, 9, 10, -1, -1, -1, -1] and not oob
    # without values only idx < 0 is empty: 7 (its value was -inf) joins row 0, row 1 has ids
    cand, n, oob = RO.union(None, IDX, 11, ldc=10)
    assert cand.shape == (3, 10)
    assert cand[0].tolist() == [0, 5, 7, 9, 10, -1, -1, -1, -1, -1]
    assert cand[1].tolist() == [2, 3, 4, 6, -1, -1, -1, -1, -1, -1] and n.tolist() == [5, 4, 4]


def test_oracle_select_hand_rows():
    cand = np.array([[0, 3, 5, 7, 9, -1], [1, 2, 3, 4, 5, 6]], np.int32)
    scores = np.array([[1.0, 2.0, 2.0, NAN, -INF, 5.0], [1.0, 1.0, INF, 1.0, 7.0, 7.0]],
                      np.float32)
    v, i = RO.select(scores, cand, np.array([6, 4], np.int32), 3)
    assert v.dtype == np.float32 and i.dtype == np.int64
    # row 0: the tie at 2.0 goes to the lower id; NaN, -inf and the cand = -1 entry are dropped
    assert i[0].tolist() == [3, 5, 0] and v[0].tolist() == [2.0, 2.0, 1.0]
    # row 1: only the first 4 entries count; +inf is a score like any other
    assert i[1].tolist() == [3, 1, 2] and v[1].tolist() == [INF, 1.0, 1.0]
    v, i = RO.select(scores, cand, np.array([5, 0], np.int32), 4)
    assert i.tolist() == [[3, 5, 0, -1], [-1] * 4]
    assert v[0].tolist() == [2.0, 2.0, 1.0, -INF] and v[1].tolist() == [-INF] * 4


def test_symbols_are_declared_and_bound():
    header = open(os.path.join(REPO, "include", "hnm.h")).read()
    for name in SYMBOLS:
        assert re.search(r"hnm_status\s+%s\s*\(" % name, header), name
        assert name in _lib.declared_symbols()
    assert len(_lib._SIGS["hnm_cand_union_i32"][1]) == 12
    assert len(_lib._SIGS["hnm_cand_topk_f32"][1]) == 9
    assert len(_lib._SIGS["hnm_widedeep_cand_topk_ex_f32"][1]) == 15
    from hnm_recommendation_amd import build
    assert "rerank.hip" in build.SOURCES and "widedeep_cand.hip" in build.SOURCES


def _sources(I=40):
    return [("item_cf", ItemCF(30, I)), ("popularity", PopularityBaseline(n_items=I))]


class NoForward(torch.nn.Module):
    num_users, num_items = 30, 40


def test_constructor_validation():
    mf = MatrixFactorization(30, 40)
    with pytest.raises(ValueError, match="at least one source"):
        Reranker(mf, [])
    with pytest.raises(ValueError, match="at most 16"):
        Reranker(mf, [(f"p{g}", PopularityBaseline(n_items=40)) for g in range(17)])
    with pytest.raises(ValueError, match="distinct"):
        Reranker(mf, [("a", ItemCF(30, 40)), ("a", PopularityBaseline(n_items=40))])
    with pytest.raises(ValueError, match="num_items"):
        Reranker(mf, [("a", ItemCF(30, 40)), ("b", PopularityBaseline(n_items=41))])
    with pytest.raises(ValueError, match="num_items"):
        Reranker(MatrixFactorization(30, 41), _sources())
    for bad in (NoForward(), object(), ItemCF(30, 40), Ensemble(_sources())):
        with pytest.raises(ValueError, match="forward"):   # no pairwise forward(users, items)
            Reranker(bad, _sources())
    for bad in (0, -3, 513):
        with pytest.raises(ValueError, match="depth"):
            Reranker(mf, _sources(), depth=bad)
    with pytest.raises(ValueError, match="depth"):
        Reranker(mf, [(f"p{g}", PopularityBaseline(n_items=40)) for g in range(5)], depth=410)
    Reranker(mf, [(f"p{g}", PopularityBaseline(n_items=40)) for g in range(16)], depth=128)


def test_surface():
    mf, icf, pop = MatrixFactorization(30, 40), ItemCF(30, 40), PopularityBaseline(n_items=40)
    r = Reranker(mf, {"item_cf": icf, "popularity": pop}, top_k=7)
    assert list(r.sources) == ["item_cf", "popularity"] and r.sources["item_cf"] is icf
    assert r.ranker is mf
    keys = set(r.state_dict())
    assert "ranker.user_embeddings.weight" in keys and "sources.item_cf.neighbor_idx" in keys
    assert r.num_items == 40 and r.num_users == 30 and r.top_k == 7 and r.metrics.top_k == 7
    assert r.hparams == {"ranker": "MatrixFactorization", "sources": ["item_cf", "popularity"],
                         "depth": None, "top_k": 7}
    assert not r.answers_baskets and not r.takes_basket_weights and r.back_fill_short_rows
    assert not Reranker(mf, [("popularity", pop)]).back_fill_short_rows
    # an Ensemble may be a source
    assert Reranker(mf, [("e", Ensemble(_sources()))]).back_fill_short_rows
    with pytest.raises(NotImplementedError, match="dense"):
        r.predict_all_items(torch.tensor([0]))
    with pytest.raises(NotImplementedError, match="visitor without a user index"):
        r.recommend_for_items([[1, 2]])
    # k > 128 is refused before any launch (so also without a GPU), top_k > num_items too
    with pytest.raises(ValueError, match="128"):
        Reranker(MatrixFactorization(30, 400), [("p", PopularityBaseline(n_items=400))]
                 ).recommend_with_scores(torch.tensor([0]), k=129)
    with pytest.raises(RuntimeError, match="out of range"):
        Reranker(mf, _sources(), top_k=41).recommend(torch.tensor([0]))
    with pytest.raises(RuntimeError, match="no CPU path|GPU"):
        r.recommend_with_scores(torch.tensor([0]))


def test_scoring_route_names_the_route():
    wd = WideDeep(30, 400, embedding_dim=8, deep_layers=[16, 8])
    pop = [("popularity", PopularityBaseline(n_items=400))]
    r = Reranker(wd, pop)
    assert r.scoring_route() == RR.ROUTE_WIDEDEEP == r.scoring_route(64)
    assert r.scoring_route(65) == RR.ROUTE_WIDEDEEP_WIDE == r.scoring_route(128)
    with pytest.raises(ValueError, match="128"):
        r.scoring_route(129)
    for ranker in (MatrixFactorization(30, 400), NeuralCF(30, 400)):
        assert Reranker(ranker, pop).scoring_route() == RR.ROUTE_PAIRS
    assert len({RR.ROUTE_WIDEDEEP, RR.ROUTE_WIDEDEEP_WIDE, RR.ROUTE_PAIRS}) == 3


# (depth, k, top_k, num_items, G) -> depth of the call: Ensemble._depth's rule
DEPTHS = [((None, 12, 12, 1000, 3), 48),      # 4 * top_k
          ((None, 100, 12, 1000, 3), 100),    # k above it
          ((None, 12, 12, 30, 3), 30),        # clamped to num_items
          ((None, 128, 200, 10 ** 5, 1), 512),   # ... to 512
          ((None, 128, 200, 10 ** 5, 16), 128),  # ... to 2,048 / G
          ((None, 128, 200, 10 ** 5, 5), 409),
          ((24, 100, 12, 1000, 2), 24),       # a given depth wins over k
          ((24, 12, 12, 10, 2), 10),
          ((None, 1, 0, 1000, 2), 1)]


@pytest.mark.parametrize("args,want", DEPTHS)
def test_depth_clamping_table(args, want):
    depth, k, top_k, num_items, G = args
    assert RR.clamp_depth(depth, k, top_k, num_items, G) == want
    mf = MatrixFactorization(30, num_items)
    srcs = [(f"p{g}", PopularityBaseline(n_items=num_items)) for g in range(G)]
    r = Reranker(mf, srcs, depth=depth, top_k=top_k)
    assert r._depth(k) == want
    if depth is None:                          # the same number an Ensemble of them would ask
        assert Ensemble(srcs, top_k=top_k)._depth(k) == want


def test_history_is_the_first_sources_and_set_history_fills_the_empty_ones():
    from hnm_recommendation_amd import UserHistory
    icf_a, icf_b, pop = ItemCF(6, 10), ItemCF(6, 10), PopularityBaseline(n_items=10)
    r = Reranker(MatrixFactorization(6, 10), [("popularity", pop), ("a", icf_a), ("b", icf_b)])
    assert r.history is None
    h1, h2 = UserHistory({1: {2}}, 6, 10, "cpu"), UserHistory({2: {3}}, 6, 10, "cpu")
    icf_b.set_history(h1)
    assert r.history is h1
    r.set_history(h2)
    assert icf_a.history is h2 and icf_b.history is h1 and r.history is h2


def test_add_reranker_host_logic():
    srv = Recommender(100, 50, device="cpu")
    srv.add_model("neural_cf", NeuralCF(100, 50), {"test_map": 0.2})
    srv.add_model("mf", MatrixFactorization(100, 50))
    srv.add_model("item_cf", ItemCF(100, 50))
    with pytest.raises(ValueError, match="nope"):
        srv.add_reranker("neural_cf", ["mf", "nope"])
    with pytest.raises(ValueError, match="nope"):
        srv.add_reranker("nope", ["mf"])
    assert "reranker" not in srv.models
    best = srv._get_best_model()
    r = srv.add_reranker("neural_cf", ["item_cf", "mf"], depth=20, top_k=5)
    assert srv.models["reranker"] is r and list(r.sources) == ["item_cf", "mf"]
    assert r.ranker is srv.models["neural_cf"] and r.depth == 20 and r.top_k == 5
    assert srv.model_metrics["reranker"] == {} and srv._get_best_model() == best
    srv.add_reranker("mf", ["item_cf"], name="second")
    assert srv.models["second"].ranker is srv.models["mf"]
    with pytest.raises(ValueError, match="basket"):
        srv.get_recommendations_for_items([1, 2], model_name="reranker")
