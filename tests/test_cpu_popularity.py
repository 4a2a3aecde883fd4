"""CPU-side checks of PopularityBaseline (no GPU): exports, constructor surface vs the
reference (`src/models/baseline.py:19-25`, `serve.py:264-268`), the empty state_dict, the two
ABI entries, host-side errors, and what serving keeps unchanged."""
import inspect

import numpy as np
import pytest
import torch

import hnm_recommendation_amd as pkg
from hnm_recommendation_amd import NeuralCF, PopularityBaseline, _lib, models
from hnm_recommendation_amd.serving import Recommender, create_model_from_checkpoint

SYMBOLS = ("hnm_popularity_fit_f64", "hnm_popularity_topk_f32")


def test_exported():
    assert "PopularityBaseline" in pkg.__all__ and "PopularityBaseline" in models.__all__
    assert pkg.PopularityBaseline is models.PopularityBaseline


def test_constructor_mirrors_reference():
    names = list(inspect.signature(PopularityBaseline.__init__).parameters)
    assert names[:5] == ["self", "n_items", "k", "time_decay", "personalized"]
    m = PopularityBaseline(50, 7, 0.02, True)
    assert m.hparams == {"n_items": 50, "k": 7, "time_decay": 0.02, "personalized": True}
    assert (m.n_items, m.num_items, m.k, m.top_k) == (50, 50, 7, 7)
    assert m.time_decay == 0.02 and m.personalized is True and m.metrics.top_k == 7
    d = PopularityBaseline(n_items=9)
    assert d.hparams == {"n_items": 9, "k": 12, "time_decay": 0.0, "personalized": False}
    # serve.py:264-268
    a = PopularityBaseline(num_items=40, top_k=100)
    assert a.hparams == {"n_items": 40, "k": 100, "time_decay": 0.0, "personalized": False}
    assert (a.num_items, a.top_k) == (40, 100)
    with pytest.raises(TypeError):
        PopularityBaseline()
    with pytest.raises(TypeError):
        PopularityBaseline(10, embedding_dim=4)
    with pytest.raises(TypeError):
        PopularityBaseline(10, num_items=10)


def test_state_dict_is_empty_and_device_needs_no_parameter():
    m = PopularityBaseline(30)
    assert list(m.parameters()) == [] and m.state_dict() == {}
    assert m.device == torch.device("cpu") and m.item_popularity is None
    m.set_popular_items([4, 2, 9])
    assert m.state_dict() == {}
    m.load_state_dict({})
    assert m.item_popularity == [4, 2, 9]
    assert m.order_val.tolist() == [3.0, 2.0, 1.0]          # len(items) - position
    rank = np.full(30, -1)
    rank[[4, 2, 9]] = [0, 1, 2]
    assert m.rank.dtype == torch.int32 and m.rank.tolist() == rank.tolist()
    m.set_popular_items(np.array([7, 1]), weights=[0.5, 0.25])
    assert m.item_popularity == [7, 1] and m.order_val.tolist() == [0.5, 0.25]
    assert m.pop.dtype == torch.float64 and m.pop[7] == 0.5 and m.pop.sum() == 0.75


def test_abi_entries_declared_and_exported():
    lib = _lib.load()
    for s in SYMBOLS:
        assert s in _lib.declared_symbols()
        assert hasattr(lib, s), s
    assert lib.hnm_abi_version() == 1


def test_set_popular_items_rejects_bad_orders():
    m = PopularityBaseline(10)
    with pytest.raises(ValueError):
        m.set_popular_items([1, 2, 1])
    with pytest.raises(ValueError):
        m.set_popular_items([1, 10])
    with pytest.raises(ValueError):
        m.set_popular_items([-1, 3])
    with pytest.raises(ValueError):
        m.set_popular_items([1, 2], weights=[1.0])
    assert m.item_popularity is None


def test_not_fitted_raises_and_there_is_no_cpu_path():
    m = PopularityBaseline(10)
    for call in (lambda: m.recommend([0, 1]), lambda: m.forward(torch.tensor([0])),
                 lambda: m.recommend_with_scores(torch.tensor([0]))):
        with pytest.raises(RuntimeError, match="not fitted"):
            call()
    m.set_popular_items([3, 1])
    with pytest.raises(RuntimeError, match="no CPU path|GPU"):
        m.recommend([0])
    with pytest.raises(RuntimeError, match="no CPU path|GPU"):
        m.fit_interactions([1, 2, 3])


def test_serving_keeps_checkpoint_dispatch_and_first_model_fallback():
    ck = {"state_dict": {}, "hyper_parameters": {}}
    assert create_model_from_checkpoint("popularity_baseline", ck, 20, 10, "cpu") is None
    srv = Recommender(20, 10, device="cpu")
    assert srv.cold_start == "error"
    srv.add_model("neural_cf", NeuralCF(20, 10))
    srv.add_model("other", NeuralCF(20, 10), {"test_map": 0.0})
    assert srv._get_best_model() == "neural_cf"           # no baseline: the first model
    base = PopularityBaseline(10)
    base.set_popular_items([1, 2])
    srv.add_model("popularity_baseline", base)
    assert srv._get_best_model() == "popularity_baseline"
    srv.add_model("scored", NeuralCF(20, 10), {"test_map": 0.2})
    assert srv._get_best_model() == "scored"
    with pytest.raises(ValueError):
        Recommender(20, 10, device="cpu", cold_start="random")
    cold = Recommender(20, 10, device="cpu", cold_start="popularity")
    cold.add_model("neural_cf", NeuralCF(20, 10))
    with pytest.raises(ValueError, match="popularity_baseline"):
        cold.get_recommendations(99)
    with pytest.raises(ValueError, match="popularity_baseline"):
        cold.get_batch_recommendations([1, 99])
