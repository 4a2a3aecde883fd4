"""CPU-side checks of models/history.py (no GPU): `basket_csr` with literal expectations, the
`HistoryModel` mixin and who inherits it, what models/base.py still exports, the capability
attributes `serving.Recommender` reads, and `_lib.call_weighted`'s naming rule."""
import inspect

import numpy as np
import pytest
import torch

from hnm_recommendation_amd import (ImplicitALS, ItemCF, LightGCN, MatrixFactorization, NeuralCF,
                                    PopularityBaseline, UserHistory, WeightedItemCF, WideDeep, _lib)
from hnm_recommendation_amd.models import base, history, implicit_als
from hnm_recommendation_amd.models.history import (HistoryModel, basket_csr, interaction_weights,
                                                   interactions_history)

CPU = torch.device("cpu")
BASKETS = [[3, 1, 3], [], [-1, 0]]


def lists(ptr, idx, n, w):
    return ptr.tolist(), idx.tolist(), n, None if w is None else w.tolist()


# ------------------------------------------------------------------ basket_csr
def test_basket_csr_sorts_dedups_and_wraps():
    ptr, idx, n, w = basket_csr(BASKETS, 5, CPU)
    assert lists(ptr, idx, n, w) == ([0, 2, 2, 4], [1, 3, 0, 4], 3, None)
    assert (ptr.dtype, idx.dtype) == (torch.int64, torch.int32)
    assert ptr.device == idx.device == CPU and ptr.is_contiguous() and idx.is_contiguous()


def test_basket_csr_sums_the_weights_of_a_repeated_item():
    ptr, idx, n, w = basket_csr(BASKETS, 5, CPU, [[1, 2, 4], [], [0.5, 0.25]])
    assert lists(ptr, idx, n, w) == ([0, 2, 2, 4], [1, 3, 0, 4], 3, [2.0, 5.0, 0.25, 0.5])
    assert (ptr.dtype, idx.dtype, w.dtype) == (torch.int64, torch.int32, torch.float32)
    assert w.device == CPU and ptr.is_contiguous() and idx.is_contiguous() and w.is_contiguous()
    # float64 sum in ascending weight order, one rounding to fp32: any order of the entries
    big, tiny = 2.0 ** 24, 0.75
    for ws in ([big, tiny, tiny], [tiny, big, tiny], [tiny, tiny, big]):
        w = basket_csr([[2, 2, 2]], 5, CPU, [ws])[3]
        assert w.tolist() == [float(np.float32(np.float64(tiny) + tiny + big))]


def test_basket_csr_takes_a_csr_as_it_is():
    ptr = np.array([0, 2, 2, 4], np.int64)
    idx = np.array([1, 3, 0, 4], np.int32)
    flat = np.array([2, 5, 0.25, 0.5], np.float32)
    for pair in ((ptr, idx), (torch.from_numpy(ptr), torch.from_numpy(idx))):
        assert lists(*basket_csr(pair, 5, CPU)) == ([0, 2, 2, 4], [1, 3, 0, 4], 3, None)
        got = basket_csr(pair, 5, CPU, flat)
        assert lists(*got) == ([0, 2, 2, 4], [1, 3, 0, 4], 3, [2.0, 5.0, 0.25, 0.5])
        assert (got[0].dtype, got[1].dtype, got[3].dtype) == (torch.int64, torch.int32,
                                                              torch.float32)


def test_basket_csr_pads_what_is_empty():
    assert lists(*basket_csr([], 5, CPU)) == ([0], [0], 0, None)
    assert lists(*basket_csr([], 5, CPU, [])) == ([0], [0], 0, [0.0])
    assert lists(*basket_csr([[], []], 5, CPU, [[], []])) == ([0, 0, 0], [0], 2, [0.0])
    empty = (np.zeros(1, np.int64), np.zeros(0, np.int32))
    assert lists(*basket_csr(empty, 5, CPU, np.zeros(0, np.float32))) == ([0], [0], 0, [0.0])


def test_basket_csr_errors():
    for bad in ([[5]], [[-6]]):
        with pytest.raises(IndexError, match="out of bounds for dimension 1 with size 5"):
            basket_csr(bad, 5, CPU)
        with pytest.raises(IndexError, match="out of bounds for dimension 1 with size 5"):
            basket_csr(bad, 5, CPU, [[1.0]])
    for ws in ([[1, 2, 4], []], [[1, 2], [], [0.5, 0.25]]):
        with pytest.raises(ValueError, match="one sequence per basket"):
            basket_csr(BASKETS, 5, CPU, ws)
    with pytest.raises(ValueError, match="finite and >= 0"):
        basket_csr(BASKETS, 5, CPU, [[1, -2, 4], [], [0.5, 0.25]])
    idx = np.array([1, 3, 0, 4], np.int32)
    for ptr in ([0, 3, 2, 4], [1, 2, 2, 4], [0, 2, 2, 5]):
        with pytest.raises(ValueError, match="start at 0, not decrease and end within idx"):
            basket_csr((np.array(ptr, np.int64), idx), 5, CPU)
    with pytest.raises(ValueError, match="at least one entry"):
        basket_csr((np.zeros(0, np.int64), idx), 5, CPU)
    with pytest.raises(ValueError, match="aligned with the CSR's idx"):
        basket_csr((np.array([0, 2, 2, 4], np.int64), idx), 5, CPU, np.ones(3, np.float32))


# ------------------------------------------------------------------ interactions_history
def test_interactions_history_is_the_front_end_of_the_fits():
    u = torch.tensor([[0, 0], [2, 0]])
    i = np.array([[1, 1], [4, 3]])
    h = interactions_history(u, i, 3, 5, CPU)
    assert h.hist_ptr.tolist() == [0, 2, 2, 3] and h.hist_idx.tolist() == [1, 3, 4]
    assert h.hist_w is None
    h = interactions_history(u, i, 3, 5, CPU, unit_weights=True)
    assert h.hist_w.tolist() == [2.0, 1.0, 1.0]
    h = interactions_history(u, i, 3, 5, CPU, weights=[1, 2, 3, 4], days_ago=[0, 0, 0, 10],
                             time_decay=0.1, unit_weights=True)
    assert h.hist_w.tolist() == [3.0, float(np.float32(4 * np.exp(-1.0))), 3.0]
    with pytest.raises(ValueError, match="time_decay"):
        interactions_history(u, i, 3, 5, CPU, time_decay=-1.0)
    with pytest.raises(IndexError):
        interactions_history(u, i, 2, 5, CPU)


# ------------------------------------------------------------------ structure
def test_the_history_models_inherit_the_mixin():
    for cls in (ItemCF, WeightedItemCF, ImplicitALS):
        assert issubclass(cls, HistoryModel)
        assert cls.set_history is HistoryModel.set_history
        assert cls._need_history is HistoryModel._need_history
    for cls in (PopularityBaseline, MatrixFactorization, NeuralCF, WideDeep, LightGCN):
        assert not issubclass(cls, HistoryModel)
    assert "item_cf" not in inspect.getsource(implicit_als)
    assert ImplicitALS._interaction_weights is interaction_weights


def test_the_mixin_keeps_each_model_s_errors():
    good = UserHistory({0: {1}}, 30, 20, CPU)
    for m, hint in ((ItemCF(30, 20), r"call set_history \(or fit_interactions\) first"),
                    (ImplicitALS(30, 20, embedding_dim=16),
                     "call fit_interactions / fit_history / set_history")):
        assert m.history is None
        with pytest.raises(RuntimeError, match="no history: " + hint):
            m._need_history()
        with pytest.raises(TypeError, match="history must be a UserHistory"):
            m.set_history({0: {1}})
        with pytest.raises(ValueError, match="built for 31 users x 20 items, model has 30 x 20"):
            m.set_history(UserHistory({}, 31, 20, CPU))
        with pytest.raises(ValueError, match="built for 30 users x 21 items"):
            m._need_history(UserHistory({}, 30, 21, CPU))
        assert m.history is None
        assert m.set_history(good) is m and m._need_history() is good
        other = UserHistory({}, 30, 20, CPU)
        assert m._need_history(other) is other and m.history is good
        assert m.set_history(None).history is None


def test_base_still_exports_its_names():
    for name in ("RecModule", "UserHistory", "_history_arrays", "interaction_weights",
                 "filter_csr", "empty_topk", "dense_topk", "f32c"):
        assert hasattr(base, name), name
    for name in ("UserHistory", "_history_arrays", "interaction_weights", "filter_csr"):
        assert getattr(base, name) is getattr(history, name)
    from hnm_recommendation_amd.models.base import (dense_topk, empty_rows,  # noqa: F401
                                                    filter_csr, interaction_weights as iw)
    assert iw is interaction_weights
    assert empty_rows(3, 2, CPU)[1].shape == (3, 2)


def test_ids_work_without_parameters():
    """RecModule._ids reads self.device: a module without parameters gets the GPU check's
    RuntimeError, not StopIteration."""
    pop = PopularityBaseline(n_items=20)
    assert list(pop.parameters()) == [] and list(ItemCF(30, 20).parameters()) == []
    for m in (pop, ItemCF(30, 20), NeuralCF(30, 20)):
        with pytest.raises(RuntimeError, match="no CPU path|GPU"):
            m._ids([0, 1], 30)


# ------------------------------------------------------------------ what serving asks
@pytest.mark.parametrize("cls,baskets,weights,back_fill", [
    (ItemCF, True, False, True), (WeightedItemCF, True, True, True),
    (ImplicitALS, True, True, False), (PopularityBaseline, False, False, False),
    (MatrixFactorization, False, False, False), (NeuralCF, False, False, False),
    (WideDeep, False, False, False), (LightGCN, False, False, False)])
def test_capability_attributes(cls, baskets, weights, back_fill):
    assert (cls.answers_baskets, cls.takes_basket_weights, cls.back_fill_short_rows) == (
        baskets, weights, back_fill)
    assert cls.answers_baskets == hasattr(cls, "recommend_for_items")
    if hasattr(cls, "weighted"):
        assert cls.takes_basket_weights is cls.weighted


# ------------------------------------------------------------------ _lib.call_weighted
@pytest.mark.parametrize("name,at", [("hnm_itemcf_fit_f32", 3), ("hnm_itemcf_scores_f32", 7),
                                     ("hnm_itemcf_topk_f32", 7), ("hnm_als_solve_rows_f32", 3)])
def test_call_weighted_names_and_places_the_sibling(monkeypatch, name, at):
    plain = list(_lib._SIGS[name][1])
    sibling = name.replace("_f32", "_weighted_f32")
    assert list(_lib._SIGS[sibling][1]) == plain[:at] + [_lib._p] + plain[at:]
    seen = []
    monkeypatch.setattr(_lib, "fn", lambda n: lambda *a: seen.append((n, a)) or _lib.HNM_OK)
    args = tuple(range(len(plain)))
    _lib.call_weighted(name, at, None, *args)
    w = torch.zeros(4)
    _lib.call_weighted(name, at, w, *args)
    assert seen[0] == (name, args)
    assert seen[1][0] == sibling and len(seen[1][1]) == len(args) + 1
    assert seen[1][1][:at] == args[:at] and seen[1][1][at + 1:] == args[at:]
    assert seen[1][1][at].value == w.data_ptr()
