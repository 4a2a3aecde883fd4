"""CPU: Wide&Deep catalogue scoring with item features -- the fixtures against the oracle, the
feature-table surface of the module, and the new ABI names (no GPU)."""
import numpy as np
import pytest
import torch

from parity import assert_scores_close, load_golden
from hnm_recommendation_amd import WideDeep, _lib
from oracle import hnm_oracle as O

CASES = ("widedeep_itemfeat_all_a.npz", "widedeep_itemfeat_all_b.npz")


def oracle_all_pairs(g, chunk=500):
    """The oracle's forward over every (user, item) pair, item_features = table[item]."""
    users, table = g["user_ids"], g["item_table"]
    uf = g["user_features"] if int(g["Fu"]) else None
    B, I = len(users), int(g["I"])
    out = []
    for s in range(0, I, chunk):
        e = min(s + chunk, I)
        eu = np.repeat(users, e - s)
        ei = np.tile(np.arange(s, e), B)
        ef = None if uf is None else np.repeat(uf, e - s, axis=0)
        out.append(O.widedeep_forward(g["sd"], eu, ei, ef, item_features=table[ei])
                   .reshape(B, e - s))
    return np.concatenate(out, axis=1)


@pytest.mark.parametrize("name", CASES)
def test_oracle_matches_reference_dense(name):
    g = load_golden(name)
    assert g["dense"].shape == (9, 4200) and g["item_table"].shape == (4200, int(g["Fi"]))
    assert_scores_close(oracle_all_pairs(g), g["dense"], what=name)
    srt = -np.sort(-g["dense"].astype(np.float64), axis=1)
    assert np.array_equal(np.sort(g["topk"], 1),
                          np.sort(np.argsort(-g["dense"], 1, kind="stable")[:, :12], 1))
    # the K-th gap is wider than the score tolerance: top-12 SETS are comparable exactly
    assert ((srt[:, 11] - srt[:, 12]) > 1e-4 * np.abs(g["dense"]).max(1)).all()


def small_model():
    return WideDeep(30, 20, num_user_features=3, num_item_features=4, embedding_dim=8,
                    deep_layers=[16, 8])


def test_feature_tables_are_not_state():
    m = small_model()
    keys = list(m.state_dict())
    m.set_item_features(np.ones((20, 4), np.float64))
    m.set_user_features(torch.ones(30, 3))
    assert list(m.state_dict()) == keys
    assert m.item_feature_table.dtype == torch.float32 and m.item_feature_table.is_contiguous()
    assert m.item_feature_table.shape == (20, 4) and m.user_feature_table.shape == (30, 3)
    # a copy: later changes of the caller's table do not reach the model
    t = torch.zeros(20, 4)
    m.set_item_features(t)
    t += 1
    assert float(m.item_feature_table.abs().sum()) == 0.0
    m.load_state_dict(small_model().state_dict())  # strict: no table keys expected
    m.set_item_features(None)
    m.set_user_features(None)
    assert m.item_feature_table is None and m.user_feature_table is None
    assert list(m.state_dict()) == keys


@pytest.mark.parametrize("setter,bad", [("set_item_features", (20, 3)),
                                        ("set_item_features", (19, 4)),
                                        ("set_item_features", (80,)),
                                        ("set_user_features", (30, 4)),
                                        ("set_user_features", (20, 3))])
def test_feature_table_shapes_are_checked(setter, bad):
    with pytest.raises(ValueError):
        getattr(small_model(), setter)(torch.zeros(*bad))


def test_new_abi_names_declared():
    for n in ("hnm_widedeep_topk_ex_f32", "hnm_widedeep_scores_ex_f32",
              "hnm_widedeep_prefilter_debug_ex_f32", "hnm_widedeep_refine_debug_ex_f32"):
        assert n in _lib.declared_symbols()
