"""GPU: Wide&Deep catalogue scoring with item features (csrc/widedeep_features.hip and the
hnm_widedeep_*_ex_f32 entries).

The reference's `forward` over every (user, item) pair with `item_features = table[item]`
(tests/golden/make_golden_itemfeat.py) is the expected dense result: the per-item features are
folded into the per-item layer-1 table Q and the per-item wide term before the scan, and every
kernel after that -- exact, certified scan, refining cascade, re-score -- reads only those.

4,200 items: just over the certified floor of 4,096, a partial 32-item tile; 9 users: partial
user blocks of 4 and of 8.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from hnm_recommendation_amd import UserHistory, WideDeep, _lib
from hnm_recommendation_amd import sharding as S
from hnm_recommendation_amd import synthetic as syn
from hnm_recommendation_amd.serving import Recommender
from oracle import hnm_oracle as O
from parity import assert_scores_close, assert_topk_equivalent, load_golden, same_topk_sets
from test_cpu_widedeep_itemfeat import oracle_all_pairs
from test_gpu_prefilter import DEV, to_module, topk_both

pytestmark = pytest.mark.gpu

FIX = {"a": "widedeep_itemfeat_all_a.npz", "b": "widedeep_itemfeat_all_b.npz"}
U, I, D, B, K = 3000, 4200, 16, 9, 12
SCALED = {"bias_scale": 0.05, "randomize_bn": True, "emb_scale": 10.0}


def build(sd, Fu, Fi, layers, **kw):
    return to_module(WideDeep(U, I, num_user_features=Fu, num_item_features=Fi, embedding_dim=D,
                              deep_layers=list(layers), top_k=K, **kw), sd)


@functools.lru_cache(maxsize=None)
def golden(tag):
    return load_golden(FIX[tag])


def user_table(Fu, seed=77):
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.standard_normal((U, Fu)).astype(np.float32)


def fixture_model(tag, registered=True, scale_wide=1.0):
    """The fixture's model; registered: its item table and a seeded user table are set."""
    g = golden(tag)
    sd = dict(g["sd"])
    if scale_wide != 1.0:
        for k in ("wide_item_features.weight", "wide_item_features.bias"):
            sd[k] = sd[k] * np.float32(scale_wide)
    m = build(sd, int(g["Fu"]), int(g["Fi"]), g["deep_layers"].tolist())
    if registered:
        m.set_item_features(g["item_table"])
        if int(g["Fu"]):
            m.set_user_features(user_table(int(g["Fu"])))
    return m


def batch(tag):
    g = golden(tag)
    users = torch.from_numpy(g["user_ids"]).to(DEV)
    uf = torch.from_numpy(g["user_features"]).to(DEV) if int(g["Fu"]) else None
    return users, uf, torch.from_numpy(g["item_table"]).to(DEV)


def bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------ 1. golden parity
@pytest.mark.parametrize("tag", "ab")
def test_golden_parity(tag):
    g = golden(tag)
    m = fixture_model(tag, registered=False)
    users, uf, table = batch(tag)
    dense = m.predict_all_items(users, uf, table).cpu().numpy()
    assert_scores_close(dense, g["dense"], what=f"dense {tag}")
    rec = m.recommend(users, uf, None, table).cpu().numpy()
    assert rec.shape == (B, K)
    assert same_topk_sets(rec, g["topk"]), tag
    top64 = m.recommend_with_scores(users, uf, k=64, item_features=table)[1].cpu().numpy()
    assert_topk_equivalent(top64, g["dense"], 64, what=f"k=64 {tag}")
    # k > 64: the dense route
    top100 = m.recommend_with_scores(users, uf, k=100, item_features=table)[1].cpu().numpy()
    assert_topk_equivalent(top100, g["dense"], 100, what=f"k=100 {tag}")


# ------------------------------------------------------------------ 2. table handling
def test_registered_and_explicit_tables_agree_bitwise():
    m = fixture_model("a", registered=False)
    users, _, table = batch("a")
    ut = torch.from_numpy(user_table(6)).to(DEV)
    uf = ut[users]
    d_exp = m.predict_all_items(users, uf, table)
    v_exp, i_exp = m.recommend_with_scores(users, uf, k=K, item_features=table)
    with pytest.raises(ValueError, match="item_features are required"):
        m.predict_all_items(users, uf)
    m.set_item_features(table.cpu().numpy())
    d_reg = m.predict_all_items(users, uf)
    v_reg, i_reg = m.recommend_with_scores(users, uf, k=K)
    assert torch.equal(bits(d_exp), bits(d_reg))
    assert torch.equal(i_exp, i_reg) and torch.equal(bits(v_exp), bits(v_reg))
    # an explicit argument wins over the registered table
    other = table.flip(0).contiguous()
    assert not torch.equal(bits(m.predict_all_items(users, uf, other)), bits(d_reg))
    # user rows gathered from the registered user table == explicit user_features
    with pytest.raises(ValueError, match="user_features are required"):
        m.predict_all_items(users)
    m.set_user_features(ut)
    assert torch.equal(bits(m.predict_all_items(users)), bits(d_reg))
    v_g, i_g = m.recommend_with_scores(users, k=K)
    assert torch.equal(i_g, i_reg) and torch.equal(bits(v_g), bits(v_reg))
    assert torch.equal(m.recommend(users), i_reg)
    assert torch.equal(m._validation_topk({"user_ids": users}), i_reg)
    m.set_item_features(None)
    with pytest.raises(ValueError, match="item_features are required"):
        m.recommend(users)
    with pytest.raises(ValueError):
        m.predict_all_items(users, None, table[:, :4])


# ------------------------------------------------------------------ 3. dense vs pairwise
@pytest.mark.parametrize("tag", "ab")
def test_dense_matches_pairwise_forward(tag):
    m = fixture_model(tag, registered=False)
    users, uf, table = batch(tag)
    dense = m.predict_all_items(users, uf, table)
    rng = np.random.Generator(np.random.PCG64(5))
    rb = torch.from_numpy(rng.integers(0, B, 300)).to(DEV)
    ri = torch.from_numpy(np.concatenate([rng.integers(0, I, 296), [0, 31, I - 9, I - 1]])).to(DEV)
    pair = m(users[rb], ri, None if uf is None else uf[rb], table[ri])
    assert_scores_close(dense[rb, ri].cpu().numpy(), pair.cpu().numpy(), what=f"pairs {tag}")


# ------------------------------------------------------------------ 4. certified == exact
def best_item_filter(m, users):
    """Removes every other item of the exact top-30 of the first three users."""
    _lib.set_prefilter(users.device, False)
    try:
        top = m.recommend_with_scores(users, k=30)[1].cpu().numpy()
    finally:
        _lib.set_prefilter(users.device, True)
    return {int(u): set(top[r, ::2].tolist()) for r, u in enumerate(users.cpu().tolist()[:3])}


def check_certified_equals_exact(m, users, want_rows):
    f = best_item_filter(m, users)
    for k in (1, 12, 64):
        for filt in (None, f):
            (ev, ei), (pv, pi), stats = topk_both(m, users, filt, k=k)
            what = (k, filt is not None, stats)
            assert np.array_equal(ei, pi), what
            assert np.array_equal(ev.view(np.uint32), pv.view(np.uint32)), what
            assert stats[0] == want_rows, what
            if filt:
                for r, u in enumerate(users.cpu().tolist()[:3]):
                    assert not (set(pi[r].tolist()) & f[int(u)]), what


@pytest.mark.parametrize("tag", "ab")
def test_certified_identical_to_exact(tag):
    m = fixture_model(tag)
    check_certified_equals_exact(m, batch(tag)[0], B)  # the certified route ran


def test_exact_only_tower_with_item_features():
    """A 40-wide first layer (K1P % 16 != 0) never takes the certified route; the fold's padded
    columns stay zero."""
    Fu, Fi, layers = 6, 5, (40, 100, 50)
    sd = syn.widedeep_state_dict(U, I, D, layers, num_user_features=Fu, num_item_features=Fi,
                                 seed=51, **SCALED)
    m = build(sd, Fu, Fi, layers)
    rng = np.random.Generator(np.random.PCG64(52))
    table = rng.standard_normal((I, Fi)).astype(np.float32)
    ut = user_table(Fu, seed=53)
    users_np = syn.user_batch(U, B, seed=54)
    users = torch.from_numpy(users_np).to(DEV)
    m.set_item_features(table)
    m.set_user_features(ut)
    (ev, ei), (pv, pi), stats = topk_both(m, users)
    assert np.array_equal(ei, pi) and np.array_equal(ev.view(np.uint32), pv.view(np.uint32))
    assert stats[0] == 0, stats
    g = {"sd": sd, "user_ids": users_np, "item_table": table, "user_features": ut[users_np],
         "Fu": Fu, "I": I}
    ref = oracle_all_pairs(g)
    assert_scores_close(m.predict_all_items(users).cpu().numpy(), ref, what="40-wide dense")
    assert_topk_equivalent(pi, ref, K, what="40-wide top-K")


# ------------------------------------------------------------------ 5. bounds hold
def debug_ex(name, m, users):
    w, keep = m._weights()
    f = m._features(None, users)
    itf, tab, ldf = m._item_table(None, users.device, keep)
    n = users.numel()
    approx = torch.empty(n, I, device=DEV)
    bound = torch.empty(n, I, device=DEV)
    _lib.check(_lib.fn(name)(_lib.ctx(users.device), w, _lib.ptr(users), n, _lib.ptr(f),
                             _lib.ptr(approx), I, _lib.ptr(bound), C.byref(itf), _lib.ptr(tab),
                             ldf), name)
    _lib.sync_check(users.device)
    return approx, bound


def check_bounds(m, users):
    exact = m.predict_all_items(users)
    for name in ("hnm_widedeep_prefilter_debug_ex_f32", "hnm_widedeep_refine_debug_ex_f32"):
        approx, bound = debug_ex(name, m, users)
        assert torch.isfinite(bound).all(), name
        ratio = ((approx - exact).abs() / bound).max().item()
        print(f"{name}: max |approx - exact| / bound = {ratio:.4f}")
        assert ((approx - exact).abs() <= bound).all(), (name, ratio)


@pytest.mark.parametrize("tag", "ab")
def test_bounds_hold(tag):
    check_bounds(fixture_model(tag), batch(tag)[0])


@pytest.mark.parametrize("tag", "ab")
def test_dominant_wide_item_feature_term(tag):
    """wide_item_features x 100: the folded wide term dominates the score; the bound's
    |wide term| must be the folded one."""
    m = fixture_model(tag, scale_wide=100.0)
    users = batch(tag)[0]
    fw = m.final_layer.weight.detach()[0]
    plain = fw[U: U + I].abs().max().item()
    d0 = fixture_model(tag).predict_all_items(users)
    d1 = m.predict_all_items(users)
    assert (d1 - d0).abs().max().item() > 20 * plain  # the feature term is far above wide_item
    check_bounds(m, users)
    check_certified_equals_exact(m, users, B)


# ------------------------------------------------------------------ 6. no wide feature term
def test_use_wide_features_false():
    Fu, Fi, layers = 6, 5, (48, 100, 50)
    sd = syn.widedeep_state_dict(U, I, D, layers, num_user_features=Fu, num_item_features=Fi,
                                 seed=61, **SCALED)
    sd = {k: v for k, v in sd.items() if not k.startswith(("wide_user_features",
                                                            "wide_item_features"))}
    fw = sd["final_layer.weight"]
    sd["final_layer.weight"] = np.concatenate([fw[:, :U + I], fw[:, U + I + Fu + Fi:]], axis=1)
    m = build(sd, Fu, Fi, layers, use_wide_features=False)
    rng = np.random.Generator(np.random.PCG64(62))
    table = rng.standard_normal((I, Fi)).astype(np.float32)
    ut = user_table(Fu, seed=63)
    users_np = syn.user_batch(U, B, seed=64)
    users = torch.from_numpy(users_np).to(DEV)
    uf = torch.from_numpy(ut[users_np]).to(DEV)
    g = {"sd": sd, "user_ids": users_np, "item_table": table, "user_features": ut[users_np],
         "Fu": Fu, "I": I}
    ref = oracle_all_pairs(g)
    tab = torch.from_numpy(table).to(DEV)
    assert_scores_close(m.predict_all_items(users, uf, tab).cpu().numpy(), ref, what="no wide")
    top = m.recommend(users, uf, None, tab).cpu().numpy()
    assert_topk_equivalent(top, ref, K, what="no wide top-K")


# ------------------------------------------------------------------ 7. item shards
@pytest.mark.parametrize("tag", "ab")
def test_item_shards_equal_single_call(tag):
    m = fixture_model(tag)
    users = batch(tag)[0]
    hist = UserHistory(best_item_filter(m, users), U, I, DEV)
    for h in (None, hist):
        vs, ids = [], []
        for lo, hi in ((0, 1400), (1400, 2800), (2800, 4200)):
            v, i = S.widedeep_shard_topk(m, lo, hi, K, history=h)(users)
            vs.append(v)
            ids.append(torch.where(i >= 0, i + lo, i))
        gv, gi = S.hip_merge(torch.stack(vs), torch.stack(ids), K)
        v1, i1 = m.recommend_with_scores(users, filter_items=h, k=K)
        assert torch.equal(gi, i1), h is not None
        assert torch.equal(bits(gv), bits(v1)), h is not None


# ------------------------------------------------------------------ 8. serving
def test_recommender_serves_registered_tables():
    m = fixture_model("b")
    hist = syn.filter_dict(np.arange(U), I, per_user=23, seed=3)
    srv = Recommender(U, I, models={"wide_deep": m}, user_history=hist, device=DEV)
    ids = [5, 17, U + 3, 17, 0, U - 1]
    out = srv.get_batch_recommendations(ids, num_items=K, include_scores=True)
    good = [j for j in range(len(ids)) if "error" not in out[j]]
    assert good == [0, 1, 3, 4, 5]
    users = torch.tensor([ids[j] for j in good], device=DEV)
    v, i = m.recommend_with_scores(users, filter_items=UserHistory(hist, U, I, DEV), k=K)
    got_i = [[int(r["article_id"]) for r in out[j]["recommendations"]] for j in good]
    got_v = [[r["score"] for r in out[j]["recommendations"]] for j in good]
    assert got_i == i.cpu().tolist()
    assert got_v == v.cpu().tolist()


# ------------------------------------------------------------------ 9. ABI edges
def topk_call(name, w, users, f, k, extra=()):
    n = users.numel()
    ov = torch.empty(n, k, dtype=torch.float32, device=DEV)
    oi = torch.empty(n, k, dtype=torch.int64, device=DEV)
    _lib.check(_lib.fn(name)(_lib.ctx(users.device), w, _lib.ptr(users), n, _lib.ptr(f), None,
                             None, k, _lib.ptr(ov), _lib.ptr(oi), *extra), name)
    _lib.sync_check(users.device)
    return ov, oi


def test_ex_without_item_features_is_the_plain_entry():
    sd = syn.widedeep_state_dict(U, I, D, (48, 100, 50), seed=71, **SCALED)
    m = build(sd, 0, 0, (48, 100, 50))
    users = torch.from_numpy(syn.user_batch(U, B, seed=72)).to(DEV)
    w, keep = m._weights()
    v0, i0 = topk_call("hnm_widedeep_topk_f32", w, users, None, K)
    v1, i1 = topk_call("hnm_widedeep_topk_ex_f32", w, users, None, K, (None, None, 0))
    empty = _lib.WideDeepItemFeatures(None, None, None, None, None, 0)
    v2, i2 = topk_call("hnm_widedeep_topk_ex_f32", w, users, None, K, (C.byref(empty), None, 0))
    assert torch.equal(i0, i1) and torch.equal(bits(v0), bits(v1))
    assert torch.equal(i0, i2) and torch.equal(bits(v0), bits(v2))
    d0 = torch.empty(B, I, device=DEV)
    d1 = torch.empty(B, I, device=DEV)
    c = _lib.ctx(users.device)
    _lib.check(_lib.fn("hnm_widedeep_scores_f32")(c, w, _lib.ptr(users), B, None, _lib.ptr(d0), I))
    _lib.check(_lib.fn("hnm_widedeep_scores_ex_f32")(c, w, _lib.ptr(users), B, None, _lib.ptr(d1),
                                                     I, None, None, 0))
    _lib.sync_check(users.device)
    assert torch.equal(bits(d0), bits(d1))


def test_abi_edges_with_item_features():
    m = fixture_model("a")
    users, _, table = batch("a")
    w, keep = m._weights()
    f = m._features(None, users)
    itf, tab, ldf = m._item_table(None, users.device, keep)
    c = _lib.ctx(users.device)
    ex = (C.byref(itf), _lib.ptr(tab), ldf)
    # B = 0: a no-op, NULL per-row pointers allowed
    assert _lib.fn("hnm_widedeep_topk_ex_f32")(c, w, None, 0, None, None, None, K, None, None,
                                               *ex) == _lib.HNM_OK
    assert _lib.fn("hnm_widedeep_scores_ex_f32")(c, w, None, 0, None, None, I, *ex) == _lib.HNM_OK
    # item features declared but no table
    with pytest.raises(ValueError, match="item_features required"):
        topk_call("hnm_widedeep_topk_ex_f32", w, users, f, K, (C.byref(itf), None, ldf))
    # a leading dimension below Fi
    with pytest.raises(ValueError, match="leading dimension"):
        topk_call("hnm_widedeep_topk_ex_f32", w, users, f, K, (C.byref(itf), _lib.ptr(tab), 4))
    # a feature model through the entry without item features keeps the old refusal
    with pytest.raises(ValueError, match="deep input must be"):
        topk_call("hnm_widedeep_topk_f32", w, users, f, K)
    # ldf > Fi: a strided view of a wider table gives the packed table's bits
    wide = torch.full((I, 8), 7.0, device=DEV)
    wide[:, :5] = table
    view = wide[:, :5]
    assert view.stride(0) == 8
    d_packed = m.predict_all_items(users)
    v_packed, i_packed = m.recommend_with_scores(users, k=K)
    assert torch.equal(bits(m.predict_all_items(users, None, view)), bits(d_packed))
    v_s, i_s = m.recommend_with_scores(users, k=K, item_features=view)
    assert torch.equal(i_s, i_packed) and torch.equal(bits(v_s), bits(v_packed))
    # an out-of-range user id (device ids: found by the kernels) still raises IndexError
    bad = users.clone()
    bad[3] = U
    with pytest.raises(IndexError):
        m.recommend_with_scores(bad, k=K)
    with pytest.raises(IndexError):
        m.predict_all_items(torch.tensor([0, U]))
