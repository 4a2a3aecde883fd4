"""Two-stage serving on the GPU: hnm_cand_union_i32 and hnm_cand_topk_f32 bit for bit against
their numpy restatement (rerank_oracle.py), hnm_widedeep_cand_topk_ex_f32 bit for bit against the
dense Wide&Deep entry, `Reranker` against the composition of its parts, and
`Recommender.add_reranker`.  Values are compared through an int32 view."""
import ctypes as C

import numpy as np
import pytest
import torch

import lattice as L
import rerank_oracle as RO
from hnm_recommendation_amd import (ImplicitALS, ItemCF, MatrixFactorization, NeuralCF,
                                    PopularityBaseline, Reranker, WideDeep, _lib)
from hnm_recommendation_amd import synthetic as syn
from hnm_recommendation_amd.models import reranker as RR
from hnm_recommendation_amd.serving import Recommender
from test_gpu_prefilter import to_module, wd_model
from test_gpu_widedeep_itemfeat import fixture_model
from test_gpu_widedeep_shapes import EXACT_TOWERS, SCALED, tid

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
INF = float("inf")
CANARY_I, CANARY_V = -7, 123.0


def bits(a):
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a).view(np.int32)


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)


def rng_of(*seed):
    return np.random.Generator(np.random.PCG64(list(seed)))


# ------------------------------------------------------------------ 1. the union
UI = 3000                                         # items of the union cases (16 * 128 < UI)
UNION_SHAPES = [(1, 1), (1, 12), (2, 33), (3, 48), (16, 128), (4, 512)]


def union_case(G, kc, B):
    """[G, B, kc] lists: row kinds by b % 5 -- 0 random lists that overlap (with idx < 0 and
    non-finite values sprinkled in, the ids 0 and UI - 1 present), 1 everything empty, 2 G
    identical lists, 3 disjoint lists, 4 an -inf value on valid ids.  B = 1: kind 0."""
    rng = rng_of(11, G, kc, B)
    idx = np.empty((G, B, kc), np.int64)
    val = rng.standard_normal((G, B, kc)).astype(np.float32)
    pool = min(UI, max(2 * kc, 8))                # a small pool: the lists of a row overlap
    for b in range(B):
        kind = b % 5
        for g in range(G):
            idx[g, b] = rng.choice(pool, size=kc, replace=kc > pool) * (UI // pool)
        if kind == 0:
            hole = rng.random((G, kc)) < 0.2
            idx[:, b][hole] = -1 - rng.integers(0, 3, int(hole.sum()))
            bad = rng.random((G, kc)) < 0.2
            val[:, b][bad] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32),
                                        int(bad.sum()))
            idx[0, b, 0], val[0, b, 0] = 0, 1.0
            idx[G - 1, b, kc - 1], val[G - 1, b, kc - 1] = UI - 1, -1.0
        elif kind == 1:
            half = rng.random((G, kc)) < 0.5
            idx[:, b][half] = -1
            val[:, b][~half] = np.nan
        elif kind == 2:
            idx[:, b] = idx[0, b]
        elif kind == 3:
            idx[:, b] = rng.permutation(UI)[:G * kc].reshape(G, kc)
        else:
            val[:, b, ::2] = -np.inf
    return val, idx


def call_union(lv, li, B, G, kc, num_items, ldc, out=None):
    """One entry call on device tensors; li / lv may be views (li's strides are passed)."""
    if out is None:
        out = (torch.full((B, ldc), CANARY_I, dtype=torch.int32, device=DEV),
               torch.full((B,), CANARY_I, dtype=torch.int32, device=DEV))
    gs, bs = (li.stride(0), li.stride(1)) if li is not None else (B * kc, kc)
    _lib.call("hnm_cand_union_i32", _lib.ctx(DEV), _lib.ptr(lv), _lib.ptr(li), B, G, gs, bs, kc,
              num_items, _lib.ptr(out[0]), ldc, _lib.ptr(out[1]))
    return out


def strided(a, fill):
    G, rows, kc = a.shape
    big = torch.full((G, rows + 3, kc + 5), fill, dtype=a.dtype, device=DEV)
    view = big[:, 1:rows + 1, 2:kc + 2]
    view.copy_(a)
    assert view.stride(1) > kc
    return view


def assert_union(got, want):
    assert np.array_equal(got[0].cpu().numpy(), want[0])
    assert np.array_equal(got[1].cpu().numpy(), want[1])


@pytest.mark.parametrize("B", [1, 5, 9])
@pytest.mark.parametrize("G,kc", UNION_SHAPES, ids=lambda v: str(v))
def test_union_is_bitwise_the_numpy_restatement(G, kc, B):
    val, idx = union_case(G, kc, B)
    want = RO.union(val, idx, UI)
    assert not want[2]
    if B > 1:                                      # what the case must provide
        assert want[1][1] == 0 and want[1][2] == len(np.unique(idx[0, 2]))
        assert want[1][3] == G * kc
        assert (want[1][4] < len(np.unique(idx[:, 4]))) or kc == 1
    assert want[0][0, want[1][0] - 1] == UI - 1 and (want[0][0, 0] == 0 or G * kc == 1)
    lv, li = dev(val), dev(idx)
    assert_union(call_union(lv, li, B, G, kc, UI, G * kc), want)
    assert_union(call_union(lv, li, B, G, kc, UI, G * kc), want)        # the same bits again
    # a strided view: what lies between the lists would be read as live ids
    assert_union(call_union(strided(lv, 1.0), strided(li, 1), B, G, kc, UI, G * kc), want)
    # ldc > G * kc: the tail is -1
    wide = RO.union(val, idx, UI, ldc=G * kc + 7)
    assert_union(call_union(lv, li, B, G, kc, UI, G * kc + 7), wide)
    # list_val = NULL: only idx < 0 is empty
    assert_union(call_union(None, li, B, G, kc, UI, G * kc), RO.union(None, idx, UI))
    _lib.sync_check(DEV)                                               # no id was out of range


def test_union_out_of_range_id_raises_and_is_skipped():
    G, kc, B = 3, 48, 9
    val, idx = union_case(G, kc, B)
    clean = RO.union(val, idx, UI)
    idx = idx.copy()
    g, j = next((g, j) for g in range(G) for j in range(kc)
                if idx[g, 5, j] >= 0 and np.isfinite(val[g, 5, j])
                and (idx[:, 5] == idx[g, 5, j]).sum() == 1)
    idx[g, 5, j] = UI
    want = RO.union(val, idx, UI)
    assert want[2] and want[1][5] == clean[1][5] - 1
    got = call_union(dev(val), dev(idx), B, G, kc, UI, G * kc)
    with pytest.raises(IndexError):
        _lib.sync_check(DEV)
    _lib.sync_check(DEV)                                               # the word was cleared
    assert_union(got, want)
    rows = [b for b in range(B) if b != 5]
    assert np.array_equal(got[0].cpu().numpy()[rows], clean[0][rows])   # the other rows intact


@pytest.mark.parametrize("G,kc", [(17, 4), (1, 513), (3, 683), (0, 4), (2, 0)])
def test_union_limits_are_unsupported_and_write_nothing(G, kc):
    """G = 17, kc = 513, G * kc = 2,049 and sizes below the limits: ValueError, the outputs keep
    their fill pattern."""
    rows = 4
    li = torch.zeros(max(G, 1) * rows * max(kc, 1), dtype=torch.int64, device=DEV)
    out = (torch.full((rows, 2100), CANARY_I, dtype=torch.int32, device=DEV),
           torch.full((rows,), CANARY_I, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="cand_union"):
        _lib.call("hnm_cand_union_i32", _lib.ctx(DEV), None, _lib.ptr(li), rows, G, rows * kc, kc,
                  kc, 100, _lib.ptr(out[0]), 2100, _lib.ptr(out[1]))
    torch.cuda.synchronize()
    assert bool((out[0] == CANARY_I).all()) and bool((out[1] == CANARY_I).all())


def test_union_degenerate_calls():
    val, idx = union_case(2, 12, 5)
    lv, li = dev(val), dev(idx)
    out = (torch.full((5, 24), CANARY_I, dtype=torch.int32, device=DEV),
           torch.full((5,), CANARY_I, dtype=torch.int32, device=DEV))
    call_union(lv, li, 0, 2, 12, UI, 24, out=out)                      # B = 0
    call_union(None, None, 0, 2, 12, UI, 24, out=out)
    with pytest.raises(ValueError, match="ldc"):                       # ldc < G * kc
        call_union(lv, li, 5, 2, 12, UI, 23, out=out)
    torch.cuda.synchronize()
    assert bool((out[0] == CANARY_I).all()) and bool((out[1] == CANARY_I).all())


# ------------------------------------------------------------------ 2. the selection
SEL_LDC = 200


def call_select(scores, cand, n, k, out=None):
    B, ldc = cand.shape
    if out is None:
        out = (torch.full((B, k), CANARY_V, dtype=torch.float32, device=DEV),
               torch.full((B, k), CANARY_I, dtype=torch.int64, device=DEV))
    _lib.call("hnm_cand_topk_f32", _lib.ctx(DEV), _lib.ptr(scores), _lib.ptr(cand), ldc,
              _lib.ptr(n), B, k, _lib.ptr(out[0]), _lib.ptr(out[1]))
    return out


def select_case(k):
    """Small-integer scores (ties everywhere), distinct ids in random order with some -1, NaN
    and -inf scores; cand_n in {0, 1, k - 1, k, ldc}, twice over plus one."""
    rng = rng_of(23, k)
    ns = np.array([0, 1, k - 1, k, SEL_LDC] * 2 + [SEL_LDC // 2], np.int32)
    B = len(ns)
    cand = np.stack([rng.permutation(5000)[:SEL_LDC] for _ in range(B)]).astype(np.int32)
    cand[rng.random((B, SEL_LDC)) < 0.05] = -1
    scores = rng.integers(-2, 3, (B, SEL_LDC)).astype(np.float32)
    scores[rng.random((B, SEL_LDC)) < 0.05] = np.nan
    scores[rng.random((B, SEL_LDC)) < 0.05] = -np.inf
    scores[B - 1, 3] = np.inf
    return scores, cand, ns


@pytest.mark.parametrize("k", [1, 12, 64, 128])
def test_select_is_bitwise_the_numpy_restatement(k):
    scores, cand, ns = select_case(k)
    wv, wi = RO.select(scores, cand, ns, k)
    ties = sum(int((wv[b, :-1] == wv[b, 1:]).sum()) for b in range(len(ns))) if k > 1 else 1
    assert ties > 0 and (wi[:, -1] < 0).any() and (wi[:, -1] >= 0).any()
    gv, gi = call_select(dev(scores), dev(cand), dev(ns), k)
    assert np.array_equal(gi.cpu().numpy(), wi) and np.array_equal(bits(gv), bits(wv))


def test_select_refuses_k_129_and_k_0():
    scores, cand, ns = select_case(12)
    out = (torch.full((len(ns), 129), CANARY_V, dtype=torch.float32, device=DEV),
           torch.full((len(ns), 129), CANARY_I, dtype=torch.int64, device=DEV))
    for k in (129, 0, -1):
        with pytest.raises(ValueError, match="cand_topk"):
            call_select(dev(scores), dev(cand), dev(ns), k, out=out)
    torch.cuda.synchronize()
    assert bool((out[0] == CANARY_V).all()) and bool((out[1] == CANARY_I).all())


# ------------------------------------------------------------------ 3. Wide&Deep candidates
WU, WI, WB, WLDC = 300, 1111, 9, 128
CAND_N = [0, 1, 31, 32, 33, 100, 100, 33, 31]     # empty, partial tile, one tile, a tile plus one


def wd_cand(m, users, cand, n, k, want_scores=True, user_features=None):
    """hnm_widedeep_cand_topk_ex_f32 on the model's weights and registered tables."""
    w, keep = m._weights()
    f = m._features(user_features, users)
    itf, tab, ldf = m._item_table(None, users.device, keep)
    B, ldc = cand.shape
    kk = max(k, 1)
    ov = torch.full((B, kk), CANARY_V, dtype=torch.float32, device=DEV)
    oi = torch.full((B, kk), CANARY_I, dtype=torch.int64, device=DEV)
    os_ = torch.full((B, ldc), CANARY_V, dtype=torch.float32, device=DEV) if want_scores else None
    _lib.call("hnm_widedeep_cand_topk_ex_f32", _lib.ctx(DEV), w, _lib.ptr(users), B, _lib.ptr(f),
              _lib.ptr(cand), ldc, _lib.ptr(n), k, _lib.ptr(ov), _lib.ptr(oi), _lib.ptr(os_),
              None if itf is None else C.byref(itf), _lib.ptr(tab), ldf)
    return ov, oi, os_


def cand_rows(I, B, ldc, ns, seed):
    """Random distinct ids per row; past cand_n the odd rows hold -1, the even rows live ids
    that must not be read as candidates."""
    rng = rng_of(31, I, B, ldc, seed)
    cand = np.stack([rng.permutation(I)[:ldc] for _ in range(B)]).astype(np.int32)
    for b in range(1, B, 2):
        cand[b, ns[b]:] = -1
    return cand


def gathered(dense, cand, ns):
    """dense [B, I] (numpy) -> out_scores' expected value: the score of cand[b, j], -inf past n."""
    B, ldc = cand.shape
    want = np.full((B, ldc), -np.inf, np.float32)
    for b in range(B):
        want[b, :ns[b]] = dense[b, cand[b, :ns[b]]]
    return want


def check_wd_candidates(m, users, user_features=None, ks=(12, 64), ns=CAND_N):
    I = m.num_items
    ns = np.asarray(ns, np.int32)
    cand = cand_rows(I, len(ns), WLDC, ns, 0)
    dense = m.predict_all_items(users, user_features).cpu().numpy()
    want_s = gathered(dense, cand, ns)
    dc, dn = dev(cand), dev(ns)
    for k in ks:
        ov, oi, os_ = wd_cand(m, users, dc, dn, k, user_features=user_features)
        # the first to hold: every candidate's score is the dense entry's, bit for bit
        assert torch.equal(os_.view(torch.int32).cpu(), torch.from_numpy(want_s).view(torch.int32))
        wv, wi = RO.select(want_s, cand, ns, k)
        assert np.array_equal(oi.cpu().numpy(), wi) and np.array_equal(bits(ov), bits(wv))
        # without out_scores: the same selection
        ov2, oi2, _ = wd_cand(m, users, dc, dn, k, want_scores=False,
                              user_features=user_features)
        assert torch.equal(oi2, oi) and np.array_equal(bits(ov2), bits(ov))
    _lib.sync_check(DEV)
    return cand, ns, want_s


@pytest.mark.parametrize("layers", EXACT_TOWERS + [[512, 256, 128]], ids=tid)
def test_wd_candidate_scores_are_bitwise_the_dense_entries(layers):
    d = 64 if layers[0] == 512 else 16
    m, _ = wd_model(WU, WI, seed=5, layers=tuple(layers), d=d, **SCALED)
    users = torch.from_numpy(syn.user_batch(WU, WB, seed=6)).to(DEV)
    check_wd_candidates(m, users)


def test_wd_candidates_with_user_and_item_features():
    m = fixture_model("a")                         # registered user and item feature tables
    assert m.num_user_features > 0 and m.num_item_features > 0
    users = torch.from_numpy(syn.user_batch(m.num_users, WB, seed=6)).to(DEV)
    check_wd_candidates(m, users, ks=(12,))
    # explicit batch features win over the registered table
    uf = torch.from_numpy(L.wd_features(WB, m.num_user_features, seed=3)).to(DEV)
    check_wd_candidates(m, users, user_features=uf, ks=(12,))


def test_wd_candidates_exact_ties_go_to_the_lower_id():
    U, I, d, tower = 200, 600, 8, (32, 16)
    sd = L.wd_state_dict(U, I, d, tower, seed=4)
    m = to_module(WideDeep(U, I, embedding_dim=d, deep_layers=list(tower)), sd)
    users = torch.from_numpy(syn.user_batch(U, WB, seed=6)).to(DEV)
    ns = [100] * WB
    cand, ns, want_s = check_wd_candidates(m, users, ks=(12, 64), ns=ns)
    wv, wi = RO.select(want_s, cand, ns, 64)
    tied = (wv[:, :-1] == wv[:, 1:])
    assert tied.sum() >= WB                        # exact ties among the selected ...
    assert (wi[:, :-1][tied] < wi[:, 1:][tied]).all()   # ... in ascending id


def test_wd_candidates_k_0_k_65_and_out_of_range():
    m, _ = wd_model(WU, WI, seed=5, layers=(40, 50, 20), d=16, **SCALED)
    users = torch.from_numpy(syn.user_batch(WU, WB, seed=6)).to(DEV)
    ns = np.asarray(CAND_N, np.int32)
    cand = cand_rows(WI, WB, WLDC, ns, 1)
    dense = m.predict_all_items(users).cpu().numpy()
    want_s = gathered(dense, cand, ns)
    # k = 0 with out_scores: only the scores are written
    ov, oi, os_ = wd_cand(m, users, dev(cand), dev(ns), 0)
    assert np.array_equal(bits(os_), bits(want_s))
    assert bool((ov == CANARY_V).all()) and bool((oi == CANARY_I).all())
    # k = 0 without, k = 65, ldc = 2,049: refused, nothing written
    with pytest.raises(ValueError, match="widedeep_cand"):
        wd_cand(m, users, dev(cand), dev(ns), 0, want_scores=False)
    big = torch.zeros(WB, 2049, dtype=torch.int32, device=DEV)
    for c, k in ((dev(cand), 65), (big, 12)):
        with pytest.raises(ValueError, match="widedeep_cand"):
            ov, oi, os_ = wd_cand(m, users, c, dev(ns), k)
    # a candidate >= num_items is flagged and skipped, one < 0 is skipped silently
    bad = cand.copy()
    bad[5, 7], bad[5, 40], bad[4, 32] = WI, -1, WI + 5
    ov, oi, os_ = wd_cand(m, users, dev(bad), dev(ns), 12)
    with pytest.raises(IndexError):
        _lib.sync_check(DEV)
    _lib.sync_check(DEV)
    want_bad = want_s.copy()
    want_bad[5, 7] = want_bad[5, 40] = want_bad[4, 32] = -np.inf
    assert np.array_equal(bits(os_), bits(want_bad))
    wv, wi = RO.select(want_bad, bad, ns, 12)
    assert np.array_equal(oi.cpu().numpy(), wi) and np.array_equal(bits(ov), bits(wv))
    # an out-of-range user id: the existing entries' IndexError
    users_bad = users.clone()
    users_bad[2] = WU
    wd_cand(m, users_bad, dev(cand), dev(ns), 12)
    with pytest.raises(IndexError):
        _lib.sync_check(DEV)


# ------------------------------------------------------------------ 4. end to end
E = 6000
EMPTY_USERS = (0, 17)
DEPTH = 24


class World:
    """The interactions, the fitted sources, the rankers and a batch, built once."""

    def __init__(self):
        users, items = syn.interactions(WU, WI, E, seed=2)
        keep = ~np.isin(users, EMPTY_USERS)                        # users without a history
        self.users, self.items = users[keep], items[keep]
        self.icf = ItemCF(WU, WI, num_neighbors=8, shrink=1.0).to(DEV)
        self.icf.fit_interactions(self.users, self.items)
        self.als = ImplicitALS(WU, WI, embedding_dim=16, iterations=2).to(DEV)
        self.als.fit_interactions(self.users, self.items)
        self.pop = PopularityBaseline(n_items=WI).to(DEV)
        self.pop.fit_interactions(self.items)
        self.hist = self.icf.history
        self.wd, _ = wd_model(WU, WI, seed=5, layers=(40, 50, 20), d=16, **SCALED)
        self.mf = to_module(MatrixFactorization(WU, WI, embedding_dim=16, sparse=False),
                            syn.mf_state_dict(WU, WI, 16, seed=5, bias_scale=0.05))
        self.ncf = to_module(NeuralCF(WU, WI), syn.ncf_state_dict(WU, WI, 64, (128, 64, 32),
                                                                  seed=3))
        rng = rng_of(3)
        self.batch = np.concatenate([[0, 17, 5, 299, 5], rng.integers(0, WU, size=20)])

    def sources(self, G):
        two = [("item_cf", self.icf), ("popularity", self.pop)]
        three = [("item_cf", self.icf), ("implicit_als", self.als), ("popularity", self.pop)]
        return two if G == 2 else three

    def seen(self, u):
        ptr, idx = self.hist.hist_ptr.cpu().numpy(), self.hist.hist_idx.cpu().numpy()
        return set(idx[ptr[u]:ptr[u + 1]].tolist())


_world = []


@pytest.fixture
def world():
    if not _world:
        _world.append(World())
    return _world[0]


def oracle_candidates(sources, ids, filt, depth):
    lists = [m.recommend_with_scores(ids, filt, k=depth) for _, m in sources]
    vals = np.stack([v.cpu().numpy() for v, _ in lists])
    idxs = np.stack([i.cpu().numpy() for _, i in lists])
    cand, n, oob = RO.union(vals, idxs, WI)
    assert not oob
    return cand, n


def assert_same(got, want):
    assert np.array_equal(got[1].cpu().numpy(), want[1])
    assert np.array_equal(bits(got[0]), bits(want[0]))


@pytest.mark.parametrize("k", [12, 100])
@pytest.mark.parametrize("G", [2, 3])
def test_widedeep_reranker_is_the_composition_of_its_parts(world, G, k):
    r = Reranker(world.wd, world.sources(G), depth=DEPTH)
    assert r._depth(k) == DEPTH
    assert r.scoring_route(k) == (RR.ROUTE_WIDEDEEP if k <= 64 else RR.ROUTE_WIDEDEEP_WIDE)
    host = torch.from_numpy(world.batch)
    dense = world.wd.predict_all_items(host).cpu().numpy()
    for ids in (host, host.to(DEV)):
        for filt in (None, world.hist):
            cand, n = oracle_candidates(world.sources(G), ids, filt, DEPTH)
            assert (n[2:] < G * DEPTH).any()               # sources overlap: the union's case
            gc, gn = r.candidates(ids, filt, depth=DEPTH)
            assert np.array_equal(gc.cpu().numpy(), cand) and np.array_equal(gn.cpu().numpy(), n)
            want = RO.select(gathered(dense, cand, n), cand, n, k)
            got = r.recommend_with_scores(ids, filter_items=filt, k=k)
            assert got[0].shape == (len(world.batch), k) and got[1].dtype == torch.int64
            assert_same(got, want)
            if filt is not None:                           # no filtered item appears
                for b, u in enumerate(world.batch):
                    assert not world.seen(int(u)) & set(got[1][b].cpu().tolist())
    if k == 12:                                            # recommend / forward: the ids alone
        r12 = Reranker(world.wd, world.sources(G), depth=DEPTH, top_k=12)
        assert torch.equal(r12.recommend(host, world.hist), got[1])
        assert torch.equal(r12(host, world.hist), got[1])


def test_user_whose_sources_return_nothing_gets_an_empty_row(world):
    r = Reranker(world.wd, [("item_cf", world.icf)], depth=DEPTH)
    v, i = r.recommend_with_scores(torch.from_numpy(world.batch), filter_items=world.hist, k=12)
    v, i = v.cpu().numpy(), i.cpu().numpy()
    for b in (0, 1):                                       # users 0 and 17: no history
        assert (i[b] == -1).all() and (v[b] == -INF).all()
    assert (i[2:, 0] >= 0).any()


@pytest.mark.parametrize("ranker", ["mf", "ncf"])
@pytest.mark.parametrize("G", [2, 3])
def test_generic_ranker_scores_are_its_forward_on_the_pairs(world, ranker, G):
    m = getattr(world, ranker)
    r = Reranker(m, world.sources(G), depth=DEPTH)
    assert r.scoring_route() == RR.ROUTE_PAIRS
    ids = torch.from_numpy(world.batch).to(DEV)
    cand, n = oracle_candidates(world.sources(G), ids, world.hist, DEPTH)
    W = cand.shape[1]
    items = torch.from_numpy(np.maximum(cand, 0).astype(np.int64)).to(DEV).reshape(-1)
    scores = m.forward(ids.repeat_interleave(W), items).reshape(len(world.batch), W)
    for k in (12, 100):
        want = RO.select(scores.cpu().numpy(), cand, n, k)
        assert_same(r.recommend_with_scores(ids, filter_items=world.hist, k=k), want)


def test_module_edge_calls(world):
    r = Reranker(world.wd, world.sources(2))
    with pytest.raises(IndexError):                         # host ids: checked on the host
        r.recommend_with_scores(torch.tensor([0, WU]))
    v, i = r.recommend_with_scores(torch.tensor([1, 2]), k=0)
    assert v.shape == (2, 0) and i.shape == (2, 0)
    v, i = r.recommend_with_scores(torch.zeros(0, dtype=torch.int64), k=5)
    assert v.shape == (0, 5) and i.shape == (0, 5)
    with pytest.raises(ValueError, match="128"):
        r.recommend_with_scores(torch.tensor([1]), k=1000)
    v, i = r.recommend_with_scores(torch.tensor([1]), k=128)   # depth 128 from each source
    assert v.shape == (1, 128) and bool((i >= 0).all())
    assert len(set(i[0].cpu().tolist())) == 128


def test_recommender_add_reranker(world):
    srv = Recommender(WU, WI, device=DEV)
    icf = srv.add_item_cf(world.users, world.items, num_neighbors=8, shrink=1.0)
    srv.add_popularity_baseline(world.items)
    srv.add_model("wide_deep", world.wd)
    best = srv._get_best_model()
    r = srv.add_reranker("wide_deep", ["item_cf", "popularity_baseline"], depth=DEPTH)
    assert srv.models["reranker"] is r and srv._get_best_model() == best
    assert srv._resolve_model("best")[0] == best
    assert r.back_fill_short_rows and not r.answers_baskets and r.history is icf.history
    ask = [3, 0, 10 ** 6, 17, 299]
    known = [3, 0, 17, 299]
    wv, wi = r.recommend_with_scores(torch.tensor(known), filter_items=srv._device_history(),
                                     k=12)
    wv, wi = wv.cpu().tolist(), wi.cpu().tolist()
    out = srv.get_batch_recommendations(ask, model_name="reranker", num_items=12,
                                        include_scores=True)
    assert "error" in out[2]
    for row, res in zip(range(4), [out[0], out[1], out[3], out[4]]):
        arts = [x["article_id"] for x in res["recommendations"]]
        assert res["model_name"] == "reranker" and len(arts) == 12
        assert arts == [str(x) for x in wi[row]]
        assert [x["score"] for x in res["recommendations"]] == wv[row]
    one = srv.get_recommendations(3, model_name="reranker", num_items=12)
    assert [x["article_id"] for x in one["recommendations"]] == \
        [x["article_id"] for x in out[0]["recommendations"]]
    # short rows are back-filled from the popularity baseline: ItemCF alone has nothing for a
    # user without a history
    solo = srv.add_reranker("wide_deep", ["item_cf"], name="solo", depth=DEPTH)
    assert bool((solo.recommend_with_scores(torch.tensor([17]), k=12)[1] == -1).all())
    res = srv.get_recommendations(17, model_name="solo", num_items=12)
    pv, pi = srv.models["popularity_baseline"].recommend_with_scores(torch.tensor([17]), k=12)
    assert [x["article_id"] for x in res["recommendations"]] == [str(x) for x in pi[0].tolist()]
    assert srv._get_best_model() == best
    with pytest.raises(ValueError, match="cannot answer from a basket"):
        srv.get_recommendations_for_items([1, 2], model_name="reranker")
