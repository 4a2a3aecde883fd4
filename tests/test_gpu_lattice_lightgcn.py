"""GPU: LightGCN -- CSR build, every SpMM route, rows_combine, the model's propagation routes,
scoring and top-K -- against the float64 oracles of tests/lgcn_lattice.py, on ids and on values
as uint32 bits.

Every degree (self-loop included) of these graphs is a power of four, so every normalized value
is a power of two (or a small integer times one) and every intermediate a dyadic rational that
fp32 holds exactly: the result is one number in any summation order and the oracle is bitwise for
the short walk, the long-row walk and its pieces, heavy segments and the finish, the plan-less
and the legacy orders alike.  Replicated graphs (R = 5 disjoint copies with identical embedding
rows) put an exact tie across every tested k, so the (score desc, item asc) order decides every
row of every top-K.  tests/test_cpu_lgcn_lattice.py checks those properties on the CPU.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import lattice as L
import lgcn_lattice as G
from hnm_recommendation_amd import LightGCN, _lib
from hnm_recommendation_amd import synthetic as syn
from hnm_recommendation_amd.models.lightgcn import NormalizedGraph

pytestmark = pytest.mark.gpu
DEV = "cuda"
CANARY = 777.0
VARIANTS = ("unweighted", "weighted")


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def same_bits(got, want, what=""):
    got = host(got) if isinstance(got, torch.Tensor) else got
    g, w = L.bits(got), L.bits(want)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {g.size} values differ, first at {i}: "
                             f"got {got[i]!r}, want {np.asarray(want)[i]!r}")


def lattice_graph(which):
    return G.legacy_graph() if which == "legacy" else G.heavy_graph(which == "weighted")


def build(g):
    return NormalizedGraph(torch.from_numpy(g.edge_index), None if g.edge_weight is None
                           else torch.from_numpy(g.edge_weight), g.N, torch.device(DEV))


@functools.lru_cache(maxsize=None)
def device_graph(which):
    return build(lattice_graph(which))


def spmm(ng, X, Y=None, alpha=0.0, acc_in=None, acc_out=None, beta=0.0, rows=None, acc_row0=0,
         plan="whole"):
    """hnm_spmm_csr_range_f32; plan: "whole" (the graph's own), None (plan-less) or a handle."""
    r0, r1 = (0, ng.num_nodes) if rows is None else rows
    _lib.check(_lib.fn("hnm_spmm_csr_range_f32")(
        _lib.ctx(X.device), ng.plan if plan == "whole" else plan, ng.num_nodes, _lib.ptr(ng.rowptr),
        _lib.ptr(ng.col), _lib.ptr(ng.val), _lib.ptr(X), X.shape[1], _lib.ptr(Y), alpha,
        _lib.ptr(acc_in), _lib.ptr(acc_out), beta, r0, r1, acc_row0), "hnm_spmm_csr_range_f32")


def combine(ng, plan, rows, layers, alphas):
    out = torch.full((rows.numel(), layers[0].shape[1]), CANARY, device=DEV)
    n = len(layers)
    ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in layers])
    al = (C.c_float * (n + 1))(*alphas)
    _lib.check(_lib.fn("hnm_spmm_rows_combine_f32")(
        _lib.ctx(rows.device), plan, ng.num_nodes, _lib.ptr(ng.rowptr), _lib.ptr(ng.col),
        _lib.ptr(ng.val), _lib.ptr(rows), rows.numel(), layers[0].shape[1], ptrs, al, n,
        _lib.ptr(out)), "hnm_spmm_rows_combine_f32")
    return out


# ------------------------------------------------------------------ CSR build
def assert_csr(ng, csr, what):
    assert np.array_equal(host(ng.rowptr), csr.rowptr), f"{what}: rowptr"
    got = host(ng.col)
    if not np.array_equal(got, csr.col):
        p = int(np.argwhere(got != csr.col)[0, 0])
        r = int(np.searchsorted(csr.rowptr, p, side="right") - 1)
        s, e = csr.rowptr[r], csr.rowptr[r + 1]
        raise AssertionError(f"{what}: col differs first in row {r}: got {got[s:e][:12]}, want "
                             f"{csr.col[s:e][:12]}")
    same_bits(ng.val, csr.val, f"{what}: val")


CSR_GRAPHS = {"regular3": lambda: G.REGULAR3[64].graph, "mixed_L1": lambda: G.MIXED_L1.graph,
              "heavy_L1": lambda: G.heavy_graph(False), "heavy_L1-weighted": lambda: G.heavy_graph(True),
              "legacy": G.legacy_graph}


@pytest.mark.parametrize("name", list(CSR_GRAPHS))
def test_csr_build_is_the_oracle(name):
    """rowptr, col and val of hnm_csr_build_norm: stable by row, the edge list's order kept
    within a row, the self-loop last, duplicates kept."""
    g = CSR_GRAPHS[name]()
    ng = device_graph(name[9:] or "unweighted") if name.startswith("heavy_L1") else \
        device_graph("legacy") if name == "legacy" else build(g)
    assert_csr(ng, g.csr, name)


def test_csr_build_reverse_row_order_with_duplicates():
    """Rows descending (the last item's edges first), each row's edges in the reverse of the
    shuffled list's order."""
    g = G.heavy_graph(True)
    o = np.argsort(-g.edge_index[0, ::-1], kind="stable")
    ei, w = g.edge_index[:, ::-1][:, o], g.edge_weight[::-1][o]
    assert (np.diff(ei[0]) <= 0).all()
    key = ei[0] * g.N + ei[1]
    assert len(np.unique(key)) < len(key)                # duplicate pairs
    rev = G.Graph(g.U, g.I, ei, w)
    assert not np.array_equal(rev.csr.col, g.csr.col)    # another order within the rows
    assert_csr(build(rev), rev.csr, "reverse")


def test_csr_build_ordinary_graph_within_rounding():
    """A graph off the lattice (zipf degrees, quarter-integer weights): structure exact; val
    within 8 * 2^-24 relative of the float64 value -- to first order 6 u (sqrt and divide for
    each of the two dinv, two multiplications), 8 u leaves the second-order terms."""
    U, I = 3000, 700
    ei = syn.bipartite_edge_index(U, I, 20_000, seed=6)
    w = (np.random.default_rng(1).integers(1, 13, ei.shape[1]) * 0.25).astype(np.float32)
    g = G.Graph(U, I, ei, w)
    csr = G.csr_oracle(ei, w, g.N, lattice=False)
    assert not np.isin(csr.deg, G.POW4).all()
    ng = build(g)
    assert np.array_equal(host(ng.rowptr), csr.rowptr) and np.array_equal(host(ng.col), csr.col)
    rel = np.abs(host(ng.val).astype(np.float64) - csr.val64) / csr.val64
    print(f"ordinary graph: max relative error of val {rel.max() * 2 ** 24:.2f} u")
    assert rel.max() <= 8 * 2.0 ** -24


# ------------------------------------------------------------------ one layer, every route
@functools.lru_cache(maxsize=None)
def layer_on_device(which, d):
    g, X, Y, _ = G.layer_case(which, d)
    ng = device_graph(which)
    ng.prepare(d)
    return g, ng, dev(X), X, Y


LAYER = pytest.mark.parametrize("which,d", [(w, d) for w in VARIANTS for d in G.LAYER_DS])


@LAYER
def test_layer_whole_graph_plan(which, d):
    """The short walk, the long-row walk (one piece and two), the 4,096-entry row's eight pieces
    and the finish, in one call."""
    g, ng, x, X, Y = layer_on_device(which, d)
    y = torch.full_like(x, CANARY)
    spmm(ng, x, y)
    same_bits(y, Y, "whole-graph plan")
    y2 = torch.full_like(x, CANARY)
    ng.spmm(x, y2, 0.0, None)                            # the model's entry
    same_bits(y2, Y, "NormalizedGraph.spmm")


@LAYER
def test_layer_without_plan(which, d):
    g, ng, x, X, Y = layer_on_device(which, d)
    y = torch.full_like(x, CANARY)
    spmm(ng, x, y, plan=None)
    same_bits(y, Y, "plan NULL")


@LAYER
def test_layer_row_ranges(which, d):
    """The users only; a window in the middle of the items that holds the heavy row's
    neighbours but not all long rows.  Rows outside stay untouched."""
    g, ng, x, X, Y = layer_on_device(which, d)
    U = g.U
    for plan in ("whole", None):
        for r0, r1 in ((0, U), (U + 50, U + 230), (U // 2 + 1, U + G.HEAVY_ITEM + 1)):
            y = torch.full_like(x, CANARY)
            spmm(ng, x, y, rows=(r0, r1), plan=plan)
            want = np.full_like(Y, CANARY)
            want[r0:r1] = Y[r0:r1]
            same_bits(y, want, f"rows [{r0}, {r1}) plan {plan}")


@LAYER
def test_layer_restricted_plans(which, d):
    """Two item shards, the first with the heavy item: each computes the users and its shard."""
    g, ng, x, X, Y = layer_on_device(which, d)
    U, I = g.U, g.I
    for lo, hi in ((0, I // 2), (I // 2, I)):
        plan = ng.restricted(((0, U), (U + lo, U + hi)), d)
        y = torch.full_like(x, CANARY)
        spmm(ng, x, y, plan=plan)
        want = np.full_like(Y, CANARY)
        want[:U], want[U + lo:U + hi] = Y[:U], Y[U + lo:U + hi]
        same_bits(y, want, f"restricted, items [{lo}, {hi})")
        y = torch.full_like(x, CANARY)                   # the last layer's form
        spmm(ng, x, y, rows=(U + lo, U + hi), plan=plan)
        want[:U] = CANARY
        same_bits(y, want, f"restricted + range, items [{lo}, {hi})")


@LAYER
def test_layer_epilogue(which, d):
    """acc = fma(alpha, y, beta * x) (acc_in NULL) and fma(alpha, y, acc) from acc_row0 = U on;
    alpha != beta, and beta must be ignored where an accumulator comes in."""
    g, ng, x, X, Y = layer_on_device(which, d)
    U = g.U
    X64, Y64 = X.astype(np.float64), Y.astype(np.float64)
    first = G.exact_f32(0.5 * Y64[U:] + 0.25 * X64[U:])
    A0 = G.small_ints(g.N - U, d, seed=14)
    second = G.exact_f32(0.25 * Y64[U:] + A0.astype(np.float64))
    for plan in ("whole", None):
        y = torch.full_like(x, CANARY)
        acc = torch.full((g.N - U, d), CANARY, device=DEV)
        spmm(ng, x, y, alpha=0.5, acc_out=acc, beta=0.25, acc_row0=U, plan=plan)
        same_bits(y, Y, f"Y beside the epilogue, plan {plan}")
        same_bits(acc, first, f"fma(alpha, y, beta * x), plan {plan}")
        acc = dev(A0)
        spmm(ng, x, None, alpha=0.25, acc_in=acc, acc_out=acc, beta=0.5, acc_row0=U, plan=plan)
        same_bits(acc, second, f"fma(alpha, y, acc), plan {plan}")
    # items only, as the model's last layer: the accumulator rows of the range alone
    acc = dev(A0)
    spmm(ng, x, None, alpha=0.25, acc_in=acc, acc_out=acc, beta=0.5, rows=(U + 3, U + 300), acc_row0=U)
    want = A0.copy()
    want[3:300] = second[3:300]
    same_bits(acc, want, "epilogue on a row range")


# ------------------------------------------------------------------ rows_combine
def combine_rows(g):
    r = G.heavy_rows(g)
    rows = [r["heavy"], *r["long2"], *r["long1"], *r["hubs"], *r["short"], r["partner"], r["last"],
            r["heavy"], 0]                               # two rows listed twice
    return np.asarray(rows, np.int64)


@LAYER
def test_rows_combine(which, d):
    """Rows of every class, with independent integer layer inputs and four different weights:
    sum_{l < L} alpha_l E_l[r] + alpha_L (A E_{L-1})[r] (hnm.h), with the plan (mode 2) and
    without (mode 0)."""
    g, ng, *_ = layer_on_device(which, d)
    layers = G.combine_layers(which, d)
    rows = combine_rows(g)
    want = G.combine_oracle(g.csr, rows, layers, G.COMBINE_ALPHAS)
    dl = [dev(x) for x in layers]
    for plan in (ng.plan, None):
        out = combine(ng, plan, dev(rows), dl, G.COMBINE_ALPHAS)
        same_bits(out, want, f"rows_combine, plan {'NULL' if plan is None else 'whole'}")


# ------------------------------------------------------------------ legacy plan (N > 2^22)
def test_legacy_plan_layer_epilogue_and_rows_combine():
    """More than 2^22 nodes: short rows one lane group each, long rows one wave, the heavy row in
    segments + the finish, all in CSR order; rows_combine in mode 1."""
    d = G.LEGACY_D
    g, ng, x, X, Y = layer_on_device("legacy", d)
    assert g.N > G.WALK_LIMIT
    U = g.U
    y = torch.full_like(x, CANARY)
    acc = torch.full((g.N - U, d), CANARY, device=DEV)
    spmm(ng, x, y, alpha=0.5, acc_out=acc, beta=0.25, acc_row0=U)
    same_bits(y, Y, "legacy layer")
    same_bits(acc, G.exact_f32(0.5 * Y[U:].astype(np.float64) + 0.25 * X[U:].astype(np.float64)),
              "legacy epilogue")
    y = torch.full_like(x, CANARY)
    spmm(ng, x, y, rows=(U - 7, U + 300))
    want = np.full_like(Y, CANARY)
    want[U - 7:U + 300] = Y[U - 7:U + 300]
    same_bits(y, want, "legacy row range")
    layers = G.combine_layers("legacy", d)
    rows = combine_rows(G.heavy_graph(True))
    rows = np.where(rows < G.HEAVY_USERS + len(G.HUB_ROWS), rows, rows + (g.U - G.heavy_graph(True).U))
    rows = np.concatenate([rows, [g.U - 1, 1 << 21]])    # inserted (isolated) users
    want = G.combine_oracle(g.csr, rows, layers, G.COMBINE_ALPHAS)
    out = combine(ng, ng.plan, dev(rows), [dev(v) for v in layers], G.COMBINE_ALPHAS)
    same_bits(out, want, "legacy rows_combine")


# ------------------------------------------------------------------ model routes
class Prop:
    def __init__(self, id_, graph, E0, num_layers, layers, F):
        self.id, self.graph, self.E0, self.L, self.layers, self.F = id_, graph, E0, num_layers, layers, F
        self.d = E0.shape[1]


@functools.lru_cache(maxsize=None)
def prop_case(name):
    if name.startswith("heavy"):
        _, which, d = name.split("-")
        E0, layers, F, _ = G.heavy_prop(which == "weighted", int(d[1:]))
        return Prop(name, G.heavy_graph(which == "weighted"), E0, 1, layers, F)
    c = next(c for c in G.MODEL_CASES if c.id == name)
    return Prop(name, c.graph, c.E0, c.L, c.prop[0], c.F)


PROP_NAMES = [c.id for c in G.MODEL_CASES] + [f"heavy_L1-{w}-d{d}" for w in VARIANTS
                                              for d in G.HEAVY_F_DS]


@functools.lru_cache(maxsize=None)
def model(name):
    p = prop_case(name)
    g = p.graph
    m = LightGCN(g.U, g.I, embedding_dim=p.d, num_layers=p.L)
    m.set_graph(torch.from_numpy(g.edge_index),
                None if g.edge_weight is None else torch.from_numpy(g.edge_weight))
    with torch.no_grad():
        m.embeddings.weight.copy_(torch.from_numpy(p.E0))
    return m.to(DEV).eval()


@pytest.mark.parametrize("name", PROP_NAMES)
def test_model_propagation_routes(name):
    """forward(), propagate() and propagate_for(users) with repeated, unsorted ids."""
    p, m = prop_case(name), model(name)
    U = p.graph.U
    with torch.no_grad():
        fu, fi = m.forward()
        same_bits(torch.cat([fu, fi]), p.F, "forward()")
        same_bits(m.propagate(), p.F, "propagate()")
        users = np.concatenate([L._rng(2, U).integers(0, U, 300), [U - 1, 0, 0, U - 1]])
        if name.startswith("heavy"):
            users = np.concatenate([users, G.heavy_rows(p.graph)["hubs"]])
        fb, fib = m.propagate_for(torch.from_numpy(users))
        same_bits(fb, p.F[users], "propagate_for: users")
        same_bits(fib, p.F[U:], "propagate_for: items")
    if not name.startswith("heavy"):                     # twins, summed in different entry orders
        I0, F = p.graph.I // G.R, host(fi)
        for a in range(1, G.R):
            assert np.array_equal(L.bits(F[:I0]), L.bits(F[a * I0:(a + 1) * I0])), a


@pytest.mark.parametrize("name", PROP_NAMES)
def test_model_item_sharded_propagation(name):
    """propagate_for_shard for a two-way split: the exchange checks the rows the rank computed
    itself against the oracle's layer, then fills the other shard's item rows from it."""
    p, m = prop_case(name), model(name)
    U, I = p.graph.U, p.graph.I
    users = torch.from_numpy(np.concatenate([L._rng(3, U).integers(0, U, 200), [0, U - 1, 0]]))
    layers = [dev(x) for x in p.layers]
    for lo, hi in ((0, I // 2 + 3), (I // 2 + 3, I)):
        seen = []

        def exchange(Y):
            want = layers[len(seen) + 1]
            seen.append(torch.equal(Y[:U], want[:U]) and torch.equal(Y[U + lo:U + hi], want[U + lo:U + hi]))
            Y[U:U + lo] = want[U:U + lo]
            Y[U + hi:] = want[U + hi:]
        with torch.no_grad():
            fb, fi = m.propagate_for_shard(users, lo, hi, exchange)
        assert seen == [True] * (p.L - 1), seen
        same_bits(fb, p.F[users.numpy()], f"shard [{lo}, {hi}): users")
        same_bits(fi, p.F[U + lo:U + hi], f"shard [{lo}, {hi}): items")


def test_model_unsupported_width_is_refused():
    """No SpMM kernel is 48 floats wide: the model says so instead of falling back."""
    b = G.regular_base()
    m = LightGCN(b.U, b.I, embedding_dim=G.UNSUPPORTED_D, num_layers=3)
    m.set_graph(torch.from_numpy(b.edge_index))
    m = m.to(DEV).eval()
    with pytest.raises(ValueError, match="4, 8, 16, 32, 64, 128, 256"):
        m.forward()


# ------------------------------------------------------------------ scoring and top-K
SCORE_IDS = [c.id for c in G.SCORE_CASES]


@pytest.mark.parametrize("case", G.SCORE_CASES, ids=SCORE_IDS)
def test_model_scores(case):
    """predict_all_items over the propagated tables' [U:] view, and predict on pairs with twins."""
    m = model(case.id)
    B = G.BATCHES[-1]
    with torch.no_grad():
        same_bits(m.predict_all_items(torch.from_numpy(case.users)), case.scores, "predict_all_items")
        I0 = case.graph.I // G.R
        rng = L._rng(4, B)
        items = rng.integers(0, I0, B)
        items = np.concatenate([items, items + 3 * I0])  # each pair again with a twin item
        rows = np.concatenate([np.arange(B), np.arange(B)])
        got = m.predict(torch.from_numpy(case.users[rows]), torch.from_numpy(items))
    same_bits(got, case.scores[rows, items], "predict")
    assert np.array_equal(L.bits(host(got)[:B]), L.bits(host(got)[B:]))


def _topk_params():
    out = []
    for case in G.SCORE_CASES:
        for B in G.BATCHES:
            for k in (*G.FUSED_KS, G.DENSE_K):
                # every filter kind at 70 rows; at 1 and 1,025 rows the tie group at k (1,025
                # rows: at k = 12 and 96 only, the reference sorts 10 M scores per (k, kind))
                kinds = ("none", *G.FILTER_KINDS) if B == 70 else \
                    ("none", "tie_group") if B == 1 or k in (12, G.DENSE_K) else ("none",)
                out += [pytest.param(case, B, k, kind, id=f"{case.id}-B{B}-k{k}-{kind}")
                        for kind in kinds]
    return out


@pytest.mark.parametrize("prefilter", (True, False), ids=("certified", "exact"))
@pytest.mark.parametrize("case,B,k,kind", _topk_params())
def test_model_topk_is_the_oracle(case, B, k, kind, prefilter):
    """recommend_with_scores: k <= 64 the fused hnm_dot_topk_f32 (certified scan or, with the
    pre-filter off, the sample-threshold path), k = 96 dense scores + the row top-K.  An exact
    tie lies across position k in every unfiltered row; ids must be np.argsort(-scores,
    kind="stable") of the oracle's scores."""
    m = model(case.id)
    rv, ri = case.ref(B, k, kind)
    if kind == "none":
        assert L.tie_fraction(case.scores[:B], k) == 1.0
    filt = case.filter_items(B, kind, k)
    d0 = torch.device(DEV)
    m.forward()                                          # the propagation is not what is counted
    _lib.set_prefilter(d0, prefilter)
    _lib.prefilter_stats(d0, reset=True)
    _lib.set_option(d0, _lib.HNM_OPT_STATS, 1)
    try:
        with torch.no_grad():
            ov, oi = m.recommend_with_scores(torch.from_numpy(case.users[:B]), filt, k=k)
        ov, oi = host(ov), host(oi)
    finally:
        _lib.set_option(d0, _lib.HNM_OPT_STATS, 0)
        _lib.set_prefilter(d0, True)
    rows, cands, fallback = _lib.prefilter_stats(d0, reset=True)
    if not np.array_equal(oi, ri):
        b = int(np.argwhere((oi != ri).any(1))[0, 0])
        raise AssertionError(f"ids differ in {int((oi != ri).any(1).sum())} rows, first row {b}: got "
                             f"{oi[b]} scores {ov[b]}, want {ri[b]} scores {rv[b]}")
    same_bits(ov, rv, "top-K scores")
    assert case.graph.I >= L.THRESH_MIN_ITEMS            # the catalogue scan, not the LIST route
    if k > 64:
        assert rows == 0, "k > 64 must take the dense route"
    elif prefilter or kind == "none":
        assert rows == B, (rows, cands, fallback)
