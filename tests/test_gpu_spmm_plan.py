"""LightGCN SpMM plans through the C ABI (planning in graph_plan.hip, kernels in graph.hip): the
short-row walk, the plan's binding to its col / val, and rows_combine's summation order with and
without a plan
(reference: lightgcn.py:136-164, `graph @ all_embeddings` per layer)."""
import ctypes as C

import numpy as np
import pytest
import torch

from hnm_recommendation_amd import LightGCN, _lib
from hnm_recommendation_amd import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _graph(U, I, edges, d):
    m = LightGCN(U, I, d)
    m.set_graph(torch.from_numpy(edges))
    m = m.to(DEV)
    return m, m._device_graph()


def _dense_ref(g, x):
    import scipy.sparse as sp
    rp, col, val = (a.cpu().numpy() for a in (g.rowptr, g.col, g.val))
    N = len(rp) - 1
    A = sp.csr_matrix((val.astype(np.float64), col, rp), shape=(N, N))
    xd = x.double().cpu().numpy()
    return A @ xd, abs(A) @ np.abs(xd)


def _spmm_raw(g, plan, x, y):
    c = _lib.ctx(x.device)
    return _lib.fn("hnm_spmm_csr_f32")(c, plan, g.num_nodes, _lib.ptr(g.rowptr), _lib.ptr(g.col),
                                       _lib.ptr(g.val), _lib.ptr(x), x.shape[1], _lib.ptr(y), 0.0,
                                       None, None)


def _combine_raw(g, plan, rows, layers, alphas, out, val=None):
    c = _lib.ctx(rows.device)
    L = len(layers)
    ptrs = (C.c_void_p * L)(*[t.data_ptr() for t in layers])
    al = (C.c_float * (L + 1))(*[float(a) for a in alphas])
    return _lib.fn("hnm_spmm_rows_combine_f32")(
        c, plan, g.num_nodes, _lib.ptr(g.rowptr), _lib.ptr(g.col),
        _lib.ptr(g.val if val is None else val), _lib.ptr(rows), rows.numel(), layers[0].shape[1],
        ptrs, al, L, _lib.ptr(out))


@pytest.mark.parametrize("d", [4, 64, 128, 256])
def test_spmm_short_walk_rows(d):
    """Rows of at most 128 entries (every user row here, plus the tail items) go through the
    column-ordered short walk (spmm_swalk_kernel): blocks of up to S consecutive rows with LDS
    accumulators.  Rows at the 127 / 128 / 129 boundary, duplicate edges, users with no edge
    (self-loop only), enough rows for several blocks per workgroup at d = 64.  Checked against
    A_hat X in float64 (1e-5 of sum |a||x|), run-to-run bitwise, and row-range calls (the users
    only; a window in the middle) bitwise equal to the whole-graph call with the rest untouched."""
    U, I = 200_000 if d == 64 else 60_000, 3_000
    rng = np.random.default_rng(11)
    base = syn.bipartite_edge_index(U, I, 4 * U, seed=5)
    gone = np.arange(5, 40)  # users 5..39 lose their random edges
    base = base[:, ~(np.isin(base[0], gone) | np.isin(base[1], gone))]
    dup = base[:, :3000]
    fix = []
    for u, n in ((5, 126), (6, 127), (7, 128), (8, 129)):
        it = rng.choice(np.arange(1, I), size=n, replace=False) + U
        fix.append(np.stack([np.full(n, u), it]))
    one = np.concatenate([dup] + fix, axis=1)
    edges = np.concatenate([base, one, one[::-1]], axis=1)
    m, g = _graph(U, I, edges, d)
    N = U + I
    x = torch.randn(N, d, generator=torch.Generator().manual_seed(2)).to(DEV)
    y1, y2 = torch.empty_like(x), torch.empty_like(x)
    g.spmm(x, y1, 0.0, None)
    g.spmm(x, y2, 0.0, None)
    ya = torch.zeros_like(x)
    g.spmm(x, ya, 0.0, None, rows=(0, U))
    mid = (U // 3, U // 3 + 5_000)
    yb = torch.zeros_like(x)
    g.spmm(x, yb, 0.0, None, rows=mid)
    torch.cuda.synchronize()
    assert torch.equal(y1, y2)
    assert torch.equal(ya[:U], y1[:U]) and not ya[U:].any()
    assert torch.equal(yb[mid[0]:mid[1]], y1[mid[0]:mid[1]])
    assert not yb[:mid[0]].any() and not yb[mid[1]:].any()
    rp = g.rowptr.cpu().numpy()
    L = np.diff(rp)
    assert (L[:U] <= 128).sum() >= U - 10 and (L[10:40] == 1).all()
    assert [int(v) for v in L[5:9]] == [127, 128, 129, 130]
    ref, mag = _dense_ref(g, x)
    err = np.abs(y1.double().cpu().numpy() - ref)
    assert (err <= 1e-5 * mag + 1e-30).all(), float((err / (mag + 1e-30)).max())
    # rows_combine sums the short rows in the walk's order: bitwise equal to the layer kernel
    rows = torch.tensor([0, 5, 6, 7, 8, 12, U - 1, U, N - 1, 7], dtype=torch.int64, device=DEV)
    out = torch.empty(rows.numel(), d, device=DEV)
    assert _combine_raw(g, g.plan, rows, [x], [0.0, 1.0], out) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, y1[rows])


def test_plan_null_rows_combine_matches_plan_null_spmm():
    """hnm.h: rows_combine with plan NULL sums every row in the plan-less SpMM's order (one wave
    per row, CSR order), so the two agree bit for bit -- short, long and >2,048-entry rows."""
    U, I, d = 3_000, 20_000, 64
    rng = np.random.default_rng(3)
    base = syn.bipartite_edge_index(U, I, 40_000, seed=4)
    extra = []
    for u, n in ((0, 100), (1, 500), (2, 3_000)):
        it = rng.choice(I, size=n, replace=False) + U
        extra.append(np.stack([np.full(n, u), it]))
    e = np.concatenate(extra, axis=1)
    edges = np.concatenate([base, e, e[::-1]], axis=1)
    m, g = _graph(U, I, edges, d)
    N = U + I
    x = torch.randn(N, d, generator=torch.Generator().manual_seed(5)).to(DEV)
    y = torch.empty_like(x)
    assert _spmm_raw(g, None, x, y) == 0
    rows = torch.tensor([0, 1, 2, 3, U - 1, U, U + 1, N - 1], dtype=torch.int64, device=DEV)
    out = torch.empty(rows.numel(), d, device=DEV)
    assert _combine_raw(g, None, rows, [x], [0.0, 1.0], out) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, y[rows])
    ref, mag = _dense_ref(g, x)
    assert (np.abs(y.double().cpu().numpy() - ref) <= 1e-5 * mag + 1e-30).all()


def test_plan_bound_to_its_values():
    """A plan snapshots the col / val of its first use: a call with another val array is
    refused (HNM_EINVAL) instead of silently mixing stale and new values (hnm.h BINDING)."""
    U, I, d = 2_000, 1_000, 64
    edges = syn.bipartite_edge_index(U, I, 10_000, seed=1)
    m, g = _graph(U, I, edges, d)
    x = torch.randn(U + I, d, generator=torch.Generator().manual_seed(1)).to(DEV)
    y = torch.empty_like(x)
    val2 = g.val.clone()
    c = _lib.ctx(x.device)
    st = _lib.fn("hnm_spmm_csr_f32")(c, g.plan, g.num_nodes, _lib.ptr(g.rowptr), _lib.ptr(g.col),
                                     _lib.ptr(val2), _lib.ptr(x), d, _lib.ptr(y), 0.0, None, None)
    assert st == _lib.HNM_EINVAL
    rows = torch.arange(4, dtype=torch.int64, device=DEV)
    out = torch.empty(4, d, device=DEV)
    assert _combine_raw(g, g.plan, rows, [x], [0.0, 1.0], out, val=val2) == _lib.HNM_EINVAL
    # the bound arrays still work, and prepare for an unsupported d is refused
    assert _spmm_raw(g, g.plan, x, y) == 0
    st = _lib.fn("hnm_spmm_plan_prepare")(c, g.plan, _lib.ptr(g.col), _lib.ptr(g.val), 48)
    assert st == _lib.HNM_EUNSUPPORTED
    torch.cuda.synchronize()


def test_legacy_plan_above_walk_limit():
    """Graphs of more than 2^22 nodes (the walks pack col << 10 into 32 bits) take the
    round-2 classes: short rows one 16-lane group each, long rows one wave, rows over 2,048
    entries in SEG-long segments + the finish tree, all in CSR order.  Checked at that size
    against A_hat X in float64 (1e-5 of sum |a||x|), and propagate_for bitwise equal to
    forward() there (rows_combine repeats each class's order: mode 1)."""
    U, I, d = (1 << 22) + 3000, 4000, 16
    base = syn.bipartite_edge_index(U, I, 2_000_000, seed=9)
    hub = np.stack([np.arange(0, U, 997), np.zeros(len(range(0, U, 997)), np.int64) + U])
    edges = np.concatenate([base, hub, hub[::-1]], axis=1)   # item 0: > 4,000 entries (heavy)
    m = LightGCN(U, I, d)
    m.set_graph(torch.from_numpy(edges))
    m = m.to(DEV)
    g = m._device_graph()
    rp = g.rowptr.cpu().numpy()
    L = np.diff(rp)
    assert L.max() > 2048 and ((L > 128) & (L <= 2048)).any()
    x = torch.randn(U + I, d, generator=torch.Generator().manual_seed(3)).to(DEV)
    y = torch.empty_like(x)
    g.spmm(x, y, 0.0, None)
    torch.cuda.synchronize()
    ref, mag = _dense_ref(g, x)
    err = np.abs(y.double().cpu().numpy() - ref)
    assert (err <= 1e-5 * mag + 1e-30).all(), float((err / (mag + 1e-30)).max())
    users = torch.tensor([0, 997, 5, U - 1, 1 << 21], dtype=torch.int64, device=DEV)
    fb, fi_b = m.propagate_for(users)
    fu, fi = m.forward()
    assert torch.equal(fi_b, fi) and torch.equal(fb, fu[users])


def _raw_graph(N, r, c, v):
    """Device CSR (rowptr int64, col int32, val fp32; entries in (row, col) order) + a plan."""
    import scipy.sparse as sp
    from types import SimpleNamespace
    A = sp.csr_matrix((v.astype(np.float32), (r, c)), shape=(N, N))  # duplicates summed
    A.sort_indices()
    g = SimpleNamespace(num_nodes=N,
                        rowptr=torch.from_numpy(A.indptr.astype(np.int64)).to(DEV),
                        col=torch.from_numpy(A.indices.astype(np.int32)).to(DEV),
                        val=torch.from_numpy(A.data.astype(np.float32)).to(DEV))
    plan = C.c_void_p()
    c = _lib.ctx(g.rowptr.device)
    _lib.check(_lib.fn("hnm_spmm_plan_create")(c, N, _lib.ptr(g.rowptr), C.byref(plan)), "plan")
    return g, plan


@pytest.mark.parametrize("kind", ["small_side_gathers_large", "not_bipartite", "isolated_edges"])
def test_spmm_bipartite_side_routing(kind):
    """The plan's bipartite-side detection (graph_plan.hip plan_bipartite_sides) on graphs unlike the
    H&M layout: a 3,000-row side whose rows (long AND short) gather a 200,000-row table, so that
    side's short rows join the user-ordered walk; the same graph with two same-side edges (no
    split exists: nothing may move); and isolated rows (self-loop only) on both sides of the
    split.  Every case against A X in float64 (1e-5 of sum |a||x|), run-to-run bitwise, a
    row-range call over the small side bitwise equal to the whole call, and rows_combine over
    moved, walked, short and isolated rows bitwise equal to the layer kernel."""
    S, I, d = 3_000, 200_000, 64
    N = S + I
    rng = np.random.default_rng(21)
    deg = rng.integers(130, 400, S)
    deg[::7] = rng.integers(1, 129, len(deg[::7]))       # short rows on the small side
    if kind == "isolated_edges":
        deg[-5:] = 0                                     # last rows below the split: no edge
    u = np.repeat(np.arange(S), deg)
    it = S + rng.integers(0, I, u.size)
    if kind == "isolated_edges":
        it = np.where(it < S + 5, it + 5, it)            # first rows above it: no edge
    r = np.concatenate([u, it])
    c = np.concatenate([it, u])
    if kind == "not_bipartite":
        r = np.concatenate([r, [0, 1, S + 7, S + 9]])
        c = np.concatenate([c, [1, 0, S + 9, S + 7]])
    loops = np.arange(0, N, 3)                            # self-loops on a third of the rows
    r = np.concatenate([r, loops])
    c = np.concatenate([c, loops])
    v = rng.uniform(0.01, 1.0, r.size)
    g, plan = _raw_graph(N, r, c, v)
    try:
        x = torch.randn(N, d, generator=torch.Generator().manual_seed(8)).to(DEV)
        y1, y2, ya = torch.empty_like(x), torch.empty_like(x), torch.zeros_like(x)
        assert _spmm_raw(g, plan, x, y1) == 0
        assert _spmm_raw(g, plan, x, y2) == 0
        cx = _lib.ctx(x.device)
        assert _lib.fn("hnm_spmm_csr_range_f32")(
            cx, plan, N, _lib.ptr(g.rowptr), _lib.ptr(g.col), _lib.ptr(g.val), _lib.ptr(x), d,
            _lib.ptr(ya), 0.0, None, None, 0.0, 0, S, 0) == 0
        torch.cuda.synchronize()
        assert torch.equal(y1, y2)
        assert torch.equal(ya[:S], y1[:S]) and not ya[S:].any()
        ref, mag = _dense_ref(g, x)
        err = np.abs(y1.double().cpu().numpy() - ref)
        assert (err <= 1e-5 * mag + 1e-30).all(), float((err / (mag + 1e-30)).max())
        short_small = np.flatnonzero(deg < 129)[:6]
        rows = torch.tensor(list(short_small) + [1, 2, S - 1, S - 5, S, S + 4, S + 11, N - 1],
                            dtype=torch.int64, device=DEV)
        out = torch.empty(rows.numel(), d, device=DEV)
        assert _combine_raw(g, plan, rows, [x], [0.0, 1.0], out) == 0
        torch.cuda.synchronize()
        assert torch.equal(out, y1[rows])
    finally:
        _lib.fn("hnm_spmm_plan_destroy")(plan)


@pytest.mark.parametrize("d", [64, 128])
def test_restricted_plan_rows_bitwise(d):
    """hnm_spmm_plan_restrict (item-sharded propagation): a plan keeping the user
    rows plus one item shard computes exactly those rows, bitwise equal to the whole-graph plan
    (same pieces, same order -- split item rows of > cap entries and the tail items the bipartite
    routing moved into the walk included), and writes nothing else; shards covering the items
    together reproduce the whole layer; an empty range, ragged shards, the acc epilogue from
    acc_row0 and rows_combine on the restricted plan agree too; bad ranges are refused."""
    from hnm_recommendation_amd import sharding as S
    U, I = 150_000, 5_000
    edges = syn.bipartite_edge_index(U, I, 900_000, seed=7, zipf=1.1)
    m, g = _graph(U, I, edges, d)
    N = U + I
    L = np.diff(g.rowptr.cpu().numpy())
    assert L[U:].max() > 2 * 512 and (L[U:] <= 128).any()     # split rows and short items
    x = torch.randn(N, d, generator=torch.Generator().manual_seed(4)).to(DEV)
    y = torch.empty_like(x)
    acc_full = torch.empty(I, d, device=DEV)
    g.spmm(x, y, 0.7, acc_full, acc_in=False, beta=0.25, acc_row0=U)
    G = 3
    cover = torch.full_like(x, float("nan"))
    for r in range(G):
        lo, hi = S.shard_range(I, r, G)
        plan = g.restricted(((0, U), (U + lo, U + hi)), d)
        yr = torch.full_like(x, float("nan"))
        acc = torch.empty(hi - lo, d, device=DEV)
        g.spmm(x, yr, 0.7, acc, acc_in=False, beta=0.25, acc_row0=U + lo, plan=plan)
        torch.cuda.synchronize()
        assert torch.equal(yr[:U], y[:U]) and torch.equal(yr[U + lo:U + hi], y[U + lo:U + hi])
        assert torch.isnan(yr[U:U + lo]).all() and torch.isnan(yr[U + hi:]).all()
        assert torch.equal(acc, acc_full[lo:hi])
        # the last layer's form: the shard's item rows only
        yl = torch.full_like(x, float("nan"))
        g.spmm(x, yl, 0.0, None, rows=(U + lo, U + hi), plan=plan)
        torch.cuda.synchronize()
        assert torch.equal(yl[U + lo:U + hi], y[U + lo:U + hi]) and torch.isnan(yl[:U + lo]).all()
        cover[U + lo:U + hi] = yr[U + lo:U + hi]
        rows = torch.tensor([0, U - 1, U + lo, U + hi - 1, N - 1], dtype=torch.int64, device=DEV)
        out = torch.empty(rows.numel(), d, device=DEV)
        assert _combine_raw(g, plan, rows, [x], [0.0, 1.0], out) == 0
        torch.cuda.synchronize()
        assert torch.equal(out, y[rows])
    assert torch.equal(cover[U:], y[U:])
    # an item-only plan with an empty range beside it
    plan = g.restricted(((U, U), (U + 10, U + 4000)), d)
    ye = torch.full_like(x, float("nan"))
    g.spmm(x, ye, 0.0, None, plan=plan)
    torch.cuda.synchronize()
    assert torch.equal(ye[U + 10:U + 4000], y[U + 10:U + 4000])
    assert torch.isnan(ye[:U + 10]).all() and torch.isnan(ye[U + 4000:]).all()
    c = _lib.ctx(x.device)
    p = C.c_void_p()
    for bad in ((5, 3), (0, N + 1), (10, 20, 15, 30)):
        flat = (C.c_int64 * len(bad))(*bad)
        assert _lib.fn("hnm_spmm_plan_restrict")(c, g.plan, flat, len(bad) // 2, C.byref(p)) == _lib.HNM_EINVAL
    flat = (C.c_int64 * 2)(0, U)
    assert _lib.fn("hnm_spmm_plan_restrict")(c, plan, flat, 1, C.byref(p)) == _lib.HNM_EINVAL


def test_restricted_legacy_plan():
    """A restricted plan without the walks (> 2^22 nodes): the kept sub-ranges by the row-class
    kernels, bitwise the whole-graph rows, other rows untouched."""
    U, I, d = (1 << 22) + 3000, 4000, 16
    base = syn.bipartite_edge_index(U, I, 2_000_000, seed=9)
    hub = np.stack([np.arange(0, U, 997), np.zeros(len(range(0, U, 997)), np.int64) + U])
    edges = np.concatenate([base, hub, hub[::-1]], axis=1)
    m, g = _graph(U, I, edges, d)
    x = torch.randn(U + I, d, generator=torch.Generator().manual_seed(3)).to(DEV)
    y = torch.empty_like(x)
    g.spmm(x, y, 0.0, None)
    plan = g.restricted(((1000, 50_000), (U, U + 1500)), d)
    yr = torch.full_like(x, float("nan"))
    g.spmm(x, yr, 0.0, None, plan=plan)
    torch.cuda.synchronize()
    assert torch.equal(yr[1000:50_000], y[1000:50_000]) and torch.equal(yr[U:U + 1500], y[U:U + 1500])
    assert torch.isnan(yr[:1000]).all() and torch.isnan(yr[50_000:U]).all() and torch.isnan(yr[U + 1500:]).all()


def test_item_sharded_propagation_full_shape():
    """LightGCN.propagate_for_shard at the full H&M shape (configs[2]/[4] graph, d = 64): each of
    8 emulated ranks runs the product method with its restricted plan, and its exchange hands it
    the other shards' item rows from a whole-graph reference run (what the all_gather delivers)
    after checking the rows the rank computed itself -- every user row and its item shard of
    layers 1 and 2 -- bit for bit.  The rank's final item rows and the batch users' final rows
    equal propagate_for's (= forward()'s) bitwise."""
    from hnm_recommendation_amd import sharding as S
    U, I, d, G = syn.HM_USERS, syn.HM_ITEMS, 64, 8
    edges = syn.bipartite_edge_index(U, I, syn.HM_INTERACTIONS, seed=2)
    m = LightGCN(U, I, embedding_dim=d, num_layers=3)
    m.set_graph(torch.from_numpy(edges))
    del edges
    sd = syn.lightgcn_state_dict(U, I, d, seed=0)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m = m.to(DEV).eval()
    g = m._device_graph()
    E0 = m.embeddings.weight.detach()
    ref = [E0]
    for _ in range(2):
        y = torch.empty_like(E0)
        g.spmm(ref[-1], y, 0.0, None)
        ref.append(y)
    users = torch.from_numpy(syn.user_batch(U, 4096, seed=5)).to(DEV)
    fb_ref, fi_ref = m.propagate_for(users)
    for r in (0, 3, G - 1):
        lo, hi = S.shard_range(I, r, G)
        seen = []

        def exchange(Y, lo=lo, hi=hi, seen=seen):
            want = ref[len(seen) + 1]
            seen.append(torch.equal(Y[:U], want[:U]) and torch.equal(Y[U + lo:U + hi], want[U + lo:U + hi]))
            Y[U:U + lo] = want[U:U + lo]
            Y[U + hi:] = want[U + hi:]
        fb, fi = m.propagate_for_shard(users, lo, hi, exchange)
        torch.cuda.synchronize()
        assert seen == [True, True], (r, seen)
        assert torch.equal(fi, fi_ref[lo:hi]), r
        assert torch.equal(fb, fb_ref), r
