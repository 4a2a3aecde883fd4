"""The LightGCN SpMM's summation order, pinned across builds.

The other SpMM tests compare the paths with each other (layer kernels == rows_combine, restricted
plan == base plan) and with float64; a change that moved the shared order in all of them at once
would pass those.  This module hashes the raw output bytes (SHA-256) of every SpMM path on a small
graph whose inputs come from integer arithmetic alone and compares them with the digests in
tests/golden/spmm_order_digests.json.

The digests are recorded by running this module as a script against a built library,

    python tests/test_gpu_spmm_order.py --record

and were recorded from the build of the commit before the SpMM source was split by stage.  A change
that alters the order on purpose re-records them (and says so); any other change must leave them
as they are.
"""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from hnm_recommendation_amd import _lib
from hnm_recommendation_amd import synthetic as syn
from hnm_recommendation_amd.models.lightgcn import LightGCN, NormalizedGraph

pytestmark = pytest.mark.gpu
DEV = "cuda"
DIGESTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spmm_order_digests.json")
DIMS = (4, 64, 128, 256)

U, I = 3000, 40
N = U + I
ISOLATED = (7, 1500, 2999)      # users with no edge: their row is the self-loop alone
# item -> number of users.  Item 0: every user with an edge (2,997 entries + the self-loop: over
# 2 x 512, so the walk cuts it into 6 pieces, and over HEAVY = 2,048: segments without a walk
# plan); item 1: 1,100 users (3 pieces); items 2-9: 200 (long rows, one piece); items 10-39: 5
# (short item rows, which the bipartite routing moves into the long walk).
COUNTS = [U - len(ISOLATED), 1100] + [200] * 8 + [5] * 30
# multipliers coprime to 3,000, one per item: users (k * mult + 37 * item) % 3000, k = 0, 1, ...
MULTS = [7, 2731, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 49, 53, 59, 61, 67, 71, 73, 77, 79,
         83, 89, 91, 97, 101, 103, 107, 109, 113, 119, 121, 127, 131, 133, 137, 139, 143, 149]


def _edges():
    """(edge_index [2, E], edge_weight [E]): both directions, items in descending order so that
    no row's entries arrive sorted by column; weights are multiples of 1/4."""
    us, its = [], []
    for it in reversed(range(I)):
        k, got = 0, 0
        while got < COUNTS[it]:
            u = (k * MULTS[it] + 37 * it) % U
            k += 1
            if u in ISOLATED:
                continue
            us.append(u)
            its.append(U + it)
            got += 1
    u = np.asarray(us, np.int64)
    i = np.asarray(its, np.int64)
    w = (1 + (u * 3 + i * 5) % 7).astype(np.float32) * np.float32(0.25)
    return np.stack([np.concatenate([u, i]), np.concatenate([i, u])]), np.concatenate([w, w])


def _table(n, d, a, b, c):
    """[n, d] fp32 from integers: ((row * a + col * b + c) % 257 - 128) / 64 -- exact in fp32."""
    r = np.arange(n, dtype=np.int64)[:, None]
    k = np.arange(d, dtype=np.int64)[None, :]
    return torch.from_numpy((((r * a + k * b + c) % 257 - 128) / 64.0).astype(np.float32)).to(DEV)


def _sha(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def _range(g, plan, x, y, alpha, acc_in, acc_out, beta, r0, r1, acc_row0):
    st = _lib.fn("hnm_spmm_csr_range_f32")(
        _lib.ctx(x.device), plan, g.num_nodes, _lib.ptr(g.rowptr), _lib.ptr(g.col), _lib.ptr(g.val),
        _lib.ptr(x), x.shape[1], _lib.ptr(y), alpha, _lib.ptr(acc_in), _lib.ptr(acc_out), beta, r0, r1,
        acc_row0)
    _lib.check(st, "hnm_spmm_csr_range_f32")


def _whole(g, plan, x, y, alpha, acc_in, acc_out):
    st = _lib.fn("hnm_spmm_csr_f32")(
        _lib.ctx(x.device), plan, g.num_nodes, _lib.ptr(g.rowptr), _lib.ptr(g.col), _lib.ptr(g.val),
        _lib.ptr(x), x.shape[1], _lib.ptr(y), alpha, _lib.ptr(acc_in), _lib.ptr(acc_out))
    _lib.check(st, "hnm_spmm_csr_f32")


def _combine(g, plan, rows, layers, alphas):
    L = len(layers)
    out = torch.empty(rows.numel(), layers[0].shape[1], device=DEV)
    ptrs = (C.c_void_p * L)(*[t.data_ptr() for t in layers])
    al = (C.c_float * (L + 1))(*alphas)
    st = _lib.fn("hnm_spmm_rows_combine_f32")(
        _lib.ctx(rows.device), plan, g.num_nodes, _lib.ptr(g.rowptr), _lib.ptr(g.col), _lib.ptr(g.val),
        _lib.ptr(rows), rows.numel(), layers[0].shape[1], ptrs, al, L, _lib.ptr(out))
    _lib.check(st, "hnm_spmm_rows_combine_f32")
    return out


_GRAPH = []


def _graph():
    if not _GRAPH:
        ei, ew = _edges()
        g = NormalizedGraph(torch.from_numpy(ei), torch.from_numpy(ew), N, torch.device(DEV, 0))
        L = np.diff(g.rowptr.cpu().numpy())
        assert L[U] == U - len(ISOLATED) + 1 and L[U + 1] == 1101 and (L[U + 2:U + 10] == 201).all()
        assert (L[U + 10:] == 6).all() and all(L[u] == 1 for u in ISOLATED) and L[:U].max() <= 128
        _GRAPH.append(g)
    return _GRAPH[0]


def small_graph_digests(d):
    """Digest of every output of every SpMM path at width d on the integer graph."""
    g = _graph()
    x = _table(N, d, 131, 31, 7)
    acc0 = _table(I, d, 17, 29, 3)
    out = {}

    def layer(tag, plan):
        # acc_in == NULL with beta != 0 (the alpha_0 E_0 term folded in), then acc_in given; the
        # accumulators start at the first item row
        y, acc = torch.zeros_like(x), torch.zeros(I, d, device=DEV)
        _range(g, plan, x, y, 0.75, None, acc, 0.375, 0, N, U)
        out[tag + "/beta/Y"], out[tag + "/beta/acc"] = _sha(y), _sha(acc)
        y, acc = torch.zeros_like(x), torch.zeros(I, d, device=DEV)
        _range(g, plan, x, y, 0.75, acc0, acc, 0.0, 0, N, U)
        out[tag + "/acc_in/Y"], out[tag + "/acc_in/acc"] = _sha(y), _sha(acc)
        # the whole-graph entry point (acc_row0 = 0: one accumulator row per node)
        y, acc = torch.zeros_like(x), torch.zeros_like(x)
        _whole(g, plan, x, y, 0.5, x, acc)
        out[tag + "/whole/Y"], out[tag + "/whole/acc"] = _sha(y), _sha(acc)

    g.prepare(d)
    layer("plan", g.plan)
    layer("noplan", None)
    # a row range that cuts through the users and through the items (item 0 in, the tail out)
    y, acc = torch.zeros_like(x), torch.zeros(I, d, device=DEV)
    _range(g, g.plan, x, y, 0.75, None, acc, 0.375, 1500, U + 20, U)
    out["range/Y"], out["range/acc"] = _sha(y), _sha(acc)
    # a restricted plan: every user, items 5 .. 24
    rp = g.restricted(((0, U), (U + 5, U + 25)), d)
    y, acc = torch.zeros_like(x), torch.zeros(I, d, device=DEV)
    _range(g, rp, x, y, 0.75, None, acc, 0.375, 0, N, U)
    out["restricted/Y"], out["restricted/acc"] = _sha(y), _sha(acc)
    # rows_combine, L = 3: short user rows (an isolated one among them), the 6-piece and the
    # 3-piece item, long unsplit items, short items; one row twice
    rows = torch.tensor([0, 1, 7, 1499, U - 2, U, U + 1, U + 2, U + 9, U + 10, U + 39, 1],
                        dtype=torch.int64, device=DEV)
    layers = [x, _table(N, d, 89, 53, 11), _table(N, d, 57, 101, 5)]
    alphas = [0.25, 0.5, 0.125, 0.375]
    out["combine/plan"] = _sha(_combine(g, g.plan, rows, layers, alphas))
    out["combine/noplan"] = _sha(_combine(g, None, rows, layers, alphas))
    out["combine/restricted"] = _sha(_combine(g, rp, rows, layers, alphas))
    return out


def legacy_graph_digests():
    """The planned kernels of graphs above the walk limit (mixed, segment, finish) at d = 4, on
    the graph of test_gpu_spmm_plan.test_legacy_plan_above_walk_limit: N > 2^22, item 0 heavy."""
    Ul, Il, d = (1 << 22) + 3000, 4000, 4
    base = syn.bipartite_edge_index(Ul, Il, 2_000_000, seed=9)
    hub = np.stack([np.arange(0, Ul, 997), np.zeros(len(range(0, Ul, 997)), np.int64) + Ul])
    edges = np.concatenate([base, hub, hub[::-1]], axis=1)
    m = LightGCN(Ul, Il, d)
    m.set_graph(torch.from_numpy(edges))
    g = m.to(DEV)._device_graph()
    Lr = np.diff(g.rowptr.cpu().numpy())
    assert Lr.max() > 2048 and ((Lr > 128) & (Lr <= 2048)).any()
    x = _table(Ul + Il, d, 131, 31, 7)
    y, acc = torch.zeros_like(x), torch.zeros(Il, d, device=DEV)
    _range(g, g.plan, x, y, 0.75, None, acc, 0.375, 0, Ul + Il, Ul)
    out = {"legacy/Y": _sha(y), "legacy/acc": _sha(acc)}
    long_row = int(np.nonzero((Lr > 128) & (Lr <= 2048))[0][0])
    rows = torch.tensor([0, 997, Ul - 1, Ul, long_row, Ul + Il - 1], dtype=torch.int64, device=DEV)
    layers = [x, _table(Ul + Il, d, 89, 53, 11), _table(Ul + Il, d, 57, 101, 5)]
    out["legacy/combine"] = _sha(_combine(g, g.plan, rows, layers, [0.25, 0.5, 0.125, 0.375]))
    return out


def _recorded():
    with open(DIGESTS) as f:
        return json.load(f)


def _compare(key, got):
    want = _recorded()[key]
    assert sorted(got) == sorted(want)
    moved = [k for k in sorted(got) if got[k] != want[k]]
    assert not moved, f"{key}: output bytes differ from the recorded build in {moved}"


@pytest.mark.parametrize("d", DIMS)
def test_spmm_order_digests(d):
    """Every SpMM path at LPR = d / 4 (1, 16, 32, 64; both short-walk step sizes): walk plan, no
    plan, row range, restricted plan, rows_combine -- bytes equal to the recorded build's."""
    _compare(f"d{d}", small_graph_digests(d))


def test_spmm_order_digests_legacy_plan():
    """The mixed / segment / finish kernels and rows_combine's heavy-row order (N > 2^22)."""
    _compare("legacy_d4", legacy_graph_digests())


if __name__ == "__main__":
    if sys.argv[1:2] != ["--record"]:
        sys.exit("usage: test_gpu_spmm_order.py --record [output.json]")
    rec = {f"d{d}": small_graph_digests(d) for d in DIMS}
    rec["legacy_d4"] = legacy_graph_digests()
    path = sys.argv[2] if len(sys.argv) > 2 else DIGESTS
    with open(path, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {sum(len(v) for v in rec.values())} digests in {path}")
