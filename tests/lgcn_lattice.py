"""LightGCN on a power-of-four lattice: graph builders and float64 oracles (no GPU needed).

csr_degree_kernel computes dinv = 1.0f / sqrtf(deg) with deg the row's weight sum, self-loop
included.  Where every deg is a power of four, dinv is a power of two, every normalized value
val = (dinv[r] * w) * dinv[c] is a power of two (unweighted edges) or a small integer times one,
and with small-integer embeddings and layer weights 1 / (L + 1) that are exact (L = 1, L = 3)
every intermediate of the propagation is a dyadic rational with few significant bits: the fp32
result is ONE number in any summation order, and a float64 numpy evaluation is a BITWISE oracle
of every SpMM route.  `propagate_oracle` / `scores_oracle` / `spmm_oracle` assert the magnitudes
that make this hold (2^s * sum |terms| < 2^24 with 2^-s the step of the terms) instead of
assuming them; a case that fails them is a wrong case.

`replicate` makes R disjoint copies of a graph with identical embedding rows: every item then has
R - 1 exact twins for every user, so exact ties sit at every position k that R does not divide,
and the library's total order (score descending, item id ascending) decides every row.

tests/test_cpu_lgcn_lattice.py checks these properties on the CPU; tests/test_gpu_lattice_lightgcn.py
compares the library with the oracles on ids and on values as uint32 bits.
"""
from __future__ import annotations

import functools

import numpy as np

import lattice as L

POW4 = 4 ** np.arange(0, 12, dtype=np.int64)
# row classes of hnm_recommendation_amd/csrc/graph_internal.h (entries a row, self-loop included)
SPMM_SHORT = 128
HEAVY = 2048
WALK_LIMIT = 1 << 22  # more nodes than this: the plan without the walks (legacy, mode 1)
WEIGHTED_DEG = 1024   # weighted degree of a `weighted_row`


# ---------------------------------------------------------------------------- graphs
class Graph:
    """U users, I items (node id U + item), directed edge list [2, E] in both directions in an
    order sorted neither by row nor by column, optional float32 weights."""

    def __init__(self, U, I, edge_index, edge_weight=None):
        self.U, self.I, self.N = int(U), int(I), int(U) + int(I)
        self.edge_index = np.ascontiguousarray(edge_index, dtype=np.int64)
        self.edge_weight = None if edge_weight is None else \
            np.ascontiguousarray(edge_weight, dtype=np.float32)
        r, c = self.edge_index
        assert r.min() >= 0 and r.max() < self.N and c.min() >= 0 and c.max() < self.N
        assert (np.diff(r) < 0).any() and (np.diff(c) < 0).any(), "edge list must not be sorted"

    @functools.cached_property
    def csr(self):
        return csr_oracle(self.edge_index, self.edge_weight, self.N)


def degree_graph(udeg, ideg, seed):
    """Bipartite graph with the given edge counts per user / item (0: isolated), from two
    shuffled stub lists paired position by position: duplicate pairs happen and are kept.
    Every count + 1 (the degree with the self-loop) must be a power of four."""
    udeg, ideg = np.asarray(udeg, np.int64), np.asarray(ideg, np.int64)
    assert udeg.sum() == ideg.sum(), (udeg.sum(), ideg.sum())
    assert np.isin(udeg + 1, POW4).all() and np.isin(ideg + 1, POW4).all()
    U, I = len(udeg), len(ideg)
    rng = L._rng(seed, U, I)
    us = rng.permutation(np.repeat(np.arange(U), udeg))
    it = rng.permutation(np.repeat(np.arange(I), ideg)) + U
    r, c = np.concatenate([us, it]), np.concatenate([it, us])
    p = rng.permutation(len(r))
    return Graph(U, I, np.stack([r[p], c[p]]))


def replicate(graph, E0, R, seed=0):
    """R disjoint copies of `graph` with identical embedding rows: user u of copy a is
    u + a * U0, item j of copy a is j + a * I0.  The edge list is re-shuffled over the whole
    graph, so twins meet their entries in different orders.  Returns (Graph, E0 [R * N0, d])."""
    U0, I0 = graph.U, graph.I
    ei, w = graph.edge_index, graph.edge_weight
    node = lambda n, a: np.where(n < U0, n + a * U0, R * U0 + (n - U0) + a * I0)
    big = np.concatenate([node(ei, a) for a in range(R)], axis=1)
    p = L._rng(seed, R, big.shape[1]).permutation(big.shape[1])
    E = np.concatenate([np.tile(E0[:U0], (R, 1)), np.tile(E0[U0:], (R, 1))])
    return (Graph(R * U0, R * I0, big[:, p], None if w is None else np.tile(w, R)[p]),
            np.ascontiguousarray(E, dtype=np.float32))


def weighted_row(n):
    """Weights of the n - 1 edges of a row with exactly n entries (self-loop included) whose
    weighted degree is 1,024: each partner is linked to this row alone with weight 3 or 15, so
    its own degree is 4 or 16.  a threes and b fifteens with a + b = n - 1 and 3 a + 15 b = 1,023
    need 12 b = 1,026 - 3 n: n = 2 (mod 4), because 4^m - 1 = 3 (mod 12)."""
    assert n % 4 == 2 and 3 * (n - 1) <= WEIGHTED_DEG - 1 <= 15 * (n - 1), n
    b = (WEIGHTED_DEG + 2 - 3 * n) // 12
    a = n - 1 - b
    assert a >= 0 and b >= 0 and 3 * a + 15 * b == WEIGHTED_DEG - 1
    return np.concatenate([np.full(a, 3.0, np.float32), np.full(b, 15.0, np.float32)])


def ternary(N, d, density, seed):
    """[N, d] float32 entries in {-1, +0, 1} (no -0)."""
    return L._ternary(L._rng(seed, N, d), (N, d), density) + np.float32(0)


def small_ints(N, d, seed):
    """[N, d] float32 integers in [-4, 4]: a raw layer input."""
    return L._rng(seed, N, d).integers(-4, 5, (N, d)).astype(np.float32)


# ---------------------------------------------------------------------------- oracles
class Csr:
    """D^-1/2 (A + I) D^-1/2: rowptr int64 [N + 1], col int32, val float32 (val64 before the one
    cast), entries of a row in edge-list order with the self-loop last."""

    def __init__(self, N, rowptr, col, val64, deg):
        self.N, self.rowptr, self.col, self.val64, self.deg = N, rowptr, col, val64, deg
        self.val = val64.astype(np.float32)
        self.len = np.diff(rowptr)

    def matmul(self, X, absolute=False):
        """A X in float64 (|A| X with `absolute`); every row has its self-loop, so reduceat over
        rowptr[:-1] sees no empty row."""
        v = np.abs(self.val64) if absolute else self.val64
        X = np.asarray(X, np.float64)
        out = np.empty((self.N, X.shape[1]))
        for c0 in range(0, X.shape[1], 64):
            out[:, c0:c0 + 64] = np.add.reduceat(v[:, None] * X[self.col, c0:c0 + 64],
                                                 self.rowptr[:-1], axis=0)
        return out


def csr_oracle(edge_index, edge_weight, N, lattice=True):
    """The contract of hnm_csr_build_norm: a stable sort of the edges by row, the self-loop
    appended last in each row, duplicates kept; deg = the row's weight sum + 1, val =
    deg[r]^-1/2 * w * deg[c]^-1/2 in float64, cast once.  lattice: assert that every degree is a
    power of four and that the cast is exact."""
    r, c = np.asarray(edge_index, np.int64)
    E = len(r)
    w = np.ones(E) if edge_weight is None else np.asarray(edge_weight, np.float64)
    order = np.argsort(r, kind="stable")
    cnt = np.bincount(r, minlength=N)
    rowptr = np.zeros(N + 1, np.int64)
    np.cumsum(cnt + 1, out=rowptr[1:])
    col = np.empty(E + N, np.int32)
    wt = np.empty(E + N)
    dst = np.arange(E) + r[order]          # rows below r each hold one self-loop entry
    col[dst], wt[dst] = c[order], w[order]
    loop = rowptr[1:] - 1
    col[loop], wt[loop] = np.arange(N), 1.0
    deg = np.bincount(r, weights=w, minlength=N) + 1.0
    dinv = 1.0 / np.sqrt(deg)
    rows = np.repeat(np.arange(N), cnt + 1)
    val64 = dinv[rows] * wt * dinv[col]
    out = Csr(N, rowptr, col, val64, deg)
    if lattice:
        assert np.isin(deg, POW4.astype(np.float64)).all(), "a degree is no power of four"
        assert np.array_equal(out.val.astype(np.float64), val64)
    return out


def step_bits(x):
    """The smallest s >= 0 with x * 2^s integral everywhere."""
    x = np.asarray(x, np.float64)
    for s in range(0, 64):
        y = np.ldexp(x, s)
        if np.array_equal(y, np.round(y)):
            return s
    raise AssertionError("not a dyadic rational with a step above 2^-64")


def _exact(what, s, mag):
    """Assert 2^s * sum |terms| < 2^24 (terms: multiples of 2^-s, `mag`: the sums of their
    magnitudes): every partial sum in any order is then exact in fp32.  Returns
    (s, log2(2^s * max mag))."""
    m = float(np.max(mag))
    assert 2.0 ** s * m < L.EXACT, (what, s, m)
    return s, s + float(np.log2(max(m, 2.0 ** -s)))


def exact_f32(x):
    """float64 -> float32 with an exact zero as +0 (as every fp32 chain that starts at +0 gives
    it), asserting that the cast loses nothing."""
    out = (np.asarray(x, np.float64) + 0.0).astype(np.float32)
    assert np.array_equal(out.astype(np.float64), x)
    return out


def spmm_oracle(csr, X, what="layer"):
    """(A X as float32, (step bits, sum-of-|terms| bits)) with the lattice assertion."""
    X = np.asarray(X, np.float64)
    info = _exact(what, step_bits(csr.val64) + step_bits(X), csr.matmul(np.abs(X), absolute=True))
    return exact_f32(csr.matmul(X)), info


def propagate_oracle(csr, E0, num_layers, alphas=None):
    """LightGCN.forward in float64: E_{l+1} = A E_l, F = sum_l alpha_l E_l (default alpha_l =
    1 / (L + 1)).  Returns (layers E_0 .. E_L as float32, F float32, info) with info[name] =
    (step bits, bits of 2^s * sum |terms|) for every layer and for F; asserts the lattice."""
    alphas = [1.0 / (num_layers + 1)] * (num_layers + 1) if alphas is None else list(alphas)
    assert all(float(np.float32(a)) == a for a in alphas), "a layer weight is not exact in fp32"
    X, M, info = [np.asarray(E0, np.float64)], [np.abs(np.asarray(E0, np.float64))], {}
    sv = step_bits(csr.val64)
    for l in range(num_layers):
        mag = csr.matmul(M[-1], absolute=True)
        info[f"E{l + 1}"] = _exact(f"E{l + 1}", sv + step_bits(X[-1]), mag)
        X.append(csr.matmul(X[-1]))
        M.append(mag)
    F = sum(a * x for a, x in zip(alphas, X))
    s = max(step_bits(a * x) for a, x in zip(alphas, X))
    info["F"] = _exact("F", s, sum(a * m for a, m in zip(alphas, M)))
    return [exact_f32(x) for x in X], exact_f32(F), info


def scores_oracle(FU, FI, users):
    """(F_U[users] @ F_I^T as float32 [B, I], (step bits, bits)) with the lattice assertion."""
    u, it = np.asarray(FU, np.float64)[users], np.asarray(FI, np.float64)
    info = _exact("scores", step_bits(u) + step_bits(it), np.abs(u) @ np.abs(it).T)
    return exact_f32(u @ it.T), info


def combine_oracle(csr, rows, layers, alphas):
    """hnm_spmm_rows_combine_f32 (hnm.h): sum_{l < L} alpha_l E_l[r] + alpha_L (A E_{L-1})[r]
    for the listed rows, the layer inputs being ANY arrays (no propagation assumed)."""
    Ls = [np.asarray(x, np.float64) for x in layers]
    last = csr.matmul(Ls[-1])
    mag = csr.matmul(np.abs(Ls[-1]), absolute=True)
    out = sum(a * x for a, x in zip(alphas[:-1], Ls)) + alphas[-1] * last
    tot = sum(a * np.abs(x) for a, x in zip(alphas[:-1], Ls)) + alphas[-1] * mag
    _exact("combine", step_bits(np.asarray(alphas)) + step_bits(csr.val64) +
           max(step_bits(x) for x in Ls), tot)
    return exact_f32(out)[np.asarray(rows)]


# ---------------------------------------------------------------------------- cases
R = 5                       # copies of the replicated cases: tie groups are multiples of 5
FUSED_KS = (1, 12, 63, 64)  # hnm_dot_topk_f32
DENSE_K = 96                # > 64: dense scores + hnm_topk_rows_f32
BATCHES = (1, 70, 1025)
FILTER_KINDS = ("tie_group", "dups_oob", "all")  # lattice.masks kinds (ids >= I dropped)


@functools.lru_cache(maxsize=None)
def regular_base():
    """2,048 + 2,048 nodes, 3 edges each (deg + 1 = 4), 8 users and 8 items isolated."""
    deg = np.full(2048, 3)
    deg[[0, 5, 77, 1000, 1001, 1500, 2046, 2047]] = 0
    return degree_graph(deg, deg[::-1].copy(), seed=41)


@functools.lru_cache(maxsize=None)
def mixed_base():
    """2,048 users with 3 / 15 edges, 1,976 items with 3 / 15 / 63 / 255."""
    udeg = np.full(2048, 3)
    udeg[::16] = 15                                    # 128 users
    ideg = np.full(1976, 3)
    ideg[[3, 1200]] = 255
    ideg[100:800:100] = 63                             # 7 items ...
    ideg[1900] = 63                                    # ... and an eighth
    ideg[1000:1064] = 15
    return degree_graph(udeg, ideg, seed=42)


class ModelCase:
    """One replicated LightGCN model: graph, E0, oracle F, users, scores, top-K references."""

    def __init__(self, name, base, num_layers, d, density):
        self.name, self.base, self.L, self.d, self.density = name, base, num_layers, d, density
        self.id = f"{name}-d{d}"

    @functools.cached_property
    def _built(self):
        b = self.base()
        return replicate(b, ternary(b.N, self.d, self.density, seed=7), R, seed=3)

    @property
    def graph(self):
        return self._built[0]

    @property
    def E0(self):
        return self._built[1]

    @functools.cached_property
    def prop(self):
        return propagate_oracle(self.graph.csr, self.E0, self.L)

    @property
    def F(self):
        return self.prop[1]

    @functools.cached_property
    def users(self):
        """1,025 distinct users of every copy, unsorted; a batch of B rows is users[:B]."""
        return L._rng(9, self.graph.U).permutation(self.graph.U)[:BATCHES[-1]].astype(np.int64)

    @functools.cached_property
    def _scores(self):
        U = self.graph.U
        return scores_oracle(self.F[:U], self.F[U:], self.users)

    @property
    def scores(self):
        return self._scores[0]

    @functools.lru_cache(maxsize=None)
    def mask(self, B, kind, k):
        return L.masks(B, self.graph.I, kind, self.scores[:B], k, seed=5)

    @functools.lru_cache(maxsize=None)
    def ref(self, B, k, kind="none"):
        """(values, ids) of lattice.ref_topk: np.argsort(-scores, kind="stable") row by row."""
        if kind == "none" and k < DENSE_K:  # a prefix of the longest unfiltered list
            rv, ri = self.ref(B, DENSE_K)
            return rv[:, :k], ri[:, :k]
        return L.ref_topk(self.scores[:B], k, self.mask(B, kind, k))

    def filter_items(self, B, kind, k):
        """The `filter_items` dict of recommend() for the batch's mask (None for "none")."""
        ptr, idx = self.mask(B, kind, k)
        if ptr is None:
            return None
        out = {}
        for b in range(B):
            m = idx[ptr[b]:ptr[b + 1]]
            out[int(self.users[b])] = m[m < self.graph.I].tolist()
        return out


REGULAR3 = {d: ModelCase("regular3", regular_base, 3, d, 0.1 if d >= 48 else 0.5)
            for d in (4, 64, 128, 256)}
MIXED_L1 = ModelCase("mixed_L1", mixed_base, 1, 64, 0.1)
MODEL_CASES = [*REGULAR3.values(), MIXED_L1]
SCORE_CASES = [REGULAR3[64], REGULAR3[128], MIXED_L1]
UNSUPPORTED_D = 48  # no SpMM kernel of this width: the library refuses it (hnm.h)

# heavy_L1: 8,192 users with 3 edges; item 7 with 4,095 (heavy: > HEAVY entries), items 100 and
# 500 with 1,023 (long, cut into two walk pieces of 512), items 200 .. 263 with 255 (long, one
# piece), the other 705 of the first 772 items with 3.  Users 8,192 / 8,193 and items 772 ..
# 1,025 are isolated in the unweighted variant; in the weighted one (every other edge weight 1)
# they are the two `weighted_row`s of 126 and 130 entries with their partners.
HEAVY_USERS, HEAVY_ITEMS = 8192, 772
HEAVY_ITEM, LONG2_ITEMS, LONG1_ITEMS = 7, (100, 500), tuple(range(200, 264))
HUB_ROWS = (126, 130)


@functools.lru_cache(maxsize=None)
def heavy_graph(weighted):
    ideg = np.full(HEAVY_ITEMS, 3)
    ideg[HEAVY_ITEM] = 4095
    ideg[list(LONG2_ITEMS)] = 1023
    ideg[list(LONG1_ITEMS)] = 255
    extra = sum(n - 1 for n in HUB_ROWS)
    g = degree_graph(np.concatenate([np.full(HEAVY_USERS, 3), np.zeros(len(HUB_ROWS), np.int64)]),
                     np.concatenate([ideg, np.zeros(extra, np.int64)]), seed=43)
    if not weighted:
        return g
    r, c, w = [g.edge_index[0]], [g.edge_index[1]], [np.ones(g.edge_index.shape[1], np.float32)]
    first = g.U + HEAVY_ITEMS
    for j, n in enumerate(HUB_ROWS):
        hub = np.full(n - 1, HEAVY_USERS + j)
        part = first + np.arange(n - 1)
        first += n - 1
        wr = L._rng(44, n).permutation(weighted_row(n))
        r += [hub, part]
        c += [part, hub]
        w += [wr, wr]
    r, c, w = np.concatenate(r), np.concatenate(c), np.concatenate(w)
    p = L._rng(45, len(r)).permutation(len(r))
    return Graph(g.U, g.I, np.stack([r[p], c[p]]), w[p])


def heavy_rows(g):
    """Row ids of every class of heavy_L1, by name."""
    U = g.U
    return {"heavy": U + HEAVY_ITEM, "long2": [U + i for i in LONG2_ITEMS],
            "long1": [U + LONG1_ITEMS[0], U + LONG1_ITEMS[-1]],
            "hubs": [HEAVY_USERS + j for j in range(len(HUB_ROWS))],
            "short": [0, U + 1], "partner": U + HEAVY_ITEMS, "last": g.N - 1}


@functools.lru_cache(maxsize=None)
def legacy_graph():
    """heavy_L1 (weighted) with isolated users inserted after its own until N > 2^22: the plan
    without the walks.  Item ids move up by the number of inserted users."""
    g = heavy_graph(True)
    U = WALK_LIMIT + 5
    shift = U - g.U
    ei = np.where(g.edge_index < g.U, g.edge_index, g.edge_index + shift)
    return Graph(U, g.I, ei, g.edge_weight)


LAYER_DS = (4, 64, 128, 256)
HEAVY_F_DS = (64, 128)
LEGACY_D = 4
COMBINE_ALPHAS = (0.25, 0.5, 0.125, 0.375)


@functools.lru_cache(maxsize=None)
def heavy_prop(weighted, d):
    """(E0, layers, F, info) of heavy_L1 at L = 1: used for F only (the table's step is 2^-13,
    the heavy item's self-loop, so a score's terms can be as fine as 2^-26)."""
    g = heavy_graph(weighted)
    E0 = ternary(g.N, d, 0.1, seed=8)
    return (E0, *propagate_oracle(g.csr, E0, 1))


@functools.lru_cache(maxsize=None)
def layer_case(which, d):
    """(graph, X, Y = A X as float32, info): one raw layer on integers in [-4, 4]."""
    g = legacy_graph() if which == "legacy" else heavy_graph(which == "weighted")
    X = small_ints(g.N, d, seed=12)
    Y, info = spmm_oracle(g.csr, X)
    return g, X, Y, info


@functools.lru_cache(maxsize=None)
def combine_layers(which, d):
    """Three INDEPENDENT integer layer inputs (not a propagation: a layer mix-up shows)."""
    g = legacy_graph() if which == "legacy" else heavy_graph(which == "weighted")
    return tuple(small_ints(g.N, d, seed=20 + l) for l in range(len(COMBINE_ALPHAS) - 1))
