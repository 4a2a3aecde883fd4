"""CPU: the LightGCN lattice cases (tests/lgcn_lattice.py) have the properties the GPU module
relies on -- the oracle's own exactness assertions hold, three independent evaluations agree bit
for bit, exact ties sit at every tested k, every row class is present -- and the deg^-1/2 fact
the lattice sidesteps."""
import numpy as np
import pytest
import torch

import lattice as L
import lgcn_lattice as G
from oracle import hnm_oracle as O
from oracle import torch_cpu as T


def _fmt(info):
    return ", ".join(f"{k}: step 2^-{s} sum|terms| {b:.1f} bits" for k, (s, b) in info.items())


@pytest.mark.parametrize("case", G.MODEL_CASES, ids=[c.id for c in G.MODEL_CASES])
def test_model_cases_are_on_the_lattice(case):
    layers, F, info = case.prop            # asserts 2^s * sum |terms| < 2^24 per layer and for F
    g = case.graph
    print(f"{case.id}: N {g.N} nnz {g.csr.rowptr[-1]} {_fmt(info)}")
    assert all(b < 24 for _, b in info.values())
    assert set(np.unique(g.csr.deg)) <= set(G.POW4.tolist())
    if case.name == "regular3":  # isolated users and items are part of the case
        assert (g.csr.deg[:g.U] == 1).any() and (g.csr.deg[g.U:] == 1).any()
    # twins: the oracle rows of the copies of a node are identical
    U0, I0 = g.U // G.R, g.I // G.R
    for a in range(1, G.R):
        assert np.array_equal(L.bits(F[:U0]), L.bits(F[a * U0:(a + 1) * U0]))
        assert np.array_equal(L.bits(F[g.U:g.U + I0]), L.bits(F[g.U + a * I0:g.U + (a + 1) * I0]))
    # ... although their rows list the entries in different orders
    rp, col = g.csr.rowptr, g.csr.col
    differ = sum(1 for j in range(I0) if not np.array_equal(
        col[rp[g.U + j]:rp[g.U + j + 1]] % U0, col[rp[g.U + I0 + j]:rp[g.U + I0 + j + 1]] % U0))
    assert differ > I0 // 4, differ


@pytest.mark.parametrize("case", G.SCORE_CASES, ids=[c.id for c in G.SCORE_CASES])
def test_scores_are_on_the_lattice_and_tie_everywhere(case):
    s, b = case._scores[1]
    fr = {k: L.tie_fraction(case.scores, k) for k in (*G.FUSED_KS, G.DENSE_K)}
    print(f"{case.id}: scores step 2^-{s} sum|terms| {b:.1f} bits, tie fractions {fr}, "
          f"distinct scores a row {np.mean([len(np.unique(r)) for r in case.scores[:70]]):.0f}")
    assert b < 24
    assert all(v == 1.0 for v in fr.values()), fr
    assert all(k % G.R for k in fr)
    # twin items score alike for every user
    I0 = case.graph.I // G.R
    assert np.array_equal(L.bits(case.scores[:, :I0]), L.bits(case.scores[:, I0:2 * I0]))
    # the rows are not degenerate: the best score is no tie of the whole catalogue
    assert np.mean(case.scores.max(1) > np.median(case.scores, 1)) > 0.5


@pytest.mark.parametrize("case", (G.REGULAR3[64], G.MIXED_L1), ids=("regular3-d64", "mixed_L1"))
def test_three_independent_evaluations_agree_bitwise(case):
    """The float64 oracle, oracle/hnm_oracle.py (fp32, np.add.at order, deg ** -0.5) and
    oracle/torch_cpu.py (fp32, coalesced CSR, torch.sparse.mm) give the same uint32 bits."""
    g, U = case.graph, case.graph.U
    z = np.float32(0)
    users = case.users[:70]
    graph = O.lightgcn_set_graph(g.edge_index, g.edge_weight, g.N)
    fu, fi = O.lightgcn_forward(case.E0, graph, U, case.L)
    assert np.array_equal(L.bits(np.concatenate([fu, fi]) + z), L.bits(case.F))
    assert np.array_equal(L.bits(O.lightgcn_predict_all_items(fu, fi, users) + z),
                          L.bits(case.scores[:70]))
    tg = T.lightgcn_graph(torch.from_numpy(g.edge_index), g.N)
    tu, ti = T.lightgcn_forward(torch.from_numpy(case.E0), tg, U, case.L)
    assert np.array_equal(L.bits(torch.cat([tu, ti]).numpy() + z), L.bits(case.F))
    ts = torch.matmul(tu[torch.from_numpy(users)], ti.t()).numpy()
    assert np.array_equal(L.bits(ts + z), L.bits(case.scores[:70]))
    # the CSR oracle holds the same numbers as the COO of hnm_oracle, entry for entry per row
    row, col, val = graph
    o = np.argsort(row[:g.edge_index.shape[1]], kind="stable")
    c = g.csr
    edges = np.ones(len(c.col), bool)
    edges[c.rowptr[1:] - 1] = False
    assert np.array_equal(c.col[edges], col[o]) and np.array_equal(L.bits(c.val[edges]), L.bits(val[o]))


@pytest.mark.parametrize("weighted", (False, True), ids=("unweighted", "weighted"))
def test_heavy_case_structure_and_lattice(weighted):
    g = G.heavy_graph(weighted)
    ln = g.csr.len
    rows = G.heavy_rows(g)
    assert ln[rows["heavy"]] == 4096 > G.HEAVY
    assert [ln[r] for r in rows["long2"]] == [1024, 1024] and [ln[r] for r in rows["long1"]] == [256, 256]
    assert (ln <= G.SPMM_SHORT).any()
    assert ((ln > G.SPMM_SHORT) & (ln <= G.HEAVY)).sum() == 66 + weighted  # + the 130-entry row
    assert (ln > G.HEAVY).sum() == 1
    assert [ln[r] for r in rows["hubs"]] == (list(G.HUB_ROWS) if weighted else [1, 1])
    if weighted:
        assert [g.csr.deg[r] for r in rows["hubs"]] == [G.WEIGHTED_DEG] * 2
        assert set(np.unique(g.csr.deg[g.U + G.HEAVY_ITEMS:])) == {4.0, 16.0}
        assert G.HUB_ROWS[0] < G.SPMM_SHORT < G.HUB_ROWS[1]
    # duplicate edges are part of the case (stub matching), and kept
    key = g.edge_index[0] * g.N + g.edge_index[1]
    assert len(np.unique(key)) < len(key)
    for d in G.HEAVY_F_DS:
        E0, layers, F, info = G.heavy_prop(weighted, d)
        print(f"heavy_L1 {'weighted' if weighted else 'unweighted'} d{d}: {_fmt(info)}")
        assert all(b < 24 for _, b in info.values())
        # this case is checked for F only: with one step for the whole table (2^-13, the heavy
        # item's self-loop) a score's terms are multiples of 2^-26, past fp32's 24 bits
        assert 2 * G.step_bits(F) > 24
    for d in G.LAYER_DS:
        _, _, _, (s, b) = G.layer_case("weighted" if weighted else "unweighted", d)
        print(f"layer d{d}: step 2^-{s} sum|terms| {b:.1f} bits")
        assert b < 24


def test_weighted_rows_exist_only_for_n_2_mod_4():
    for n in range(70, 340):
        ok = n % 4 == 2
        if ok:
            w = G.weighted_row(n)
            assert len(w) == n - 1 and w.sum() == G.WEIGHTED_DEG - 1 and set(w) <= {3.0, 15.0}
        else:  # 3 a + 15 b = 1,023 with a + b = n - 1 has no integer solution
            assert (G.WEIGHTED_DEG + 2 - 3 * n) % 12 != 0
    assert (np.bincount(G.weighted_row(126).astype(int))[[3, 15]] == [71, 54]).all()
    assert (np.bincount(G.weighted_row(130).astype(int))[[3, 15]] == [76, 53]).all()


def test_legacy_case_is_above_the_walk_limit():
    g = G.legacy_graph()
    assert g.N > G.WALK_LIMIT
    ln = g.csr.len
    assert (ln > G.HEAVY).sum() == 1 and ((ln > G.SPMM_SHORT) & (ln <= G.HEAVY)).sum() == 67
    assert (ln == 1).sum() > G.WALK_LIMIT - 10_000      # mostly self-loops
    _, _, _, (s, b) = G.layer_case("legacy", G.LEGACY_D)
    print(f"legacy layer d{G.LEGACY_D}: step 2^-{s} sum|terms| {b:.1f} bits")
    rows = np.array([0, g.U + G.HEAVY_ITEM, g.N - 1])
    G.combine_oracle(g.csr, rows, G.combine_layers("legacy", G.LEGACY_D), G.COMBINE_ALPHAS)


def test_csr_oracle_keeps_edge_order_and_duplicates():
    ei = np.array([[2, 0, 2, 1, 2, 0], [0, 2, 1, 2, 0, 2]])
    c = G.csr_oracle(ei, None, 4, lattice=False)
    assert c.rowptr.tolist() == [0, 3, 5, 9, 10]
    assert c.col.tolist() == [2, 2, 0, 2, 1, 0, 1, 0, 2, 3]   # edge order, self-loop last
    assert c.deg.tolist() == [3, 2, 4, 1]
    assert np.allclose(c.val64[:3], [1 / np.sqrt(12), 1 / np.sqrt(12), 1 / 3])


def test_inverse_sqrt_degree_forms():
    """deg^-1/2 as the kernel computes it (1 / sqrt, both correctly rounded) and as
    oracle/hnm_oracle.py does (deg ** -0.5) agree on the powers of four -- what the lattice
    relies on -- and differ by an ulp on many ordinary degrees; torch's CPU pow(-0.5) is
    compared with both (the counts are printed; DESIGN.md §2.1 quotes them)."""
    p4 = (4.0 ** np.arange(12)).astype(np.float32)
    want = (2.0 ** -np.arange(12)).astype(np.float32)
    tp4 = torch.from_numpy(p4)
    for got in (p4 ** np.float32(-0.5), np.float32(1) / np.sqrt(p4), tp4.pow(-0.5).numpy(),
                (1.0 / torch.sqrt(tp4)).numpy()):
        assert got.dtype == np.float32 and np.array_equal(L.bits(got), L.bits(want))
    deg = np.arange(1, 5000, dtype=np.float32)
    kern = np.float32(1) / np.sqrt(deg)
    orac = deg ** np.float32(-0.5)
    tor = torch.from_numpy(deg).pow(-0.5).numpy()
    n_ko = int((L.bits(kern) != L.bits(orac)).sum())
    n_tk = int((L.bits(tor) != L.bits(kern)).sum())
    n_to = int((L.bits(tor) != L.bits(orac)).sum())
    print(f"degrees 1..4999: 1/sqrt vs numpy ** -0.5 differ on {n_ko}; torch pow(-0.5) differs "
          f"from 1/sqrt on {n_tk}, from numpy ** -0.5 on {n_to}")
    ulp = np.abs(L.bits(kern).astype(np.int64) - L.bits(orac).astype(np.int64))
    assert ulp.max() <= 1
