"""CPU-side checks of the conjugate-gradient ImplicitALS fit (no GPU): the two declared entries,
the validation of `solver` / `cg_steps`, no CPU path, the unchanged hparams, and the sanity of the
float64 oracle the GPU tests compare against."""
import os
import re

import numpy as np
import pytest

import cg_oracle as CO
from hnm_recommendation_amd import ImplicitALS, UserHistory, _lib
from hnm_recommendation_amd import synthetic as syn
from hnm_recommendation_amd.serving import Recommender

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAIN, WEIGHTED = "hnm_als_cg_rows_f32", "hnm_als_cg_rows_weighted_f32"


def header_params(name):
    src = open(os.path.join(REPO, "include", "hnm.h")).read()
    m = re.search(r"^hnm_status\s+" + name + r"\s*\(([^;]*)\);", src, re.M)
    assert m, f"{name} is not declared in hnm.h"
    return [p.strip() for p in m.group(1).split(",")]


def test_entries_are_declared_and_exported():
    lib = _lib.load()
    for name in (PLAIN, WEIGHTED):
        params = header_params(name)
        assert name in _lib.declared_symbols() and hasattr(lib, name), name
        assert len(_lib._SIGS[name][1]) == len(params), name     # one ctypes argument each
        assert params[-1] == "int steps" and params[-3] == "float* x"
    plain, weighted = _lib._SIGS[PLAIN][1], _lib._SIGS[WEIGHTED][1]
    assert weighted == plain[:3] + [_lib._p] + plain[3:]         # w right after idx
    assert header_params(WEIGHTED)[3] == "const float* w"
    # the solve entry's arguments, out / ldo as x / ldx, plus steps
    assert plain[:-1] == _lib._SIGS["hnm_als_solve_rows_f32"][1]
    assert lib.hnm_abi_version() == 1


def test_solver_and_cg_steps_are_validated_before_any_gpu_requirement():
    m = ImplicitALS(30, 20, embedding_dim=16)                    # a CPU model
    u, i = syn.interactions(30, 20, 100, seed=1)
    h = UserHistory.from_interactions(u, i, 30, 20, "cpu")
    with pytest.raises(ValueError, match="solver"):
        m.fit_history(h, solver="lu")
    with pytest.raises(ValueError, match="solver"):
        m.fit_interactions(u, i, solver="lu")
    for steps in (0, 33, -1, 2.5):
        with pytest.raises(ValueError, match="cg_steps"):
            m.fit_history(h, solver="cg", cg_steps=steps)
        with pytest.raises(ValueError, match="cg_steps"):
            m.fit_interactions(u, i, solver="cg", cg_steps=steps)
    srv = Recommender(30, 20, device="cpu")
    with pytest.raises(ValueError, match="solver"):
        srv.add_als(u, i, embedding_dim=16, solver="lu")


def test_no_cpu_path_for_the_cg_fit():
    m = ImplicitALS(30, 20, embedding_dim=16)
    u, i = syn.interactions(30, 20, 100, seed=1)
    with pytest.raises(RuntimeError, match="no CPU path|GPU"):
        m.fit_interactions(u, i, solver="cg")
    with pytest.raises(RuntimeError, match="no CPU path|GPU"):
        m.fit_history(UserHistory.from_interactions(u, i, 30, 20, "cpu"), solver="cg", cg_steps=1)
    with pytest.raises(RuntimeError, match="no CPU path|GPU"):
        Recommender(30, 20, device="cpu").add_als(u, i, embedding_dim=16, solver="cg", cg_steps=5)


def test_the_solver_is_not_a_hyperparameter():
    m = ImplicitALS(30, 20)
    assert set(m.hparams) == {"num_users", "num_items", "embedding_dim", "regularization",
                              "alpha", "iterations", "seed", "top_k"}
    assert m.fit_solver == ("cholesky", None)
    with pytest.raises(TypeError):
        ImplicitALS(30, 20, solver="cg")
    assert not any("solver" in k or "cg" in k for k in m.state_dict())


def d16_system(row=4):
    """(A, b) of a row of the raw-entry cases at d = 16 (row 4: 17 entries), in float64."""
    ptr, idx = CO.solve_rows()
    T = CO.case_inputs(16, 0.1, "zeros")[0].astype(np.float64)
    return CO.system(idx[ptr[row]:ptr[row + 1]], T, T.T @ T, 40.0, 0.01)


def test_oracle_cg_with_d_steps_reaches_the_exact_solution():
    A, b = d16_system()
    want = np.linalg.solve(A, b)
    for x0 in (np.zeros(16), np.random.default_rng(1).normal(0, 1.0, 16)):
        got = CO.cg(A, b, x0, 16)
        assert np.abs(got - want).max() <= 1e-8 * np.abs(want).max()
    assert np.abs(CO.cg(A, b, np.zeros(16), 2) - want).max() > 1e-4 * np.abs(want).max()


def test_every_oracle_cg_step_lowers_the_quadratic():
    A, b = d16_system(row=6)
    x0 = np.random.default_rng(3).normal(0, 1.0, 16)
    f = lambda x: 0.5 * x @ A @ x - b @ x                       # noqa: E731
    trace = []
    CO.cg(A, b, x0, 8, trace)
    vals = [f(x0)] + [f(x) for x in trace]
    assert len(trace) == 8 and all(b_ < a_ for a_, b_ in zip(vals, vals[1:]))


def test_oracle_half_step_rules_and_fp32_restatement():
    ptr, idx = CO.solve_rows()
    assert len(ptr) - 1 == 20 and np.diff(ptr)[:8].tolist() == CO.LENGTHS
    T, X0 = CO.case_inputs(16, 0.1, "random")
    ref = CO.cg_half_step(ptr, idx, T, 10.0, 0.1, X0, 3)
    empty = np.diff(ptr) == 0
    assert empty.any() and X0[empty].all() and not ref[empty].any()   # x0 of an empty row ignored
    assert np.array_equal(CO.cg_half_step(ptr, idx, T, 10.0, 0.1, X0[[5, 2]], 3, rows=[5, 2]),
                          ref[[5, 2]])
    # unit weights are the unweighted system
    one = np.ones(len(idx))
    assert np.allclose(CO.cg_half_step(ptr, idx, T, 10.0, 0.1, X0, 3, w=one), ref,
                       rtol=1e-12, atol=1e-14)
    # the fp32 restatement, in either summation order, is the same recurrence
    for rev in (False, True):
        assert CO.bar_use(CO.cg32_half_step(ptr, idx, T, 10.0, 0.1, X0, 3, rev), ref) < 0.25
