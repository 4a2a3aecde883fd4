"""CPU-side checks of ImplicitALS (no GPU): constructor, state_dict surface, dispatch, declared
entries, no CPU path, and the sanity of the float64 oracle the GPU tests compare against."""
import numpy as np
import pytest
import torch

import als_oracle as AO
from hnm_recommendation_amd import ImplicitALS, MatrixFactorization, UserHistory, _lib
from hnm_recommendation_amd import synthetic as syn
from hnm_recommendation_amd.serving import (_DISPATCH, Recommender, create_model_from_checkpoint,
                                            load_checkpoint)


def test_constructor_validation_and_hparams():
    m = ImplicitALS(30, 20, embedding_dim=32, regularization=0.1, alpha=10.0, iterations=3,
                    seed=7, top_k=5)
    assert m.hparams == {"num_users": 30, "num_items": 20, "embedding_dim": 32,
                         "regularization": 0.1, "alpha": 10.0, "iterations": 3, "seed": 7,
                         "top_k": 5}
    for kw in ({"embedding_dim": 8}, {"embedding_dim": 24}, {"embedding_dim": 144},
               {"regularization": 0.0}, {"regularization": -1.0},
               {"regularization": float("nan")}, {"alpha": -0.5}, {"alpha": float("inf")},
               {"iterations": -1}):
        with pytest.raises(ValueError):
            ImplicitALS(30, 20, **kw)
    ImplicitALS(30, 20, alpha=0.0, iterations=0)


def test_state_is_a_matrix_factorization_state():
    m = ImplicitALS(30, 20, embedding_dim=16, seed=3)
    mf = MatrixFactorization(30, 20, embedding_dim=16)
    ours = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert ours == {k: tuple(v.shape) for k, v in mf.state_dict().items()}
    for k in ("user_bias.weight", "item_bias.weight", "global_bias", "user_embeddings.weight"):
        assert not m.state_dict()[k].any(), k
    mf.load_state_dict(m.state_dict())            # loads as a MatrixFactorization ...
    m2 = ImplicitALS(30, 20, embedding_dim=16)
    m2.load_state_dict(mf.state_dict())           # ... and the reverse
    assert torch.equal(m2.item_embeddings.weight, m.item_embeddings.weight)
    # the seeded start: the same seed gives the same item table, another seed another one
    assert torch.equal(ImplicitALS(30, 20, embedding_dim=16, seed=3).item_embeddings.weight,
                       m.item_embeddings.weight)
    assert not torch.equal(ImplicitALS(30, 20, embedding_dim=16, seed=4).item_embeddings.weight,
                           m.item_embeddings.weight)
    assert 0.005 < float(m.item_embeddings.weight.detach().std()) < 0.02


def test_dispatch_and_checkpoint_on_cpu(tmp_path):
    assert dict(_DISPATCH)["implicit_als"] is ImplicitALS
    src = ImplicitALS(50, 40, embedding_dim=16, alpha=5.0, seed=2)
    hp = dict(src.hparams)
    hp["num_users"], hp["num_items"] = 1, 1
    path = tmp_path / "als.ckpt"
    torch.save({"state_dict": src.state_dict(), "hyper_parameters": hp}, path)
    m = create_model_from_checkpoint("runs/implicit_als", load_checkpoint(str(path)), 50, 40,
                                     "cpu")
    assert type(m) is ImplicitALS and m.alpha == 5.0 and not m.training
    for k, v in src.state_dict().items():
        assert torch.equal(m.state_dict()[k], v), k
    # the same state under the other name is a MatrixFactorization
    ck = {"state_dict": src.state_dict(), "hyper_parameters": {"embedding_dim": 16}}
    assert type(create_model_from_checkpoint("matrix_factorization", ck, 50, 40, "cpu")) \
        is MatrixFactorization


def test_entries_are_declared():
    assert {"hnm_als_gram_f32", "hnm_als_solve_rows_f32"} <= set(_lib.declared_symbols())
    lib = _lib.load()
    assert hasattr(lib, "hnm_als_gram_f32") and hasattr(lib, "hnm_als_solve_rows_f32")


def test_no_cpu_path():
    m = ImplicitALS(30, 20, embedding_dim=16)
    u, i = syn.interactions(30, 20, 100, seed=1)
    with pytest.raises(RuntimeError, match="no CPU path|GPU"):
        m.fit_interactions(u, i)
    with pytest.raises(RuntimeError, match="no CPU path|GPU"):
        m.fit_history(UserHistory.from_interactions(u, i, 30, 20, "cpu"))
    with pytest.raises(RuntimeError, match="no CPU path|GPU"):
        m.user_factors([[1, 2]])
    with pytest.raises(RuntimeError, match="no CPU path|GPU"):
        m.recommend(torch.tensor([0]))
    srv = Recommender(30, 20, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU path|GPU"):
        srv.add_als(u, i, embedding_dim=16)


@pytest.mark.parametrize("alpha,reg", [(10.0, 0.1), (40.0, 0.01)])
def test_oracle_half_step_zeroes_the_gradient(alpha, reg):
    """The oracle's half-steps are the exact minimisers of L in their own block: dL/dX = 0 after
    the user step, dL/dY = 0 after the item step (float64, relative to the gradient before)."""
    U, I, d = 40, 30, 8
    users, items = syn.interactions(U, I, 300, seed=4)
    keep = (users % 7 != 0) & (items % 11 != 0)            # empty users and empty items
    ptr, idx = AO.csr(users[keep], items[keep], U, I)
    tptr, tidx = AO.transpose(ptr, idx, U, I)
    rng = np.random.default_rng(0)
    Y = rng.normal(0, 0.1, (I, d))
    X0 = rng.normal(0, 0.1, (U, d))
    g0 = np.abs(AO.grad_users(X0, Y, ptr, idx, alpha, reg)).max()
    X = AO.half_step(ptr, idx, Y, alpha, reg)
    g = AO.grad_users(X, Y, ptr, idx, alpha, reg)
    nonempty = np.diff(ptr) > 0
    assert np.abs(g[nonempty]).max() <= 1e-10 * g0
    assert not X[~nonempty].any() and (~nonempty).sum() >= 5
    # the item step is the user step of the transposed problem
    Y1 = AO.half_step(tptr, tidx, X, alpha, reg)
    gy = AO.grad_users(Y1, X, tptr, tidx, alpha, reg)
    assert np.abs(gy[np.diff(tptr) > 0]).max() <= 1e-10 * g0
    assert (np.diff(tptr) == 0).sum() >= 2
    # and the loss goes down at each half-step
    l0 = AO.loss_dense(X0, Y, ptr, idx, alpha, reg)
    l1 = AO.loss_dense(X, Y, ptr, idx, alpha, reg)
    l2 = AO.loss_dense(X, Y1, ptr, idx, alpha, reg)
    assert l2 < l1 < l0
