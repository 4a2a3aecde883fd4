"""CPU-side checks (no GPU) of the deep-tower route query: hnm_ncf_deep_route is declared and
exported, and NeuralCF.scoring_route() needs no GPU for the fused tower but has no CPU path for
a deep one."""
import pytest

from hnm_recommendation_amd import NeuralCF, _lib


def test_route_query_declared_and_exported():
    assert "hnm_ncf_deep_route" in _lib.declared_symbols()
    assert hasattr(_lib.load(), "hnm_ncf_deep_route")


def test_scoring_route_surface():
    assert callable(NeuralCF(50, 40).scoring_route)
    assert NeuralCF(50, 40).scoring_route() == "fused"
    m = NeuralCF(50, 40, mlp_dims=[256, 128, 64])
    assert not m._fused()
    with pytest.raises(RuntimeError, match="no CPU path|GPU"):
        m.scoring_route()
