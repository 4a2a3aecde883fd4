"""GPU: the threshold pass of the certified NeuralCF scan with its user-pair loop pipelined by hand
(ncf_cert_scan.hip ncf16_scan_kernel<SCAN_THRESH, false, 1, true>, HNM_OPT_SCAN_PIPE = 1) against
the plain loop (0) and the exact fp32 scan.

The pipelined loop reads the next pair's P~ fragments and forms its B operands one k-step ahead,
so it can break where a tile or a wave's user range ends: a catalogue whose last 32-item tile is
partial and one of whole tiles; the minimum batch, an odd last pair (no user b), a partial wave,
and a second 128-user block holding one user (prologue and drain only) or one pair (no steady
state).  It issues the same MFMAs on the same operands in the same chains, so at option 1

  (a) the top-k (items and score bits: plain, with a 40-item history on every second user, and as
      one two-shard call) equals the exact scan's (HNM_OPT_PREFILTER = 0);
  (b) the pre-filter counters (rows, candidates re-scored, exact-fallback rows) equal, exactly,
      those of the same call at option 0.  The candidates are the items whose test value passed,
      so one changed test value near a threshold moves the count."""
import functools

import numpy as np
import pytest
import torch

from hnm_recommendation_amd import NeuralCF, _lib
from hnm_recommendation_amd import sharding as S
from hnm_recommendation_amd import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda"
U, K = 3001, 12
OPT = _lib.HNM_OPT_SCAN_PIPE
SHIPPED = 1  # the option's default (hnm_ctx_create)

TOWERS = {
    "default": dict(mf_dim=64, mlp_dims=[128, 64, 32]),
    "mf16": dict(mf_dim=16, mlp_dims=[64, 32, 16]),
}
WEIGHTS = ["init", "norms", "student_t"]
CATALOGUES = [8229, 8256]
BATCHES = [16, 17, 37, 129, 130]


@functools.lru_cache(maxsize=None)
def _state(tower, weights, I):
    t = TOWERS[tower]
    sd = syn.ncf_state_dict(U, I, t["mf_dim"], tuple(t["mlp_dims"]), seed=21, bias_scale=0.05)
    if weights != "init":
        sd = syn.stress_state_dict(sd, weights, syn.NCF_EMB_KEYS, "mlp_item_embedding.weight", 3)
    return sd


@functools.lru_cache(maxsize=2)
def model(tower, weights, I):
    m = NeuralCF(U, I, **TOWERS[tower])
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in _state(tower, weights, I).items()})
    return m.to(DEV).eval()


def bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy()


def history(users, I, seed=0):
    rng = np.random.default_rng(seed)
    return {int(u): set(rng.integers(0, I, 40).tolist()) for u in users.cpu().numpy()[::2]}


def topk(m, users, filt):
    """Top-k without / with the filter (score bits, items) and the counters of each call."""
    dev = users.device
    out = {}
    _lib.prefilter_stats(dev, reset=True)
    _lib.set_option(dev, _lib.HNM_OPT_STATS, 1)
    try:
        for name, f in (("plain", None), ("filtered", filt)):
            v, i = m.recommend_with_scores(users, filter_items=f, k=K)
            out[name + ".scores"], out[name + ".items"] = bits(v), i.cpu().numpy()
            out[name + ".stats"] = tuple(int(x) for x in _lib.prefilter_stats(dev, reset=True))
    finally:
        _lib.set_option(dev, _lib.HNM_OPT_STATS, 0)
    return out


@pytest.fixture(autouse=True)
def _restore_options():
    yield
    _lib.set_option(torch.device(DEV, 0), OPT, SHIPPED)
    _lib.set_prefilter(torch.device(DEV, 0), True)


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("I", CATALOGUES)
@pytest.mark.parametrize("weights", WEIGHTS)
@pytest.mark.parametrize("tower", list(TOWERS))
def test_scan_pipe_topk_exact_and_counters(tower, weights, I, B):
    m = model(tower, weights, I)
    users = torch.from_numpy(syn.user_batch(U, B, seed=B)).to(DEV)
    dev = users.device
    filt = history(users, I)
    _lib.set_prefilter(dev, False)
    try:
        exact = topk(m, users, filt)
    finally:
        _lib.set_prefilter(dev, True)
    got = {}
    for opt in (0, 1):
        _lib.set_option(dev, OPT, opt)
        got[opt] = topk(m, users, filt)
    for opt, g in got.items():  # every figure first
        print(f"\n    {tower}-{weights}-{I}-{B} option {opt}: {(g['plain.stats'], g['filtered.stats'])}")
    for name in ("plain", "filtered"):
        for part in (".items", ".scores"):
            assert np.array_equal(got[1][name + part], exact[name + part]), \
                f"option 1: {name}{part} differs from the exact scan"
        assert got[1][name + ".stats"][0] == B, (name, got[1][name + ".stats"])
        assert got[1][name + ".stats"] == got[0][name + ".stats"], \
            (name, got[1][name + ".stats"], got[0][name + ".stats"])


def two_shards(m, users, I, G=2):
    """One item-sharded call (sharding.ncf_shard_topk, emulated shards, the bound lists merged as
    tests/test_gpu_sharding.py does): merged scores, items and the call's counters."""
    dev = users.device
    _lib.prefilter_stats(dev, reset=True)
    _lib.set_option(dev, _lib.HNM_OPT_STATS, 1)
    try:
        shards = [S.ncf_shard_topk(m, *S.shard_range(I, r, G), K) for r in range(G)]
        lists = []
        for s in shards:
            lists.append(s.begin_lists(users))
            s.abort()
        assert all(torch.isfinite(x).all() for x in lists)  # both shards are certified
        merged = torch.topk(torch.cat(lists, dim=1), K, dim=1).values[:, K - 1].contiguous()
        vs, ids = [], []
        for r, s in enumerate(shards):
            s.begin_lists(users)
            val, idx = s.finish(users, merged)
            lo = S.shard_range(I, r, G)[0]
            vs.append(val)
            ids.append(torch.where(idx >= 0, idx + lo, idx))
        gv, gi = S.hip_merge(torch.stack(vs), torch.stack(ids), K)
        stats = tuple(int(x) for x in _lib.prefilter_stats(dev, reset=True))
    finally:
        _lib.set_option(dev, _lib.HNM_OPT_STATS, 0)
    return bits(gv), gi.cpu().numpy(), stats


@pytest.mark.parametrize("weights", WEIGHTS)
@pytest.mark.parametrize("tower", list(TOWERS))
def test_scan_pipe_two_shards(tower, weights):
    """Two shards of 8,229 and 8,230 items (a partial last tile each), 129 users."""
    I, B = 16_459, 129
    m = model(tower, weights, I)
    users = torch.from_numpy(syn.user_batch(U, B, seed=4)).to(DEV)
    dev = users.device
    _lib.set_prefilter(dev, False)
    try:
        ve, ie = m.recommend_with_scores(users, k=K)
    finally:
        _lib.set_prefilter(dev, True)
    got = {}
    for opt in (0, 1):
        _lib.set_option(dev, OPT, opt)
        got[opt] = two_shards(m, users, I)
        print(f"\n    {tower}-{weights} two shards, option {opt}: {got[opt][2]}")
    assert np.array_equal(got[1][1], ie.cpu().numpy())
    assert np.array_equal(got[1][0], bits(ve))
    assert got[1][2][0] > 0 and got[1][2] == got[0][2], (got[1][2], got[0][2])
