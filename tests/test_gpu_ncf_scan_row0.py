"""GPU: the certified NeuralCF scan with a user pair's 64 test values in one accumulator register
(ncf_cert_scan.hip ncf16_scan_kernel<.., ROW0 = true>, HNM_OPT_SCAN_ROW0 = 1: the sparse epilogue's
A operand holds wm in rows 0, 4, 8, 12, so lane 32 user + item ends with that pair's value, the
threshold test is one compare and the sample / debug passes store one value a lane) against the
four-register layout (0: rows 0-3, the values in lanes 0-15) and the exact fp32 scan.

Both options form the same products and sum them in the same order: only the lanes that hold the
test values differ.  So beside the exact top-k everything the scan itself reports is EQUAL between
the options, not close:

  (a) at either option the top-k (items and score bits: plain, with a 40-item history on every
      second user, and as one two-shard call) equals the exact scan's (HNM_OPT_PREFILTER = 0);
  (b) the counters (rows, candidates, exact-fallback rows) of every call are the same at both
      options, every row is counted and none takes the fallback, so a broken pass test or append
      can neither hide behind the fallback nor behind a wider candidate list;
  (c) the approximate scores and the bounds of the scan's debug pass (hnm_ncf_prefilter_debug_f32,
      which takes the option's epilogue and store lanes) are bitwise the same at both options.

Shapes are the smallest the certified path takes and at which the lane layout can go wrong: a
catalogue whose last 32-item tile is partial (padded items pass the early test and the tile mask
drops them) and one of whole tiles; batches of whole pairs in a partial wave (16), an odd last
pair with no user b (17, 37), a second 128-user block of one pair (130) and of one user (129); the
default tower and one whose units are half padding (h2 = 16)."""
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
OPT = _lib.HNM_OPT_SCAN_ROW0
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


def prefilter_debug(m, users):
    w, keep = m._weights()
    B, I = users.numel(), m.num_items
    approx = torch.empty(B, I, device=DEV)
    bound = torch.empty(B, I, device=DEV)
    _lib.check(_lib.fn("hnm_ncf_prefilter_debug_f32")(_lib.ctx(users.device), w, _lib.ptr(users),
                                                      B, _lib.ptr(approx), I, _lib.ptr(bound)),
               "hnm_ncf_prefilter_debug_f32")
    _lib.sync_check(users.device)
    return approx, bound


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
            out[name + ".stats"] = tuple(int(x) for x in _lib.prefilter_stats(dev, reset=True))[:3]
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
def test_scan_row0_topk_counters_and_debug(tower, weights, I, B):
    m = model(tower, weights, I)
    users = torch.from_numpy(syn.user_batch(U, B, seed=B)).to(DEV)
    dev = users.device
    filt = history(users, I)
    # the reference, once: the exact fp32 scan's top-k
    _lib.set_prefilter(dev, False)
    try:
        exact_topk = topk(m, users, filt)
    finally:
        _lib.set_prefilter(dev, True)
    got, dbg = {}, {}
    for opt in (1, 0):
        _lib.set_option(dev, OPT, opt)
        got[opt] = topk(m, users, filt)
        approx, bound = prefilter_debug(m, users)
        dbg[opt] = (bits(approx), bits(bound))
        print(f"\n    {tower}-{weights}-{I}-{B} option {opt}: (rows, candidates, fallback rows) plain "
              f"{got[opt]['plain.stats']} filtered {got[opt]['filtered.stats']}")
    for opt in (1, 0):
        for name in ("plain", "filtered"):
            for part in (".items", ".scores"):  # (a)
                assert np.array_equal(got[opt][name + part], exact_topk[name + part]), \
                    f"option {opt}: {name}{part} differs from the exact scan"
            rows, cands, fallback = got[opt][name + ".stats"]  # (b)
            assert rows == B, (opt, name, rows)
            assert fallback == 0, (opt, name, fallback)
    for name in ("plain", "filtered"):  # (b)
        assert got[1][name + ".stats"] == got[0][name + ".stats"], name
    assert np.array_equal(dbg[1][0], dbg[0][0]), "approximate scores differ between the options"  # (c)
    assert np.array_equal(dbg[1][1], dbg[0][1]), "bounds differ between the options"


def two_shards(m, users, I, G=2):
    """One item-sharded call (sharding.ncf_shard_topk, emulated shards, the bound lists merged as
    tests/test_gpu_sharding.py does): merged scores and items."""
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
    return bits(gv), gi.cpu().numpy()


def test_scan_row0_two_shards():
    """Two shards of 8,229 and 8,230 items (a partial last tile each), 129 users (an odd last pair
    in a second block), at either option: the merged top-k is the exact scan's."""
    I, B = 16_459, 129
    m = model("default", "init", I)
    users = torch.from_numpy(syn.user_batch(U, B, seed=4)).to(DEV)
    dev = users.device
    _lib.set_prefilter(dev, False)
    try:
        ve, ie = m.recommend_with_scores(users, k=K)
    finally:
        _lib.set_prefilter(dev, True)
    for opt in (1, 0):
        _lib.set_option(dev, OPT, opt)
        gv, gi = two_shards(m, users, I)
        assert np.array_equal(gi, ie.cpu().numpy()), opt
        assert np.array_equal(gv, bits(ve)), opt
