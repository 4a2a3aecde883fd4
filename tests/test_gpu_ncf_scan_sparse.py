"""GPU: the epilogue of the certified NeuralCF scan on the 2:4 sparse matrix instruction
(ncf_cert_scan.hip ncf16_scan_kernel<.., SPARSE = true>, HNM_OPT_SCAN_SPARSE = 1: wm . relu(H~) of a
user pair as 2 v_smfmac_f32_16x16x64_f16, the two users' converted accumulators interleaved in one
B operand) against the dense epilogue (0) and the exact fp32 scan.

The sparse epilogue sums the dense one's exact products in another order, so the two options'
approximate scores, and with them the candidate counts, need not agree and are not compared: the
counts are printed.  What must hold at either option:

  (a) the top-k (items and score bits: plain, with a 40-item history on every second user, and as
      one two-shard call) equals the exact scan's (HNM_OPT_PREFILTER = 0);
  (b) the counters report every row and no exact-fallback row (tests/test_gpu_ncf_scan_shape.py
      asserts zero on these inputs for both layouts), so a broken epilogue cannot hide behind the
      fallback;
  (c) the certified bound, pair by pair, on the approximate scores the scan's own debug pass
      returns (hnm_ncf_prefilter_debug_f32 takes the option's epilogue): the bound is finite and
      max |approx + bp - exact| / bound <= 1.

Shapes are the smallest the certified path takes and at which the interleaved operand can go
wrong: a catalogue whose last 32-item tile is partial and one of whole tiles; an odd last pair (no
user b in the operand), a partial wave, and a second 128-user block of one pair; the default tower
and one whose units are half padding (h2 = 16)."""
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
OPT = _lib.HNM_OPT_SCAN_SPARSE
SHIPPED = 1  # the option's default (hnm_ctx_create)

TOWERS = {
    "default": dict(mf_dim=64, mlp_dims=[128, 64, 32]),
    "mf16": dict(mf_dim=16, mlp_dims=[64, 32, 16]),
}
WEIGHTS = ["init", "norms", "student_t"]
CATALOGUES = [8229, 8256]
BATCHES = [17, 37, 130]


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
def test_scan_sparse_topk_counters_and_bound(tower, weights, I, B):
    m = model(tower, weights, I)
    users = torch.from_numpy(syn.user_batch(U, B, seed=B)).to(DEV)
    dev = users.device
    filt = history(users, I)
    # the references, once: the exact fp32 scan's top-k and the exact dense scores
    _lib.set_prefilter(dev, False)
    try:
        exact_topk = topk(m, users, filt)
    finally:
        _lib.set_prefilter(dev, True)
    exact = m.predict_all_items(users)
    bp = float(m.prediction_layer.bias.detach())
    for opt in (1, 0):
        _lib.set_option(dev, OPT, opt)
        got = topk(m, users, filt)
        approx, bound = prefilter_debug(m, users)
        finite = bool(torch.isfinite(bound).all())
        ratio = ((approx + bp - exact).abs() / bound).max().item()
        print(f"\n    {tower}-{weights}-{I}-{B} option {opt}: (rows, candidates, fallback rows) plain "
              f"{got['plain.stats'][:3]} filtered {got['filtered.stats'][:3]}, "
              f"max |approx + bp - exact| / bound = {ratio:.4f}")
        for name in ("plain", "filtered"):
            for part in (".items", ".scores"):
                assert np.array_equal(got[name + part], exact_topk[name + part]), \
                    f"option {opt}: {name}{part} differs from the exact scan"
            rows, cands, fallback = got[name + ".stats"][:3]
            assert rows == B, (opt, name, rows)
            assert fallback == 0, (opt, name, fallback)
        assert finite, opt
        assert ratio <= 1.0, (opt, ratio)


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


def test_scan_sparse_two_shards():
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
