"""GPU: the two layouts of the certified NeuralCF scan (ncf_cert_scan.hip ncf16_scan_kernel,
HNM_OPT_SCAN_SHAPE): layer 2 and the GMF on v_mfma_f32_16x16x32_f16 (1) or on
v_mfma_f32_32x32x16_f16 (0).

The scan only prunes, and every returned score is recomputed in exact fp32, so under either
layout the top-k (items and score bits, plain and with a history filter) must equal the exact
fp32 scan's (HNM_OPT_PREFILTER = 0) and therefore each other's.  The two layouts sum the same exact
products in a different order, so their approximate scores need not agree bit for bit and are
never compared with each other: each must satisfy the certified bound against the exact scores,
pair by pair (|approx + bp - exact| <= bound, the form tests/test_gpu_prefilter.py checks on the
full catalogue).  The `huge` weights make the bound unusable by construction (a table entry above
2^40 sets CertParams.bad), which the library reports by sending every row to the exact fallback:
there the test asserts that, and the pair-by-pair inequality on the three usable weight sets.

Shapes are the smallest the certified path takes (>= 8,192 items, >= 16 rows): a catalogue whose
last 32-item tile is partial and one of whole tiles; a batch with a partial wave and an odd last
user pair, and one with a second 128-user block of two rows; the default tower and one whose k
and units are padded (h1 = 32, h2 = 16, mf 16)."""
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
OPT = _lib.HNM_OPT_SCAN_SHAPE
SHIPPED = 1  # the option's default (hnm_ctx_create)

TOWERS = {
    "default": dict(mf_dim=64, mlp_dims=[128, 64, 32]),
    "mf16": dict(mf_dim=16, mlp_dims=[64, 32, 16]),
}
WEIGHTS = ["init", "norms", "student_t", "huge"]
CATALOGUES = [8229, 8256]
BATCHES = [37, 130]


@functools.lru_cache(maxsize=None)
def _state(tower, weights, I):
    t = TOWERS[tower]
    sd = syn.ncf_state_dict(U, I, t["mf_dim"], tuple(t["mlp_dims"]), seed=21, bias_scale=0.05)
    if weights != "init":
        sd = syn.stress_state_dict(sd, weights, syn.NCF_EMB_KEYS, "mlp_item_embedding.weight", 3)
    return sd


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


def topk(m, users, filt, k):
    """Top-k without / with the filter (score bits, items) and the counters of both calls."""
    dev = users.device
    out = {}
    _lib.prefilter_stats(dev, reset=True)
    _lib.set_option(dev, _lib.HNM_OPT_STATS, 1)
    try:
        for name, f in (("plain", None), ("filtered", filt)):
            v, i = m.recommend_with_scores(users, filter_items=f, k=k)
            out[name + ".scores"], out[name + ".items"] = bits(v), i.cpu().numpy()
            out[name + ".stats"] = np.asarray(_lib.prefilter_stats(dev, reset=True))
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
def test_scan_shape_topk_and_bound(tower, weights, I, B):
    m = model(tower, weights, I)
    users = torch.from_numpy(syn.user_batch(U, B, seed=B)).to(DEV)
    dev = users.device
    filt = history(users, I)
    k = 64 if weights == "huge" else K
    # the references, once: the exact fp32 scan's top-k and the exact dense scores
    _lib.set_prefilter(dev, False)
    try:
        exact_topk = {}
        for name, f in (("plain", None), ("filtered", filt)):
            v, i = m.recommend_with_scores(users, filter_items=f, k=k)
            exact_topk[name + ".scores"], exact_topk[name + ".items"] = bits(v), i.cpu().numpy()
    finally:
        _lib.set_prefilter(dev, True)
    exact = m.predict_all_items(users)
    bp = float(m.prediction_layer.bias.detach())
    got = {}
    for opt in (1, 0):
        _lib.set_option(dev, OPT, opt)
        got[opt] = topk(m, users, filt, k)
        for key, ref in exact_topk.items():
            assert np.array_equal(got[opt][key], ref), f"option {opt}: {key} differs from the exact scan"
        for name in ("plain", "filtered"):
            rows, cands, fallback = got[opt][name + ".stats"][:3]
            assert rows == B, (opt, name)
            assert fallback == (B if weights == "huge" else 0), (opt, name, fallback)
        if weights != "huge":
            approx, bound = prefilter_debug(m, users)
            assert torch.isfinite(bound).all(), opt
            ratio = ((approx + bp - exact).abs() / bound).max().item()
            print(f"option {opt}: max |approx + bp - exact| / bound = {ratio:.4f}")
            assert ratio <= 1.0, (opt, ratio)
    for key in exact_topk:
        assert np.array_equal(got[1][key], got[0][key]), f"option 1 vs 0: {key} differs"


@pytest.mark.parametrize("tower", list(TOWERS))
def test_scan_shape_two_shards(tower):
    """The item-sharded protocol (sharding.ncf_shard_topk, two emulated shards of >= 8,192 items
    each, the bound lists merged as tests/test_gpu_sharding.py does) under option 1: the merged
    top-k is bitwise the unsharded answer."""
    I, B, G = 16_459, 37, 2
    m = model(tower, "init", I)
    users = torch.from_numpy(syn.user_batch(U, B, seed=4)).to(DEV)
    _lib.set_option(users.device, OPT, 1)
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
    v1, i1 = m.recommend_with_scores(users, k=K)
    assert np.array_equal(gi.cpu().numpy(), i1.cpu().numpy())
    assert np.array_equal(bits(gv), bits(v1))
    _lib.set_prefilter(users.device, False)
    ve, ie = m.recommend_with_scores(users, k=K)
    assert np.array_equal(i1.cpu().numpy(), ie.cpu().numpy())
    assert np.array_equal(bits(v1), bits(ve))
