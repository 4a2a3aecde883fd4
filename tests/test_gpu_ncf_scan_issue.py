"""GPU: the certified NeuralCF scan (ncf_cert_scan.hip ncf16_scan_kernel) after its issue
stream per pair was shortened -- 32-bit tile indices, a pass test that leaves a pair iteration at
the OR of its four compares when nothing passes, and that test run one pair late (the last pair
of a tile after the loop).

None of this may change a test value or an append: every seed keeps
(ga * cg + sgn * fmaf(cu, d, b)) - tau in that order, the compares stay ordered, the early exit
only skips work whose result was an empty pass mask, and the late test sees the same values in
the same pair order.  So, at the smallest shapes the certified path takes (>= 8,192 items, >= 16
rows: a catalogue whose last 32-item tile is partial and one of whole tiles; a batch with a
partial wave and an odd last user pair, and one with a second 128-user block of two rows), for
both layouts of the two-layer scan (HNM_OPT_SCAN_SHAPE) and for the deep scan:

  * the top-k (items and score bits, plain and with a 40-item history on every second user)
    equals the exact fp32 scan's (HNM_OPT_PREFILTER = 0);
  * the pre-filter counters (rows, candidates re-scored, exact-fallback rows) equal, exactly,
    those of the build before the change (commit fe6545b), recorded below from a run of this
    file's cases on that build.  The candidates are the items whose test value passed, so one
    changed test value near a threshold moves the count."""
import functools

import numpy as np
import pytest
import torch

from hnm_recommendation_amd import NeuralCF, _lib
from hnm_recommendation_amd import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda"
U, K = 3001, 12
OPT = _lib.HNM_OPT_SCAN_SHAPE
SHIPPED = 1  # the option's default (hnm_ctx_create)

TOWERS = {
    "default": dict(mf_dim=64, mlp_dims=[128, 64, 32]),
    "mf16": dict(mf_dim=16, mlp_dims=[64, 32, 16]),
    "deep": dict(mf_dim=64, mlp_dims=[128, 64, 32, 16]),  # the deep scan: one layout only
}
CASES = [(t, w) for t in ("default", "mf16") for w in ("init", "norms", "student_t")]
CASES.append(("deep", "norms"))
CATALOGUES = [8229, 8256]
BATCHES = [37, 130]

# (rows, candidates, fallback rows) of the plain and of the filtered call at commit fe6545b, by
# "tower-weights-I-B-layout"
PARENT_STATS = {
    "default-init-8229-37-1": ((37, 5162, 0), (37, 5161, 0)),
    "default-init-8229-37-0": ((37, 5162, 0), (37, 5161, 0)),
    "default-init-8229-130-1": ((130, 17493, 0), (130, 17465, 0)),
    "default-init-8229-130-0": ((130, 17493, 0), (130, 17465, 0)),
    "default-init-8256-37-1": ((37, 5575, 0), (37, 5566, 0)),
    "default-init-8256-37-0": ((37, 5575, 0), (37, 5566, 0)),
    "default-init-8256-130-1": ((130, 19177, 0), (130, 19163, 0)),
    "default-init-8256-130-0": ((130, 19177, 0), (130, 19163, 0)),
    "default-norms-8229-37-1": ((37, 2401, 0), (37, 2399, 0)),
    "default-norms-8229-37-0": ((37, 2401, 0), (37, 2399, 0)),
    "default-norms-8229-130-1": ((130, 8387, 0), (130, 8372, 0)),
    "default-norms-8229-130-0": ((130, 8387, 0), (130, 8372, 0)),
    "default-norms-8256-37-1": ((37, 2324, 0), (37, 2324, 0)),
    "default-norms-8256-37-0": ((37, 2324, 0), (37, 2324, 0)),
    "default-norms-8256-130-1": ((130, 8410, 0), (130, 8381, 0)),
    "default-norms-8256-130-0": ((130, 8410, 0), (130, 8381, 0)),
    "default-student_t-8229-37-1": ((37, 14557, 0), (37, 14527, 0)),
    "default-student_t-8229-37-0": ((37, 14557, 0), (37, 14527, 0)),
    "default-student_t-8229-130-1": ((130, 68653, 0), (130, 68595, 0)),
    "default-student_t-8229-130-0": ((130, 68653, 0), (130, 68595, 0)),
    "default-student_t-8256-37-1": ((37, 80519, 0), (37, 80334, 0)),
    "default-student_t-8256-37-0": ((37, 80519, 0), (37, 80334, 0)),
    "default-student_t-8256-130-1": ((130, 270980, 0), (130, 270845, 0)),
    "default-student_t-8256-130-0": ((130, 270980, 0), (130, 270845, 0)),
    "mf16-init-8229-37-1": ((37, 5773, 0), (37, 5763, 0)),
    "mf16-init-8229-37-0": ((37, 5773, 0), (37, 5763, 0)),
    "mf16-init-8229-130-1": ((130, 17141, 0), (130, 17120, 0)),
    "mf16-init-8229-130-0": ((130, 17141, 0), (130, 17120, 0)),
    "mf16-init-8256-37-1": ((37, 2522, 0), (37, 2520, 0)),
    "mf16-init-8256-37-0": ((37, 2522, 0), (37, 2520, 0)),
    "mf16-init-8256-130-1": ((130, 8914, 0), (130, 8910, 0)),
    "mf16-init-8256-130-0": ((130, 8914, 0), (130, 8910, 0)),
    "mf16-norms-8229-37-1": ((37, 2356, 0), (37, 2356, 0)),
    "mf16-norms-8229-37-0": ((37, 2356, 0), (37, 2356, 0)),
    "mf16-norms-8229-130-1": ((130, 8303, 0), (130, 8298, 0)),
    "mf16-norms-8229-130-0": ((130, 8303, 0), (130, 8298, 0)),
    "mf16-norms-8256-37-1": ((37, 2150, 0), (37, 2150, 0)),
    "mf16-norms-8256-37-0": ((37, 2150, 0), (37, 2150, 0)),
    "mf16-norms-8256-130-1": ((130, 7597, 0), (130, 7592, 0)),
    "mf16-norms-8256-130-0": ((130, 7597, 0), (130, 7592, 0)),
    "mf16-student_t-8229-37-1": ((37, 744, 0), (37, 747, 0)),
    "mf16-student_t-8229-37-0": ((37, 744, 0), (37, 747, 0)),
    "mf16-student_t-8229-130-1": ((130, 2873, 0), (130, 2869, 0)),
    "mf16-student_t-8229-130-0": ((130, 2873, 0), (130, 2869, 0)),
    "mf16-student_t-8256-37-1": ((37, 1255, 0), (37, 1255, 0)),
    "mf16-student_t-8256-37-0": ((37, 1255, 0), (37, 1255, 0)),
    "mf16-student_t-8256-130-1": ((130, 4551, 0), (130, 4569, 0)),
    "mf16-student_t-8256-130-0": ((130, 4551, 0), (130, 4569, 0)),
    "deep-norms-8229-37-1": ((37, 2388, 0), (37, 2386, 0)),
    "deep-norms-8229-130-1": ((130, 8317, 0), (130, 8317, 0)),
    "deep-norms-8256-37-1": ((37, 2346, 0), (37, 2345, 0)),
    "deep-norms-8256-130-1": ((130, 8401, 0), (130, 8401, 0)),
}


def layouts(tower):
    return (SHIPPED,) if tower == "deep" else (1, 0)


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


def run_case(tower, weights, I, B):
    """The exact scan's top-k and, per layout, the certified call's top-k and counters."""
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
    for opt in layouts(tower):
        _lib.set_option(dev, OPT, opt)
        got[opt] = topk(m, users, filt)
    return exact, got


@pytest.fixture(autouse=True)
def _restore_options():
    yield
    _lib.set_option(torch.device(DEV, 0), OPT, SHIPPED)
    _lib.set_prefilter(torch.device(DEV, 0), True)


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("I", CATALOGUES)
@pytest.mark.parametrize("tower,weights", CASES)
def test_scan_topk_exact_and_counters_unchanged(tower, weights, I, B):
    exact, got = run_case(tower, weights, I, B)
    for opt, g in got.items():  # every figure first
        print(f'\n    "{tower}-{weights}-{I}-{B}-{opt}": {(g["plain.stats"], g["filtered.stats"])},')
    for opt, g in got.items():
        key = f"{tower}-{weights}-{I}-{B}-{opt}"
        stats = (g["plain.stats"], g["filtered.stats"])
        for name in ("plain", "filtered"):
            for part in (".items", ".scores"):
                assert np.array_equal(g[name + part], exact[name + part]), \
                    f"{key}: {name}{part} differs from the exact scan"
        assert stats == PARENT_STATS[key], (key, stats, PARENT_STATS[key])
