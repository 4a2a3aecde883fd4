"""GPU: every instantiated Wide&Deep tower shape (the WD_SHAPES table of widedeep_internal.h).

The exact fp32 kernel exists for ten (RB2, OB) shapes -- layer-2 / layer-3 widths in blocks of
32 rounded up to a power of two -- and the certified scan, refine and re-score kernels for six
of them.  The other suites run the default tower and three small ones; here each table entry
goes through its own kernels, on towers whose widths are no multiples of 32 (zero padding),
with 9 users (a partial last block for 4 and for 8 users a block) and item counts that are no
multiple of the 32-item tile.  A shape outside the table is refused; an exact-only shape never
takes the certified route.
"""
import functools

import numpy as np
import pytest
import torch

from hnm_recommendation_amd import _lib
from hnm_recommendation_amd import synthetic as syn
from oracle import hnm_oracle as O
from parity import assert_scores_close, assert_topk_equivalent
from test_gpu_prefilter import DEV, topk_both, wd_model, wd_prefilter_debug, wd_refine_debug

pytestmark = pytest.mark.gpu

SCALED = {"bias_scale": 0.05, "randomize_bn": True, "emb_scale": 10.0}
B = 9

# layer 1 is 40 wide: K1P % 16 != 0, so these can never take the certified route
EXACT_TOWERS = [[40, 200, 100],  # (8, 4)
                [40, 100, 50],   # (4, 2)
                [40, 50, 20],    # (2, 1)
                [40, 20],        # (1, 0)
                [40, 50],        # (2, 0)
                [40, 100],       # (4, 0)
                [40, 200],       # (8, 0)
                [40, 20, 10],    # (1, 1)
                [40, 100, 100],  # (4, 4)
                [40, 200, 50]]   # (8, 2)
# layer 1 is 48 wide: K1P % 16 == 0.  Weights: the scaled setting of the other suites.
CERT_TOWERS = [[48, 200, 100],  # (8, 4)
               [48, 100, 50],   # (4, 2)
               [48, 50, 20],    # (2, 1)
               [48, 20, 10],    # (1, 1)
               [48, 20],        # (1, 0)
               [48, 50]]        # (2, 0)
CERT_U, CERT_I = 3000, 4200  # at least the certified floor of 4096 items, a partial last tile


def tid(layers):
    return "-".join(map(str, layers))


@pytest.mark.parametrize("layers", EXACT_TOWERS, ids=tid)
def test_exact_shape_vs_oracle(layers):
    U, I = 300, 1111
    m, sd = wd_model(U, I, seed=5, layers=tuple(layers), d=16, **SCALED)
    users = syn.user_batch(U, B, seed=6)
    tu = torch.from_numpy(users).to(DEV)
    ref = O.widedeep_predict_all_items(sd, users)
    assert_scores_close(m.predict_all_items(tu).cpu().numpy(), ref, f"wd {layers}")
    assert_topk_equivalent(m.recommend(tu).cpu().numpy(), ref, 12, what=f"wd {layers}")
    # a filter on three of the users that takes their best items away
    f = syn.filter_dict(users[:3], I, per_user=23, seed=7)
    for b, u in enumerate(users[:3]):
        f[int(u)] |= set(int(x) for x in np.argsort(-ref[b])[:5])
    masked = O.apply_filter(ref, users, f)
    assert_topk_equivalent(m.recommend(tu, filter_items=f).cpu().numpy(), masked, 12,
                           what=f"wd {layers} filtered")
    # the pairwise forward on 8 pairs against the same dense entries
    pu = np.arange(8) % B
    pi = syn.user_batch(I, 8, seed=8)
    got = m(tu[pu], torch.from_numpy(pi).to(DEV)).cpu().numpy()
    assert_scores_close(got, ref[pu, pi], f"wd {layers} pairs")


@functools.lru_cache(maxsize=None)
def cert_case(layers):
    m, _ = wd_model(CERT_U, CERT_I, seed=11, layers=layers, d=16, **SCALED)
    users_np = syn.user_batch(CERT_U, B, seed=12)
    return m, users_np, torch.from_numpy(users_np).to(DEV)


@pytest.mark.parametrize("layers", CERT_TOWERS, ids=tid)
def test_certified_shape_identical_to_exact(layers):
    m, users_np, users = cert_case(tuple(layers))
    _lib.set_prefilter(users.device, False)
    try:
        _, top = m.recommend_with_scores(users, k=30)
    finally:
        _lib.set_prefilter(users.device, True)
    top = top.cpu().numpy()
    rng = np.random.default_rng(1)
    f = {int(u): set(top[r, ::2].tolist()) | set(rng.integers(0, CERT_I, 50).tolist())
         for r, u in enumerate(users_np[:3])}
    for k in (1, 12, 64):
        for filt in (None, f):
            (ev, ei), (pv, pi), stats = topk_both(m, users, filt, k=k)
            what = (layers, k, filt is not None)
            print(f"W&D {layers} k={k} filter={filt is not None}: rows {stats[0]}, "
                  f"fallback rows {stats[2]}")
            assert np.array_equal(ei, pi), what
            assert np.array_equal(ev.view(np.uint32), pv.view(np.uint32)), what
            assert stats[0] == B, what  # the certified route ran
            if filt:
                for r, u in enumerate(users_np[:3]):
                    assert not (set(pi[r].tolist()) & f[int(u)]), what


@pytest.mark.parametrize("layers", CERT_TOWERS, ids=tid)
def test_certified_shape_bounds_hold(layers):
    """|approx - exact| <= bound for every pair, for the scan and for the refining stage."""
    m, _, users = cert_case(tuple(layers))
    exact = m.predict_all_items(users)
    for dbg in (wd_prefilter_debug, wd_refine_debug):
        approx, bound = dbg(m, users)
        ratio = ((approx - exact).abs() / bound).max().item()
        print(f"W&D {layers} {dbg.__name__}: max |approx - exact| / bound = {ratio:.4f}")
        assert torch.isfinite(bound).all(), dbg.__name__
        assert ((approx - exact).abs() <= bound).all(), (dbg.__name__, ratio)


def test_shape_outside_the_table_is_refused():
    m, _ = wd_model(300, 1111, seed=5, layers=(48, 64, 64), d=16, **SCALED)  # (2, 2)
    users = torch.from_numpy(syn.user_batch(300, B, seed=6)).to(DEV)
    with pytest.raises(ValueError, match="not instantiated"):
        m.predict_all_items(users)
    with pytest.raises(ValueError, match="not instantiated"):
        m.recommend_with_scores(users)


def test_exact_only_shape_never_takes_the_certified_route():
    m, _ = wd_model(CERT_U, CERT_I, seed=11, layers=(48, 100, 100), d=16, **SCALED)  # (4, 4)
    users = torch.from_numpy(syn.user_batch(CERT_U, B, seed=12)).to(DEV)
    (ev, ei), (pv, pi), stats = topk_both(m, users)
    assert np.array_equal(ei, pi)
    assert np.array_equal(ev.view(np.uint32), pv.view(np.uint32))
    assert stats[0] == 0, stats
