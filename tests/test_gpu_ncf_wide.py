"""GPU: NeuralCF towers with layers 65..128 units wide (e.g. mlp_dims [256, 128, 64]) on the
fp32-MFMA tile kernel (ncf_deep.hip `ncf_deep_mfma_kernel`, W = 128 rows and up to 4 32-unit
tiles a layer).

* `scoring_route()` reports "mfma" for them and "per_pair" under HNM_OPT_DEEP_MFMA = 0.
* Scores are bitwise the per-pair LDS kernel's (the f32 MFMA is the fmaf chain in k order) and
  agree with the CPU oracle (oracle/hnm_oracle.py ncf_predict_all_items) within the fp32
  tolerance of tests/parity.py.
* The fused top-k equals the (score desc, item asc) order of those dense rows exactly, filtered
  and unfiltered, k = 12 and k = 64, and the per-pair route's lists; over the full catalogue
  (many partitions); item shards merge to the unsharded lists.
* Towers wider than 128 stay on the per-pair kernel.
"""
import numpy as np
import pytest
import torch

from oracle import hnm_oracle as O
from parity import assert_scores_close
from hnm_recommendation_amd import NeuralCF, _lib
from hnm_recommendation_amd import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda"

TOWERS = [  # (mf, mlp_dims)
    (64, (256, 128, 64)),        # d1 = 128, two output tiles: the golden's tower
    (64, (256, 128, 128, 16)),   # a 128 -> 128 layer (4 tiles in and out), 16x16x4 last, K = 128
    (20, (200, 100, 72, 40)),    # odd widths above 64; mf padded
    (128, (192, 96, 128, 8)),    # a layer that widens, mf 128: the largest LDS footprint
    (32, (256, 128)),            # a single Linear 128 wide: no MFMA layer, 128-unit prediction
    (100, (160, 80, 48)),        # two tiles with mf padded to 128 (the remaining instantiation)
]


def model(U, I, mf, dims, seed):
    sd = syn.ncf_state_dict(U, I, mf, dims, seed=seed, bias_scale=0.05, emb_scale=8.0)
    m = NeuralCF(U, I, mf_dim=mf, mlp_dims=list(dims))
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return m.to(DEV).eval(), sd


def per_pair(fn):
    """Run fn with the per-pair LDS kernel (and the dense-chunk top-k) forced."""
    _lib.set_option(DEV, _lib.HNM_OPT_DEEP_MFMA, 0)
    try:
        return fn()
    finally:
        _lib.set_option(DEV, _lib.HNM_OPT_DEEP_MFMA, 1)


def exact(fn):
    """Run fn with the certified pre-filter off (the exact deep kernels everywhere)."""
    _lib.set_prefilter(DEV, False)
    try:
        return fn()
    finally:
        _lib.set_prefilter(DEV, True)


def topk_order(scores, k):
    """(score desc, item asc) per row -- the library's total order."""
    idx = np.empty((scores.shape[0], k), np.int64)
    items = np.arange(scores.shape[1])
    for b in range(scores.shape[0]):
        idx[b] = np.lexsort((items, -scores[b].astype(np.float64)))[:k]
    return idx, np.take_along_axis(scores, idx, 1)


@pytest.mark.parametrize("mf,dims", TOWERS)
@pytest.mark.parametrize("B", [37, 300])
def test_wide_mfma_bitwise_and_fused_topk(mf, dims, B):
    U, I, K = 700, 3001, 12
    m, sd = model(U, I, mf, dims, seed=len(dims) + mf)
    assert not m._fused()
    assert m.scoring_route() == "mfma"
    assert per_pair(m.scoring_route) == "per_pair"
    users_np = syn.user_batch(U, B, seed=B)
    users = torch.from_numpy(users_np).to(DEV)
    fast = m.predict_all_items(users)
    slow = per_pair(lambda: m.predict_all_items(users))
    assert torch.equal(fast.view(torch.int32), slow.view(torch.int32)), "MFMA vs per-pair"
    dense = fast.cpu().numpy()
    # every row (B = 37) / every 4th row and the last (B = 300) against the oracle
    rows = list(range(B)) if B <= 64 else list(range(0, B, 4)) + [B - 1]
    assert_scores_close(dense[rows], O.ncf_predict_all_items(sd, users_np[rows]), "wide oracle")

    ref_i, ref_v = topk_order(dense, K)
    v, i = m.recommend_with_scores(users, k=K)
    np.testing.assert_array_equal(i.cpu().numpy(), ref_i)
    np.testing.assert_array_equal(v.cpu().numpy().view(np.int32), ref_v.view(np.int32))
    v2, i2 = per_pair(lambda: m.recommend_with_scores(users, k=K))
    assert torch.equal(i2, i) and torch.equal(v2.view(torch.int32), v.view(torch.int32))

    # history filter: each row's current top-3 plus random items, every 3rd row
    rng = np.random.default_rng(B)
    filt = {}
    for b in range(0, B, 3):
        u = int(users_np[b])
        filt.setdefault(u, set()).update(int(x) for x in ref_i[b, :3])
        filt[u].update(int(x) for x in rng.integers(0, I, 40))
    masked = dense.copy()
    for b in range(B):
        for it in filt.get(int(users_np[b]), ()):
            masked[b, it] = -np.inf
    ref_i, ref_v = topk_order(masked, K)
    v, i = m.recommend_with_scores(users, filter_items=filt, k=K)
    np.testing.assert_array_equal(i.cpu().numpy(), ref_i)
    np.testing.assert_array_equal(v.cpu().numpy().view(np.int32), ref_v.view(np.int32))
    v2, i2 = per_pair(lambda: m.recommend_with_scores(users, filter_items=filt, k=K))
    assert torch.equal(i2, i) and torch.equal(v2.view(torch.int32), v.view(torch.int32))
    # k = 64, the fused path's maximum
    ref_i, _ = topk_order(dense, 64)
    np.testing.assert_array_equal(m.recommend_with_scores(users, k=64)[1].cpu().numpy(), ref_i)


def test_wide_mfma_full_catalogue_topk():
    """[256,128,64] over the full H&M catalogue (105,542 items, many partitions) at B = 256: the
    fused top-12 equals the per-pair route's lists bitwise; oracle rows agree."""
    U, I, B = 3000, syn.HM_ITEMS, 256
    m, sd = model(U, I, 64, (256, 128, 64), seed=21)
    assert m.scoring_route() == "mfma"
    users_np = syn.user_batch(U, B, seed=4)
    users = torch.from_numpy(users_np).to(DEV)
    v, i = m.recommend_with_scores(users)
    v2, i2 = per_pair(lambda: m.recommend_with_scores(users))
    assert torch.equal(i, i2) and torch.equal(v.view(torch.int32), v2.view(torch.int32))
    rows = list(range(0, B, 32)) + [B - 1]  # 9 rows x 105,542 items
    ref = O.ncf_predict_all_items(sd, users_np[rows])
    got = m.predict_all_items(users[rows]).cpu().numpy()
    assert_scores_close(got, ref, "wide full-catalogue rows")


def test_wide_item_shards_merge_to_the_unsharded_topk():
    """Item-sharded [256,128,64] (sharding.ncf_shard_topk -> ncf_deep_shard_topk on shard tables,
    ragged shards, with and without the history filter): the shards' lists merged by
    hnm_topk_merge_f32 are bitwise the unsharded fused top-k."""
    from hnm_recommendation_amd import sharding as S
    from hnm_recommendation_amd import UserHistory
    U, I, K, B = 900, 7001, 12, 260
    m, _ = model(U, I, 64, (256, 128, 64), seed=8)
    assert m.scoring_route() == "mfma"
    users_np = syn.user_batch(U, B, seed=5)
    users = torch.from_numpy(users_np).to(DEV)
    rng = np.random.default_rng(2)
    filt = {int(u): set(int(x) for x in rng.integers(0, I, 30)) for u in users_np[::4]}
    hist = UserHistory(filt, U, I, torch.device(DEV))
    for f, h in ((None, None), (filt, hist)):
        full_v, full_i = m.recommend_with_scores(users, filter_items=f, k=K)
        vs, is_ = [], []
        for r in range(3):
            lo, hi = S.shard_range(I, r, 3)
            sc = S.ncf_shard_topk(m, lo, hi, K, history=h)
            assert isinstance(sc, S.ncf_deep_shard_topk)
            v, i = sc(users)
            vs.append(v)
            is_.append(torch.where(i >= 0, i + lo, i))
        mv, mi = S.hip_merge(torch.stack(vs).contiguous(), torch.stack(is_).contiguous(), K)
        assert torch.equal(mi, full_i)
        assert torch.equal(mv.view(torch.int32), full_v.view(torch.int32))


def test_wider_than_128_stays_per_pair():
    """(512, 256, 64): a 256-wide layer is out of the matrix pipe's range; the route query says so
    with the option at its default, and the rows still match the oracle."""
    U, I, B = 700, 3001, 37
    m, sd = model(U, I, 32, (512, 256, 64), seed=6)
    assert m.scoring_route() == "per_pair"
    users_np = syn.user_batch(U, B, seed=B)
    users = torch.from_numpy(users_np).to(DEV)
    dense = m.predict_all_items(users).cpu().numpy()
    assert_scores_close(dense, O.ncf_predict_all_items(sd, users_np), "512-wide oracle")
