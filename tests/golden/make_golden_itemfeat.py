"""Golden fixtures for Wide&Deep catalogue scoring WITH item features, from the REFERENCE.

Run in the build container only (like make_golden.py, whose stubs and save helpers it uses):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_itemfeat.py

The reference's `predict_all_items` passes `item_features=None` (`wide_deep.py:275`), which a
model with item features cannot run.  What such a model computes for a catalogue is its
`forward` over every (user, item) pair with `item_features = table[item]`: that is what is
stored, in 500-item chunks like `predict_all_items` (`:254-276`), as `dense [B, I]` with the
top-12 record of make_golden.py, the inputs (`user_ids`, `user_features`, `item_table`) and the
state dict.

4,200 items: just over the certified scan's floor of 4,096, with a partial 32-item tile; 9
users leave partial user blocks.
"""
from __future__ import annotations

import numpy as np
import torch

from make_golden import (_topk_record, install_stubs, load, save, syn, tagged_users,
                         with_prefix)

U, I, D, B, K = 3000, 4200, 16, 9, 12
CASES = (("widedeep_itemfeat_all_a.npz", 6, 5, (48, 100, 50), 31),
         ("widedeep_itemfeat_all_b.npz", 0, 5, (48, 20), 41))


def all_pairs(m, users, uf, table, chunk=500):
    out = []
    with torch.no_grad():
        for s in range(0, I, chunk):
            e = min(s + chunk, I)
            n = e - s
            eu = torch.from_numpy(np.repeat(users, n))
            ei = torch.from_numpy(np.tile(np.arange(s, e), len(users)))
            ef = None if uf is None else torch.from_numpy(np.repeat(uf, n, axis=0))
            eif = torch.from_numpy(table[ei.numpy()])
            out.append(m(eu, ei, ef, eif).numpy().reshape(len(users), n))
    return np.concatenate(out, axis=1)


def gen(models):
    for name, Fu, Fi, layers, seed in CASES:
        sd = syn.widedeep_state_dict(U, I, D, layers, num_user_features=Fu, num_item_features=Fi,
                                     seed=seed, bias_scale=0.05, randomize_bn=True,
                                     emb_scale=10.0)
        m = load(models.WideDeep(num_users=U, num_items=I, num_user_features=Fu,
                                 num_item_features=Fi, embedding_dim=D,
                                 deep_layers=list(layers), top_k=K), sd)
        rng = np.random.Generator(np.random.PCG64(seed + 1))
        users = tagged_users(U, B, seed=seed + 2)
        uf = rng.standard_normal((B, Fu)).astype(np.float32) if Fu else None
        table = rng.standard_normal((I, Fi)).astype(np.float32)
        dense = all_pairs(m, users, uf, table)
        rec = np.asarray(torch.topk(torch.from_numpy(dense), K, dim=1)[1])
        srt = -np.sort(-dense, axis=1)
        tol = 1e-4 * np.abs(dense).max(1)
        print(f"{name}: smallest K-th gap / tol = {((srt[:, K - 1] - srt[:, K]) / tol).min():.2f}")
        save(name, U=U, I=I, K=K, Fu=Fu, Fi=Fi, d=D, deep_layers=np.array(layers), dense=dense,
             user_features=np.zeros((B, 0), np.float32) if uf is None else uf, item_table=table,
             **_topk_record(dense, rec, users, 0), **with_prefix("sd/", sd))


if __name__ == "__main__":
    torch.manual_seed(0)
    torch.set_num_threads(8)
    gen(install_stubs())
