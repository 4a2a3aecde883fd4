"""Golden fixture for PopularityBaseline, from the REFERENCE (`src/models/baseline.py`).

Run in the build container only (like make_golden.py, whose stubs and save helper it uses;
it needs pandas):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_popularity.py

Seeded synthetic transactions (user, item, day): 300 items of which 80 are never bought, 200
users, 20,000 rows, items Zipf-distributed as in `synthetic.interactions`, days_ago uniform in
[0, 90).  User HEAVY has bought the entire top 40 of both fitted orders (their window of the
order must extend past k), user NOHIST has no row.

Recorded, for time_decay in {0, 0.02} (tags d0 / d1): the reference's per-item popularity (the
Series its `fit_popularity` sorts, captured as it reaches `sort_values`, stored dense with 0 for
items never bought), its `item_popularity` order, and `recommend()` for a user batch,
personalized and not, k in {5, 12}.  Inputs and recorded outputs only.
"""
from __future__ import annotations

import numpy as np
import pandas as pd

from make_golden import install_stubs, save, syn

I, BOUGHT, U, N, DAYS = 300, 220, 200, 20_000, 90
HEAVY, NOHIST, TOP = 0, U - 1, 40
DECAYS = (("d0", 0.0), ("d1", 0.02))
KS = (5, 12)


def frame(users, items, days):
    base = pd.Timestamp("2020-09-22")
    return pd.DataFrame({"customer_idx": users, "article_idx": items,
                         "t_dat": base - pd.to_timedelta(days, unit="D")})


def ref_fit(models, df, decay, personalized):
    """(model, the popularity Series the reference sorted)."""
    m = models.PopularityBaseline(n_items=I, k=12, time_decay=decay, personalized=personalized)
    seen = []
    orig = pd.Series.sort_values

    def spy(self, *a, **kw):
        seen.append(self.copy())
        return orig(self, *a, **kw)

    pd.Series.sort_values = spy
    try:
        m.fit_popularity(df.copy())
    finally:
        pd.Series.sort_values = orig
    return m, seen[0]


def gen(models):
    rng = np.random.Generator(np.random.PCG64(77))
    users, ranks = syn.interactions(U - 1, BOUGHT, N, seed=71)       # users 0 .. U-2
    items = rng.permutation(I)[:BOUGHT][ranks].astype(np.int64)      # 80 ids never drawn
    days = rng.integers(0, DAYS, size=N).astype(np.int64)
    days[-1] = 0                                                     # the max date exists
    # HEAVY buys the whole top 40 of both orders: overwrite leading rows until that holds
    for _ in range(20):
        need = []
        for _, decay in DECAYS:
            m, _s = ref_fit(models, frame(users, items, days), decay, False)
            mine = set(items[users == HEAVY].tolist())
            need += [x for x in m.item_popularity[:TOP] if x not in mine and x not in need]
        if not need:
            break
        free = np.nonzero(users != HEAVY)[0][:len(need)]
        users[free] = HEAVY
        items[free] = need
    else:
        raise RuntimeError("the heavy user's history did not converge")
    assert not (users == NOHIST).any() and days.min() == 0 and days.max() == DAYS - 1
    assert np.unique(items).size <= BOUGHT

    batch = np.concatenate([[HEAVY, NOHIST], syn.user_batch(U - 1, 14, seed=72)]).astype(np.int64)
    out = {"I": I, "U": U, "users": users.astype(np.int32), "items": items.astype(np.int32),
           "days": days.astype(np.int32), "batch": batch, "heavy": HEAVY, "nohist": NOHIST}
    df = frame(users, items, days)
    for tag, decay in DECAYS:
        for pers, ptag in ((False, "np"), (True, "p")):
            m, s = ref_fit(models, df, decay, pers)
            if not pers:
                pop = np.zeros(I, np.float64)
                pop[s.index.to_numpy()] = s.to_numpy(dtype=np.float64)
                out[f"pop_{tag}"] = pop
                out[f"order_{tag}"] = np.asarray(m.item_popularity, np.int64)
                out[f"decay_{tag}"] = np.float64(decay)
                assert set(m.item_popularity[:TOP]) <= set(items[users == HEAVY].tolist())
            for k in KS:
                rec = m.recommend(batch.tolist(), k=k)
                rows = np.asarray([rec[int(u)] for u in batch], np.int64)
                assert rows.shape == (len(batch), k)
                out[f"rec_{tag}_{ptag}_k{k}"] = rows
    save("popularity_small.npz", **out)


if __name__ == "__main__":
    gen(install_stubs())
