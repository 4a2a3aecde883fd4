"""PopularityBaseline on the GPU, measured (GPU only; not a test):

    python tools/popularity_bench.py [--out profiles/popularity_bench.txt] [--rounds 7]

(a) recommend_with_scores at B = 4,096, I = 105,542, K = 12, ~23 history items a user
    (`synthetic.filter_dict`, held as a device `UserHistory`): hnm_popularity_topk_f32 against
    the route the package had before it -- order_val scattered into a [B, I] matrix, then
    `dense_topk` with the same mask (also timed without the scatter, on a matrix built once).
    Ids and score bits are asserted equal before anything is timed.
(b) the fit at n = 31,788,324 rows, I = 105,542, 734 days, time_decay = 0.01 (days_ago
    descending, as in a transaction file sorted by date): hnm_popularity_fit_f64 against a
    torch restatement on the same GPU -- bincount over item * D + day, then a float64 matvec.
    Counts are asserted equal, pop within float64 summation error.

Each side is warmed up, then timed in interleaved rounds (order alternating) of at least
`--steps` calls (and ~50 ms) between device synchronisations; medians and the spread of the
per-round means are reported.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
from hnm_recommendation_amd import PopularityBaseline, UserHistory, _lib  # noqa: E402
from hnm_recommendation_amd import synthetic as syn  # noqa: E402
from hnm_recommendation_amd.models.base import dense_topk  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(R, "profiles", "popularity_bench.txt"))
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--fit-steps", type=int, default=3)
ap.add_argument("--rows", type=int, default=syn.HM_INTERACTIONS)
args = ap.parse_args()

if not torch.cuda.is_available():
    raise SystemExit("popularity_bench needs an AMD GPU: there is no CPU path")
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def interleaved(sides, steps, rounds, warm=3):
    """{name: [ms per call, one per round]}: every round times each side (order alternating)."""
    res = {n: [] for n in sides}
    reps = {}
    for n, f in sides.items():
        for _ in range(warm):
            f()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            f()
        torch.cuda.synchronize()
        # a timed window of at least ~50 ms, so that the clock and the scheduler do not show
        per = (time.perf_counter() - t0) / steps
        reps[n] = int(min(5000, max(steps, 0.05 / max(per, 1e-7))))
    for rnd in range(rounds):
        names = list(sides)[::-1] if rnd % 2 else list(sides)
        for n in names:
            f = sides[n]
            f()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps[n]):
                f()
            torch.cuda.synchronize()
            res[n].append((time.perf_counter() - t0) / reps[n] * 1e3)
    return res


def report(title, res, base):
    say(title)
    med = {n: statistics.median(v) for n, v in res.items()}
    for n, v in res.items():
        say(f"  {n:<44s} median {med[n]:9.4f} ms/call  (min {min(v):.4f}, max {max(v):.4f}, "
            f"{len(v)} rounds)  {med[base] / med[n]:7.2f}x vs {base}")
    return med


# ------------------------------------------------------------------ (a) top-K
I, B, K, RANKED = syn.HM_ITEMS, 4096, 12, 90_000
rng = np.random.Generator(np.random.PCG64(11))
order = rng.permutation(I)[:RANKED].astype(np.int64)
weights = np.arange(RANKED, 0, -1).astype(np.float32)          # distinct: one valid order
m = PopularityBaseline(I, k=K).to(dev).set_popular_items(order, weights)
users = syn.user_batch(syn.HM_USERS, B, seed=100)
h = syn.filter_dict(users, I, per_user=23, seed=3)
for j, u in enumerate(users[:256]):                              # histories inside the top
    h[int(u)] |= set(order[:j % 40 + 1].tolist())
hist = UserHistory(h, syn.HM_USERS, I, dev)
u = torch.from_numpy(users).to(dev)
scores = torch.full((B, I), float("-inf"), dtype=torch.float32, device=dev)


def scatter():
    scores.fill_(float("-inf"))
    scores[:, m.order] = m.order_val
    return scores


def new_route():
    return m.recommend_with_scores(u, filter_items=hist, k=K)


def dense_route(build=True):
    s = scatter() if build else scores
    mptr, midx = hist.mask_for(u)
    return dense_topk(s, K, mptr, midx)


pv, pi = new_route()
dv, di = dense_route()
assert torch.equal(pi, di) and torch.equal(pv.view(torch.int32), dv.view(torch.int32))
_lib.sync_check(dev)
say(f"(a) recommend_with_scores: B = {B}, I = {I}, K = {K}, {RANKED} ranked items, "
    f"{sum(len(h[int(x)]) for x in users) / B:.1f} history items a user "
    f"(ids and score bits equal on both routes)")
report("", interleaved({"hnm_popularity_topk_f32 (new)": new_route,
                        "scatter [B, I] + dense_topk (before)": dense_route,
                        "dense_topk alone, matrix built once": lambda: dense_route(False)},
                       args.steps, args.rounds), "scatter [B, I] + dense_topk (before)")
del scores

# ------------------------------------------------------------------ (b) fit
n, D, decay = args.rows, 734, 0.01
_, items_np = syn.interactions(syn.HM_USERS, I, n, seed=2)
days_np = np.sort(np.random.Generator(np.random.PCG64(12)).integers(0, D, size=n))[::-1]
items = torch.from_numpy(items_np).to(dev)
days = torch.from_numpy(np.ascontiguousarray(days_np.astype(np.int32))).to(dev)
w = torch.from_numpy(np.exp(-decay * np.arange(D))).to(dev)
count = torch.empty(I, dtype=torch.int64, device=dev)
pop = torch.empty(I, dtype=torch.float64, device=dev)
del items_np, days_np


def hip_fit():
    _lib.check(_lib.fn("hnm_popularity_fit_f64")(_lib.ctx(dev), _lib.ptr(items), n, _lib.ptr(days),
                                                 _lib.ptr(w), I, D, 0, _lib.ptr(count),
                                                 _lib.ptr(pop)), "hnm_popularity_fit_f64")
    return count, pop


def torch_fit():
    cnt = torch.bincount(items * D + days, minlength=I * D).view(I, D)
    return cnt.sum(1), cnt.to(torch.float64) @ w


fm = PopularityBaseline(I, time_decay=decay).to(dev)


def model_fit():
    return fm.fit_interactions(items, days_ago=days, window_days=D)


c1, p1 = hip_fit()
c2, p2 = torch_fit()
assert torch.equal(c1, c2)
assert torch.allclose(p1, p2, rtol=1e-12, atol=0.0)
_lib.sync_check(dev)
p1 = p1.clone()
assert torch.equal(hip_fit()[1].view(torch.int64), p1.view(torch.int64))     # same bits again
del c2, p2
say(f"(b) fit: n = {n}, I = {I}, {D} days, time_decay = {decay} (counts equal, pop within "
    f"1e-12 of the torch sum, same bits on a second run)")
report("", interleaved({"hnm_popularity_fit_f64 (new)": hip_fit,
                        "torch bincount + f64 matvec": torch_fit,
                        "fit_interactions (fit + sort + tables)": model_fit},
                       args.fit_steps, args.rounds, warm=1), "torch bincount + f64 matvec")

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
