"""SegmentPopularity on the GPU, measured (GPU only; not a test):

    python tools/segpop_bench.py [--out profiles/segpop_bench.txt] [--rounds 5]

Synthetic H&M shape: n = 31,788,324 transactions, 734 days (days_ago descending, as in a
transaction file sorted by date), I = 105,542 items, 1,371,980 users, S = 12 segments (a tenth of
the users without one), time_decay = 0.01.

(a) the fit: hnm_segpop_fit_f64 next to hnm_popularity_fit_f64 on the same transactions (the
    baseline does one segment's worth of work: the global row), and `fit_interactions` (the fit
    + id check + the S + 1 sorts and rank rows).  Row S is asserted bitwise the baseline's, the
    segment counts equal to a torch bincount, and a second run the same bits.
(b) the top-K call on the fitted tables, B = 4,096, K = 12, random request segments in
    [-1, S), ~23 history items a row as a CSR built once: hnm_segpop_topk_f32 next to
    hnm_popularity_topk_f32 over the global order with the same mask, the two modules'
    `recommend_with_scores` for known users (each gathers its mask from a device `UserHistory`
    per call), and a torch dense route on the same GPU: float32 `pop[seg]` gathered to [B, I],
    the mask scattered in as -inf, `torch.topk`.  The dense route gives a segment's own list
    only (no continuation from the global one); the share of rows on which its ids equal the
    kernel's is reported, not asserted (ties at the cut are torch's to break).

Each side is warmed up, then timed in interleaved rounds (order alternating) of at least
`--steps` calls (and ~50 ms) between device synchronisations, host clock; medians and the
spread of the per-round means are reported.
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
from hnm_recommendation_amd import (PopularityBaseline, SegmentPopularity, UserHistory,  # noqa: E402
                                    _lib)
from hnm_recommendation_amd import synthetic as syn  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(R, "profiles", "segpop_bench.txt"))
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--fit-steps", type=int, default=3)
ap.add_argument("--rows", type=int, default=syn.HM_INTERACTIONS)
args = ap.parse_args()

if not torch.cuda.is_available():
    raise SystemExit("segpop_bench needs an AMD GPU: there is no CPU path")
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


def report(res, base):
    med = {n: statistics.median(v) for n, v in res.items()}
    for n, v in res.items():
        say(f"  {n:<52s} median {med[n]:9.4f} ms/call  (min {min(v):.4f}, max {max(v):.4f}, "
            f"{len(v)} rounds)  {med[n] / med[base]:7.2f}x {base}")
    return med


# ------------------------------------------------------------------ (a) fit
I, U, S, B, K = syn.HM_ITEMS, syn.HM_USERS, 12, 4096, 12
n, D, decay = args.rows, 734, 0.01
users_np, items_np = syn.interactions(U, I, n, seed=2)
rng = np.random.Generator(np.random.PCG64(12))
days_np = np.sort(rng.integers(0, D, size=n))[::-1]
useg_np = rng.integers(0, S, size=U).astype(np.int32)
useg_np[rng.random(U) < 0.1] = -1
items = torch.from_numpy(items_np).to(dev)
users = torch.from_numpy(users_np).to(dev)
days = torch.from_numpy(np.ascontiguousarray(days_np.astype(np.int32))).to(dev)
useg = torch.from_numpy(useg_np).to(dev)
w = torch.from_numpy(np.exp(-decay * np.arange(D))).to(dev)
count = torch.empty(S + 1, I, dtype=torch.int64, device=dev)
pop = torch.empty(S + 1, I, dtype=torch.float64, device=dev)
bcount = torch.empty(I, dtype=torch.int64, device=dev)
bpop = torch.empty(I, dtype=torch.float64, device=dev)
del items_np, users_np, days_np


def seg_fit():
    _lib.call("hnm_segpop_fit_f64", _lib.ctx(dev), _lib.ptr(items), _lib.ptr(users), n,
              _lib.ptr(useg), U, _lib.ptr(days), _lib.ptr(w), I, S, D, 0, _lib.ptr(count),
              _lib.ptr(pop))


def base_fit():
    _lib.call("hnm_popularity_fit_f64", _lib.ctx(dev), _lib.ptr(items), n, _lib.ptr(days),
              _lib.ptr(w), I, D, 0, _lib.ptr(bcount), _lib.ptr(bpop))


model = SegmentPopularity(I, S, k=K, time_decay=decay).to(dev)
base = PopularityBaseline(I, k=K, time_decay=decay).to(dev)


def model_fit():
    model.fit_interactions(items, users, useg, days_ago=days, window_days=D)


def base_model_fit():
    base.fit_interactions(items, days_ago=days, window_days=D)


seg_fit()
base_fit()
_lib.sync_check(dev)
assert torch.equal(count[S], bcount) and torch.equal(pop[S].view(torch.int64), bpop.view(torch.int64))
s_of = useg[users].to(torch.int64)
known = s_of >= 0
assert torch.equal(torch.bincount(s_of[known] * I + items[known], minlength=S * I).view(S, I),
                   count[:S])
p1 = pop.clone()
seg_fit()
assert torch.equal(pop.view(torch.int64), p1.view(torch.int64))
del s_of, known, p1
slab = max(1, (256 << 20) // ((S + 1) * I * 4))
say(f"(a) fit: n = {n}, I = {I}, U = {U}, S = {S}, {D} days, time_decay = {decay}; "
    f"[slab, S + 1, I] int32 table: slab = {slab} days, {-(-D // slab)} passes over the "
    f"transactions (the baseline: slab = {(256 << 20) // (I * 4)}, "
    f"{-(-D // ((256 << 20) // (I * 4)))} passes); row S bitwise the baseline's, segment counts "
    f"equal to a torch bincount, same bits on a second run")
report(interleaved({"hnm_popularity_fit_f64 (baseline, global row only)": base_fit,
                    "hnm_segpop_fit_f64": seg_fit,
                    "PopularityBaseline.fit_interactions": base_model_fit,
                    "SegmentPopularity.fit_interactions (fit + 13 sorts)": model_fit},
                   args.fit_steps, args.rounds, warm=1),
       "hnm_popularity_fit_f64 (baseline, global row only)")
del items, users, days

# ------------------------------------------------------------------ (b) top-K
# on the tables the timed fit_interactions calls left in the two models
lens = (model.order_ptr[1:] - model.order_ptr[:-1]).cpu().tolist()
batch = syn.user_batch(U, B, seed=100)
h = syn.filter_dict(batch, I, per_user=23, seed=3)
g0 = int(model.order_ptr[S])
top = model.order[g0:g0 + 64].cpu().tolist()
for j, u in enumerate(batch[:256]):                              # histories inside the top
    h[int(u)] |= set(top[:j % 40 + 1])
hist = UserHistory(h, U, I, dev)
u = torch.from_numpy(batch).to(dev)
mptr, midx = hist.mask_for(u)
seg = torch.from_numpy(rng.integers(-1, S, size=B).astype(np.int32)).to(dev)
ov = torch.empty(B, K, dtype=torch.float32, device=dev)
oi = torch.empty(B, K, dtype=torch.int64, device=dev)
on = torch.empty(B, dtype=torch.int32, device=dev)
bv, bi = torch.empty_like(ov), torch.empty_like(oi)


def seg_topk(s=seg):
    _lib.call("hnm_segpop_topk_f32", _lib.ctx(dev), _lib.ptr(model.order),
              _lib.ptr(model.order_val), _lib.ptr(model.order_ptr), _lib.ptr(model.rank), I, S,
              _lib.ptr(s), _lib.ptr(mptr), _lib.ptr(midx), B, K, 0, _lib.ptr(ov), _lib.ptr(oi),
              _lib.ptr(on))


def base_topk():
    _lib.call("hnm_popularity_topk_f32", _lib.ctx(dev), _lib.ptr(base.order),
              _lib.ptr(base.order_val), base.order.numel(), _lib.ptr(base.rank), I, _lib.ptr(mptr),
              _lib.ptr(midx), B, K, 0, _lib.ptr(bv), _lib.ptr(bi))


pop32 = model.pop.to(torch.float32)
rows_of = torch.repeat_interleave(torch.arange(B, device=dev), mptr[1:] - mptr[:-1])
cols_of = midx[:int(mptr[-1])].to(torch.int64)
seg_row = torch.where(seg < 0, torch.full_like(seg, S), seg).to(torch.int64)


def dense_route():
    scores = pop32[seg_row]                                      # [B, I] gathered
    scores[rows_of, cols_of] = float("-inf")
    return torch.topk(scores, K, dim=1)


base_topk()
seg_topk(torch.full_like(seg, -1))
assert torch.equal(oi, bi) and torch.equal(ov.view(torch.int32), bv.view(torch.int32))
seg_topk()
_lib.sync_check(dev)
same = (dense_route()[1] == oi).all(1).float().mean().item()
say(f"(b) top-K: B = {B}, K = {K}, I = {I}, S = {S}; order lengths {lens[:S]} and "
    f"{lens[S]} (global); {int(mptr[-1]) / B:.1f} history items a row; rows with a segment "
    f"{(seg >= 0).float().mean().item():.3f}, mean out_nseg {on.float().mean().item():.2f}; "
    f"with every row at -1 the output is bitwise hnm_popularity_topk_f32's; the dense route's "
    f"ids equal the kernel's on {same:.4f} of the rows")
report(interleaved({"hnm_popularity_topk_f32 (baseline, same mask)": base_topk,
                    "hnm_segpop_topk_f32": seg_topk,
                    "PopularityBaseline.recommend_with_scores": lambda: base.recommend_with_scores(
                        u, filter_items=hist, k=K),
                    "SegmentPopularity.recommend_with_scores": lambda: model.recommend_with_scores(
                        u, filter_items=hist, k=K),
                    "torch: pop[seg] -> [B, I], mask, topk": dense_route},
                   args.steps, args.rounds), "hnm_popularity_topk_f32 (baseline, same mask)")

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
