"""SequentialCF on the GPU, measured (GPU only; not a test):

    python tools/seqcf_bench.py [--out profiles/seqcf_bench.txt] [--rounds 5]

At the synthetic H&M shape (U = 1,371,980, I = 105,542, 31,788,324 transactions over 734 days,
N = 64).  The (user, item) pairs are `synthetic.interactions`' (the ItemCF benchmark's); the days
are drawn here: every user gets `--visits` shopping days, uniform over the 734, and each
transaction falls on one of its user's visits -- so a user's purchases come in same-day baskets,
as real ones do, but the spacing of the visits is uniform, which real ones are not.

(a) the fit, hnm_seqcf_fit_f32, at max_gap 7 / 28 / 90 (default window) and at max_gap 28 with
    8,192 counters a pass, beside hnm_itemcf_fit_f32 and hnm_itemcf_fit_weighted_f32 on the same
    transactions in the same process: the yardstick.  Printed with it: the events, the mean
    forward-range length at each max_gap, the window count, and the two work terms -- windows x
    sum of forward-range lengths (every pass re-reads every range) against ItemCF's sum over
    users of history length squared.
(b) a torch restatement of the max_gap 28 fit on the same GPU: for shift k = 1, 2, ... pair
    seq[p] with seq[p + k] where the user matches and the gap qualifies, accumulate gap_q by key
    a * I + b (`unique` + `index_add_`), sim in float64, then the row top-64 by sorting.  The
    tables are compared before anything is timed.
(c) recommend_with_scores for 4,096 users, K = 12, history filter.

Each side is warmed up, then timed in interleaved rounds (order alternating) between device
synchronisations; medians and the spread of the per-round means are reported.
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
from hnm_recommendation_amd import (ItemCF, SequentialCF, UserHistory, UserSequence,  # noqa: E402
                                    WeightedItemCF, _lib)
from hnm_recommendation_amd import synthetic as syn  # noqa: E402
from hnm_recommendation_amd.models.sequential_cf import gap_table  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(R, "profiles", "seqcf_bench.txt"))
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--fit-steps", type=int, default=2)
ap.add_argument("--rows", type=int, default=syn.HM_INTERACTIONS)
ap.add_argument("--days", type=int, default=734)
ap.add_argument("--visits", type=int, default=8)
ap.add_argument("--gap-decay", type=float, default=0.05)
args = ap.parse_args()

if not torch.cuda.is_available():
    raise SystemExit("seqcf_bench needs an AMD GPU: there is no CPU path")
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def write_out():
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


def interleaved(sides, steps, rounds, warm=1):
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


def report(title, res, base):
    if title:
        say(title)
    med = {n: statistics.median(v) for n, v in res.items()}
    for n, v in res.items():
        say(f"  {n:<52s} median {med[n]:10.4f} ms/call  (min {min(v):.4f}, max {max(v):.4f}, "
            f"{len(v)} rounds)  {med[n] / med[base]:8.2f}x the time of {base}")
    return med


U, I, N, B, K = syn.HM_USERS, syn.HM_ITEMS, 64, 4096, 12
GAPS = (7, 28, 90)
users_np, items_np = syn.interactions(U, I, args.rows, seed=2)
rng = np.random.Generator(np.random.PCG64(17))
visit_day = rng.integers(0, args.days, size=(U, args.visits), dtype=np.int16)
days_np = visit_day[users_np, rng.integers(0, args.visits, size=args.rows)].astype(np.int64)
del visit_day
seq = UserSequence.from_interactions(users_np, items_np, days_np, U, I, dev)
whist = UserHistory.from_interactions(users_np, items_np, U, I, dev,
                                      weights=np.ones(args.rows, np.float64))
hist = UserHistory.from_interactions(users_np, items_np, U, I, dev)
say(f"data: U = {U}, I = {I}, {args.rows} transactions over {args.days} days, {args.visits} "
    f"visits a user; {seq.nnz} events (distinct user, day, item), longest sequence {seq.max_len}; "
    f"{hist.nnz} distinct (user, item) pairs, longest history {hist.max_len}")

# the two work terms, on the host
ptr = seq.seq_ptr.cpu().numpy()
day = seq.seq_day.cpu().numpy()[:seq.nnz].astype(np.int64)
big = int(day.max(initial=0)) + max(GAPS) + 2
key = np.repeat(np.arange(U, dtype=np.int64), np.diff(ptr)) * big + day   # ascending
lo = np.searchsorted(key, key, side="right")
hlen = np.diff(hist.hist_ptr.cpu().numpy()).astype(np.float64)
cooc = float((hlen * hlen).sum())
windows = -(-I // 16384)
range_sum = {}
for G in GAPS:
    range_sum[G] = float((np.searchsorted(key, key + G, side="right") - lo).sum())
    say(f"      max_gap {G:3d}: mean forward range {range_sum[G] / seq.nnz:7.3f} events, "
        f"{windows} windows of 16,384: {windows * range_sum[G]:.3e} range reads; ItemCF's sum of "
        f"history length squared {cooc:.3e}: ratio {windows * range_sum[G] / cooc:.2f}")
del key, lo


def same_table(m, idx, val, cnt):
    return (torch.equal(m.neighbor_idx, idx) and torch.equal(m.item_count, cnt)
            and torch.equal(m.neighbor_val.view(torch.int32), val.view(torch.int32)))


# ------------------------------------------------------------------ (a) the fit
models = {G: SequentialCF(U, I, num_neighbors=N, max_gap=G, gap_decay=args.gap_decay).to(dev)
          for G in GAPS}
for G, m in models.items():
    m.fit_sequence(seq, whist)
ref = {G: (m.neighbor_idx.clone(), m.neighbor_val.clone(), m.item_count.clone())
       for G, m in models.items()}
for G, m in models.items():                                  # twice, and at another window
    m.fit_sequence(seq, whist)
    assert same_table(m, *ref[G]), G
models[28].fit_sequence(seq, whist, _window=8192)
assert same_table(models[28], *ref[28])
plain = ItemCF(U, I, num_neighbors=N).to(dev).fit_history(hist)
wcf = WeightedItemCF(U, I, num_neighbors=N).to(dev).fit_history(whist)
filled = {G: float((ref[G][0] >= 0).float().mean()) for G in GAPS}
say(f"(a) fit: N = {N}, gap_decay = {args.gap_decay}; each fit gives equal bits twice, max_gap 28 "
    "also at 8,192 counters a pass; neighbour slots filled: "
    + ", ".join(f"{filled[G] * 100:.1f} % at max_gap {G}" for G in GAPS)
    + f" (ItemCF: {float((plain.neighbor_idx >= 0).float().mean()) * 100:.1f} %)")
base = "hnm_itemcf_fit_weighted_f32 (window 16384)"
sides = {base: lambda: wcf.fit_history(whist),
         "hnm_itemcf_fit_f32 (window 16384)": lambda: plain.fit_history(hist)}
for G in GAPS:
    sides[f"hnm_seqcf_fit_f32, max_gap {G}"] = (lambda G=G: models[G].fit_sequence(seq, whist))
sides["hnm_seqcf_fit_f32, max_gap 28, window 8192"] = \
    lambda: models[28].fit_sequence(seq, whist, _window=8192)
fit_ms = report("", interleaved(sides, args.fit_steps, args.rounds), base)
write_out()

# ------------------------------------------------------------------ (b) torch, max_gap 28
G = 28
gq = torch.from_numpy(gap_table(G, args.gap_decay).astype(np.int64)).to(dev)
s_item = seq.seq_item[:seq.nnz].to(torch.int64)
s_day = seq.seq_day[:seq.nnz].to(torch.int64)
s_user = torch.repeat_interleave(torch.arange(U, device=dev), seq.seq_ptr[1:] - seq.seq_ptr[:-1])
shifts = [0]


def torch_fit():
    keys, ws = [], []
    k = 0
    while True:
        k += 1
        if k >= seq.nnz:
            break
        gap = s_day[k:] - s_day[:-k]
        ok = (s_user[k:] == s_user[:-k]) & (gap <= G)        # sorted by day: gap >= 0
        if not bool(ok.any()):                               # no later shift can qualify
            break
        ok &= (gap >= 1) & (s_item[k:] != s_item[:-k])
        keys.append(s_item[:-k][ok] * I + s_item[k:][ok])
        ws.append(gq[gap[ok] - 1])
    shifts[0] = k - 1
    uniq, inv = torch.unique(torch.cat(keys), return_inverse=True)
    T = torch.zeros(uniq.numel(), dtype=torch.int64, device=dev).index_add_(0, inv, torch.cat(ws))
    n = torch.bincount(s_item, minlength=I).to(torch.float64)
    a, b = uniq // I, uniq % I
    live = T > 0
    a, b, T = a[live], b[live], T[live]
    sim = (T.to(torch.float64) / (32768.0 * torch.sqrt(n[a] * n[b]))).to(torch.float32)
    order = torch.sort(sim, descending=True, stable=True).indices      # keys ascend: b ascending
    order = order[torch.sort(a[order], stable=True).indices]           # then by row, stably
    a, b, sim = a[order], b[order], sim[order]
    start = torch.searchsorted(a, torch.arange(I, device=dev))
    rank = torch.arange(a.numel(), device=dev) - start[a]
    keep = rank < N
    idx = torch.full((I, N), -1, dtype=torch.int32, device=dev)
    val = torch.zeros((I, N), dtype=torch.float32, device=dev)
    idx[a[keep], rank[keep]] = b[keep].to(torch.int32)
    val[a[keep], rank[keep]] = sim[keep]
    return idx, val


try:
    tidx, tval = torch_fit()
    eq_i = float((tidx == ref[G][0]).float().mean())
    eq_v = float((tval.view(torch.int32) == ref[G][1].view(torch.int32)).float().mean())
    say(f"(b) torch restatement at max_gap {G} (in one piece: not chunked; {shifts[0]} shifts): "
        f"{eq_i * 100:.4f} % of the neighbour ids and {eq_v * 100:.4f} % of the value bits equal "
        "hnm_seqcf_fit_f32's")
    assert eq_i > 0.999
    del tidx, tval
    name = f"torch shifts + unique + index_add_ + sort, max_gap {G}"
    kern = f"hnm_seqcf_fit_f32, max_gap {G}"
    report("", interleaved({name: torch_fit, kern: sides[kern]}, 1, min(args.rounds, 3)), name)
except Exception as e:  # noqa: BLE001
    say(f"(b) the torch restatement failed here: {type(e).__name__}: {e}")
write_out()

# ------------------------------------------------------------------ (c) top-K
m = models[28].fit_sequence(seq, whist)
ub = torch.from_numpy(syn.user_batch(U, B, seed=100)).to(dev)
x = m.recommend_with_scores(ub, filter_items=whist, k=K)
y = m.recommend_with_scores(ub, filter_items=whist, k=K)
assert torch.equal(x[1], y[1]) and torch.equal(x[0].view(torch.int32), y[0].view(torch.int32))
_lib.sync_check(dev)
say(f"(c) recommend_with_scores: B = {B}, K = {K}, history filter; "
    f"{m.scoring_route(ub).count('dense')} of {B} rows take the dense route; "
    f"{float((x[1] >= 0).float().mean()) * 100:.1f} % of the slots filled; equal bits twice")
basek = "WeightedItemCF (hnm_itemcf_topk_weighted_f32)"
report("", interleaved(
    {basek: lambda: wcf.recommend_with_scores(ub, filter_items=whist, k=K),
     "SequentialCF, max_gap 28 (the same entry)": lambda: m.recommend_with_scores(
         ub, filter_items=whist, k=K)}, args.steps, args.rounds, warm=3), basek)
write_out()
