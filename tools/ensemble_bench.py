"""The ensemble's fusion on the GPU, measured (GPU only; not a test):

    python tools/ensemble_bench.py [--out profiles/ensemble_bench.txt] [--rounds 5]

At the H&M shape (U = 1,371,980, I = 105,542, E = 31,788,324 synthetic interactions), B = 4,096
users, k = 12, depth 48, with the history filter:

(a) hnm_fuse_topk_f32 alone on the members' real lists, G = 2, 3, 4 (MatrixFactorization, ItemCF,
    PopularityBaseline, a second MatrixFactorization), in the three modes.
(b) the whole `Ensemble.recommend_with_scores` for MF + ItemCF + popularity, next to the three
    members' own calls (what the ensemble adds to them: the copies into one [G, B, depth] pair,
    one more mask gather, the fuse call).
(c) the same reciprocal rank fusion formed on the same GPU by torch: a [B, num_items] matrix of
    zeros, one scatter_add per list, -inf on the history, torch.topk.  The two answers are
    compared before anything is timed (ids where the fused scores are not tied; torch.topk
    leaves ties unspecified).  No ratio is required of it.

Each side is warmed up, then timed in interleaved rounds (order alternating) of at least
`--steps` calls (and ~50 ms) between device synchronisations; medians and the spread of the
per-round means are reported.
"""
import argparse
import os
import statistics
import sys
import time

import torch

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
from hnm_recommendation_amd import (Ensemble, ItemCF, MatrixFactorization,  # noqa: E402
                                    PopularityBaseline, _lib)
from hnm_recommendation_amd import synthetic as syn  # noqa: E402
from hnm_recommendation_amd.models.base import empty_rows  # noqa: E402
from hnm_recommendation_amd.models.ensemble import MODES  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(R, "profiles", "ensemble_bench.txt"))
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--rows", type=int, default=syn.HM_INTERACTIONS)
args = ap.parse_args()

if not torch.cuda.is_available():
    raise SystemExit("ensemble_bench needs an AMD GPU: there is no CPU path")
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


def report(title, res):
    say(title)
    med = {n: statistics.median(v) for n, v in res.items()}
    for n, v in res.items():
        say(f"  {n:<58s} median {med[n]:10.4f} ms/call  (min {min(v):.4f}, max {max(v):.4f}, "
            f"{len(v)} rounds)")
    return med


U, I, B, K, DEPTH = syn.HM_USERS, syn.HM_ITEMS, 4096, 12, 48
users_np, items_np = syn.interactions(U, I, args.rows, seed=2)


def mf(seed):
    m = MatrixFactorization(U, I, embedding_dim=64, sparse=False)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in
                       syn.mf_state_dict(U, I, 64, seed=seed, bias_scale=0.05).items()})
    return m.to(dev).eval()


icf = ItemCF(U, I, num_neighbors=64).to(dev)
icf.fit_interactions(users_np, items_np)
hist = icf.history
pop = PopularityBaseline(n_items=I).to(dev)
pop.fit_interactions(items_np)
members = [("mf", mf(5)), ("item_cf", icf), ("popularity", pop), ("mf2", mf(6))]
say(f"data: U = {U}, I = {I}, E = {args.rows} drawn, {hist.nnz} distinct (user, item) pairs; "
    f"B = {B}, k = {K}, depth = {DEPTH}, history filter")

u = torch.from_numpy(syn.user_batch(U, B, seed=100)).to(dev)
lists = [m.recommend_with_scores(u, hist, k=DEPTH) for _, m in members]
lv = torch.stack([v for v, _ in lists]).contiguous()
li = torch.stack([i for _, i in lists]).contiguous()
mptr, midx = hist.mask_for(u)
live = (li >= 0) & torch.isfinite(lv)
say("    live entries per list of " + str(DEPTH) + ": " + ", ".join(
    f"{n} {float(live[g].sum(1).float().mean()):.1f}" for g, (n, _) in enumerate(members)))

# ------------------------------------------------------------------ (a) the fuse call alone
out_v, out_i = empty_rows(B, K, dev)


def fuse_call(G, mode, coef):
    _lib.call("hnm_fuse_topk_f32", _lib.ctx(dev), _lib.ptr(lv), _lib.ptr(li), B, G, B * DEPTH,
              DEPTH, DEPTH, MODES[mode], _lib.ptr(coef), I, _lib.ptr(mptr), _lib.ptr(midx), K,
              _lib.ptr(out_v), _lib.ptr(out_i))


sides = {}
for G in (2, 3, 4):
    e = Ensemble(members[:G], depth=DEPTH)
    rank = e.rank_weights(DEPTH).to(dev).contiguous()
    ones = torch.ones(G, dtype=torch.float32, device=dev)
    for mode, coef in (("rrf", rank), ("score", ones), ("cascade", None)):
        f = (lambda G=G, mode=mode, coef=coef: fuse_call(G, mode, coef))
        f()
        first = (out_v.clone(), out_i.clone())
        f()
        assert torch.equal(first[1], out_i) and torch.equal(first[0].view(torch.int32),
                                                            out_v.view(torch.int32))
        sides[f"hnm_fuse_topk_f32 G = {G}, {mode}"] = f
_lib.sync_check(dev)
report(f"(a) the fuse call alone ([G, {B}, {DEPTH}] lists in, [{B}, {K}] out; equal bits twice)",
       interleaved(sides, args.steps, args.rounds))

# ------------------------------------------------------------------ (b) the module
ens = Ensemble(members[:3])
assert ens._depth(K) == DEPTH
got = ens.recommend_with_scores(u, filter_items=hist, k=K)
fuse_call(3, "rrf", ens.rank_weights(DEPTH).to(dev).contiguous())
assert torch.equal(got[1], out_i) and torch.equal(got[0].view(torch.int32), out_v.view(torch.int32))
sides = {"Ensemble.recommend_with_scores (mf + item_cf + popularity)":
         lambda: ens.recommend_with_scores(u, filter_items=hist, k=K),
         "the three members' own calls, k = depth":
         lambda: [m.recommend_with_scores(u, hist, k=DEPTH) for _, m in members[:3]]}
for n, m in members[:3]:
    sides[f"  {n}.recommend_with_scores, k = depth"] = \
        (lambda m=m: m.recommend_with_scores(u, hist, k=DEPTH))
report("(b) the whole call, device ids", interleaved(sides, args.steps, args.rounds))

# ------------------------------------------------------------------ (c) torch on the same GPU
coef3 = ens.rank_weights(DEPTH).to(dev)                       # [3, depth]
dense = torch.empty(B, I, dtype=torch.float32, device=dev)
rows_of_mask = torch.repeat_interleave(torch.arange(B, device=dev), mptr[1:] - mptr[:-1])
mask_items = midx[:rows_of_mask.numel()].to(torch.int64)


def torch_route():
    dense.zero_()
    for g in range(3):
        add = torch.where(live[g], coef3[g].expand(B, DEPTH), torch.zeros((), device=dev))
        dense.scatter_add_(1, li[g].clamp(min=0), add)
    dense[rows_of_mask, mask_items] = float("-inf")
    return torch.topk(dense, K, dim=1)


tv, ti = torch_route()
untied = torch.ones_like(got[0], dtype=torch.bool)
untied[:, 1:] &= got[0][:, 1:] != got[0][:, :-1]
untied[:, :-1] &= got[0][:, :-1] != got[0][:, 1:]
untied[:, -1] = False                                         # the cut may fall inside a tie
same = float((ti[untied] == got[1][untied]).float().mean())
close = float(torch.isclose(tv, got[0], rtol=1e-5, atol=0.0).float().mean())
say(f"(c) torch route: {close * 100:.3f} % of the scores within 1e-5, {same * 100:.3f} % of the "
    f"untied ids equal ({float(untied.float().mean()) * 100:.1f} % of the slots are untied)")
assert close > 0.999 and same > 0.999
report("", interleaved(
    {"hnm_fuse_topk_f32 G = 3, rrf": lambda: fuse_call(3, "rrf", coef3),
     f"[B, I] zeros + 3 scatter_add + history -inf + torch.topk({K})": torch_route},
    args.steps, args.rounds))

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
