"""Two-stage serving on the GPU, measured (GPU only; not a test):

    python tools/rerank_bench.py [--out profiles/rerank_bench.txt] [--rounds 5]

At the H&M shape (U = 1,371,980, I = 105,542, synthetic interactions), B = 4,096 users, k = 12,
the default Wide&Deep tower (512/256/128, d = 64) as the ranker, ItemCF + ImplicitALS +
PopularityBaseline as the sources, with the history filter, at depths 24, 48 and 64:

(a) hnm_cand_union_i32 alone on the sources' real lists; the mean and maximum candidates a row
    (how much the sources overlap) and the row width.
(b) hnm_widedeep_cand_topk_ex_f32 alone, split into the per-call preparation (wd_setup: folded
    weights, the layer-1 tables of the batch and of the whole catalogue) and the candidate
    kernel (the ctx's scoring-kernel timer).
(c) the whole `Reranker.recommend_with_scores`, next to its sources' own calls.
(d) the same answer without the new entry: `WideDeep.forward` on the flattened, padded (user,
    candidate) pairs, -inf on the padding, torch.topk.  Its input is the candidate matrix of
    (a), so the sources' time is not in it: (b) against (d) is the acceptance figure.  The two
    answers are compared before anything is timed.
(e) `WideDeep.recommend_with_scores` over the whole catalogue: a DIFFERENT answer (no recall
    stage), for scale only.

Each side is warmed up, then timed in interleaved rounds (order alternating) between device
synchronisations; medians and the spread of the per-round means are reported.
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import torch

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
from hnm_recommendation_amd import (ImplicitALS, ItemCF, PopularityBaseline,  # noqa: E402
                                    Reranker, WideDeep, _lib)
from hnm_recommendation_amd import synthetic as syn  # noqa: E402
from hnm_recommendation_amd.models.base import empty_rows  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(R, "profiles", "rerank_bench.txt"))
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--rows", type=int, default=syn.HM_INTERACTIONS)
ap.add_argument("--als-iterations", type=int, default=2)
ap.add_argument("--depths", type=int, nargs="+", default=[24, 48, 64])
args = ap.parse_args()

if not torch.cuda.is_available():
    raise SystemExit("rerank_bench needs an AMD GPU: there is no CPU path")
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def interleaved(sides, steps, rounds, warm=2):
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
    if title:
        say(title)
    med = {n: statistics.median(v) for n, v in res.items()}
    for n, v in res.items():
        say(f"  {n:<66s} median {med[n]:10.4f} ms/call  (min {min(v):.4f}, max {max(v):.4f}, "
            f"{len(v)} rounds)")
    return med


U, I, B, K = syn.HM_USERS, syn.HM_ITEMS, 4096, 12
users_np, items_np = syn.interactions(U, I, args.rows, seed=2)
icf = ItemCF(U, I, num_neighbors=64).to(dev)
icf.fit_interactions(users_np, items_np)
hist = icf.history
als = ImplicitALS(U, I, embedding_dim=64, iterations=args.als_iterations).to(dev)
als.fit_interactions(users_np, items_np)
pop = PopularityBaseline(n_items=I).to(dev)
pop.fit_interactions(items_np)
wd = WideDeep(U, I)
wd.load_state_dict({k: torch.from_numpy(v) for k, v in
                    syn.widedeep_state_dict(U, I, 64, (512, 256, 128), seed=5).items()})
wd = wd.to(dev).eval()
sources = [("item_cf", icf), ("implicit_als", als), ("popularity", pop)]
G = len(sources)
say(f"data: U = {U}, I = {I}, E = {args.rows} drawn, {hist.nnz} distinct (user, item) pairs; "
    f"B = {B}, k = {K}, history filter; sources item_cf (64 neighbours) + implicit_als (d = 64, "
    f"{args.als_iterations} sweeps) + popularity; ranker WideDeep 512/256/128, d = 64")
u = torch.from_numpy(syn.user_batch(U, B, seed=100)).to(dev)
w, keep = wd._weights()
ctx = _lib.ctx(dev)
NEG = float("-inf")

for depth in args.depths:
    say("")
    say(f"==== depth {depth}: [{G}, {B}, {depth}] lists, candidate rows of width {G * depth}")
    rr = Reranker(wd, sources, depth=depth)
    lists = [m.recommend_with_scores(u, hist, k=depth) for _, m in sources]
    lv = torch.stack([v for v, _ in lists]).contiguous()
    li = torch.stack([i for _, i in lists]).contiguous()
    W = G * depth
    cand = torch.empty(B, W, dtype=torch.int32, device=dev)
    n = torch.empty(B, dtype=torch.int32, device=dev)

    def union_call():
        _lib.call("hnm_cand_union_i32", ctx, _lib.ptr(lv), _lib.ptr(li), B, G, B * depth, depth,
                  depth, I, _lib.ptr(cand), W, _lib.ptr(n))

    union_call()
    first = (cand.clone(), n.clone())
    union_call()
    assert torch.equal(first[0], cand) and torch.equal(first[1], n)
    _lib.sync_check(dev)
    live = ((li >= 0) & torch.isfinite(lv)).sum(2).float().mean(1).tolist()
    say(f"    live entries per list: " + ", ".join(f"{nm} {x:.1f}" for (nm, _), x in
                                                    zip(sources, live)))
    say(f"    candidates a row (out_n): mean {float(n.float().mean()):.1f}, max {int(n.max())}, "
        f"min {int(n.min())}; row width used {W}")

    out_v, out_i = empty_rows(B, K, dev)

    def cand_call():
        _lib.call("hnm_widedeep_cand_topk_ex_f32", ctx, w, _lib.ptr(u), B, None, _lib.ptr(cand),
                  W, _lib.ptr(n), K, _lib.ptr(out_v), _lib.ptr(out_i), None, None, None, 0)

    # ---------------------------------------------------------- (d) the pairs route, checked
    u_rep = u.repeat_interleave(W)
    items_flat = cand.clamp(min=0).to(torch.int64).reshape(-1)
    pad = torch.arange(W, device=dev).unsqueeze(0) >= n.unsqueeze(1)

    def pairs_route():
        s = wd(u_rep, items_flat).reshape(B, W).masked_fill(pad, NEG)
        return torch.topk(s, K, dim=1)

    cand_call()
    got_v, got_i = out_v.clone(), out_i.clone()
    whole = rr.recommend_with_scores(u, filter_items=hist, k=K)
    assert torch.equal(whole[1], got_i) and torch.equal(whole[0].view(torch.int32),
                                                        got_v.view(torch.int32))
    tv, tpos = pairs_route()
    ti = torch.gather(cand.to(torch.int64), 1, tpos)
    full = (n >= K).unsqueeze(1).expand(B, K)
    close = float(torch.isclose(tv[full], got_v[full], rtol=1e-4, atol=1e-5).float().mean())
    same = float((ti[full] == got_i[full]).float().mean())
    say(f"    pairs route against the new entry (rows with >= {K} candidates): "
        f"{close * 100:.3f} % of the scores within 1e-4, {same * 100:.3f} % of the ids equal")
    assert close > 0.99 and same > 0.98

    # ---------------------------------------------------------- (b) split: kernel / setup
    _lib.enable_timing(dev, _lib.TIME_SCORE)
    for _ in range(10):
        cand_call()
    kt, kn = _lib.kernel_timing(dev)
    _lib.enable_timing(dev, 0)
    kernel_ms = kt / max(kn, 1)

    res = interleaved({
        "(a) hnm_cand_union_i32": union_call,
        "(b) hnm_widedeep_cand_topk_ex_f32": cand_call,
        "(c) Reranker.recommend_with_scores (sources + union + ranker)":
            lambda: rr.recommend_with_scores(u, filter_items=hist, k=K),
        "(c') the three sources' own calls, k = depth":
            lambda: [m.recommend_with_scores(u, hist, k=depth) for _, m in sources],
        "(d) WideDeep.forward on the padded pairs + torch.topk": pairs_route,
    }, args.steps, args.rounds)
    med = report("", res)
    b, d = res["(b) hnm_widedeep_cand_topk_ex_f32"], \
        res["(d) WideDeep.forward on the padded pairs + torch.topk"]
    say(f"    (b) split: candidate kernel {kernel_ms:.4f} ms (scoring-kernel timer, {kn} calls), "
        f"preparation (wd_setup) {med['(b) hnm_widedeep_cand_topk_ex_f32'] - kernel_ms:.4f} ms = "
        f"{(1 - kernel_ms / med['(b) hnm_widedeep_cand_topk_ex_f32']) * 100:.1f} % of the call")
    ratios = [y / x for x, y in zip(b, d)]
    say(f"    (d) / (b) per round: " + ", ".join(f"{r:.2f}" for r in ratios) +
        f"; the new entry is faster in {sum(r > 1 for r in ratios)} of {len(ratios)} rounds; "
        f"median ratio {statistics.median(ratios):.2f}")

say("")
res = interleaved({"(e) WideDeep.recommend_with_scores, whole catalogue (a different answer)":
                   lambda: wd.recommend_with_scores(u, filter_items=hist, k=K)},
                  max(2, args.steps // 2), args.rounds)
report("(e) for scale", res)

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
