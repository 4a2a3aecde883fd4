"""ItemCF on the GPU, measured (GPU only; not a test):

    python tools/itemcf_bench.py [--out profiles/itemcf_bench.txt] [--rounds 5]

At the H&M shape (U = 1,371,980, I = 105,542, E = 31,788,324 synthetic interactions, N = 64):

(a) the fit, hnm_itemcf_fit_f32, at LDS windows of 4,096 / 8,192 / 16,384 item columns; and, at
    the largest scale (all users and items divided by the same factor) that scipy finishes
    inside `--cpu-budget` seconds, against scipy's `A.T @ A` plus a per-row top-N on the CPU.
(b) recommend_with_scores for B = 4,096, K = 12 with the history filter: hnm_itemcf_topk_f32
    against the same answer formed on the same GPU by torch -- a [B, I] history matrix times the
    sparse truncated similarity matrix (torch.sparse.mm), then `dense_topk` -- and against the
    package's own dense route (hnm_itemcf_scores_f32 + `dense_topk`).  The lists are compared
    before anything is timed (ids where the torch sums are not within rounding of a tie).
(c) the same call as baskets with 64 of the 4,096 rows replaced by 2,000-item bulk buyers (the
    dense route): the synthetic generator draws users uniformly, so (b) holds no such row.

(d) the weighted siblings (pair weights count * exp(-0.01 days)) on the same CSR:
    hnm_itemcf_fit_weighted_f32 at windows of 4,096 / 8,192 (64 KiB of 64-bit counters, two
    workgroups a CU) / 16,384 (128 KiB, one) against hnm_itemcf_fit_f32, and the weighted per-user
    top-12 against the unweighted one.  Checked before timing: the weighted fit gives the same
    bits twice and at every window, and unit weights give the unweighted table.
    `--weighted-only` runs (d) alone (default --out then: profiles/witemcf_bench.txt).

Each side is warmed up, then timed in interleaved rounds (order alternating) of at least
`--steps` calls (and ~50 ms) between device synchronisations; medians and the spread of the
per-round means are reported.
"""
import argparse
import copy
import os
import statistics
import sys
import time

import numpy as np
import torch

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
from hnm_recommendation_amd import ItemCF, UserHistory, WeightedItemCF, _lib  # noqa: E402
from hnm_recommendation_amd import synthetic as syn  # noqa: E402
from hnm_recommendation_amd.models.base import dense_topk  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--weighted-only", action="store_true")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--fit-steps", type=int, default=2)
ap.add_argument("--rows", type=int, default=syn.HM_INTERACTIONS)
ap.add_argument("--cpu-budget", type=float, default=60.0)
args = ap.parse_args()
if args.out is None:
    args.out = os.path.join(R, "profiles",
                            "witemcf_bench.txt" if args.weighted_only else "itemcf_bench.txt")

if not torch.cuda.is_available():
    raise SystemExit("itemcf_bench needs an AMD GPU: there is no CPU path")
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


def report(title, res, base):
    say(title)
    med = {n: statistics.median(v) for n, v in res.items()}
    for n, v in res.items():
        say(f"  {n:<52s} median {med[n]:10.4f} ms/call  (min {min(v):.4f}, max {max(v):.4f}, "
            f"{len(v)} rounds)  {med[base] / med[n]:8.2f}x vs {base}")
    return med


U, I, N, B, K = syn.HM_USERS, syn.HM_ITEMS, 64, 4096, 12
users_np, items_np = syn.interactions(U, I, args.rows, seed=2)
hist = UserHistory.from_interactions(users_np, items_np, U, I, dev)
lens = (hist.hist_ptr[1:] - hist.hist_ptr[:-1])
say(f"data: U = {U}, I = {I}, E = {args.rows} drawn, {hist.nnz} distinct (user, item) pairs, "
    f"history mean {hist.nnz / U:.1f}, max {int(lens.max())}")



def write_out():
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


def same_table(m, idx, val, cnt):
    return (torch.equal(m.neighbor_idx, idx) and torch.equal(m.item_count, cnt)
            and torch.equal(m.neighbor_val.view(torch.int32), val.view(torch.int32)))


# ------------------------------------------------------------------ (d) weighted
def weighted_section():
    g = torch.Generator(device="cpu").manual_seed(5)
    n_w = hist.hist_idx.numel()
    w = (torch.randint(1, 9, (n_w,), generator=g).to(torch.float64)
         * torch.exp(-0.01 * torch.randint(0, 366, (n_w,), generator=g).to(torch.float64)))
    whist = copy.copy(hist)                                # the same CSR, with weights
    whist.hist_w = w.to(torch.float32).to(dev)
    ones = copy.copy(hist)
    ones.hist_w = torch.ones(n_w, dtype=torch.float32, device=dev)
    say(f"(d) weighted: pair weights count * exp(-0.01 days): min "
        f"{float(whist.hist_w[:hist.nnz].min()):.4f}, mean "
        f"{float(whist.hist_w[:hist.nnz].mean()):.4f}, max "
        f"{float(whist.hist_w[:hist.nnz].max()):.4f}")
    plain = ItemCF(U, I, num_neighbors=N).to(dev).fit_history(hist)
    wm = WeightedItemCF(U, I, num_neighbors=N).to(dev).fit_history(ones)
    assert same_table(wm, plain.neighbor_idx, plain.neighbor_val, plain.item_count)
    wm.fit_history(whist)
    ref = (wm.neighbor_idx.clone(), wm.neighbor_val.clone(), wm.item_count.clone())
    assert not torch.equal(ref[0], plain.neighbor_idx)
    sides = {"hnm_itemcf_fit_f32 (unweighted, window 16384)": lambda: plain.fit_history(hist)}
    for W in (4096, 8192, 16384):
        sides[f"hnm_itemcf_fit_weighted_f32, window {W}"] = \
            (lambda W=W: wm.fit_history(whist, _window=W))
    for name, f in list(sides.items())[1:] * 2:                   # every window, twice
        f()
        assert same_table(wm, *ref), name
    say(f"    fit: N = {N}; unit weights give the unweighted table's bits; the weighted fit gives "
        "equal bits twice and at the three windows")
    base = "hnm_itemcf_fit_f32 (unweighted, window 16384)"
    report("", interleaved(sides, args.fit_steps, args.rounds, warm=1), base)
    wm.fit_history(whist)
    ub = torch.from_numpy(syn.user_batch(U, B, seed=100)).to(dev)
    a = wm.recommend_with_scores(ub, filter_items=whist, k=K)
    b = wm.recommend_with_scores(ub, filter_items=whist, k=K)
    assert torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
    wm_ones = WeightedItemCF(U, I, num_neighbors=N).to(dev)
    wm_ones.load_state_dict(plain.state_dict())
    wm_ones.set_history(ones)
    a = wm_ones.recommend_with_scores(ub, filter_items=hist, k=K)
    b = plain.recommend_with_scores(ub, filter_items=hist, k=K)
    assert torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
    _lib.sync_check(dev)
    say(f"    recommend_with_scores: B = {B}, K = {K}, history filter; the weighted call gives "
        "equal bits twice, and the unweighted call's with unit weights")
    base = "hnm_itemcf_topk_f32 (unweighted)"
    report("", interleaved(
        {base: lambda: plain.recommend_with_scores(ub, filter_items=hist, k=K),
         "hnm_itemcf_topk_weighted_f32": lambda: wm.recommend_with_scores(ub, filter_items=whist,
                                                                          k=K)},
        args.steps, args.rounds), base)


if args.weighted_only:
    weighted_section()
    write_out()
    sys.exit(0)

# ------------------------------------------------------------------ (a) fit
model = ItemCF(U, I, num_neighbors=N).to(dev)
model.fit_history(hist)
ref_idx, ref_val = model.neighbor_idx.clone(), model.neighbor_val.clone()
sides = {}
for W in (4096, 8192, 16384):
    sides[f"hnm_itemcf_fit_f32, window {W}"] = (lambda W=W: model.fit_history(hist, _window=W))
for f in sides.values():                                       # the window does not change a bit
    f()
    assert torch.equal(model.neighbor_idx, ref_idx)
    assert torch.equal(model.neighbor_val.view(torch.int32), ref_val.view(torch.int32))
say(f"(a) fit: N = {N}; the three windows give equal bits")
report("", interleaved(sides, args.fit_steps, args.rounds, warm=1),
       "hnm_itemcf_fit_f32, window 8192")


def scipy_fit(u, i, nu, ni, n):
    import scipy.sparse as sp
    a = sp.csr_matrix((np.ones(len(u)), (u, i)), shape=(nu, ni))
    a.data[:] = 1.0                                              # duplicates summed: back to 0/1
    c = (a.T @ a).tocsr()
    cnt = np.asarray(a.sum(0)).reshape(-1)
    c.setdiag(0)
    c.eliminate_zeros()
    rows = np.repeat(np.arange(ni), np.diff(c.indptr))
    c.data = c.data / np.sqrt(cnt[rows] * cnt[c.indices])
    out = np.full((ni, n), -1, np.int32)
    for r in range(ni):
        lo, hi = c.indptr[r], c.indptr[r + 1]
        top = np.lexsort((c.indices[lo:hi], -c.data[lo:hi].astype(np.float32)))[:n]
        out[r, :len(top)] = c.indices[lo:hi][top]
    return out


try:
    import scipy  # noqa: F401
    done = None
    for div in (64, 16, 4):                                      # the full scale is never tried
        su, si = U // div, I // div
        u_s, i_s = syn.interactions(su, si, args.rows // div, seed=2)
        t0 = time.perf_counter()
        cpu_idx = scipy_fit(u_s, i_s, su, si, N)
        cpu_s = time.perf_counter() - t0
        small = ItemCF(su, si, num_neighbors=N).to(dev)
        small.fit_interactions(u_s, i_s)
        h_s = small.history
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            small.fit_history(h_s)
        gpu_ms = (time.perf_counter() - t0) / 3 * 1e3
        same = float((small.neighbor_idx.cpu().numpy() == cpu_idx).mean())
        done = (div, su, si, args.rows // div, cpu_s, gpu_ms, same)
        say(f"    scale 1/{div}: U = {su}, I = {si}, E = {args.rows // div}: scipy A.T @ A + "
            f"per-row top-{N} {cpu_s:.2f} s on the CPU, hnm_itemcf_fit_f32 {gpu_ms:.2f} ms "
            f"({same * 100:.2f} % of the neighbour slots equal)")
        if cpu_s * 10 > args.cpu_budget:                         # the next scale costs > 4x
            break
        del small
    say(f"    largest scale scipy finished inside {args.cpu_budget:.0f} s: 1/{done[0]}")
except ImportError:
    say("    scipy is not installed: no CPU comparison")

# ------------------------------------------------------------------ (b) top-K
model.fit_history(hist)
users = syn.user_batch(U, B, seed=100)
u = torch.from_numpy(users).to(dev)
route = model.scoring_route(u)
say(f"(b) recommend_with_scores: B = {B}, K = {K}, history filter; "
    f"{route.count('dense')} of {B} rows take the dense route")

# S^T as a sparse [I (target i), I (source j)] matrix, H^T as a dense [I, B] 0/1 matrix
src = torch.arange(I, device=dev).repeat_interleave(N)
tgt = model.neighbor_idx.reshape(-1).to(torch.int64)
keep = tgt >= 0
st = torch.sparse_coo_tensor(torch.stack([tgt[keep], src[keep]]),
                             model.neighbor_val.reshape(-1)[keep], (I, I)).coalesce()
try:
    st = st.to_sparse_csr()
except Exception:  # noqa: BLE001
    pass
ht = torch.zeros(I, B, dtype=torch.float32, device=dev)


def torch_route():
    mptr, midx = hist.mask_for(u)
    ht.zero_()
    col = torch.repeat_interleave(torch.arange(B, device=dev), mptr[1:] - mptr[:-1])
    ht[midx[:col.numel()].to(torch.int64), col] = 1.0
    scores = torch.sparse.mm(st, ht).t().contiguous()
    return dense_topk(scores, K, mptr, midx)


def fused_route():
    return model.recommend_with_scores(u, filter_items=hist, k=K)


def dense_route():
    mptr, midx = hist.mask_for(u)
    return dense_topk(model.predict_all_items(u), K, mptr, midx)


fv, fi = fused_route()
dv, di = dense_route()
pos = fv > 0
assert torch.equal(fi[pos], di[pos]) and torch.equal(fv[pos].view(torch.int32),
                                                     dv[pos].view(torch.int32))
sides = {"hnm_itemcf_topk_f32 (fused)": fused_route,
         "hnm_itemcf_scores_f32 + dense_topk": dense_route}
try:
    tv, ti = torch_route()
    close = torch.isclose(tv[pos], fv[pos], rtol=1e-5, atol=0.0)
    say(f"    torch.sparse.mm route: {float(close.float().mean()) * 100:.3f} % of the scores within "
        f"1e-5, {float((ti[pos] == fi[pos]).float().mean()) * 100:.3f} % of the ids equal (its "
        "summation order is its own)")
    assert float(close.float().mean()) > 0.999
    sides["[B, I] history x sparse similarity + dense_topk (torch)"] = torch_route
    base = "[B, I] history x sparse similarity + dense_topk (torch)"
except Exception as e:  # noqa: BLE001
    say(f"    torch.sparse.mm route failed here: {type(e).__name__}: {e}")
    base = "hnm_itemcf_scores_f32 + dense_topk"
_lib.sync_check(dev)
report("", interleaved(sides, args.steps, args.rounds), base)

# ------------------------------------------------------------------ (c) bulk buyers
ptr = hist.hist_ptr.cpu().numpy()
idx = hist.hist_idx.cpu().numpy()
rows = [idx[ptr[x]:ptr[x + 1]] for x in users]
rng = np.random.Generator(np.random.PCG64(7))
bulk = list(rows)
for r in range(0, B, B // 64):
    bulk[r] = np.sort(rng.choice(I, size=2000, replace=False)).astype(np.int32)


def csr(rs):
    p = np.concatenate([[0], np.cumsum([len(x) for x in rs])]).astype(np.int64)
    return p, np.concatenate(rs).astype(np.int32)


plain_csr = tuple(torch.from_numpy(a).to(dev) for a in csr(rows))
bulk_csr = tuple(torch.from_numpy(a).to(dev) for a in csr(bulk))
bv, bi = model.recommend_for_items(plain_csr, k=K)
assert torch.equal(bi, fi) and torch.equal(bv.view(torch.int32), fv.view(torch.int32))
say(f"(c) recommend_for_items: B = {B} baskets, K = {K}; 64 rows replaced by 2,000-item baskets "
    "(dense route)")
report("", interleaved({"baskets = the users' histories": lambda: model.recommend_for_items(plain_csr, k=K),
                        "64 of them 2,000-item baskets": lambda: model.recommend_for_items(bulk_csr, k=K)},
                       args.steps, args.rounds), "baskets = the users' histories")

weighted_section()
write_out()
