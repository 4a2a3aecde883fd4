"""ContentKNN on the GPU, measured (GPU only; not a test):

    python tools/content_bench.py [--out profiles/content_bench.txt] [--rounds 5]

At the H&M catalogue size (I = 105,542) with `synthetic.item_attributes` defaults (eleven
categorical columns, 30 % of the rows exact copies of another row; the tool's shape, not the real
articles table), idf weighting, N = 64:

(a) the fit, hnm_content_fit_f32 (the C entry on uploaded tables: the host encoding is not timed),
    at LDS tiles of 64 / 128 / 256 / 512 column items.  Checked before timing: every tile gives
    the same bits, twice.
(b) baselines.  torch on the same GPU: the one-hot [I, V] fp32 matrix scaled by sqrt(q) / sqrt(n),
    X[chunk] @ X.T in chunks of `--chunk` rows with the diagonal masked, torch.topk(64).  Its
    neighbour sets are compared with ours where the sims are untied (every neighbour of ours
    strictly above the row's 64th value must be in torch's set; its scores round their own way).
    numpy on the CPU, the same product in float32, at 1/64, 1/16, 1/4 of the catalogue, stopping
    at the largest scale that stays inside `--cpu-budget` seconds.
(c) serving the content table through ItemCF's entries: recommend_with_scores (history filter) and
    recommend_for_items for 4,096 rows, K = 12, on a synthetic history of `--users` users.  A
    report, no claim: it is the ItemCF serve kernel on a denser table.

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
from hnm_recommendation_amd import ContentKNN, UserHistory, _lib  # noqa: E402
from hnm_recommendation_amd import synthetic as syn  # noqa: E402
from hnm_recommendation_amd.models.content_knn import encode_attributes  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(R, "profiles", "content_bench.txt"))
ap.add_argument("--items", type=int, default=syn.HM_ITEMS)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--fit-steps", type=int, default=2)
ap.add_argument("--chunk", type=int, default=4096)
ap.add_argument("--users", type=int, default=200_000)
ap.add_argument("--cpu-budget", type=float, default=60.0)
args = ap.parse_args()

if not torch.cuda.is_available():
    raise SystemExit("content_bench needs an AMD GPU: there is no CPU path (unmeasured)")
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
    if title:
        say(title)
    med = {n: statistics.median(v) for n, v in res.items()}
    for n, v in res.items():
        say(f"  {n:<52s} median {med[n]:10.4f} ms/call  (min {min(v):.4f}, max {max(v):.4f}, "
            f"{len(v)} rounds)  {med[base] / med[n]:8.2f}x vs {base}")
    return med


I, N, B, K = args.items, 64, 4096, 12
attrs = syn.item_attributes(I)
codes, code_ptr, code_q = encode_attributes(attrs, I)
F, V = codes.shape[1], int(code_ptr[-1])
dups = I - len(np.unique(attrs, axis=0))
say(f"data: I = {I}, F = {F} columns, V = {V} codes in all, {dups} rows equal to an earlier row, "
    f"{I * (I - 1)} ordered pairs")

# ------------------------------------------------------------------ (a) fit
d_codes = torch.from_numpy(codes).to(dev)
d_ptr = torch.from_numpy(code_ptr).to(dev)
d_q = torch.from_numpy(np.append(code_q, np.uint32(0)).view(np.int32)).to(dev)
out_idx = torch.empty(I, N, dtype=torch.int32, device=dev)
out_val = torch.empty(I, N, dtype=torch.float32, device=dev)
out_cnt = torch.empty(I, dtype=torch.int64, device=dev)


def fit(tile):
    _lib.call("hnm_content_fit_f32", _lib.ctx(dev), _lib.ptr(d_codes), I, F, _lib.ptr(d_ptr),
              _lib.ptr(d_q), N, tile, _lib.ptr(out_idx), _lib.ptr(out_val), _lib.ptr(out_cnt))


fit(0)
_lib.sync_check(dev)
ref_idx, ref_val = out_idx.clone(), out_val.clone()
TILES = (64, 128, 256, 512)
for tile in TILES * 2:
    fit(tile)
    torch.cuda.synchronize()
    assert torch.equal(out_idx, ref_idx), tile
    assert torch.equal(out_val.view(torch.int32), ref_val.view(torch.int32)), tile
full = float((ref_idx[:, -1] >= 0).float().mean())
tied = float((ref_val[:, 0] == ref_val[:, -1]).float().mean())
say(f"(a) fit: N = {N}; the four tiles give equal bits, twice; {full * 100:.1f} % of the rows are "
    f"full, {tied * 100:.1f} % hold one value from first to last place")
sides = {f"hnm_content_fit_f32, tile {t}": (lambda t=t: fit(t)) for t in TILES}
fit_med = report("", interleaved(sides, args.fit_steps, args.rounds, warm=1),
                 "hnm_content_fit_f32, tile 256")
write_out()

# ------------------------------------------------------------------ (b) baselines
clean = np.where(codes >= 0, codes + code_ptr[:-1][None, :], -1)
qi = np.where(codes >= 0, code_q[np.maximum(clean, 0)], 0).astype(np.float64)
nsum = qi.sum(1)


def one_hot(rows):
    x = np.zeros((len(rows), V), np.float32)
    w = np.sqrt(qi[rows] / np.maximum(nsum[rows], 1.0)[:, None]).astype(np.float32)
    r, f = np.nonzero(clean[rows] >= 0)
    x[r, clean[rows][r, f]] = w[r, f]
    return x


X = torch.from_numpy(one_hot(np.arange(I))).to(dev)
t_idx = torch.empty(I, N, dtype=torch.int64, device=dev)


def torch_fit():
    for lo in range(0, I, args.chunk):
        hi = min(I, lo + args.chunk)
        s = X[lo:hi] @ X.T
        s[torch.arange(hi - lo, device=dev), torch.arange(lo, hi, device=dev)] = float("-inf")
        t_idx[lo:hi] = torch.topk(s, N, dim=1).indices


try:
    torch_fit()
    torch.cuda.synchronize()
    fit(0)
    torch.cuda.synchronize()
    clear = (ref_val > ref_val[:, -1:] * (1.0 + 1e-5)) & (ref_idx >= 0)    # strictly above the cut
    hit = (ref_idx.to(torch.int64)[:, :, None] == t_idx[:, None, :]).any(2)
    say(f"(b) torch one-hot [I, {V}] fp32 X[chunk {args.chunk}] @ X.T + torch.topk({N}): "
        f"{int(clear.sum())} of our {int((ref_idx >= 0).sum())} neighbours stand strictly above "
        f"their row's last value; {float(hit[clear].float().mean()) * 100:.4f} % of them are in "
        "torch's set")
    base = "torch X[chunk] @ X.T + topk"
    med = report("", interleaved({base: torch_fit, "hnm_content_fit_f32 (default tile)":
                                  lambda: fit(0)}, args.fit_steps, args.rounds, warm=1), base)
except Exception as e:  # noqa: BLE001
    say(f"(b) torch baseline failed here: {type(e).__name__}: {e} (unmeasured)")
del X
write_out()

done = None
for div in (64, 16, 4):                                          # the full scale is never tried
    n = I // div
    rows = np.arange(n)
    t0 = time.perf_counter()
    x = one_hot(rows)
    cpu_idx = np.empty((n, N), np.int64)
    for lo in range(0, n, 1024):
        s = x[lo:lo + 1024] @ x.T
        s[np.arange(s.shape[0]), np.arange(lo, lo + s.shape[0])] = -np.inf
        part = np.argpartition(-s, N - 1, axis=1)[:, :N]
        cpu_idx[lo:lo + 1024] = np.take_along_axis(
            part, np.argsort(-np.take_along_axis(s, part, 1), axis=1, kind="stable"), 1)
    cpu_s = time.perf_counter() - t0
    sub = ContentKNN(1, n, num_neighbors=N).to(dev)
    sub.fit_attributes(attrs[:n])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(3):
        sub.fit_attributes(attrs[:n])
    gpu_ms = (time.perf_counter() - t0) / 3 * 1e3
    done = div
    say(f"    scale 1/{div}: I = {n}: numpy one-hot product + per-row top-{N} {cpu_s:.2f} s on the "
        f"CPU, ContentKNN.fit_attributes (host encoding included) {gpu_ms:.2f} ms")
    if cpu_s * 16 > args.cpu_budget:                             # the next scale costs 16x
        break
say(f"    largest scale numpy finished inside {args.cpu_budget:.0f} s: 1/{done}")
write_out()

# ------------------------------------------------------------------ (c) serving
U = args.users
model = ContentKNN(U, I, num_neighbors=N).to(dev)
model.load_state_dict({"neighbor_idx": ref_idx, "neighbor_val": ref_val, "item_count": out_cnt})
users_np, items_np = syn.interactions(U, I, 20 * U, seed=2)
hist = UserHistory.from_interactions(users_np, items_np, U, I, dev)
model.set_history(hist)
u = torch.from_numpy(syn.user_batch(U, B, seed=100)).to(dev)
route = model.scoring_route(u)
ptr, idx = hist.hist_ptr.cpu().numpy(), hist.hist_idx.cpu().numpy()
rows = [idx[ptr[x]:ptr[x + 1]] for x in u.cpu().numpy()]
p = np.concatenate([[0], np.cumsum([len(x) for x in rows])]).astype(np.int64)
baskets = (torch.from_numpy(p).to(dev), torch.from_numpy(np.concatenate(rows).astype(np.int32)).to(dev))
a = model.recommend_with_scores(u, filter_items=hist, k=K)
b = model.recommend_for_items(baskets, k=K)
assert torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
_lib.sync_check(dev)
say(f"(c) serving the content table: B = {B}, K = {K}, U = {U} synthetic users (history mean "
    f"{hist.nnz / U:.1f}); {route.count('dense')} rows take the dense route; users and baskets "
    "give equal bits")
report("", interleaved(
    {"recommend_with_scores (history filter)":
     lambda: model.recommend_with_scores(u, filter_items=hist, k=K),
     "recommend_for_items (the same rows as baskets)":
     lambda: model.recommend_for_items(baskets, k=K)}, args.steps, args.rounds),
    "recommend_with_scores (history filter)")
write_out()
