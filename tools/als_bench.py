"""ImplicitALS on the GPU, measured (GPU only; not a test):

    python tools/als_bench.py [--out profiles/als_bench.txt] [--rounds 5]

At the H&M shape (U = 1,371,980, I = 105,542, E = 31,788,324 synthetic interactions):

(a) one sweep at d = 64 and d = 128, split into its four calls: hnm_als_gram_f32 of Y, the user
    step, hnm_als_gram_f32 of X, the item step (hnm_als_solve_rows_f32 both).
(b) a whole fit of 15 sweeps at d = 64 and d = 128 (transpose and final sync included).
(c) the user step at d = 64 against the same half-step formed on the same GPU by torch: per
    chunk of users a padded gather of Y, `bmm` for sum y y^T, `torch.linalg.cholesky` and
    `cholesky_solve`.  The two answers are compared before anything is timed.
(d) one sweep at d = 64 on the CPU in numpy/LAPACK (batched `np.linalg.solve` in float32) at the
    reduced scales ItemCF's table uses (users, items and interactions divided by the same
    factor), the largest that finishes inside `--cpu-budget` seconds, against the GPU sweep at
    that scale.
(e) fold-in + top-12 for 4,096 baskets (`recommend_for_items`), d = 64.
(w) the weighted half-step (hnm_als_solve_rows_weighted_f32) against the unweighted one: user
    step and item step at d = 64 and d = 128 on the same CSR and tables, pair weights
    count * exp(-0.01 * days) (count in 1..8, days in 0..365).  Checked first: unit weights give
    the unweighted entry's bits, the weighted answer is the same bits twice, finite, and its
    rows r = 0, n / 256, 2 n / 256, ... and its longest row agree with a float64
    `torch.linalg.solve` of the same systems.
(g) the conjugate-gradient half-step (hnm_als_cg_rows_f32 and its weighted sibling) against the
    Cholesky one, by (w)'s protocol -- the same CSR, tables and pair weights, calls interleaved
    in this one process: user step and item step at d = 64 and d = 128, unweighted and weighted,
    the Cholesky entry against the CG entry at 1, 3 and 5 steps.  The CG entry works in place, so
    each timed CG call first restores its start vectors (the previous sweep's table) with one
    device copy, which is timed alone as well.  Checked first: the CG answers are finite and the
    same bits on a second run.  Then a whole `--sweeps` fit with each solver (cg_steps = 3) and
    `loss()` of both fits.

`--sections` picks the legs (default all, e.g. `--sections w`).  Each side of (a), (c), (e) and
(w), (g) is warmed up, then timed in interleaved rounds (order alternating)
between device synchronisations; medians and the spread of the per-round means are reported.
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
from hnm_recommendation_amd import ImplicitALS, UserHistory, _lib  # noqa: E402
from hnm_recommendation_amd import synthetic as syn  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(R, "profiles", "als_bench.txt"))
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=2)
ap.add_argument("--rows", type=int, default=syn.HM_INTERACTIONS)
ap.add_argument("--sweeps", type=int, default=15)
ap.add_argument("--cpu-budget", type=float, default=60.0)
ap.add_argument("--torch-chunk", type=int, default=4096)
ap.add_argument("--sections", default="abcdewg")
args = ap.parse_args()

if not torch.cuda.is_available():
    raise SystemExit("als_bench needs an AMD GPU: there is no CPU path")
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
lines = []
ALPHA, REG = 40.0, 0.01


def say(s):
    print(s, flush=True)
    lines.append(s)


def interleaved(sides, steps, rounds, warm=1):
    """{name: [ms per call, one per round]}: every round times each side (order alternating)."""
    res = {n: [] for n in sides}
    for f in sides.values():
        for _ in range(warm):
            f()
    torch.cuda.synchronize()
    for rnd in range(rounds):
        names = list(sides)[::-1] if rnd % 2 else list(sides)
        for n in names:
            f = sides[n]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                f()
            torch.cuda.synchronize()
            res[n].append((time.perf_counter() - t0) / steps * 1e3)
    return res


def report(title, res, base=None):
    say(title)
    med = {n: statistics.median(v) for n, v in res.items()}
    for n, v in res.items():
        rel = f"  {med[base] / med[n]:8.2f}x vs {base}" if base else ""
        say(f"  {n:<58s} median {med[n]:10.3f} ms/call  (min {min(v):.3f}, max {max(v):.3f}, "
            f"{len(v)} rounds){rel}")
    return med


U, I = syn.HM_USERS, syn.HM_ITEMS
users_np, items_np = syn.interactions(U, I, args.rows, seed=2)
hist = UserHistory.from_interactions(users_np, items_np, U, I, dev)
lens = hist.hist_ptr[1:] - hist.hist_ptr[:-1]
tptr, tusers, _ = ImplicitALS._transpose(hist)
tlens = tptr[1:] - tptr[:-1]
say(f"data: U = {U}, I = {I}, E = {args.rows} drawn, {hist.nnz} distinct (user, item) pairs; "
    f"history mean {hist.nnz / U:.1f}, max {int(lens.max())}; users per item mean "
    f"{hist.nnz / I:.1f}, max {int(tlens.max())}")
say(f"alpha = {ALPHA}, reg = {REG}")
SEC = set(args.sections)
if "w" in SEC or "g" in SEC:
    g_w = torch.Generator(device="cpu").manual_seed(7)
    n_w = hist.hist_idx.numel()
    hist_w = (torch.randint(1, 9, (n_w,), generator=g_w).to(torch.float64)
              * torch.exp(-0.01 * torch.randint(0, 366, (n_w,), generator=g_w).to(torch.float64)))
    whist = copy.copy(hist)                                # the same CSR, with weights
    whist.hist_w = hist_w.to(torch.float32).to(dev)
    tw = ImplicitALS._transpose(whist)[2]
    say(f"(w, g) pair weights count * exp(-0.01 days): min {float(whist.hist_w[:hist.nnz].min()):.4f}, "
        f"mean {float(whist.hist_w[:hist.nnz].mean()):.4f}, max {float(whist.hist_w[:hist.nnz].max()):.4f}")


def check_weighted(m, ptr, idx, w, n_rows, tab, gram, out, what):
    """The weighted answer before it is timed (see the module docstring)."""
    d = m.embedding_dim
    ones = torch.ones_like(w)
    a = m._solve(ptr, idx, n_rows, tab, gram, None, n_rows, out).clone()
    b = m._solve(ptr, idx, n_rows, tab, gram, None, n_rows, out, ones)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{what}: unit weights"
    a = m._solve(ptr, idx, n_rows, tab, gram, None, n_rows, out, w).clone()
    b = m._solve(ptr, idx, n_rows, tab, gram, None, n_rows, out, w)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and bool(torch.isfinite(a).all())
    hp = ptr.cpu()
    rows = sorted(set(range(0, n_rows, max(1, n_rows // 256))) | {int((hp[1:] - hp[:-1]).argmax())})
    G64 = gram.double() + REG * torch.eye(d, device=dev, dtype=torch.float64)
    worst = 0.0
    for r in rows:
        p0, p1 = int(hp[r]), int(hp[r + 1])
        if p1 == p0:
            assert not bool(a[r].any())
            continue
        tg, wg = tab[idx[p0:p1].to(torch.int64)].double(), w[p0:p1].double()
        x64 = torch.linalg.solve(G64 + ALPHA * (tg * wg[:, None]).T @ tg,
                                 ((1.0 + ALPHA * wg)[:, None] * tg).sum(0))
        worst = max(worst, float((a[r] - x64).abs().max() / x64.abs().max()))
    assert worst < 1e-3, f"{what}: {worst}"
    _lib.sync_check(dev)
    return worst


# ------------------------------------------------------------------ (a) one sweep, (b) a fit
models = {}
for d in (64, 128):
    m = ImplicitALS(U, I, embedding_dim=d, regularization=REG, alpha=ALPHA).to(dev)
    m.fit_history(hist, iterations=1)                      # tables of a fitted scale
    models[d] = m
    X, Y = m._tables()
    g = torch.empty(d, d, dtype=torch.float32, device=dev)
    gy, gx = m._gram_of(Y).clone(), m._gram_of(X).clone()
    x_out, y_out = torch.empty_like(X), torch.empty_like(Y)
    # the answers before the timing: the same bits on a second run, finite everywhere
    a = m._solve(hist.hist_ptr, hist.hist_idx, U, Y, gy, None, U, x_out).clone()
    b = m._solve(hist.hist_ptr, hist.hist_idx, U, Y, gy, None, U, x_out)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and bool(torch.isfinite(a).all())
    a = m._solve(tptr, tusers, I, X, gx, None, I, y_out).clone()
    b = m._solve(tptr, tusers, I, X, gx, None, I, y_out)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and bool(torch.isfinite(a).all())
    _lib.sync_check(dev)
    if "w" in SEC:
        eu = check_weighted(m, hist.hist_ptr, hist.hist_idx, whist.hist_w, U, Y, gy, x_out, "user")
        ei = check_weighted(m, tptr, tusers, tw, I, X, gx, y_out, "item")
        say(f"(w) d = {d}: unit weights give the unweighted entry's bits (user and item step); the "
            f"weighted answers are the same bits twice, finite, and within {eu:.1e} (user step) and "
            f"{ei:.1e} (item step) of a row's scale of float64 torch.linalg.solve on every "
            "(n / 256)-th row and the longest row")
        wsides = {
            f"user step, unweighted: hnm_als_solve_rows_f32, {U} rows": lambda: m._solve(
                hist.hist_ptr, hist.hist_idx, U, Y, gy, None, U, x_out),
            f"user step, weighted: hnm_als_solve_rows_weighted_f32, {U} rows": lambda: m._solve(
                hist.hist_ptr, hist.hist_idx, U, Y, gy, None, U, x_out, whist.hist_w),
            f"item step, unweighted: hnm_als_solve_rows_f32, {I} rows": lambda: m._solve(
                tptr, tusers, I, X, gx, None, I, y_out),
            f"item step, weighted: hnm_als_solve_rows_weighted_f32, {I} rows": lambda: m._solve(
                tptr, tusers, I, X, gx, None, I, y_out, tw),
        }
        wmed = report(f"(w) weighted against unweighted half-steps, d = {d}",
                      interleaved(wsides, args.steps, args.rounds))
        names = list(wmed)
        say(f"    weighted / unweighted: user step {wmed[names[1]] / wmed[names[0]]:.3f}, item "
            f"step {wmed[names[3]] / wmed[names[2]]:.3f}")
    if "g" in SEC:
        x_cg, y_cg = torch.empty_like(X), torch.empty_like(Y)

        def cg_user(steps, w=None):
            x_cg.copy_(X)
            return m._cg(hist.hist_ptr, hist.hist_idx, U, Y, gy, x_cg, steps, w)

        def cg_item(steps, w=None):
            y_cg.copy_(Y)
            return m._cg(tptr, tusers, I, X, gx, y_cg, steps, w)

        for tag, wu, wi in (("unweighted", None, None), ("weighted", whist.hist_w, tw)):
            for steps in (1, 3, 5):
                for f, w_ in ((cg_user, wu), (cg_item, wi)):
                    a = f(steps, w_).clone()
                    b = f(steps, w_)
                    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
                    assert bool(torch.isfinite(a).all())
            _lib.sync_check(dev)
            say(f"(g) d = {d}, {tag}: the CG answers (1, 3, 5 steps; user and item step) are "
                "finite and the same bits on a second run")
            gsides = {f"user step, Cholesky, {U} rows": lambda wu=wu: m._solve(
                hist.hist_ptr, hist.hist_idx, U, Y, gy, None, U, x_out, wu)}
            for steps in (1, 3, 5):
                gsides[f"user step, CG {steps} steps (+ x0 copy)"] = \
                    lambda steps=steps, wu=wu: cg_user(steps, wu)
            gsides[f"x0 copy alone [{U}, {d}]"] = lambda: x_cg.copy_(X)
            gsides[f"item step, Cholesky, {I} rows"] = lambda wi=wi: m._solve(
                tptr, tusers, I, X, gx, None, I, y_out, wi)
            for steps in (1, 3, 5):
                gsides[f"item step, CG {steps} steps (+ x0 copy)"] = \
                    lambda steps=steps, wi=wi: cg_item(steps, wi)
            gmed = report(f"(g) CG against Cholesky half-steps, d = {d}, {tag}",
                          interleaved(gsides, args.steps, args.rounds))
            names = list(gmed)
            say("    Cholesky / CG: user step " + ", ".join(
                f"{gmed[names[0]] / gmed[names[k]]:.2f}x at {st} steps"
                for k, st in ((1, 1), (2, 3), (3, 5))) + "; item step " + ", ".join(
                f"{gmed[names[5]] / gmed[names[k]]:.2f}x at {st} steps"
                for k, st in ((6, 1), (7, 3), (8, 5))))
        del x_cg, y_cg
        mf = ImplicitALS(U, I, embedding_dim=d, regularization=REG, alpha=ALPHA).to(dev)
        for tag, h_ in (("unweighted", hist), ("weighted", whist)):
            got = {}
            for solver in ("cholesky", "cg"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                mf.fit_history(h_, iterations=args.sweeps, solver=solver, cg_steps=3)
                torch.cuda.synchronize()
                got[solver] = (time.perf_counter() - t0, mf.loss())
            say(f"(g) fit_history, {args.sweeps} sweeps, d = {d}, {tag}: cholesky "
                f"{got['cholesky'][0]:.3f} s, loss {got['cholesky'][1]:.6e}; cg (3 steps) "
                f"{got['cg'][0]:.3f} s, loss {got['cg'][1]:.6e}; time ratio "
                f"{got['cholesky'][0] / got['cg'][0]:.2f}x, loss ratio cg / cholesky "
                f"{got['cg'][1] / got['cholesky'][1]:.4f}")
        del mf
    if "a" not in SEC:
        del x_out, y_out
        continue
    sides = {
        f"hnm_als_gram_f32 of Y [{I}, {d}]": lambda: m._gram_of(Y, g),
        f"user step: hnm_als_solve_rows_f32, {U} rows": lambda: m._solve(
            hist.hist_ptr, hist.hist_idx, U, Y, gy, None, U, x_out),
        f"hnm_als_gram_f32 of X [{U}, {d}]": lambda: m._gram_of(X, g),
        f"item step: hnm_als_solve_rows_f32, {I} rows": lambda: m._solve(
            tptr, tusers, I, X, gx, None, I, y_out),
    }
    med = report(f"(a) one sweep, d = {d}", interleaved(sides, args.steps, args.rounds))
    say(f"    sum of the four calls: {sum(med.values()):.1f} ms")
    del x_out, y_out

for d in (64, 128) if "b" in SEC else ():
    m = models[d]
    times = []
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m.fit_history(hist, iterations=args.sweeps)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    say(f"(b) fit_history, {args.sweeps} sweeps, d = {d}: {min(times):.3f} s (two runs: "
        f"{times[0]:.3f}, {times[1]:.3f}); loss {m.loss():.6e}")
del models[128]

# ------------------------------------------------------------------ (c) torch on the same GPU
m = models[64]
d = 64
X, Y = m._tables()
gy = m._gram_of(Y).clone()
x_hip = torch.empty_like(X)
x_torch = torch.empty_like(X)
H = int(lens.max())
eye = torch.eye(d, device=dev) * REG


def hip_user_step():
    return m._solve(hist.hist_ptr, hist.hist_idx, U, Y, gy, None, U, x_hip)


def torch_user_step():
    pos = torch.arange(H, device=dev)
    for u0 in range(0, U, args.torch_chunk):
        u1 = min(U, u0 + args.torch_chunk)
        p0, ln = hist.hist_ptr[u0:u1], lens[u0:u1]
        ok = pos[None, :] < ln[:, None]
        at = torch.where(ok, p0[:, None] + pos[None, :], torch.zeros_like(p0[:, None]))
        yg = Y[hist.hist_idx[at].to(torch.int64)] * ok[:, :, None]          # [C, H, d]
        A = gy + ALPHA * torch.bmm(yg.transpose(1, 2), yg) + eye
        b = (1.0 + ALPHA) * yg.sum(1)
        L = torch.linalg.cholesky(A)
        x_torch[u0:u1] = torch.cholesky_solve(b[:, :, None], L)[:, :, 0] * (ln > 0)[:, None]
    return x_torch


if "c" in SEC:
    try:
        hip_user_step()
        torch_user_step()
        assert bool(torch.isfinite(x_hip).all())
        ok_rows = torch.isfinite(x_torch).all(1)
        scale = x_hip.abs().amax(1, keepdim=True).clamp_min(1e-30)
        worst = float(((x_hip - x_torch).abs() / scale)[ok_rows].max())
        say(f"(c) user step, d = {d}: torch (chunks of {args.torch_chunk} users: padded gather, bmm, "
            f"linalg.cholesky, cholesky_solve) against the kernel: max row-relative difference "
            f"{worst:.2e} over the {int(ok_rows.sum())} of {U} rows torch returned finite (the "
            "kernel's rows are all finite)")
        label = "torch chunked cholesky / cholesky_solve"
        if not (worst < 1e-3 and bool(ok_rows.all())):
            # which side is off: float64 torch.linalg.solve of the first 4,096 systems
            n64 = 4096
            pos = torch.arange(H, device=dev)
            ok = pos[None, :] < lens[:n64, None]
            at = torch.where(ok, hist.hist_ptr[:n64, None] + pos[None, :], torch.zeros_like(pos[None, :]))
            yg = (Y[hist.hist_idx[at].to(torch.int64)] * ok[:, :, None]).double()
            A = gy.double() + ALPHA * torch.bmm(yg.transpose(1, 2), yg) + eye.double()
            x64 = torch.linalg.solve(A, ((1.0 + ALPHA) * yg.sum(1))[:, :, None])[:, :, 0]
            x64 = x64 * (lens[:n64] > 0)[:, None]
            s64 = x64.abs().amax(1, keepdim=True).clamp_min(1e-30)
            e_hip = float(((x_hip[:n64] - x64).abs() / s64).max())
            t_rows = ok_rows[:n64]
            e_torch = float(((x_torch[:n64] - x64).abs() / s64)[t_rows].max())
            say(f"    against float64 torch.linalg.solve of the first {n64} systems: the kernel is off "
                f"by at most {e_hip:.2e} of a row's scale, torch's float32 cholesky route by "
                f"{e_torch:.2e} on its {int(t_rows.sum())} finite rows: its time below is that of a "
                "route whose answer was NOT reproduced")
            label += " (answer not reproduced)"
        report("", interleaved({"hnm_als_solve_rows_f32": hip_user_step, label: torch_user_step},
                               args.steps, args.rounds), label)
    except Exception as e:  # noqa: BLE001
        say(f"(c) the torch route failed here: {type(e).__name__}: {e}")
del x_torch

# ------------------------------------------------------------------ (d) numpy / LAPACK on the CPU


def cpu_half_step(ptr, idx, T, chunk=2048):
    T = T.astype(np.float32)
    dd = T.shape[1]
    G = T.T @ T
    n = len(ptr) - 1
    out = np.zeros((n, dd), np.float32)
    rows = np.nonzero(np.diff(ptr) > 0)[0]
    reg_eye = np.float32(REG) * np.eye(dd, dtype=np.float32)
    for c0 in range(0, len(rows), chunk):
        rs = rows[c0:c0 + chunk]
        A = np.empty((len(rs), dd, dd), np.float32)
        b = np.empty((len(rs), dd), np.float32)
        for q, r in enumerate(rs):
            Tr = T[idx[ptr[r]:ptr[r + 1]]]
            A[q] = G + np.float32(ALPHA) * (Tr.T @ Tr) + reg_eye
            b[q] = np.float32(1.0 + ALPHA) * Tr.sum(0)
        out[rs] = np.linalg.solve(A, b[:, :, None])[:, :, 0]
    return out


done = None
for div in (64, 16, 4) if "d" in SEC else ():                    # the full scale is never tried
    su, si = U // div, I // div
    u_s, i_s = syn.interactions(su, si, args.rows // div, seed=2)
    small = ImplicitALS(su, si, embedding_dim=64, regularization=REG, alpha=ALPHA).to(dev)
    y0 = small.item_embeddings.weight.detach().cpu().numpy().copy()
    small.fit_interactions(u_s, i_s, iterations=1)
    h_s = small.history
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(3):
        small.fit_history(h_s, iterations=1)
    torch.cuda.synchronize()
    gpu_ms = (time.perf_counter() - t0) / 3 * 1e3
    ptr_s, idx_s = h_s.hist_ptr.cpu().numpy(), h_s.hist_idx.cpu().numpy()
    tp, tu = (a.cpu().numpy() for a in ImplicitALS._transpose(h_s)[:2])
    t0 = time.perf_counter()
    x_cpu = cpu_half_step(ptr_s, idx_s, y0)
    y_cpu = cpu_half_step(tp, tu, x_cpu)
    cpu_s = time.perf_counter() - t0
    y_gpu = small.item_embeddings.weight.detach().cpu().numpy()
    rel = float((np.abs(y_gpu - y_cpu).max(1) / np.maximum(np.abs(y_cpu).max(1), 1e-30)).max())
    done = div
    say(f"(d) scale 1/{div}: U = {su}, I = {si}, E = {args.rows // div}, d = 64: one sweep in "
        f"numpy/LAPACK float32 {cpu_s:.2f} s on the CPU, on the GPU (fit_history, 1 sweep, "
        f"transpose included) {gpu_ms:.2f} ms; Y differs by at most {rel:.1e} of a row's scale")
    if cpu_s * 6 > args.cpu_budget:                              # the next scale costs > 4x
        break
    del small
if "d" in SEC:
    say(f"    largest scale tried inside {args.cpu_budget:.0f} s: 1/{done}")

# ------------------------------------------------------------------ (e) fold-in + top-12
if "e" in SEC:
    B, K = 4096, 12
    bu = syn.user_batch(U, B, seed=100)
    ptr = hist.hist_ptr.cpu().numpy()
    idx = hist.hist_idx.cpu().numpy()
    rows = [idx[ptr[x]:ptr[x + 1]] for x in bu]
    bptr = np.concatenate([[0], np.cumsum([len(x) for x in rows])]).astype(np.int64)
    baskets = (torch.from_numpy(bptr).to(dev), torch.from_numpy(np.concatenate(rows)).to(dev))
    fv, fi = m.recommend_for_items(baskets, k=K)
    f2 = m.user_factors(baskets)
    m.refresh_users(torch.from_numpy(bu))
    assert torch.equal(m._tables()[0][torch.from_numpy(bu).to(dev)].view(torch.int32),
                       f2.view(torch.int32))                          # fold-in == the user step
    wv, wi = m.recommend_with_scores(torch.from_numpy(bu), filter_items=hist, k=K)
    same = torch.equal(wi, fi) and torch.equal(wv.view(torch.int32), fv.view(torch.int32))
    assert bool((fi >= 0).all()) and bool(torch.isfinite(fv).all())
    say(f"(e) fold-in + top-{K}: B = {B} baskets (the histories of {B} users, mean "
        f"{bptr[-1] / B:.1f} items), d = 64; lists bitwise equal to recommend_with_scores of those "
        f"users after refresh_users: {same}")
    report("", interleaved({
        "recommend_for_items (fold-in + hnm_dot_topk_f32, filtered)": lambda: m.recommend_for_items(
            baskets, k=K),
        "user_factors (fold-in alone)": lambda: m.user_factors(baskets),
        "recommend_with_scores of stored users (filtered)": lambda: m.recommend_with_scores(
            torch.from_numpy(bu), filter_items=hist, k=K)}, 20, args.rounds),
        "recommend_with_scores of stored users (filtered)")

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
