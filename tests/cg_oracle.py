"""Float64 numpy restatement of the conjugate-gradient half-step (include/hnm.h,
hnm_als_cg_rows_f32 and its weighted sibling), shared by test_cpu_als_cg.py and
test_gpu_als_cg.py.  Nothing here touches the library.

    half-step of CSR row r against T from the start vector x0:
        A = T^T T + alpha sum_j w_j t_j t_j^T + reg I,  b = sum_j (1 + alpha w_j) t_j   (w = 1)
        `steps` CG steps on A x = b from x0

Also the 20-row CSR the raw-entry tests run on, and an fp32 restatement of the recurrence in two
summation orders, used only to vet the GPU test's case list: how much of the bar fp32 rounding
alone takes, whatever the order of the sums.
"""
import functools

import numpy as np

NI = 193
LENGTHS = [0, 1, 2, 5, 17, 64, 150, 193]


@functools.lru_cache(maxsize=None)
def solve_rows():
    """(ptr, idx): rows of the fixed lengths plus a dozen random ones below 40; each row is a
    random subset of the table in random (unsorted) order."""
    rng = np.random.default_rng(11)
    lens = LENGTHS + rng.integers(0, 40, 12).tolist()
    rows = [rng.permutation(NI)[:n].astype(np.int32) for n in lens]
    ptr = np.zeros(len(rows) + 1, np.int64)
    np.cumsum(lens, out=ptr[1:])
    return ptr, np.concatenate(rows)


def case_inputs(d, std, x0_kind):
    """(T f32 [NI, d], X0 f32 [20, d]) of a raw-entry case: the table N(0, std^2); x0 zeros, or
    N(0, s^2) with s = 1 for std 0.1 and 0.1 for std 1 ("random").  The empty rows start from
    1.0 in both kinds: their x0 must be ignored."""
    T = np.random.default_rng(d * 7 + int(std * 10)).normal(0, std, (NI, d)).astype(np.float32)
    ptr, _ = solve_rows()
    n = len(ptr) - 1
    if x0_kind == "zeros":
        X0 = np.zeros((n, d), np.float32)
    else:
        s = 1.0 if std < 0.5 else 0.1
        X0 = np.random.default_rng(d * 13 + int(std * 10) + 1).normal(0, s, (n, d)).astype(np.float32)
    X0[np.diff(ptr) == 0] = 1.0
    return T, X0


def cg(A, b, x0, steps, trace=None):
    """`steps` CG steps on A x = b from x0, in the dtype of A (float64 here).  trace: a list that
    receives x after every step."""
    x = np.array(x0, dtype=A.dtype)
    r = b - A @ x
    p = r.copy()
    rs = r @ r
    for _ in range(steps):
        if not rs > 0:
            break
        q = A @ p
        pq = p @ q
        if not pq > 0:
            break
        a = rs / pq
        x = x + a * p
        r = r - a * q
        rn = r @ r
        p = r + (rn / rs) * p
        rs = rn
        if trace is not None:
            trace.append(x.copy())
    return x


def system(items, T, G, alpha, reg, w=None):
    """(A, b) of one row in float64 (T, G float64; w: the row's weights or None)."""
    Tr = T[items]
    d = T.shape[1]
    if w is None:
        return G + alpha * (Tr.T @ Tr) + reg * np.eye(d), (1.0 + alpha) * Tr.sum(0)
    w = np.asarray(w, np.float64)
    return (G + alpha * ((Tr * w[:, None]).T @ Tr) + reg * np.eye(d),
            ((1.0 + alpha * w)[:, None] * Tr).sum(0))


def cg_half_step(ptr, idx, T, alpha, reg, X0, steps, w=None, rows=None):
    """[len(rows), d] float64: the CG half-step of CSR rows `rows` (default all) against the
    table T (read as given, e.g. an fp32 table, and widened), row b starting from X0[b]; an empty
    row -> 0 whatever its X0.  w: float weights aligned with idx (wals_oracle's convention)."""
    T = np.asarray(T, np.float64)
    G = T.T @ T
    rows = range(len(ptr) - 1) if rows is None else rows
    out = np.zeros((len(rows), T.shape[1]), np.float64)
    for b, r in enumerate(rows):
        lo, hi = ptr[r], ptr[r + 1]
        if hi == lo:
            continue
        A, rhs = system(idx[lo:hi], T, G, alpha, reg, None if w is None else w[lo:hi])
        out[b] = cg(A, rhs, np.asarray(X0[b], np.float64), steps)
    return out


def transpose(ptr, idx, U, I, w=None):
    """The item -> user CSR (rows ascending by user id), the weights carried along."""
    rows = np.repeat(np.arange(U, dtype=np.int64), np.diff(ptr))
    items = idx[:ptr[-1]].astype(np.int64)
    order = np.argsort(items, kind="stable")
    tptr = np.zeros(I + 1, np.int64)
    np.cumsum(np.bincount(items, minlength=I), out=tptr[1:])
    return tptr, rows[order].astype(np.int32), None if w is None else np.asarray(w)[:ptr[-1]][order]


def cg_sweeps(ptr, idx, U, I, Y0, alpha, reg, n, steps, w=None):
    """[(X, Y) after sweep 1, ..., after sweep n] in float64: X from zeros, Y from Y0, every
    half-step `steps` CG steps from the previous sweep's rows."""
    tptr, tidx, tw = transpose(ptr, idx, U, I, w)
    Y = np.asarray(Y0, np.float64)
    X = np.zeros((U, Y.shape[1]), np.float64)
    out = []
    for _ in range(n):
        X = cg_half_step(ptr, idx, Y, alpha, reg, X, steps, w)
        Y = cg_half_step(tptr, tidx, X, alpha, reg, Y, steps, tw)
        out.append((X, Y))
    return out


# ------------------------------------------------------------------ fp32, two summation orders
def _dot32(u, v, reverse):
    s = np.float32(0.0)
    prod = (u * v).astype(np.float32)
    for z in (prod[::-1] if reverse else prod):
        s = np.float32(s + z)
    return s


def _matvec32(A, v, reverse):
    order = range(len(v) - 1, -1, -1) if reverse else range(len(v))
    acc = np.zeros(A.shape[0], np.float32)
    for j in order:
        acc = (acc + A[:, j] * v[j]).astype(np.float32)
    return acc


def cg32(A, b, x0, steps, reverse=False):
    """The recurrence in fp32 with every sum taken one term at a time, ascending (forward) or
    descending (reversed): two fp32 answers that differ only in summation order."""
    A, b = A.astype(np.float32), b.astype(np.float32)
    x = np.array(x0, np.float32)
    r = (b - _matvec32(A, x, reverse)).astype(np.float32)
    p = r.copy()
    rs = _dot32(r, r, reverse)
    for _ in range(steps):
        if not rs > 0:
            break
        q = _matvec32(A, p, reverse)
        pq = _dot32(p, q, reverse)
        if not pq > 0:
            break
        a = np.float32(rs / pq)
        x = (x + a * p).astype(np.float32)
        r = (r - a * q).astype(np.float32)
        rn = _dot32(r, r, reverse)
        p = (r + np.float32(rn / rs) * p).astype(np.float32)
        rs = rn
    return x


def cg32_half_step(ptr, idx, T32, alpha, reg, X0, steps, reverse=False, w=None):
    """cg_half_step with the system formed and the recurrence run in fp32."""
    T32 = np.asarray(T32, np.float32)
    G = (T32.T @ T32).astype(np.float32)
    d = T32.shape[1]
    out = np.zeros((len(ptr) - 1, d), np.float32)
    for r in range(len(ptr) - 1):
        lo, hi = ptr[r], ptr[r + 1]
        if hi == lo:
            continue
        Tr = np.ascontiguousarray(T32[idx[lo:hi]])
        if w is None:
            A = G + np.float32(alpha) * (Tr.T @ Tr)
            rhs = np.float32(1.0 + alpha) * Tr.sum(0, dtype=np.float32)
        else:
            wr = np.asarray(w[lo:hi], np.float32)
            A = G + np.float32(alpha) * ((Tr * wr[:, None]).T @ Tr)
            rhs = ((np.float32(1.0) + np.float32(alpha) * wr)[:, None] * Tr).sum(0, dtype=np.float32)
        A = (A + np.float32(reg) * np.eye(d, dtype=np.float32)).astype(np.float32)
        out[r] = cg32(A, rhs.astype(np.float32), X0[r], steps, reverse)
    return out


def bar_use(got, ref):
    """max |got - ref| / (the tolerance parity.assert_scores_close allows there): 1e-4 of the
    row's scale plus 1e-4 relative."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = np.maximum(np.abs(ref).max(1, keepdims=True), 1e-30)
    return float((np.abs(got - ref) / (1e-4 * scale + 1e-4 * np.abs(ref))).max())
