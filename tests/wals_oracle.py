"""Float64 numpy restatement of the weighted ImplicitALS contract (include/hnm.h,
hnm_als_solve_rows_weighted_f32), shared by test_cpu_wals.py and test_gpu_wals.py.  Nothing here
touches the library.

    L(X, Y) = sum_{u,i} c_ui (p_ui - x_u . y_i)^2 + reg (|X|^2 + |Y|^2),  c_ui = 1 + alpha w_ui
    half-step of CSR row r against T:
        (T^T T + alpha sum_j w_j t_j t_j^T + reg I) x = sum_j (1 + alpha w_j) t_j
"""
import numpy as np

import als_oracle as AO


def pair_weights(users, items, weights, U, I):
    """(ptr, idx, w64): the de-duplicated user -> item CSR (UserHistory's layout) and the float64
    weight of every distinct pair, its transactions' weights summed one by one in ascending
    order -- a plain loop, nothing shared with UserHistory."""
    key = np.asarray(users, np.int64) * I + np.asarray(items, np.int64)
    groups = {}
    for k, w in zip(key.tolist(), np.asarray(weights, np.float64).tolist()):
        groups.setdefault(k, []).append(w)
    keys = sorted(groups)
    w64 = np.empty(len(keys), np.float64)
    for n, k in enumerate(keys):
        s = 0.0
        for w in sorted(groups[k]):
            s += w
        w64[n] = s
    r, it = np.divmod(np.asarray(keys, np.int64), I)
    ptr = np.zeros(U + 1, np.int64)
    np.cumsum(np.bincount(r, minlength=U), out=ptr[1:])
    return ptr, it.astype(np.int32), w64


def transpose(ptr, idx, w, U, I):
    """The item -> user CSR (rows ascending by user id) with the weights carried along."""
    rows = np.repeat(np.arange(U, dtype=np.int64), np.diff(ptr))
    items = idx[:ptr[-1]].astype(np.int64)
    order = np.argsort(items, kind="stable")
    tptr = np.zeros(I + 1, np.int64)
    np.cumsum(np.bincount(items, minlength=I), out=tptr[1:])
    return tptr, rows[order].astype(np.int32), np.asarray(w)[:ptr[-1]][order]


def half_step(ptr, idx, w, T, alpha, reg, rows=None):
    """[len(rows), d] float64 solutions (rows: CSR row numbers, default all); empty row -> 0."""
    T = np.asarray(T, np.float64)
    w = np.asarray(w, np.float64)
    d = T.shape[1]
    G = T.T @ T
    rows = range(len(ptr) - 1) if rows is None else rows
    out = np.zeros((len(rows), d), np.float64)
    for b, r in enumerate(rows):
        Tr = T[idx[ptr[r]:ptr[r + 1]]]
        if len(Tr) == 0:
            continue
        wr = w[ptr[r]:ptr[r + 1]]
        A = G + alpha * ((Tr * wr[:, None]).T @ Tr) + reg * np.eye(d)
        out[b] = np.linalg.solve(A, ((1.0 + alpha * wr)[:, None] * Tr).sum(0))
    return out


def sweeps(ptr, idx, w, U, I, Y0, alpha, reg, n):
    """[(X, Y) after sweep 1, ..., after sweep n] in float64 from the initial Y0."""
    tptr, tidx, tw = transpose(ptr, idx, w, U, I)
    Y = np.asarray(Y0, np.float64)
    out = []
    for _ in range(n):
        X = half_step(ptr, idx, w, Y, alpha, reg)
        Y = half_step(tptr, tidx, tw, X, alpha, reg)
        out.append((X, Y))
    return out


def dense_terms(ptr, idx, w, U, I, alpha):
    """(P, C): the dense preference and confidence matrices [U, I]."""
    P = np.zeros((U, I), np.float64)
    C = np.ones((U, I), np.float64)
    r = np.repeat(np.arange(U), np.diff(ptr))
    P[r, idx[:ptr[-1]]] = 1.0
    C[r, idx[:ptr[-1]]] = 1.0 + alpha * np.asarray(w, np.float64)[:ptr[-1]]
    return P, C


def loss_dense(X, Y, ptr, idx, w, alpha, reg):
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    P, C = dense_terms(ptr, idx, w, X.shape[0], Y.shape[0], alpha)
    return float((C * (P - X @ Y.T) ** 2).sum() + reg * ((X ** 2).sum() + (Y ** 2).sum()))


def grad_users(X, Y, ptr, idx, w, alpha, reg):
    """dL/dX [U, d] in float64."""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    P, C = dense_terms(ptr, idx, w, X.shape[0], Y.shape[0], alpha)
    return 2.0 * (C * (X @ Y.T - P)) @ Y + 2.0 * reg * X


def system32(items, w32, T32, G32, alpha, reg):
    """(A, b) of one row formed in float32 from a float32 table, its float32 Gram and float32
    weights."""
    Tr = np.ascontiguousarray(T32[items])
    w32 = np.asarray(w32, np.float32)
    d = T32.shape[1]
    A = G32 + np.float32(alpha) * ((Tr * w32[:, None]).T @ Tr) \
        + np.float32(reg) * np.eye(d, dtype=np.float32)
    b = ((np.float32(1.0) + np.float32(alpha) * w32)[:, None] * Tr).sum(0, dtype=np.float32)
    return A.astype(np.float32), b.astype(np.float32)
