"""Float64 numpy restatement of the ImplicitALS contract (include/hnm.h), shared by
test_cpu_als.py and test_gpu_als.py.  Nothing here touches the library.

    L(X, Y) = sum_{u,i} c_ui (p_ui - x_u . y_i)^2 + reg (|X|^2 + |Y|^2)
    half-step of CSR row r against T:  (T^T T + alpha sum_j t_j t_j^T + reg I) x = (1 + alpha) sum_j t_j
"""
import numpy as np


def csr(users, items, U, I):
    """De-duplicated user -> item CSR, rows ascending (UserHistory's layout)."""
    key = np.unique(np.asarray(users, np.int64) * I + np.asarray(items, np.int64))
    r, it = np.divmod(key, I)
    ptr = np.zeros(U + 1, np.int64)
    np.cumsum(np.bincount(r, minlength=U), out=ptr[1:])
    return ptr, it.astype(np.int32)


def transpose(ptr, idx, U, I):
    """The item -> user CSR, rows ascending by user id."""
    rows = np.repeat(np.arange(U, dtype=np.int64), np.diff(ptr))
    items = idx[:ptr[-1]].astype(np.int64)
    order = np.argsort(items, kind="stable")
    tptr = np.zeros(I + 1, np.int64)
    np.cumsum(np.bincount(items, minlength=I), out=tptr[1:])
    return tptr, rows[order].astype(np.int32)


def half_step(ptr, idx, T, alpha, reg, rows=None):
    """[len(rows), d] float64 solutions (rows: CSR row numbers, default all); empty row -> 0."""
    T = np.asarray(T, np.float64)
    d = T.shape[1]
    G = T.T @ T
    rows = range(len(ptr) - 1) if rows is None else rows
    out = np.zeros((len(rows), d), np.float64)
    for b, r in enumerate(rows):
        Tr = T[idx[ptr[r]:ptr[r + 1]]]
        if len(Tr) == 0:
            continue
        A = G + alpha * (Tr.T @ Tr) + reg * np.eye(d)
        out[b] = np.linalg.solve(A, (1.0 + alpha) * Tr.sum(0))
    return out


def sweeps(ptr, idx, U, I, Y0, alpha, reg, n):
    """[(X, Y) after sweep 1, ..., after sweep n] in float64 from the initial Y0."""
    tptr, tidx = transpose(ptr, idx, U, I)
    Y = np.asarray(Y0, np.float64)
    out = []
    for _ in range(n):
        X = half_step(ptr, idx, Y, alpha, reg)
        Y = half_step(tptr, tidx, X, alpha, reg)
        out.append((X, Y))
    return out


def dense_terms(ptr, idx, U, I, alpha):
    """(P, C): the dense preference and confidence matrices [U, I]."""
    P = np.zeros((U, I), np.float64)
    P[np.repeat(np.arange(U), np.diff(ptr)), idx[:ptr[-1]]] = 1.0
    return P, 1.0 + alpha * P


def loss_dense(X, Y, ptr, idx, alpha, reg):
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    P, C = dense_terms(ptr, idx, X.shape[0], Y.shape[0], alpha)
    return float((C * (P - X @ Y.T) ** 2).sum() + reg * ((X ** 2).sum() + (Y ** 2).sum()))


def grad_users(X, Y, ptr, idx, alpha, reg):
    """dL/dX [U, d] in float64."""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    P, C = dense_terms(ptr, idx, X.shape[0], Y.shape[0], alpha)
    return 2.0 * (C * (X @ Y.T - P)) @ Y + 2.0 * reg * X


def system32(items, T32, G32, alpha, reg):
    """(A, b) of one row formed in float32 from a float32 table and its float32 Gram."""
    Tr = np.ascontiguousarray(T32[items])
    d = T32.shape[1]
    A = G32 + np.float32(alpha) * (Tr.T @ Tr) + np.float32(reg) * np.eye(d, dtype=np.float32)
    b = np.float32(1.0 + alpha) * Tr.sum(0, dtype=np.float32)
    return A.astype(np.float32), b.astype(np.float32)
