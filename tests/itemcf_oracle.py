"""The numpy restatement of the ItemCF contract (include/hnm.h), the oracle of
test_gpu_itemcf.py and test_gpu_witemcf.py: everything the entries compute is compared BITWISE
with these functions.  No GPU, no library.

Plain entries (hnm_itemcf_fit_f32 / _scores_f32 / _topk_f32):

* fit: n and C over the kept users, sim = float32(C / (sqrt(float64(n_i) * n_j) + shrink)), the
  N best per row in (sim desc, j asc) order, padded with (-1, 0.0f);
* scores: fp32 sums over the history items in ascending order, plain adds;
* top-K: the unmasked items with score > 0 in (score desc, item asc) order, padded with
  (-inf, -1).

Weighted siblings (hnm_itemcf_*_weighted_f32):

* fit: w_max over the kept users' entries, s = 32768 / w_max, q = rint(w * s) in float64,
  A_q^T A_q in integers (n_w on the diagonal), sim = float32(C_w / (sqrt(float64(n_i) * n_j) +
  (shrink * s) * s)), the N best per row as above, item_count = kept users holding the item
  with q > 0;
* scores: fp32 sums over the history items in ascending order of float32(w_j * val), plain adds;
* top-K: the plain selection.
"""
import numpy as np

NEG_INF = float("-inf")


def np_csr(users, items, U, I):
    key = np.unique(np.asarray(users, np.int64) * I + np.asarray(items, np.int64))
    r, it = np.divmod(key, I)
    ptr = np.zeros(U + 1, np.int64)
    np.cumsum(np.bincount(r, minlength=U), out=ptr[1:])
    return ptr, it.astype(np.int32)


def np_fit(ptr, idx, U, I, N, shrink=0.0, max_history=0):
    """(nbr_idx int32 [I, N], nbr_val f32 [I, N], n int64 [I], sim f32 [I, I], C) -- dense."""
    lens = np.diff(ptr)
    A = np.zeros((U, I), np.float64)                       # exact: small integers
    A[np.repeat(np.arange(U), lens), idx] = 1
    if max_history:
        A = A[lens <= max_history]
    C = (A.T @ A).astype(np.int64)
    n = np.diag(C).copy()
    np.fill_diagonal(C, 0)
    nf = n.astype(np.float64)
    den = np.sqrt(nf[:, None] * nf[None, :]) + shrink
    sim = np.divide(C, den, out=np.zeros((I, I)), where=C > 0).astype(np.float32)
    nbr_idx = np.full((I, N), -1, np.int32)
    nbr_val = np.zeros((I, N), np.float32)
    for i in range(I):
        cand = np.nonzero(C[i] > 0)[0]
        top = cand[np.lexsort((cand, -sim[i, cand]))][:N]
        nbr_idx[i, :len(top)] = top
        nbr_val[i, :len(top)] = sim[i, top]
    return nbr_idx, nbr_val, n, sim, C


def np_scores(nbr_idx, nbr_val, I, rows, descending=False):
    """fp32, one plain add per (history item, neighbour), history items in ascending order."""
    out = np.zeros((len(rows), I), np.float32)
    for b, h in enumerate(rows):
        for j in (sorted(h, reverse=True) if descending else sorted(h)):
            ok = nbr_idx[j] >= 0
            out[b, nbr_idx[j][ok]] += nbr_val[j][ok]      # distinct items: one add each
    return out


def np_topk(scores, masks, k):
    B = scores.shape[0]
    ids = np.full((B, k), -1, np.int64)
    vals = np.full((B, k), NEG_INF, np.float32)
    for b in range(B):
        s = scores[b].copy()
        if masks is not None and len(masks[b]):
            s[np.asarray(sorted(masks[b]), np.int64)] = 0.0
        cand = np.nonzero(s > 0)[0]
        top = cand[np.lexsort((cand, -s[cand]))][:k]
        ids[b, :len(top)] = top
        vals[b, :len(top)] = s[top]
    return vals, ids


def np_quantise(ptr, w, U, max_history=0):
    """(q uint64 per entry, s float64, kept bool [U]); s = inf and q = 0 when w_max == 0."""
    lens = np.diff(ptr)
    keep = np.ones(U, bool) if not max_history else lens <= max_history
    ke = keep[np.repeat(np.arange(U), lens)]
    wmax = np.float64(w[ke].max()) if ke.any() else np.float64(0)
    if wmax == 0:
        return np.zeros(len(w), np.uint64), np.float64(np.inf), keep
    s = np.float64(32768.0) / wmax
    return np.rint(w.astype(np.float64) * s).astype(np.uint64), s, keep


def np_fit_w(ptr, idx, w, U, I, N, shrink=0.0, max_history=0, exact_uint64=False):
    """(nbr_idx int32 [I, N], nbr_val f32 [I, N], item_count int64 [I], sim f32 [I, I], C) --
    dense.  The products are taken in float64 after asserting that every sum stays below 2^53
    (then float64 is exact and equals the uint64 sums; `exact_uint64` takes them in uint64)."""
    w = np.asarray(w, np.float32)
    q, s, keep = np_quantise(ptr, w, U, max_history)
    rows = np.repeat(np.arange(U), np.diff(ptr))
    if exact_uint64:
        A = np.zeros((U, I), np.uint64)
        A[rows, idx] = q
        A = A[keep]
        C = A.T @ A
    else:
        A = np.zeros((U, I), np.float64)
        A[rows, idx] = q
        A = A[keep]
        assert float((A * A).sum(0).max(initial=0)) < 2.0 ** 53      # n_w bounds every C_w
        C = (A.T @ A).astype(np.uint64)
    n = np.diag(C).copy()
    np.fill_diagonal(C, 0)
    count = (A > 0).sum(0).astype(np.int64)
    nf = n.astype(np.float64)
    shrink_ss = (np.float64(shrink) * s) * s if np.isfinite(s) else np.float64(0)
    den = np.sqrt(nf[:, None] * nf[None, :]) + shrink_ss
    sim = np.divide(C.astype(np.float64), den, out=np.zeros((I, I)), where=C > 0).astype(np.float32)
    nbr_idx = np.full((I, N), -1, np.int32)
    nbr_val = np.zeros((I, N), np.float32)
    for i in range(I):
        cand = np.nonzero(C[i] > 0)[0]
        top = cand[np.lexsort((cand, -sim[i, cand]))][:N]
        nbr_idx[i, :len(top)] = top
        nbr_val[i, :len(top)] = sim[i, top]
    return nbr_idx, nbr_val, count, sim, C


def np_scores_w(nbr_idx, nbr_val, I, rows, wrows):
    """fp32: per history item j in ascending order, one rounded product and one plain add per
    neighbour.  rows / wrows: ascending item lists and their raw fp32 weights."""
    out = np.zeros((len(rows), I), np.float32)
    for b, (h, ws) in enumerate(zip(rows, wrows)):
        assert list(h) == sorted(h)
        for j, wj in zip(h, ws):
            ok = nbr_idx[j] >= 0
            prod = np.float32(wj) * nbr_val[j][ok]            # float32 * float32: rounded once
            assert prod.dtype == np.float32
            out[b, nbr_idx[j][ok]] += prod                    # distinct items: one add each
    return out
