"""The numpy restatement of the ContentKNN contract (include/hnm.h, hnm_content_fit_f32), the
oracle of test_gpu_content.py: everything the entry computes is compared BITWISE with these
functions.  No GPU, no library, nothing imported from the package.

* weighting (the host rule of ContentKNN.fit_attributes): per column the non-negative values are
  remapped to a dense vocabulary in ascending order, idf = ln((1 + I) / (1 + df)) + 1 (or 1),
  g = (column_weight * idf)^2, q = rint(g * 2^20 / g_max), all in float64;
* fit: q_if = the weight of item i's code in column f (0: missing, or a code outside the
  vocabulary), n_i = sum_f q_if, S_ij = sum_f [a_if == a_jf >= 0] q_if by broadcasting (dense),
  sim = float32(S / sqrt(float64(n_i) * n_j)) for S > 0, the N best per row by
  lexsort((j, -sim)), padded with (-1, 0.0f); item_count = columns with q_if > 0.
"""
import numpy as np

Q_ONE = float(1 << 20)


def np_weights(attrs, column_weights=None, weighting="idf"):
    """(codes int32 [I, F], code_ptr int64 [F + 1], code_q uint32) from raw attribute values."""
    a = np.asarray(attrs)
    I, F = a.shape
    cw = np.ones(F) if column_weights is None else np.asarray(column_weights, np.float64)
    codes = np.full((I, F), -1, np.int32)
    ptr = [0]
    g = []
    for f in range(F):
        vocab = sorted(set(int(v) for v in a[:, f] if v >= 0))
        where = {v: c for c, v in enumerate(vocab)}
        df = np.zeros(len(vocab), np.float64)
        for i in range(I):
            if a[i, f] >= 0:
                codes[i, f] = where[int(a[i, f])]
                df[codes[i, f]] += 1
        idf = np.log((1.0 + I) / (1.0 + df)) + 1.0 if weighting == "idf" else np.ones(len(vocab))
        g.append((cw[f] * idf) ** 2)
        ptr.append(ptr[-1] + len(vocab))
    g = np.concatenate(g) if g else np.zeros(0)
    g_max = g.max() if g.size else 0.0
    q = np.rint(g * Q_ONE / g_max) if g_max > 0 else np.zeros_like(g)
    return codes, np.asarray(ptr, np.int64), q.astype(np.uint32)


def np_item_q(codes, code_ptr, code_q):
    """(clean codes int64 [I, F] with -1 for missing or out of vocabulary, q int64 [I, F])."""
    codes = np.asarray(codes, np.int64)
    I, F = codes.shape
    clean = np.full((I, F), -1, np.int64)
    q = np.zeros((I, F), np.int64)
    for f in range(F):
        V = int(code_ptr[f + 1] - code_ptr[f])
        ok = (codes[:, f] >= 0) & (codes[:, f] < V)
        clean[ok, f] = codes[ok, f]
        q[ok, f] = np.asarray(code_q, np.int64)[code_ptr[f] + codes[ok, f]]
    return clean, q


def np_content_fit(codes, code_ptr, code_q, N):
    """(nbr_idx int32 [I, N], nbr_val f32 [I, N], item_count int64 [I], sim f32 [I, I], S) --
    dense."""
    clean, q = np_item_q(codes, code_ptr, code_q)
    I, F = clean.shape
    n = q.sum(1)
    count = (q > 0).sum(1).astype(np.int64)
    S = np.zeros((I, I), np.int64)
    for f in range(F):                                        # [I, I] per column, q of the ROW item
        match = (clean[:, None, f] == clean[None, :, f]) & (clean[:, None, f] >= 0)
        S += match * q[:, None, f]
    np.fill_diagonal(S, 0)
    nf = n.astype(np.float64)
    den = np.sqrt(nf[:, None] * nf[None, :])
    sim = np.divide(S.astype(np.float64), den, out=np.zeros((I, I)), where=S > 0).astype(np.float32)
    nbr_idx = np.full((I, N), -1, np.int32)
    nbr_val = np.zeros((I, N), np.float32)
    for i in range(I):
        cand = np.nonzero(S[i] > 0)[0]
        top = cand[np.lexsort((cand, -sim[i, cand]))][:N]
        nbr_idx[i, :len(top)] = top
        nbr_val[i, :len(top)] = sim[i, top]
    return nbr_idx, nbr_val, count, sim, S
