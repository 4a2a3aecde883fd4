"""numpy restatement of hnm_fuse_topk_f32's contract (include/hnm.h): the fusion of G
overlapping top-K lists per row.  A per-row dict of np.float32 sums taken in ascending g, a
`sorted` by (-score, item); the cascade rule, the empty entries, the CSR mask and the skip of
out-of-range ids.  Written for clarity, not speed: a test computes a case once and shares it
(`fuse_full` does not depend on the mask or on k, `cut` applies both)."""
import numpy as np

RANK, SCORE, CASCADE = 0, 1, 2
MODES = {"rrf": RANK, "score": SCORE, "cascade": CASCADE}


def rank_table(weights, rank_constant, depth):
    """coef[g, j] = float32(w_g) / (float32(c) + float32(j + 1)), every step in float32: what
    `Ensemble.rank_weights()` returns."""
    w = np.asarray(weights, np.float32).reshape(-1, 1)
    ranks = np.arange(1, depth + 1, dtype=np.float32).reshape(1, -1)
    return (w / (np.float32(rank_constant) + ranks)).astype(np.float32)


def fuse_row(vals, idxs, mode, coef, num_items):
    """One row, before the mask and the cut at k.  vals f32[G, kc], idxs int64[G, kc]; coef:
    RANK f32[G, kc], SCORE f32[G], CASCADE ignored.  Returns ([(score, item), ...] in output
    order, saw_out_of_range)."""
    G, kc = idxs.shape
    vals = np.asarray(vals, np.float32)
    if mode != CASCADE:
        coef = np.asarray(coef, np.float32)
    fused, first, oob = {}, {}, False
    for g in range(G):
        for j, it in enumerate(idxs[g].tolist()):
            v = vals[g, j]                                # an np.float32
            if it < 0 or not np.isfinite(v):
                continue                                  # empty
            if it >= num_items:
                oob = True                                # raises the error word, skipped
                continue
            if mode == CASCADE:
                first.setdefault(it, (g * kc + j, v))     # the lowest g, then its position
                continue
            c = coef[g, j] if mode == RANK else coef[g] * v      # one fp32 rounding
            # the sum starts from the first contribution itself, then plain fp32 adds
            fused[it] = c if it not in fused else fused[it] + c
    if mode == CASCADE:
        return [(v, it) for _, it, v in sorted((key, it, v) for it, (key, v) in first.items())], oob
    order = sorted((-float(s), it) for it, s in fused.items())
    return [(fused[it], it) for _, it in order], oob


def fuse_full(vals, idxs, mode, coef, num_items):
    """vals f32[G, B, kc], idxs int64[G, B, kc] -> ([row lists], saw_out_of_range)."""
    rows, any_oob = [], False
    for b in range(idxs.shape[1]):
        r, oob = fuse_row(vals[:, b], idxs[:, b], mode, coef, num_items)
        rows.append(r)
        any_oob |= oob
    return rows, any_oob


def cut(rows, k, mask_ptr=None, mask_idx=None):
    """The outputs: per row the first k entries whose item is not in the row of the CSR mask,
    padded with (-inf, -1).  (out_val f32[B, k], out_idx int64[B, k], entries per row before
    the cut at k)."""
    B = len(rows)
    out_v = np.full((B, k), -np.inf, np.float32)
    out_i = np.full((B, k), -1, np.int64)
    count = np.zeros(B, np.int64)
    for b, r in enumerate(rows):
        if mask_ptr is not None:
            masked = set(mask_idx[int(mask_ptr[b]):int(mask_ptr[b + 1])].tolist())
            r = [(v, it) for v, it in r if it not in masked]
        count[b] = len(r)
        for s, (v, it) in enumerate(r[:k]):
            out_v[b, s], out_i[b, s] = v, it
    return out_v, out_i, count


def fuse(vals, idxs, mode, coef, num_items, k, mask_ptr=None, mask_idx=None):
    """(out_val f32[B, k], out_idx int64[B, k], entries per row before the cut,
    saw_out_of_range)."""
    rows, oob = fuse_full(vals, idxs, mode, coef, num_items)
    return (*cut(rows, k, mask_ptr, mask_idx), oob)
