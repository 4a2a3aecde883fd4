"""numpy restatement of the candidate entries' contracts in include/hnm.h
(hnm_cand_union_i32, hnm_cand_topk_f32): what the GPU tests compare against, bit for bit."""
import numpy as np


def union(list_val, list_idx, num_items, ldc=None):
    """list_val [G, B, kc] float32 or None, list_idx [G, B, kc] int64 ->
    (cand int32 [B, ldc], n int32 [B], oob): row b = the distinct non-empty ids of the row's G
    lists, ascending, -1 from n[b] on.  Empty: idx < 0, or a value given and not finite.
    idx >= num_items is skipped and reported (oob)."""
    G, B, kc = list_idx.shape
    ldc = G * kc if ldc is None else ldc
    assert ldc >= G * kc
    cand = np.full((B, ldc), -1, np.int32)
    n = np.zeros(B, np.int32)
    oob = False
    for b in range(B):
        idx = list_idx[:, b, :].reshape(-1)
        live = idx >= 0
        if list_val is not None:
            live &= np.isfinite(list_val[:, b, :].reshape(-1))
        oob |= bool((live & (idx >= num_items)).any())
        ids = np.unique(idx[live & (idx < num_items)])
        n[b] = len(ids)
        cand[b, :len(ids)] = ids
    return cand, n, oob


def select(scores, cand, n, k):
    """scores float32 [B, ldc], cand int32 [B, ldc], n [B] -> (val float32 [B, k], idx int64
    [B, k]): of row b's first n[b] entries those with cand >= 0 and a score that is neither NaN
    nor -inf, best k by (score descending, id ascending); (-inf, -1) past the last one."""
    B, ldc = cand.shape
    val = np.full((B, k), -np.inf, np.float32)
    idx = np.full((B, k), -1, np.int64)
    for b in range(B):
        m = int(min(max(int(n[b]), 0), ldc))
        s, c = scores[b, :m], cand[b, :m]
        ok = (c >= 0) & ~np.isnan(s) & (s != -np.inf)
        s, c = s[ok], c[ok]
        order = np.lexsort((c, -s))[:k]
        val[b, :len(order)] = s[order]
        idx[b, :len(order)] = c[order]
    return val, idx
