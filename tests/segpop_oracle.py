"""numpy / Python restatement of SegmentPopularity's two contracts (include/hnm.h):

* `fit`     -- the integer [S + 1, I, D] table (row S = every kept transaction, row s = those of
               users in segment s), then the ascending-day float64 chain acc = acc + cnt * w[d];
* `orders`  -- per row the items with count >= min_count (row S: >= 1), (pop desc, id asc);
* `topk`    -- seg_part = [x for x in order[s] if x not in hist][:k], then the global order
               without hist and seg_part, padded with (-inf, -1), and len(seg_part).

Written for clarity, not speed; tests compute a case once and share it."""
import numpy as np


def fit(items, users, user_segment, days, w, num_items, S, D):
    """(count int64[S + 1, I], pop f64[S + 1, I], skipped): a transaction with an item outside
    [0, I), a user outside the segment table or a segment >= S is skipped entirely (`skipped`
    counts them: the error word); a day outside [0, D) is ignored."""
    items, users = np.asarray(items, np.int64), np.asarray(users, np.int64)
    useg = np.asarray(user_segment, np.int64)
    d = np.zeros(len(items), np.int64) if days is None else np.asarray(days, np.int64)
    ok = (items >= 0) & (items < num_items) & (users >= 0) & (users < len(useg))
    seg = np.full(len(items), -1, np.int64)
    seg[ok] = useg[users[ok]]
    ok &= seg < S
    keep = ok & (d >= 0) & (d < D)
    cnt = np.zeros((S + 1, num_items, D), np.int64)
    np.add.at(cnt, (np.full(keep.sum(), S), items[keep], d[keep]), 1)
    known = keep & (seg >= 0)
    np.add.at(cnt, (seg[known], items[known], d[known]), 1)
    acc = np.zeros((S + 1, num_items), np.float64)
    for j in range(D):
        acc = acc + cnt[:, :, j] * w[j]
    return cnt.sum(2), acc, int((~ok).sum())


def orders(count, pop, min_count=1):
    """([order int64 per row], [order_val f32 per row], rank int32[S + 1, I])."""
    S1, I = count.shape
    out, vals = [], []
    rank = np.full((S1, I), -1, np.int32)
    for s in range(S1):
        ids = np.nonzero(count[s] >= (min_count if s < S1 - 1 else 1))[0]
        o = ids[np.lexsort((ids, -pop[s][ids]))].astype(np.int64)
        rank[s, o] = np.arange(len(o))
        out.append(o)
        vals.append(pop[s][o].astype(np.float32))
    return out, vals, rank


def topk(order_list, val_list, segs, rows, k):
    """(vals f32[B, k], ids int64[B, k], nseg int32[B]).  order_list / val_list: S + 1 arrays,
    the last one global; segs[b] < 0 or >= S: no segment part; rows[b]: the history."""
    S = len(order_list) - 1
    B = len(segs)
    ids = np.full((B, k), -1, np.int64)
    vals = np.full((B, k), -np.inf, np.float32)
    nseg = np.zeros(B, np.int32)
    glob = order_list[S].tolist()
    gval = dict(zip(glob, val_list[S].tolist()))
    for b in range(B):
        s = int(segs[b])
        hist = set(rows[b])
        seg_part, sval = [], {}
        if 0 <= s < S:
            seg_part = [x for x in order_list[s].tolist() if x not in hist][:k]
            sval = dict(zip(order_list[s].tolist(), val_list[s].tolist()))
        taken = set(seg_part)
        rest = [x for x in glob if x not in hist and x not in taken][:k - len(seg_part)]
        row = seg_part + rest
        ids[b, :len(row)] = row
        vals[b, :len(row)] = [sval[x] for x in seg_part] + [gval[x] for x in rest]
        nseg[b] = len(seg_part)
    return vals, ids, nseg
