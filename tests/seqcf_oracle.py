"""The numpy / Python restatement of the SequentialCF contract (include/hnm.h,
hnm_seqcf_fit_f32), the oracle of test_cpu_seqcf.py and test_gpu_seqcf.py: what the entry computes
is compared BITWISE with these functions.  No GPU, no library.

* events: the distinct (user, day, item) triples, a user's sorted by (day ascending, item
  ascending), day = max(days_ago) - days_ago;
* gap table: rint(32768 * exp(-decay * g)), g = 0 .. max_gap - 1, in float64;
* fit: users with more than max_history events are dropped; n[a] = events of a; T[a, b] = the sum
  of gap_q[t - s - 1] over the ordered pairs (a, s), (b, t) of one user with 1 <= t - s <=
  max_gap (a != b unless repeat_buys), in Python integers; sim = float32(float64(T) / (32768 *
  (sqrt(float64(n_a) * n_b) + shrink))) for T > 0; the N best per row in (sim desc, b asc) order,
  padded with (-1, 0.0f).

Everything the fitted table answers is ItemCF's: itemcf_oracle.np_scores_w / np_topk.
"""
import numpy as np


def np_seq_events(u, i, days_ago, U=None):
    """(ptr int64 [U + 1], item int32, day int32) from transaction lists; U defaults to
    max(u) + 1.  Plain Python: a set of triples, sorted."""
    u = [int(x) for x in np.asarray(u).reshape(-1)]
    i = [int(x) for x in np.asarray(i).reshape(-1)]
    d = [int(x) for x in np.asarray(days_ago).reshape(-1)]
    assert len(u) == len(i) == len(d)
    U = (max(u) + 1 if u else 0) if U is None else int(U)
    top = max(d) if d else 0
    ev = sorted({(a, top - c, b) for a, b, c in zip(u, i, d)})
    ptr = np.zeros(U + 1, np.int64)
    for a, _, _ in ev:
        ptr[a + 1] += 1
    np.cumsum(ptr, out=ptr)
    return (ptr, np.asarray([b for _, _, b in ev], np.int32),
            np.asarray([c for _, c, _ in ev], np.int32))


def np_gap_table(max_gap, gap_decay=0.0):
    g = np.arange(int(max_gap), dtype=np.float64)
    return np.rint(32768.0 * np.exp(-np.float64(gap_decay) * g)).astype(np.uint32)


def np_seqcf_fit(ptr, item, day, I, N, shrink, max_history, max_gap, gap_q, repeat_buys):
    """(nbr_idx int32 [I, N], nbr_val f32 [I, N], item_count int64 [I], sim f32 [I, I], T) --
    dense; T is an object array of Python ints (nothing can overflow)."""
    gap_q = [int(x) for x in gap_q]
    assert len(gap_q) == max_gap
    T = np.zeros((I, I), dtype=object)
    T[:] = 0
    n = np.zeros(I, np.int64)
    for u in range(len(ptr) - 1):
        p0, p1 = int(ptr[u]), int(ptr[u + 1])
        if p1 - p0 > max_history:
            continue
        ev = [(int(item[p]), int(day[p])) for p in range(p0, p1)]
        for x, (a, s) in enumerate(ev):
            n[a] += 1
            for b, t in ev[x + 1:]:                       # later positions: t >= s
                g = t - s
                if g < 1 or g > max_gap or (a == b and not repeat_buys):
                    continue
                T[a, b] += gap_q[g - 1]
    assert all(int(x) < 2 ** 64 for x in T.reshape(-1))
    pos = np.array([[int(x) > 0 for x in row] for row in T], dtype=bool).reshape(I, I)
    Tf = np.array([[float(int(x)) for x in row] for row in T], np.float64).reshape(I, I)
    nf = n.astype(np.float64)
    den = np.float64(32768.0) * (np.sqrt(nf[:, None] * nf[None, :]) + np.float64(shrink))
    sim = np.divide(Tf, den, out=np.zeros((I, I)), where=pos).astype(np.float32)
    nbr_idx = np.full((I, N), -1, np.int32)
    nbr_val = np.zeros((I, N), np.float32)
    for a in range(I):
        cand = np.nonzero(pos[a])[0]
        top = cand[np.lexsort((cand, -sim[a, cand]))][:N]
        nbr_idx[a, :len(top)] = top
        nbr_val[a, :len(top)] = sim[a, top]
    return nbr_idx, nbr_val, n, sim, T
