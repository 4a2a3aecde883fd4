"""The seeded inputs of test_gpu_ensemble.py's raw-entry cases (numpy only, so that what the
cases provide -- ties, short and full rows, negative scores -- can be counted with the oracle
alone): G lists of kc entries for B rows over num_items items, with empties, fully empty rows,
rows whose lists are identical, and a CSR mask."""
import functools

import numpy as np

import fuse_oracle as FO

B = 257
SHAPES = [(1, 1, 1), (2, 12, 12), (3, 48, 12), (4, 64, 64), (8, 256, 128), (16, 128, 100)]
HEAVY, SPARSE = 300, 50_000          # num_items: every hash chain collides / sparse overlap
EMPTY_ROWS, SAME_ROWS = (5, 100, 256), (7, 200)


@functools.lru_cache(maxsize=None)
def lists(G, kc, num_items, seed=0):
    """(vals f32[G, B, kc], idxs int64[G, B, kc]): every list the prefix of a random permutation
    of the items with descending normal scores; then idx = -1, val = -inf and val = nan entries
    at the ends and in the middle."""
    rng = np.random.Generator(np.random.PCG64([seed, G, kc, num_items]))
    idxs = np.empty((G, B, kc), np.int64)
    vals = np.empty((G, B, kc), np.float32)
    for g in range(G):
        for b in range(B):
            idxs[g, b] = rng.choice(num_items, size=kc, replace=False)
            vals[g, b] = np.sort(rng.standard_normal(kc).astype(np.float32))[::-1]
    for g in range(G):
        for b in range(B):
            if rng.random() < 0.5:                         # an empty tail, as a short top-K row
                n = int(rng.integers(1, max(2, kc // 3 + 1)))
                if (b + g) % 3 or kc == 1:
                    idxs[g, b, kc - n:], vals[g, b, kc - n:] = -1, -np.inf
                else:                                      # the dot top-K's: ids stay, -inf
                    vals[g, b, kc - n:] = -np.inf
            for j in rng.integers(0, kc, size=rng.integers(0, 3)):   # holes in the middle
                kind = int(rng.integers(0, 3))
                if kind == 0:
                    idxs[g, b, j] = -1
                else:
                    vals[g, b, j] = -np.inf if kind == 1 else np.nan
    for b in SAME_ROWS:                                    # G identical lists
        idxs[:, b], vals[:, b] = idxs[0, b], vals[0, b]
    for b in EMPTY_ROWS:
        idxs[:, b], vals[:, b] = -1, -np.inf
    idxs.setflags(write=False)
    vals.setflags(write=False)
    return vals, idxs


@functools.lru_cache(maxsize=None)
def mask(G, kc, num_items, seed=0):
    """(mask_ptr int64[B + 1], mask_idx int32): per row up to 24 items, ascending and unique,
    half of them drawn from the row's own lists (so that the mask bites at 50,000 items too);
    every fourth row is empty."""
    _, idxs = lists(G, kc, num_items, seed)
    rng = np.random.Generator(np.random.PCG64([seed + 1, G, kc, num_items]))
    rows = []
    for b in range(B):
        if b % 4 == 3:
            rows.append(np.zeros(0, np.int32))
            continue
        own = idxs[:, b].reshape(-1)
        own = own[own >= 0]
        n = int(rng.integers(1, 13))
        pick = rng.choice(own, size=min(n, own.size), replace=False) if own.size else own
        rows.append(np.unique(np.concatenate([pick, rng.integers(0, num_items, size=n)]))
                    .astype(np.int32))
    ptr = np.zeros(B + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=ptr[1:])
    return ptr, np.concatenate(rows + [np.zeros(1, np.int32)])    # never a zero-size tensor


def coef(mode, G, kc):
    """RANK: equal weights, c = 60 (so that ranks tie exactly); SCORE: a weight per list that
    is no power of two (the product rounds); CASCADE: none."""
    if mode == FO.RANK:
        return FO.rank_table([1.0] * G, 60.0, kc)
    if mode == FO.SCORE:
        return (np.float32(0.3) + np.float32(0.7) * np.arange(1, G + 1, dtype=np.float32)
                / np.float32(3)).astype(np.float32)
    return None


@functools.lru_cache(maxsize=None)
def reference(mode, G, kc, num_items, seed=0):
    """The oracle's row lists before mask and cut (computed once per case, shared)."""
    vals, idxs = lists(G, kc, num_items, seed)
    rows, oob = FO.fuse_full(vals, idxs, mode, coef(mode, G, kc), num_items)
    assert not oob
    return rows


def tie_rows(rows, k):
    """Rows with an exact tie of fused scores among the first k + 1 places."""
    n = 0
    for r in rows:
        head = [float(v) for v, _ in r[:k + 1]]
        n += any(a == b for a, b in zip(head, head[1:]))
    return n
