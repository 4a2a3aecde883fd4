"""Lattice inputs and plain-numpy references for the top-K order tests (no GPU needed).

With embeddings and weights that are small integers (biases: quarter-integers for the dot
models, integers for NeuralCF) every product and every partial sum of a score is exactly
representable in fp32, so the fp32 score is the same number in any summation order, fused or
not, on the matrix pipe or the vector pipe: an integer computation in numpy is a BITWISE
oracle of the GPU's fp32 score.  Such scores take a few dozen distinct values, so exact ties
sit at every position of every top-K, and the library's total order (score descending, item
id ascending) decides most rows.

Wide&Deep joins them through BatchNorm statistics whose sqrt(running_var + eps) is 0.5, 1 or 2
exactly in fp32 (see WD_EPS below): its intermediates are multiples of 2^-3.

`dot_scores` / `ncf_scores` / `wd_scores` assert the magnitudes that make the argument hold
instead of assuming them.  NaN never appears in any input here (the routes treat it differently by
design).  The GPU modules share the case tables at the bottom with tests/test_cpu_lattice.py,
which checks on the CPU that the inputs have the properties the GPU tests rely on.
"""
from __future__ import annotations

import functools

import numpy as np

EXACT = float(1 << 24)  # integers of magnitude below 2^24 are exact in fp32


def _rng(*seed):
    return np.random.Generator(np.random.PCG64([int(s) & 0xFFFFFFFF for s in seed]))


# ---------------------------------------------------------------------------- generators
def dot_tables(U, I, d, values=(-1, 0, 1), bias=False, seed=0):
    """Integer user / item tables [U, d] / [I, d]; with `bias` the user, item and constant
    biases are multiples of 0.25 in [-2, 2].  float32."""
    rng = _rng(seed, U, I, d)
    vals = np.asarray(values, np.float32)
    t = {"ut": vals[rng.integers(0, len(vals), (U, d))],
         "it": vals[rng.integers(0, len(vals), (I, d))],
         "ub": None, "ib": None, "cb": None}
    if bias:
        q = (np.arange(17, dtype=np.float32) - 8) * np.float32(0.25)
        # item biases cluster on few of the 17 quarter-integers so that ties stay frequent
        t["ub"] = q[rng.integers(0, 17, U)]
        t["ib"] = q[rng.choice(17, I, p=_peaked(17))]
        t["cb"] = q[rng.integers(0, 17, 1)]
    return t


def _peaked(n):
    p = np.full(n, 0.02 / (n - 3))
    p[[n // 2 - 4, n // 2, n // 2 + 4]] = 0.98 / 3  # -1, 0, +1
    return p / p.sum()


def clustered_tables(U, I, d, block=300, start=2000, seed=0):
    """Ternary tables whose item rows [start, start + block) are copies of one row, user 0's
    best item (sign(u_0): no other row scores as high for user 0).  Every user ties the block,
    it lies in one item partition, and user 0's top-k is the block's first k ids."""
    t = dot_tables(U, I, d, seed=seed)
    t["it"][start:start + block] = np.sign(t["ut"][0])
    return t


NCF_DENSITIES = {"emb": 0.5, "w": 0.1, "pred": 0.3}


def _ternary(rng, shape, density):
    return (rng.choice(np.array([-1, 1], np.float32), shape) *
            (rng.random(shape) < density)).astype(np.float32)


def ncf_state_dict(U, I, mf=64, mlp_dims=(128, 64, 32), densities=None, seed=0):
    """NeuralCF state dict (key layout of synthetic.ncf_state_dict) with sparse ternary weights
    and integer biases in [-2, 2]; any tower depth (len(mlp_dims) - 1 Linear layers)."""
    dn = dict(NCF_DENSITIES, **(densities or {}))
    rng = _rng(seed, U, I, mf, len(mlp_dims))
    h = mlp_dims[0] // 2
    sd = {"gmf_user_embedding.weight": _ternary(rng, (U, mf), dn["emb"]),
          "gmf_item_embedding.weight": _ternary(rng, (I, mf), dn["emb"]),
          "mlp_user_embedding.weight": _ternary(rng, (U, h), dn["emb"]),
          "mlp_item_embedding.weight": _ternary(rng, (I, h), dn["emb"])}
    for l in range(len(mlp_dims) - 1):
        sd[f"mlp_layers.{3 * l}.weight"] = _ternary(rng, (mlp_dims[l + 1], mlp_dims[l]), dn["w"])
        sd[f"mlp_layers.{3 * l}.bias"] = rng.integers(-2, 3, mlp_dims[l + 1]).astype(np.float32)
    sd["prediction_layer.weight"] = _ternary(rng, (1, mf + mlp_dims[-1]), dn["pred"])
    sd["prediction_layer.bias"] = rng.integers(-2, 3, 1).astype(np.float32)
    return sd


def ncf_deep_state_dict(U, I, mf=64, mlp_dims=(128, 64, 32, 16), densities=None, seed=0):
    """The 3-layer deep-tower variant (hnm_ncf_deep_*)."""
    return ncf_state_dict(U, I, mf, mlp_dims, densities, seed)


DENSE_KINDS = ("levels", "zeros", "inf", "denormal", "const", "ramp_up", "ramp_down")


def dense_rows(B, I, kind, seed=0):
    """[B, I] float32 rows for the stand-alone selection kernels."""
    rng = _rng(seed, B, I, DENSE_KINDS.index(kind))
    if kind == "levels":  # 8 distinct values
        s = (rng.integers(0, 8, (B, I)) - 3) * 0.5
    elif kind == "zeros":  # +0 and -0 among few levels
        s = np.array([0.0, -0.0, 0.0, -0.0, 1.0, -1.0], np.float32)[rng.integers(0, 6, (B, I))]
    elif kind == "inf":  # some +inf, some natural -inf, otherwise levels
        s = ((rng.integers(0, 8, (B, I)) - 3) * 0.5).astype(np.float32)
        r = rng.random((B, I))
        s[r < 0.03] = np.inf
        s[r > 0.95] = -np.inf
    elif kind == "denormal":  # {1, 2, 3} * 2^-149, their negatives, zeros
        s = np.ldexp(np.float32(1), -149) * (rng.integers(0, 7, (B, I)) - 3).astype(np.float32)
    elif kind == "const":
        s = np.full((B, I), 2.5)
    elif kind == "ramp_up":  # strictly monotone in id: every item displaces the list's tail
        s = np.arange(I, dtype=np.float32)[None, :] + np.arange(B, dtype=np.float32)[:, None]
    elif kind == "ramp_down":
        s = -np.arange(I, dtype=np.float32)[None, :] - np.arange(B, dtype=np.float32)[:, None]
    else:
        raise ValueError(kind)
    s = np.ascontiguousarray(s, dtype=np.float32)
    assert not np.isnan(s).any()
    return s


MASK_KINDS = ("none", "random", "dups_oob", "tie_group", "all_but_few", "all", "empty_between")


def _mask_row(rng, I, kind, row, k):
    """Masked ids of one row, ascending.  `row`: the row's scores (tie_group only)."""
    if kind == "none" or I == 0:
        return np.zeros(0, np.int64)
    if kind == "random":
        return np.unique(rng.integers(0, I, max(1, min(I // 3, 40))))
    if kind == "dups_oob":  # duplicates inside the row, ids >= I at its tail
        m = rng.integers(0, I, max(2, min(I // 3, 40)))
        return np.sort(np.concatenate([m, m[: len(m) // 2 + 1], [I, I + 1, I + 7]]))
    if kind == "tie_group":  # every member of the tie group at position k except the last
        order = np.argsort(-row, kind="stable")
        grp = np.nonzero(row == row[order[min(k, I) - 1]])[0]
        return grp[:-1]
    if kind == "all_but_few":  # all but k - 3 items (none left for k <= 3)
        keep = rng.choice(I, min(max(k - 3, 0), I), replace=False)
        return np.setdiff1d(np.arange(I), keep)
    if kind == "all":
        return np.arange(I)
    raise ValueError(kind)


def masks(B, I, kind, scores=None, k=1, seed=0):
    """CSR mask (mask_ptr int64[B + 1], mask_idx int32, rows ascending), or (None, None).
    "empty_between": an empty row between two masked rows; "mixed": the kinds row by row."""
    if kind == "none":
        return None, None
    rng = _rng(seed, B, I, k)
    cycle = ("tie_group", "random", "all_but_few", "none", "all", "dups_oob")
    rows = []
    for b in range(B):
        kd = kind
        if kind == "empty_between":
            kd = "none" if b % 3 == 1 else "random"
        elif kind == "mixed":
            kd = cycle[b % len(cycle)]
        rows.append(_mask_row(rng, I, kd, None if scores is None else scores[b], k))
    ptr = np.zeros(B + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=ptr[1:])
    idx = np.concatenate(rows + [np.zeros(1, np.int64)]).astype(np.int32)  # never empty
    return ptr, idx


# ---------------------------------------------------------------------------- references
def apply_mask(scores, mask):
    d = np.array(scores, np.float32, copy=True)
    if mask is not None and mask[0] is not None:
        ptr, idx = mask
        for b in range(d.shape[0]):
            m = idx[ptr[b]:ptr[b + 1]]
            d[b, m[(m >= 0) & (m < d.shape[1])]] = -np.inf
    return d


def ref_topk(scores, k, mask=None):
    """(values [B, k] float32, ids [B, k] int64) in (score desc, id asc) order: masked entries
    are -inf, the values are the bits of the masked matrix at the chosen positions (a returned
    -0 stays -0), positions past the row are (-inf, -1)."""
    d = apply_mask(scores, mask)
    B, I = d.shape
    order = np.argsort(-d, axis=1, kind="stable")[:, :k]
    vals = np.take_along_axis(d, order, 1)
    if k > I:
        vals = np.concatenate([vals, np.full((B, k - I), -np.inf, np.float32)], 1)
        order = np.concatenate([order, np.full((B, k - I), -1, np.int64)], 1)
    return vals, order.astype(np.int64)


def ref_merge(vals, gids, k):
    """vals / gids [B, N]: over the candidates with id >= 0, the first k in (value desc, id asc)
    order, padded with (-inf, -1); (-inf, id >= 0) is a real candidate and ranks before padding."""
    vals = np.asarray(vals, np.float32)
    gids = np.asarray(gids, np.int64)
    B = vals.shape[0]
    ov = np.full((B, k), -np.inf, np.float32)
    oi = np.full((B, k), -1, np.int64)
    for b in range(B):
        ok = np.nonzero(gids[b] >= 0)[0]
        o = ok[np.lexsort((gids[b, ok], -vals[b, ok]))][:k]
        ov[b, :len(o)] = vals[b, o]
        oi[b, :len(o)] = gids[b, o]
    return ov, oi


def ref_kth(lists, k):
    """lists [G, B, kc]: the k-th best value of each row's union of the G lists."""
    G, B, kc = lists.shape
    u = np.sort(np.transpose(lists, (1, 0, 2)).reshape(B, G * kc), axis=1)[:, ::-1]
    return np.ascontiguousarray(u[:, k - 1])


def assert_short_rows(got_v, got_i, ref_v, ref_i, bound):
    """A two-phase `finish` with short_ok = 1 and a caller's bound: every row is a prefix of the
    reference top-k, at least as long as the number of top-k items scoring >= the bound,
    followed only by (-inf, -1).  The exact length is not fixed (hnm.h does not fix it)."""
    for b in range(ref_i.shape[0]):
        need = int(np.sum(ref_v[b] >= bound[b]))
        n = int(np.sum(got_i[b] >= 0))
        assert n >= need, (b, n, need)
        assert np.array_equal(got_i[b, :n], ref_i[b, :n]), (b, got_i[b], ref_i[b])
        assert np.array_equal(bits(got_v[b, :n]), bits(ref_v[b, :n])), b
        assert (got_i[b, n:] == -1).all() and np.isneginf(got_v[b, n:]).all(), b


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def dot_scores(t, users, check_orders=True):
    """Exact scores [B, I] (float32) of users against every item: float64 arithmetic, with the
    assertions that make it a bitwise oracle of ANY fp32 evaluation -- every partial sum is a
    multiple of 0.25 of magnitude below 2^22 -- and the check that two fp32 evaluations in
    different summation orders give exactly this matrix."""
    u = t["ut"][users].astype(np.float64)
    it = t["it"].astype(np.float64)
    s = u @ it.T
    mag = np.abs(u) @ np.abs(it).T
    for key, sel in (("ub", users), ("ib", slice(None)), ("cb", 0)):
        if t[key] is not None:
            b = t[key].astype(np.float64)[sel]
            b = b[:, None] if key == "ub" else b
            s = s + b
            mag = mag + np.abs(b)
            assert np.array_equal(b * 4, np.round(b * 4)), key
    assert np.array_equal(u, np.round(u)) and np.array_equal(it, np.round(it))
    assert 4 * mag.max() < EXACT, mag.max()
    out = (s + 0.0).astype(np.float32)  # an exact zero is +0 in every fp32 chain that starts at +0
    assert np.array_equal(out.astype(np.float64), s)
    if check_orders:
        u32, i32 = t["ut"][users], t["it"]
        d = u32.shape[1]
        for order in (range(d), range(d - 1, -1, -1)):
            acc = np.zeros(s.shape, np.float32)
            for c in order:
                acc += u32[:, c, None] * i32[None, :, c]
            if t["ub"] is not None:
                acc = (acc + (t["ub"][users] + t["cb"][0])[:, None]) + t["ib"][None, :]
            assert np.array_equal(bits(acc + np.float32(0)), bits(out + np.float32(0)))
    return out


def ncf_scores(sd, users, items=None):
    """Exact NeuralCF scores: [B, I] over every item, or [n] over (users, items) pairs; any tower
    depth.  float64 arithmetic on integer-valued weights (exact far beyond fp32's range), with
    the assertions that every weight is an integer and that the sum of absolute values behind
    every intermediate stays below 2^24, so fp32 is exact in any summation order."""
    Z = {k: np.asarray(v).astype(np.float64) for k, v in sd.items()}
    for v in Z.values():
        assert np.array_equal(v, np.round(v))
    nl = sum(1 for k in Z if k.startswith("mlp_layers.") and k.endswith(".weight"))
    users = np.asarray(users)
    if items is None and len(users) > 16:  # [rows, I, h1] intermediates: a few rows at a time
        return np.concatenate([ncf_scores(sd, users[i:i + 16]) for i in range(0, len(users), 16)])
    gu, mu = Z["gmf_user_embedding.weight"][users], Z["mlp_user_embedding.weight"][users]
    gi, mi = Z["gmf_item_embedding.weight"], Z["mlp_item_embedding.weight"]
    pair = items is not None
    if pair:
        gi, mi = gi[items], mi[items]
    mf, h0 = gu.shape[1], mu.shape[1]
    wp, bp = Z["prediction_layer.weight"][0], Z["prediction_layer.bias"][0]
    W1, b1 = Z["mlp_layers.0.weight"], Z["mlp_layers.0.bias"]
    pu, qi = mu @ W1[:, :h0].T, mi @ W1[:, h0:].T
    apu, aqi = np.abs(mu) @ np.abs(W1[:, :h0]).T, np.abs(mi) @ np.abs(W1[:, h0:]).T
    if pair:
        x, ax = pu + qi + b1, apu + aqi + np.abs(b1)
        gmf, agmf = (gu * gi) @ wp[:mf], (np.abs(gu) * np.abs(gi)) @ np.abs(wp[:mf])
    else:
        x = pu[:, None, :] + qi[None, :, :] + b1
        ax = apu[:, None, :] + aqi[None, :, :] + np.abs(b1)
        gmf, agmf = (gu * wp[:mf]) @ gi.T, (np.abs(gu) * np.abs(wp[:mf])) @ np.abs(gi).T
    x = np.maximum(x, 0)
    for l in range(1, nl):
        Wl, bl = Z[f"mlp_layers.{3 * l}.weight"], Z[f"mlp_layers.{3 * l}.bias"]
        assert ax.max() < EXACT
        x, ax = np.maximum(x @ Wl.T + bl, 0), ax @ np.abs(Wl).T + np.abs(bl)
    s = gmf + x @ wp[mf:] + bp
    amag = agmf + ax @ np.abs(wp[mf:]) + abs(bp)
    assert amag.max() < EXACT, amag.max()
    assert np.array_equal(s, np.round(s))
    return (s + 0.0).astype(np.float32)


# ---------------------------------------------------------------------------- Wide&Deep
# nn.BatchNorm1d in eval mode divides by sqrt(running_var + eps).  With eps = 1e-5 in fp32,
# fl(fl(t - eps) + eps) == t for t in {0.25, 1, 4}: running_var = float32(t) - float32(eps) makes
# the divisor 0.5, 1 or 2 exactly, in the folded form (a = gamma / sqrt(var + eps),
# c = beta - mean * a) and in the unfolded one alike.  wd_state_dict asserts it bit for bit.
WD_EPS = np.float32(1e-5)
WD_SQRT = np.array([0.5, 1.0, 2.0], np.float32)
WD_DENSITIES = {"emb": 0.3, "w": 0.05, "final": 0.15, "wide": 0.5}


def _wd_bn(rng, n):
    s = WD_SQRT[rng.integers(0, 3, n)]
    var = (s * s).astype(np.float32) - WD_EPS
    assert var.dtype == np.float32
    assert np.array_equal(bits(var + WD_EPS), bits(s * s)), "running_var + eps is not the square"
    assert np.array_equal(bits(np.sqrt(var + WD_EPS)), bits(s))
    gamma = rng.choice(np.array([-2, -1, 0, 1, 2], np.float32), n, p=[0.1, 0.15, 0.1, 0.4, 0.25])
    return {"weight": gamma.astype(np.float32), "bias": rng.integers(-2, 3, n).astype(np.float32),
            "running_mean": rng.integers(-2, 3, n).astype(np.float32), "running_var": var}


def wd_state_dict(U, I, d, deep_layers, num_user_features=0, num_item_features=0, densities=None,
                  seed=0, wide_user_item=True):
    """Wide&Deep state dict (key layout of synthetic.widedeep_state_dict) on the lattice: ternary
    embeddings, Linear weights and feature Linears, integer biases in [-2, 2]; BatchNorm with
    sqrt(var + eps) in {0.5, 1, 2}, integer gamma in {-2..2} (zeros and negatives included),
    integer mean and beta in [-2, 2]; final_layer = [integer wide user weights | wide item weights
    in {-1, 0, 1} | ternary feature weights | ternary deep part], integer bias.  Every intermediate
    of a score is then a multiple of 2^-3 (one halving a layer at most).  wide_user_item=False:
    the layout of a model built with use_wide_user_item=False (no one-hot wide part)."""
    dn = dict(WD_DENSITIES, **(densities or {}))
    Fu, Fi = num_user_features, num_item_features
    rng = _rng(seed, U, I, d, len(deep_layers), Fu, Fi)
    ints = lambda n: rng.integers(-2, 3, n).astype(np.float32)
    sd = {}
    if wide_user_item:
        sd["wide_user_embedding.weight"] = _ternary(rng, (U, 1), dn["emb"])  # unused by forward
        sd["wide_item_embedding.weight"] = _ternary(rng, (I, 1), dn["emb"])
    if Fu > 0:
        sd["wide_user_features.weight"] = _ternary(rng, (Fu, Fu), 0.5)
        sd["wide_user_features.bias"] = ints(Fu)
    if Fi > 0:
        sd["wide_item_features.weight"] = _ternary(rng, (Fi, Fi), 0.5)
        sd["wide_item_features.bias"] = ints(Fi)
    sd["deep_user_embedding.weight"] = _ternary(rng, (U, d), dn["emb"])
    sd["deep_item_embedding.weight"] = _ternary(rng, (I, d), dn["emb"])
    if Fu > 0:
        sd["deep_user_features.weight"] = _ternary(rng, (d, Fu), 0.5)
        sd["deep_user_features.bias"] = ints(d)
    if Fi > 0:
        sd["deep_item_features.weight"] = _ternary(rng, (d, Fi), 0.5)
        sd["deep_item_features.bias"] = ints(d)
    prev = (2 + (Fu > 0) + (Fi > 0)) * d
    for li, h in enumerate(deep_layers):
        sd[f"deep_network.{4 * li}.weight"] = _ternary(rng, (h, prev), dn["w"])
        sd[f"deep_network.{4 * li}.bias"] = ints(h)
        for key, v in _wd_bn(rng, h).items():
            sd[f"deep_network.{4 * li + 2}.{key}"] = v
        sd[f"deep_network.{4 * li + 2}.num_batches_tracked"] = np.zeros((), np.int64)
        prev = h
    parts = []
    if wide_user_item:
        parts += [ints(U), _ternary(rng, I, dn["wide"])]
    parts += [_ternary(rng, Fu, 0.5), _ternary(rng, Fi, 0.5), _ternary(rng, prev, dn["final"])]
    sd["final_layer.weight"] = np.concatenate(parts).astype(np.float32)[None, :]
    sd["final_layer.bias"] = ints(1)
    return sd


def wd_features(n, F, seed=0):
    """[n, F] float32 feature rows with entries in {-1, 0, 1} (None for F == 0)."""
    if F == 0:
        return None
    return _rng(seed, n, F).integers(-1, 2, (n, F)).astype(np.float32)


def _wd_lin(sd):
    return sorted(int(k.split(".")[1]) for k, v in sd.items()
                  if k.startswith("deep_network.") and k.endswith(".weight") and np.ndim(v) == 2)


def _wd_check_lattice(Z, lin):
    """Every input of a score is on the lattice: integers everywhere, except running_var, for
    which sqrt(var + eps) evaluated in fp32 is 0.5, 1 or 2.  Returns the divisors per layer."""
    sq = {}
    for k, v in Z.items():
        if k.endswith("num_batches_tracked"):
            continue
        if k.endswith("running_var"):
            s = np.sqrt(np.asarray(v, np.float32) + WD_EPS)
            assert s.dtype == np.float32 and np.isin(s, WD_SQRT).all(), k
            sq[int(k.split(".")[1]) - 2] = s.astype(np.float64)
            continue
        a = np.asarray(v, np.float64)
        assert np.array_equal(a, np.round(a)), k
        assert np.abs(a).max(initial=0) < 2 ** 20, k
    return [sq[li] for li in lin]


def wd_scores(sd, users, user_features=None, item_table=None):
    """Exact Wide&Deep scores [B, I] (float32) of `users` against every item, in float64 in the
    reference's unfolded form (Linear -> ReLU -> (x - mean) / sqrt(var + eps) * gamma + beta per
    layer; wide terms; final bias), with the assertions that make it a bitwise oracle of ANY
    fp32 evaluation: every input is on the lattice (_wd_check_lattice), 2^3 * (sum of |terms|)
    behind every layer's values stays below 2^24, and the result equals an fp32 evaluation of
    the FOLDED form the fused kernels use (W2 * a1, b2 + W2 c1, ..., w_d * a_last; a = gamma /
    sqrt(var + eps), c = beta - mean * a) in two different summation orders.
    user_features [B, Fu] / item_table [I, Fi]: integer feature rows (models built with them)."""
    users = np.asarray(users)
    if len(users) > 16:  # [rows, I, width] intermediates: a few rows at a time
        uf = user_features
        return np.concatenate([wd_scores(sd, users[i:i + 16], None if uf is None else uf[i:i + 16],
                                         item_table) for i in range(0, len(users), 16)])
    lin = _wd_lin(sd)
    sq = _wd_check_lattice(sd, lin)
    Z = {k: np.asarray(v, np.float64) for k, v in sd.items()}
    eu, ei = Z["deep_user_embedding.weight"][users], Z["deep_item_embedding.weight"]
    B, I, d = len(users), ei.shape[0], ei.shape[1]
    U = Z["deep_user_embedding.weight"].shape[0]
    wf = Z["final_layer.weight"][0]
    Fu = Z["wide_user_features.weight"].shape[0] if "wide_user_features.weight" in Z else 0
    Fi = Z["wide_item_features.weight"].shape[0] if "wide_item_features.weight" in Z else 0
    assert (user_features is not None) == (Fu > 0) and (item_table is not None) == (Fi > 0)
    # ---- wide part: per-user and per-item terms (and the sums of |terms| behind them)
    wu, awu, wi, awi, off = np.zeros(B), np.zeros(B), np.zeros(I), np.zeros(I), 0
    if "wide_user_embedding.weight" in Z:
        wu, wi, off = wf[users], wf[U:U + I], U + I
        awu, awi = np.abs(wu), np.abs(wi)
    xu, axu, xi, axi = eu, np.abs(eu), ei, np.abs(ei)  # deep inputs [B, *] / [I, *]
    if Fu:
        f = np.asarray(user_features, np.float64)
        assert f.shape == (B, Fu) and np.array_equal(f, np.round(f))
        W, b = Z["wide_user_features.weight"], Z["wide_user_features.bias"]
        wu = wu + (f @ W.T + b) @ wf[off:off + Fu]
        awu = awu + (np.abs(f) @ np.abs(W).T + np.abs(b)) @ np.abs(wf[off:off + Fu])
        W, b = Z["deep_user_features.weight"], Z["deep_user_features.bias"]
        xu = np.concatenate([xu, f @ W.T + b], 1)
        axu = np.concatenate([axu, np.abs(f) @ np.abs(W).T + np.abs(b)], 1)
    off += Fu
    if Fi:
        f = np.asarray(item_table, np.float64)
        assert f.shape == (I, Fi) and np.array_equal(f, np.round(f))
        W, b = Z["wide_item_features.weight"], Z["wide_item_features.bias"]
        wi = wi + (f @ W.T + b) @ wf[off:off + Fi]
        awi = awi + (np.abs(f) @ np.abs(W).T + np.abs(b)) @ np.abs(wf[off:off + Fi])
        W, b = Z["deep_item_features.weight"], Z["deep_item_features.bias"]
        xi = np.concatenate([xi, f @ W.T + b], 1)
        axi = np.concatenate([axi, np.abs(f) @ np.abs(W).T + np.abs(b)], 1)
    off += Fi
    wd_, bf = wf[off:], Z["final_layer.bias"][0]
    # ---- layer 1 as its per-user and per-item halves (input order: e_u, e_i, user f., item f.)
    W1, b1 = Z[f"deep_network.{lin[0]}.weight"], Z[f"deep_network.{lin[0]}.bias"]
    cu_ = np.r_[0:d, 2 * d:2 * d + (d if Fu else 0)]
    ci_ = np.setdiff1d(np.arange(W1.shape[1]), cu_)
    assert len(cu_) == xu.shape[1] and len(ci_) == xi.shape[1]
    pu, qi = xu @ W1[:, cu_].T, xi @ W1[:, ci_].T
    apu, aqi = axu @ np.abs(W1[:, cu_]).T, axi @ np.abs(W1[:, ci_]).T
    z = pu[:, None, :] + qi[None, :, :] + b1                       # [B, I, l1]
    az = apu[:, None, :] + aqi[None, :, :] + np.abs(b1)
    pre = []  # post-ReLU values of every layer, for the folded evaluation
    for n, li in enumerate(lin):
        if n > 0:
            Wl, bl = Z[f"deep_network.{li}.weight"], Z[f"deep_network.{li}.bias"]
            z, az = z @ Wl.T + bl, az @ np.abs(Wl).T + np.abs(bl)
        assert 8 * az.max() < EXACT, (li, az.max())
        z = np.maximum(z, 0)
        p = f"deep_network.{li + 2}."
        g, be, m = Z[p + "weight"], Z[p + "bias"], Z[p + "running_mean"]
        z = (z - m) / sq[n] * g + be
        az = (az + np.abs(m)) / sq[n] * np.abs(g) + np.abs(be)
    deep = z @ wd_
    amag = az @ np.abs(wd_) + awu[:, None] + awi[None, :] + abs(bf)
    assert 8 * amag.max() < EXACT, amag.max()
    s = wu[:, None] + wi[None, :] + deep + bf
    assert np.array_equal(s * 8, np.round(s * 8))
    out = (s + 0.0).astype(np.float32)  # an exact zero is +0, as in the oracle's fp32 chain
    assert np.array_equal(out.astype(np.float64), s)
    # ---- the folded form in fp32, two summation orders
    F = np.float32
    a = [(Z[f"deep_network.{li + 2}.weight"] / sq[n]).astype(F) for n, li in enumerate(lin)]
    c = [(Z[f"deep_network.{li + 2}.bias"].astype(F) -
          Z[f"deep_network.{li + 2}.running_mean"].astype(F) * a[n]) for n, li in enumerate(lin)]
    for rev in (False, True):
        o = (lambda x: x[..., ::-1]) if rev else (lambda x: x)
        h = np.maximum((pu.astype(F)[:, None, :] + qi.astype(F)[None, :, :]) + b1.astype(F), F(0))
        for n, li in enumerate(lin[1:], 1):
            Wl = Z[f"deep_network.{li}.weight"].astype(F)
            bl = Z[f"deep_network.{li}.bias"].astype(F)
            Wf = Wl * a[n - 1][None, :]
            bfold = bl + np.ascontiguousarray(o(Wl)) @ np.ascontiguousarray(o(c[n - 1]))
            h = np.maximum(np.ascontiguousarray(o(h)) @ np.ascontiguousarray(o(Wf)).T + bfold, F(0))
            assert h.dtype == F
        wdf = wd_.astype(F) * a[-1]
        bias = F(bf) + np.ascontiguousarray(o(wd_.astype(F))) @ np.ascontiguousarray(o(c[-1]))
        fold = np.ascontiguousarray(o(h)) @ np.ascontiguousarray(o(wdf))
        fold = (fold + (bias + wu.astype(F))[:, None]) + wi.astype(F)[None, :]
        assert fold.dtype == F
        assert np.array_equal(bits(fold + F(0)), bits(out)), ("folded fp32 form differs", rev)
    return out


def tie_group_sizes(scores, k, mask=None):
    """Members of the tie group at position k, per row."""
    d = apply_mask(scores, mask)
    kth = -np.sort(-d, axis=1)[:, k - 1]
    return (d == kth[:, None]).sum(1)


def tie_fraction(scores, k, mask=None):
    """Fraction of rows whose reference has score[k - 1] == score[k]."""
    d = apply_mask(scores, mask)
    top = -np.sort(-d, axis=1)[:, :k + 1]
    return float(np.mean(top[:, k - 1] == top[:, k]))


# ---------------------------------------------------------------------------- shared cases
# Sample-threshold constants of hnm_dot_topk_f32 with the pre-filter off, copied from
# hnm_recommendation_amd/csrc/score.hip (THRESH_MIN_ITEMS, THRESH_SAMPLE, and `stride` / `cap`
# in the threshold path of hnm_dot_topk_f32): the sample is items 0, stride, 2 stride, ...
THRESH_MIN_ITEMS = 8192
THRESH_SAMPLE = 4096


def thresh_stride(I):
    return max(1, I // THRESH_SAMPLE)


def thresh_cap(I, k):
    return min(8192, max(256, 8 * k * thresh_stride(I)))


def thresh_counts(case):
    """#{score >= the sample's k-th score} per row: the appends of the threshold path's main
    pass (masks applied to sample and catalogue alike), which its select kernel then ranks."""
    d = apply_mask(case.scores, case.mask_csr)
    sample = d[:, ::thresh_stride(case.I)]
    tau = -np.sort(-sample, axis=1)[:, case.k - 1]
    return (d >= tau[:, None]).sum(1)


DCERT_RHO = 3.0 * 2.0 ** -11  # dot_cert.hip: E_u = 3 u16 ||u|| max||i|| + 2^-22 (|ub| + max|ib|)


class DotCase:
    """One hnm_dot_topk_f32 case of tests/test_gpu_lattice_dot.py."""

    def __init__(self, kind, I, B, d, k, bias=False, pad=False, mask="none"):
        self.kind, self.I, self.B, self.d, self.k = kind, I, B, d, k
        self.bias, self.pad, self.mask = bias, pad, mask
        self.id = f"{kind}-I{I}-B{B}-d{d}-k{k}" + ("-bias" if bias else "") + \
                  ("-pad" if pad else "") + ("" if mask == "none" else f"-{mask}")

    @functools.cached_property
    def tables(self):
        U = self.B + 3
        if self.kind == "sparse":
            return dot_tables(U, self.I, self.d, bias=self.bias, seed=11)
        if self.kind == "dense":
            return dot_tables(U, self.I, self.d, values=(0, 1), bias=self.bias, seed=12)
        return clustered_tables(U, self.I, self.d, seed=13)

    @functools.cached_property
    def users(self):
        u = _rng(5, self.B).permutation(self.B + 3)[:self.B].astype(np.int64)
        if self.kind == "clustered" and 0 not in u:
            u[0] = 0  # the user whose best item the cluster copies
        return u

    @functools.cached_property
    def scores(self):
        return dot_scores(self.tables, self.users)

    @functools.cached_property
    def mask_csr(self):
        return masks(self.B, self.I, self.mask, self.scores, self.k, seed=3)

    @functools.cached_property
    def ref(self):
        return ref_topk(self.scores, self.k, self.mask_csr)


def _dot_cases():
    C = DotCase
    return [
        # LIST route (I < 8,192)
        C("sparse", 1000, 5, 64, 12), C("sparse", 1000, 129, 32, 64, bias=True, mask="mixed"),
        C("sparse", 1000, 5, 128, 1, pad=True), C("dense", 1000, 5, 4, 63, mask="random"),
        # threshold (pre-filter off) and certified (on) routes
        C("sparse", 8192, 129, 64, 64), C("sparse", 8192, 5, 64, 63, pad=True),
        C("sparse", 8192, 300, 32, 12, bias=True, mask="mixed"),
        C("sparse", 8200, 300, 64, 12), C("sparse", 8200, 129, 64, 12),
        C("sparse", 8200, 129, 64, 12, mask="mixed"),
        C("sparse", 8200, 129, 68, 12, pad=True), C("sparse", 8200, 1, 64, 12),
        C("sparse", 8200, 5, 128, 12, bias=True, pad=True),
        C("sparse", 9001, 129, 64, 1), C("sparse", 9001, 300, 128, 12, mask="tie_group"),
        C("sparse", 9001, 5, 68, 64, bias=True, mask="dups_oob"),
        C("sparse", 9001, 129, 32, 63, pad=True, mask="empty_between"),
        C("dense", 8200, 129, 4, 12), C("dense", 9001, 5, 4, 64, mask="all_but_few"),
        C("dense", 8192, 300, 4, 1, pad=True, mask="all"),
        C("clustered", 8200, 129, 64, 12), C("clustered", 9001, 300, 64, 12, mask="random"),
    ]


DOT_CASES = _dot_cases()
SPARSE_STATS_CASE = next(c for c in DOT_CASES if c.id == "sparse-I8200-B300-d64-k12")
TWO_PHASE_DOT_CASE = next(c for c in DOT_CASES if c.id == "sparse-I8200-B129-d64-k12")


class NcfCase:
    """One NeuralCF model + user batch of tests/test_gpu_lattice_ncf.py."""

    def __init__(self, I, B, mlp_dims=(128, 64, 32), seed=0):
        self.I, self.B, self.U, self.mlp_dims, self.seed = I, B, B + 7, mlp_dims, seed
        self.id = f"I{I}-B{B}" + ("-deep" if len(mlp_dims) > 3 else "")

    @functools.cached_property
    def sd(self):
        return ncf_state_dict(self.U, self.I, 64, self.mlp_dims, seed=21 + self.seed)

    @functools.cached_property
    def users(self):
        return _rng(6, self.B).permutation(self.U)[:self.B].astype(np.int64)

    @functools.cached_property
    def scores(self):
        return ncf_scores(self.sd, self.users)

    @functools.lru_cache(maxsize=None)
    def mask_csr(self, kind, k):
        return masks(self.B, self.I, kind, self.scores, k, seed=4)

    @functools.lru_cache(maxsize=None)
    def ref(self, k, kind="none"):
        return ref_topk(self.scores, k, self.mask_csr(kind, k))


NCF_SMALL = NcfCase(1500, 37)
NCF_SMALL_KS = (1, 12, 64, 100)
# seeds chosen so that the one-row batches tie at the top too (test_cpu_lattice.py checks it)
NCF_CERT = {(I, B): NcfCase(I, B, seed=3 if (I, B) == (8192, 1) else 0)
            for I in (8192, 9001) for B in (1, 5, 130)}
NCF_CERT_KS = (1, 12, 64)
NCF_DEEP = NcfCase(8200, 33, (128, 64, 32, 16))
NCF_TWO_PHASE = NcfCase(8200, 129)


# Wide&Deep (tests/test_gpu_lattice_widedeep.py).  WDC_BF_MIN: the survivors above which a row of
# the certified cascade refines best first in two phases, copied from
# hnm_recommendation_amd/csrc/widedeep_rescore.hip; 4,096 items: the floor of wdc_eligible
# (widedeep_cert.hip), below which -- and for a layer-1 width that is no multiple of 16 -- the
# exact fused kernel answers.
WDC_BF_MIN = 96
WDC_MIN_ITEMS = 4096
WD_D1 = {"emb": 0.3, "w": 0.05, "final": 0.15}
WD_D2 = {"emb": 0.5, "w": 0.1, "final": 0.3}
WD_D3 = {"emb": 0.5, "w": 0.2, "final": 0.5}


class WdCase:
    """One Wide&Deep model + user batch; densities and seed tuned per tower so that the
    reference alone shows the tie pressure tests/test_cpu_lattice.py asserts."""

    def __init__(self, name, tower, I, B, ks, densities, seed=0, Fu=0, Fi=0, wide=True,
                 sparse=True):
        self.id, self.tower, self.I, self.B, self.ks = name, tuple(tower), I, B, tuple(ks)
        self.densities, self.seed, self.Fu, self.Fi, self.wide = densities, seed, Fu, Fi, wide
        self.sparse = sparse  # sparse ties: the median tie group at k has at most 64 members
        self.U, self.d = B + 7, 16
        self.certified = tower[0] % 16 == 0 and I >= WDC_MIN_ITEMS

    @functools.cached_property
    def sd(self):
        return wd_state_dict(self.U, self.I, self.d, self.tower, self.Fu, self.Fi, self.densities,
                             self.seed, self.wide)

    @functools.cached_property
    def users(self):
        return _rng(6, self.B).permutation(self.U)[:self.B].astype(np.int64)

    @functools.cached_property
    def user_table(self):  # [U, Fu]; the batch's rows: user_table[users]
        return wd_features(self.U, self.Fu, seed=1)

    @functools.cached_property
    def item_table(self):  # [I, Fi]
        return wd_features(self.I, self.Fi, seed=2)

    @property
    def user_features(self):
        return None if self.Fu == 0 else self.user_table[self.users]

    @functools.cached_property
    def scores(self):
        return wd_scores(self.sd, self.users, self.user_features, self.item_table)

    @functools.lru_cache(maxsize=None)
    def mask_csr(self, kind, k):
        return masks(self.B, self.I, kind, self.scores, k, seed=8)

    @functools.lru_cache(maxsize=None)
    def ref(self, k, kind="none"):
        return ref_topk(self.scores, k, self.mask_csr(kind, k))


WD_CERT_KS = (1, 12, 64)
WD_EXACT_KS = (1, 12, 63, 64)
# the six certified tower shapes of tests/test_gpu_widedeep_shapes.py (CERT_TOWERS), sparse ties
WD_CERT_FULL = ((48, 200, 100), (48, 50))  # every k x mask kind; the others: k = 12, no mask
WD_CERT = {t: WdCase("cert-" + "-".join(map(str, t)), t, 4200, 9,
                     WD_EXACT_KS if t in WD_CERT_FULL else WD_CERT_KS, dn, seed)
           for t, dn, seed in (((48, 200, 100), WD_D1, 3), ((48, 100, 50), WD_D1, 0),
                               ((48, 50, 20), WD_D2, 0), ((48, 20, 10), WD_D3, 0),
                               ((48, 20), WD_D2, 0), ((48, 50), WD_D1, 1))}
# layer 1 40 wide / 1,111 items: the exact fused kernel whatever the pre-filter switch
WD_EXACT = WdCase("exact-40-100-50", (40, 100, 50), 1111, 9, WD_EXACT_KS, WD_D1, 0)
WD_EXACT_WIDE = WdCase("exact-40-200-100", (40, 200, 100), 1111, 9, WD_EXACT_KS, WD_D1, 4)
WD_B70 = WdCase("cert-48-50-B70", (48, 50), 4200, 70, (12,), WD_D1, 0)
# tie groups of 136 .. 215 members at k = 64 in five of the nine rows: more than WDC_BF_MIN
# survivors, so those rows run the cascade's second phase (wdc_filter_kernel)
WD_BEST_FIRST = WdCase("bestfirst-48-50", (48, 50), 4200, 9, (12, 64), WD_D1, 0, sparse=False)
WD_FEAT_EXACT = WdCase("feat-exact-40-100-50", (40, 100, 50), 1111, 9, WD_EXACT_KS, WD_D1, 0,
                       Fu=3, Fi=4)
WD_FEAT_CERT = WdCase("feat-cert-48-100-50", (48, 100, 50), 4200, 9, WD_CERT_KS, WD_D1, 2,
                      Fu=3, Fi=4)
# exact zeros among the scores, 17 of them inside the rows' top-64: the sign of zero is compared
WD_NOWIDE = WdCase("nowide-48-50", (48, 50), 4200, 9, WD_CERT_KS, WD_D2, 2, wide=False)
# no deep and no item term in the final layer: every item of a row ties.  Run with so many rows
# that wd_partition (widedeep.hip) gives the scan ONE item partition -- 4,224 items a segment,
# above its WDC_CAP = 4,096 appends -- every segment overflows and the row takes the exact kernel.
WD_OVERFLOW = WdCase("overflow-48-20", (48, 20), 4200, 9, (12,), dict(WD_D2, final=0.0, wide=0.0),
                     0, sparse=False)
WDC_CAP = 4096
WD_CASES = [*WD_CERT.values(), WD_EXACT, WD_EXACT_WIDE, WD_B70, WD_BEST_FIRST, WD_FEAT_EXACT,
            WD_FEAT_CERT, WD_NOWIDE, WD_OVERFLOW]
WD_DENSE_K = 100  # k > 64: dense scores + hnm_topk_rows_f32 (recommend_with_scores)
WD_DENSE_K_CASES = (WD_EXACT, WD_CERT[(48, 200, 100)])
