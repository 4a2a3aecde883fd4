"""ContentKNN: item-attribute nearest neighbours, the answer for articles nobody has bought yet
(no reference module: `GEMINI.md` stage 5 names "product metadata -> TF-IDF -> similarity-based
content recommendation", and `scripts/analyze_recommendation_challenges.py:274-275` lists the
article attribute columns it would use; `src/models` never built it).

Every purchase-based model is blind to a new article: no co-occurrence row in `ItemCF`, a zero
row in `ImplicitALS`, the last place of the popularity order.  The catalogue's categorical
attributes (product type, colour group, department, ...) are known from the first day.  One HIP
entry (`hnm_content_fit_f32`, `csrc/content.hip`, contract in `include/hnm.h`) scans all item
pairs and keeps each item's `num_neighbors` most similar items, in `ItemCF`'s table: the buffers,
state_dict keys and every answering method are `ItemCF`'s, served by the same kernels.

Similarity.  An item is the one-hot vector of its codes, a code of column f weighted
`column_weight_f * idf` with `idf = ln((1 + I) / (1 + df)) + 1` (`weighting="idf"`, df = items
holding the code) or 1 (`"uniform"`); the similarity is the cosine of two such vectors.  The fit
works on the squared entries in fixed point, `q = rint(g * 2^20 / g_max)`, `g = (column_weight *
idf)^2`: the matching weight S and the norms n are then integers, `sim = float32(S / sqrt(n_i *
n_j))` is the same bits on every run, and a numpy restatement (tests/content_oracle.py) is
bitwise.  The weights are computed on the host in float64: plumbing over F <= 16 columns.

Users' rows come from `set_history(UserHistory)`; `recommend_for_items` and `similar_items` need
none.  The model is fitted by `fit_attributes`, never from interactions.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from .. import _lib
from .item_cf import ItemCF

MAX_COLUMNS = 16     # hnm_content_fit_f32: F
Q_ONE = 1 << 20      # the fixed point: the largest squared weight maps here
WEIGHTINGS = ("idf", "uniform")


def encode_attributes(item_attrs, num_items: int, column_weights=None, weighting: str = "idf"):
    """(codes int32 [I, F], code_ptr int64 [F + 1], code_q uint32 [code_ptr[F]]) -- what
    `hnm_content_fit_f32` takes, on the host.  Each column's non-negative values are remapped to a
    dense vocabulary in ascending order of value (negative stays -1: missing); the weight of a
    code is q = rint(g * 2^20 / g_max), g = (column_weight * idf)^2 in float64.  ValueError for a
    table that is not [num_items, 1..16] integers, or weights that are not F finite values >= 0
    with a positive one among them."""
    if weighting not in WEIGHTINGS:
        raise ValueError(f'weighting must be one of {WEIGHTINGS}, got "{weighting}"')
    a = item_attrs.detach().cpu().numpy() if isinstance(item_attrs, torch.Tensor) \
        else np.asarray(item_attrs)
    if a.ndim != 2 or not np.issubdtype(a.dtype, np.integer):
        raise ValueError("item_attrs must be a [num_items, F] table of integer codes")
    I, F = a.shape
    if not 1 <= F <= MAX_COLUMNS:
        raise ValueError(f"item_attrs has {F} columns, 1 .. {MAX_COLUMNS} are supported")
    if I != int(num_items):
        raise ValueError(f"item_attrs has {I} rows, the model {num_items} items")
    cw = np.ones(F, np.float64) if column_weights is None else \
        np.asarray(column_weights, np.float64).reshape(-1)
    if cw.shape[0] != F or not np.isfinite(cw).all() or (cw < 0).any():
        raise ValueError(f"column_weights must be {F} finite values >= 0")
    if not (cw > 0).any():
        raise ValueError("column_weights are all zero: nothing to compare")
    codes = np.full((I, F), -1, np.int32)
    code_ptr = np.zeros(F + 1, np.int64)
    g = []
    for f in range(F):
        have = a[:, f] >= 0
        vals, inv, df = np.unique(a[have, f], return_inverse=True, return_counts=True)
        codes[have, f] = inv.reshape(-1)
        code_ptr[f + 1] = code_ptr[f] + len(vals)
        idf = np.ones(len(vals), np.float64) if weighting == "uniform" else \
            np.log((1.0 + I) / (1.0 + df.astype(np.float64))) + 1.0
        g.append((cw[f] * idf) ** 2)
    g = np.concatenate(g)
    g_max = g.max() if g.size else 0.0
    q = np.rint(g * float(Q_ONE) / g_max) if g_max > 0 else np.zeros_like(g)
    return codes, code_ptr, q.astype(np.uint32)


class ContentKNN(ItemCF):
    """`ItemCF`'s table and answers, fitted on item attributes (`fit_attributes`)."""
    weighted = takes_basket_weights = False
    _NO_HISTORY = "no history: call set_history first (baskets and similar_items need none)"

    def __init__(self, num_users: int, num_items: int, num_neighbors: int = 64,
                 weighting: str = "idf", top_k: int = 12):
        if weighting not in WEIGHTINGS:
            raise ValueError(f'weighting must be one of {WEIGHTINGS}, got "{weighting}"')
        super().__init__(num_users, num_items, num_neighbors=num_neighbors, top_k=top_k)
        self.weighting = weighting
        self.hparams = {"num_users": num_users, "num_items": num_items,
                        "num_neighbors": num_neighbors, "weighting": weighting, "top_k": top_k}

    def _fitted(self):
        if self._is_fitted is None:
            self._is_fitted = bool((self.item_count > 0).any())
        if not self._is_fitted:
            raise RuntimeError("not fitted: call fit_attributes, or load a fitted state_dict")

    def fit_attributes(self, item_attrs, column_weights=None, *, _tile: int = 0):
        """Fit on `item_attrs`, [num_items, F] integer codes (numpy or tensor; F in [1, 16];
        negative = missing; any non-negative integers, remapped per column).  `column_weights`: F
        finite values >= 0, default 1; a column of weight 0 is ignored.  One
        `hnm_content_fit_f32` call (`_tile`: column items per LDS tile, for tests).  The model's
        history is left as it is."""
        codes, code_ptr, code_q = encode_attributes(item_attrs, self.num_items, column_weights,
                                                    self.weighting)
        _lib.require_gpu(self.neighbor_idx)
        dev = self.device
        for name, dtype in (("neighbor_idx", torch.int32), ("neighbor_val", torch.float32),
                            ("item_count", torch.int64)):
            t = getattr(self, name)
            if t.dtype != dtype or not t.is_contiguous():
                setattr(self, name, t.to(dtype).contiguous())
        a = torch.from_numpy(codes).to(dev)
        p = torch.from_numpy(code_ptr).to(dev)
        # uint32 travels as its int32 bit pattern; an empty vocabulary still needs an address
        q = torch.from_numpy(np.concatenate([code_q, np.zeros(1, np.uint32)]).view(np.int32)).to(dev)
        _lib.call("hnm_content_fit_f32", _lib.ctx(dev), _lib.ptr(a), self.num_items,
                  codes.shape[1], _lib.ptr(p), _lib.ptr(q), self.num_neighbors, int(_tile),
                  _lib.ptr(self.neighbor_idx), _lib.ptr(self.neighbor_val),
                  _lib.ptr(self.item_count))
        _lib.sync_check(dev)
        self._is_fitted = True
        return self

    def _not_from_interactions(self, *args, **kwargs):
        raise TypeError("a ContentKNN is fitted on item attributes: call fit_attributes(item_attrs) "
                        "and give the users' rows with set_history(UserHistory)")

    fit_history = fit_interactions = _not_from_interactions
