"""The history side of the fitted models (PopularityBaseline, ItemCF, ImplicitALS): the
device-resident `UserHistory`, the per-transaction weights it is built with, the CSR of a
batch's filter or of a request's baskets, and the `HistoryModel` mixin of the models that keep
a history of their own.  `models/base.py` re-exports the public names.
"""
from __future__ import annotations

import itertools
from typing import Dict, Optional

import numpy as np
import torch

from .. import _lib


def _host(a) -> np.ndarray:
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _flat_items(sets, num_items: int):
    """(rows int64, items int64) of a list of item-id iterables, flattened: negative ids wrap
    like torch indexing, ids outside [-num_items, num_items) raise IndexError as
    `scores[i, items] = -inf` would."""
    lens = np.fromiter((len(x) for x in sets), dtype=np.int64, count=len(sets))
    total = int(lens.sum())
    flat = np.fromiter(itertools.chain.from_iterable(sets), dtype=np.int64, count=total)
    bad = (flat >= num_items) | (flat < -num_items)
    if bad.any():
        raise IndexError(f"index {int(flat[bad][0])} is out of bounds for dimension 1 "
                         f"with size {num_items}")
    flat = np.where(flat < 0, flat + num_items, flat)
    return np.repeat(np.arange(len(sets), dtype=np.int64), lens), flat


def _history_arrays(keys, sets, num_items: int):
    """Vectorized CSR of `{key: iterable of item ids}` rows in `keys` order (`_flat_items`'
    id rules), rows sorted ascending and de-duplicated (one lexicographic np.unique over
    (row, item), no per-row numpy calls)."""
    rows, flat = _flat_items(sets, num_items)
    key = np.unique(rows * num_items + flat)          # sorted by (row, item), unique
    r, items = np.divmod(key, num_items)
    ptr = np.zeros(len(sets) + 1, np.int64)
    np.cumsum(np.bincount(r, minlength=len(sets)), out=ptr[1:])
    return ptr, items.astype(np.int32)


def interaction_weights(n: int, weights, days_ago, time_decay: float):
    """float64 [n] per-transaction weights, `weights` (default 1) times
    exp(-time_decay * days_ago) (PopularityBaseline's convention), or None when neither
    `weights` nor `days_ago` is given.  ValueError for a negative time_decay, fractional or
    negative days, or a shape mismatch.  The rule of every fitted model that takes weights
    (ImplicitALS, a weighted ItemCF)."""
    time_decay = float(time_decay)
    if not time_decay >= 0.0 or not np.isfinite(time_decay):
        raise ValueError("time_decay must be finite and >= 0")
    if weights is None and days_ago is None:
        return None

    def host(a, what):
        a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
        a = a.reshape(-1)
        if a.shape[0] != n:
            raise ValueError(f"{what} must have one entry per interaction")
        return a

    w = np.ones(n, np.float64) if weights is None else host(weights, "weights").astype(np.float64)
    if days_ago is not None:
        days = host(days_ago, "days_ago")
        if days.dtype.kind not in "iu":
            d64 = days.astype(np.float64)
            if not (np.isfinite(d64).all() and (d64 == np.floor(d64)).all()):
                raise ValueError("days_ago must be whole days")
            days = d64
        if days.size and days.min() < 0:
            raise ValueError("days_ago must be >= 0")
        w = w * np.exp(-time_decay * days.astype(np.float64))
    return w


class UserHistory:
    """Device-resident per-user item history (CSR over user ids), built ONCE, for the
    -inf filter of batched recommend calls without a host round trip per batch.

    `recommend_with_scores(user_ids, filter_items=history)` (every model) gathers the
    batch's rows on the GPU (hnm_mask_gather_csr) and passes them to the fused top-K kernels
    as the same CSR mask a `filter_items` dict produces -- identical results (tests), but the
    per-call cost is two small kernel launches instead of a Python/numpy pass over the batch.
    This is what `serving.Recommender` holds for its purchase history (serve.py:166-168,
    350-352); the item-sharded scorers take it too (`mask_for(ids, item_range)`)."""

    def __init__(self, history: Dict[int, set], num_users: int, num_items: int, device):
        users = sorted(u for u in history if 0 <= int(u) < num_users and history[u])
        ptr_rows, idx = _history_arrays(users, [history[u] for u in users], num_items)
        full = np.zeros(int(num_users) + 1, np.int64)
        if users:
            full[np.asarray(users, np.int64) + 1] = np.diff(ptr_rows)
        np.cumsum(full, out=full)
        self._set(full, idx, num_users, num_items, device)

    @classmethod
    def from_interactions(cls, user_ids, item_ids, num_users: int, num_items: int, device,
                          weights=None):
        """From (user, item) interaction arrays -- e.g. the training transactions that are a
        customer's purchase history (serve.py:166-168) -- de-duplicated and sorted per user.

        `weights`: one finite weight >= 0 per transaction (a quantity, a recency decay, their
        product; ValueError otherwise).  The weight of a distinct pair is the float64 sum of its
        transactions' weights, taken in ascending weight order and then rounded to fp32, so a
        permutation of the transactions gives the same bits: `hist_w`, an fp32 device tensor
        aligned with `hist_idx` (None without `weights`).  ImplicitALS reads it as the pair's
        confidence, a weighted ItemCF in its fit and in a user's sums."""
        u = np.asarray(user_ids, np.int64)
        i = np.asarray(item_ids, np.int64)
        if u.shape != i.shape:
            raise ValueError("user_ids and item_ids must have the same shape")
        if u.size and (u.min() < 0 or u.max() >= num_users or i.min() < 0 or i.max() >= num_items):
            raise IndexError("interaction ids out of range")
        pair_w = None
        if weights is None:
            key = np.unique(u * num_items + i)
        else:
            if isinstance(weights, torch.Tensor):
                weights = weights.detach().cpu().numpy()
            w = np.asarray(weights, np.float64)
            if w.shape != u.shape:
                raise ValueError("weights must have the shape of user_ids")
            if w.size and not (np.isfinite(w).all() and (w >= 0).all()):
                raise ValueError("weights must be finite and >= 0")
            k, w = (u * num_items + i).reshape(-1), w.reshape(-1)
            order = np.lexsort((w, k))                    # by pair, then by ascending weight
            k, w = k[order], w[order]
            starts = np.nonzero(np.r_[True, k[1:] != k[:-1]])[0] if k.size else np.zeros(0, np.int64)
            key = k[starts]
            pair_w = (np.add.reduceat(w, starts) if k.size else w).astype(np.float32)
            if not np.isfinite(pair_w).all():
                raise ValueError("a pair's summed weight exceeds the fp32 range")
        r, items = np.divmod(key, num_items)
        full = np.zeros(int(num_users) + 1, np.int64)
        np.cumsum(np.bincount(r, minlength=num_users), out=full[1:])
        obj = cls.__new__(cls)
        obj._set(full, items.astype(np.int32), num_users, num_items, device, pair_w)
        return obj

    def _set(self, ptr, idx, num_users, num_items, device, w=None):
        self.num_users, self.num_items = int(num_users), int(num_items)
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        lens = np.diff(ptr)
        self.max_len = int(lens.max()) if lens.size else 0
        self.nnz = int(ptr[-1])
        self.hist_ptr = torch.from_numpy(ptr).to(self.device)
        self.hist_idx = torch.from_numpy(idx if idx.size else np.zeros(1, np.int32)).to(self.device)
        self.hist_w = None if w is None else torch.from_numpy(
            w if w.size else np.zeros(1, np.float32)).to(self.device)

    def mask_for(self, user_ids: torch.Tensor, item_range=None):
        """(mask_ptr int64[B+1], mask_idx int32) for a batch of device user ids -- with
        item_range = (lo, hi): only history items in [lo, hi), renumbered i - lo (an item
        shard) -- or (None, None) when no history row can be non-empty."""
        if self.nnz == 0:
            return None, None
        u = user_ids
        if u.device != self.device:
            raise ValueError(f"history lives on {self.device}, user ids on {u.device}")
        lo, hi = (0, 2 ** 63 - 1) if item_range is None else (int(item_range[0]), int(item_range[1]))
        B = u.numel()
        cap = max(B * self.max_len, 1)
        mptr = torch.empty(B + 1, dtype=torch.int64, device=u.device)
        midx = torch.empty(cap, dtype=torch.int32, device=u.device)
        _lib.call("hnm_mask_gather_csr", _lib.ctx(u.device), _lib.ptr(self.hist_ptr),
                  _lib.ptr(self.hist_idx), self.num_users, _lib.ptr(u), B, lo, hi, cap,
                  _lib.ptr(mptr), _lib.ptr(midx))
        return mptr, midx


def filter_csr(user_ids: torch.Tensor, filter_items, num_items: int, device: torch.device):
    """Per-row CSR -inf mask for a batch: from a `UserHistory` (gathered on the device) or
    from the reference's `filter_items` dict.

    Mirrors the loop in every `recommend` (`neural_cf.py:316-321`): row i masks
    `filter_items[user_ids[i]]`; negative ids wrap like torch indexing; ids >= num_items
    raise IndexError as `scores[i, items] = -inf` would.
    Returns (mask_ptr int64[B+1], mask_idx int32[nnz]) on `device`, or (None, None).
    """
    if filter_items is None:
        return None, None
    if isinstance(filter_items, UserHistory):
        if filter_items.num_items != num_items:
            raise ValueError(f"history built for {filter_items.num_items} items, model has "
                             f"{num_items}")
        return filter_items.mask_for(user_ids)
    uids = user_ids.detach().cpu().tolist()
    empty = ()
    sets = [filter_items.get(u) or empty for u in uids]
    ptr, idx = _history_arrays(uids, sets, num_items)
    if ptr[-1] == 0:
        return None, None
    return (torch.from_numpy(ptr).to(device), torch.from_numpy(idx).to(device))


def basket_csr(baskets, num_items: int, device, weights=None):
    """(ptr int64[n + 1], idx int32, n, w) on `device`, contiguous, for n baskets: visitors
    without a user index.  `w`: fp32 weights aligned with idx, None without `weights`.

    A list of item-id iterables is sorted and de-duplicated here (`_flat_items`' id rules);
    `weights` then is a list of per-basket sequences aligned with the items, and a repeated
    item's weights are summed by `UserHistory.from_interactions`' rule.  A (ptr, idx) pair of
    tensors or arrays is a CSR whose rows already are ascending and unique; `weights` then is a
    flat array aligned with idx.  idx and w hold one padding element when nothing is stored."""
    if isinstance(baskets, tuple) and len(baskets) == 2 and all(
            isinstance(x, (torch.Tensor, np.ndarray)) for x in baskets):
        ptr = torch.as_tensor(baskets[0]).reshape(-1).to(torch.int64)
        idx = torch.as_tensor(baskets[1]).reshape(-1).to(torch.int32)
        if ptr.numel() < 1:
            raise ValueError("a basket CSR needs ptr of at least one entry")
        p = ptr.cpu()
        if int(p[0]) != 0 or bool((p[1:] < p[:-1]).any()) or int(p[-1]) > idx.numel():
            raise ValueError("basket ptr must start at 0, not decrease and end within idx")
        w = None
        if weights is not None:
            w = torch.as_tensor(weights).reshape(-1).to(torch.float32)
            if w.numel() != idx.numel():
                raise ValueError("weights must be aligned with the CSR's idx")
    else:
        sets = [list(b) for b in baskets]
        if weights is None:
            p, i = _history_arrays(range(len(sets)), sets, num_items)
            ptr, idx, w = torch.from_numpy(p), torch.from_numpy(i), None
        else:
            ws = [list(x) for x in weights]
            if len(ws) != len(sets) or any(len(a) != len(b) for a, b in zip(sets, ws)):
                raise ValueError("weights must hold one sequence per basket, aligned with its "
                                 "items")
            rows, flat = _flat_items(sets, num_items)
            wflat = np.fromiter(itertools.chain.from_iterable(ws), np.float64, count=len(flat))
            h = UserHistory.from_interactions(rows, flat, max(len(sets), 1), num_items, device,
                                              weights=wflat)
            ptr, idx, w = h.hist_ptr[:len(sets) + 1], h.hist_idx, h.hist_w
    if idx.numel() == 0:
        idx = torch.zeros(1, dtype=torch.int32)
        w = None if w is None else torch.zeros(1, dtype=torch.float32)
    return (ptr.to(device).contiguous(), idx.to(device).contiguous(), ptr.numel() - 1,
            None if w is None else w.to(device).contiguous())


def interactions_history(user_ids, item_ids, num_users: int, num_items: int, device,
                         weights=None, days_ago=None, time_decay: float = 0.0,
                         unit_weights: bool = False) -> UserHistory:
    """The `UserHistory` of (user, item) interaction arrays or tensors, any shape, with
    `interaction_weights(weights, days_ago, time_decay)` per transaction.  `unit_weights`: with
    neither `weights` nor `days_ago` every transaction weighs 1.0 (a pair its number of
    purchases) instead of the history carrying no weights."""
    u, i = _host(user_ids).reshape(-1), _host(item_ids).reshape(-1)
    w = interaction_weights(u.shape[0], weights, days_ago, time_decay)
    if w is None and unit_weights:
        w = np.ones(u.shape[0], np.float64)
    return UserHistory.from_interactions(u, i, num_users, num_items, device, weights=w)


class HistoryModel:
    """Mixin of the models that are fitted on a `UserHistory` and keep it (ItemCF,
    ImplicitALS); the model supplies `num_users`, `num_items` and `device`."""
    history: Optional[UserHistory] = None
    _NO_HISTORY = "no history: call fit_interactions / fit_history / set_history"

    def _check_history(self, h):
        if not isinstance(h, UserHistory):
            raise TypeError("history must be a UserHistory")
        if h.num_items != self.num_items or h.num_users != self.num_users:
            raise ValueError(f"history built for {h.num_users} users x {h.num_items} items, "
                             f"model has {self.num_users} x {self.num_items}")

    def set_history(self, history: Optional[UserHistory]):
        """The history `recommend*`, `predict_all_items` and `refresh_users` read a user's row
        from."""
        if history is not None:
            self._check_history(history)
        self.history = history
        return self

    def _need_history(self, history: Optional[UserHistory] = None) -> UserHistory:
        """`history`, or the model's own: of the model's shape and on its device."""
        h = self.history if history is None else history
        if h is None:
            raise RuntimeError(self._NO_HISTORY)
        self._check_history(h)
        if h.device != self.device:
            raise ValueError(f"history lives on {h.device}, the model on {self.device}")
        return h
