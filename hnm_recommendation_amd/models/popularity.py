"""PopularityBaseline drop-in (reference: `src/models/baseline.py:16-194`).

The model the reference server always has (`serve.py:260-280`) and falls back to when no
checkpoint carries a `test_map` (`:415-430`).  Two HIP entries (`csrc/popularity.hip`):

* `hnm_popularity_fit_f64` -- the fit: a weighted per-item histogram over all transactions
  (`value_counts` / `groupby('article_idx')['weight'].sum()`, `baseline.py:146-156`), summed
  per item in ascending `days_ago` so the float64 popularity is the same bits on every run.
* `hnm_popularity_topk_f32` -- the per-user answer (`[x for x in item_popularity if x not in
  history][:k]`, `:78-85, 183-187`): one wave per user over the first k + h entries of the
  order instead of a [B, num_items] score matrix.

Differences from the reference, on purpose:

* Order.  pandas leaves the order of equally popular items unspecified; here the order is
  DEFINED as (popularity descending, item id ascending) over the items bought at least once.
* Before any fit the reference's `forward` returns random items; this module raises
  `RuntimeError("not fitted")` -- a server must not answer with noise.
* `fit_popularity` does not add `days_ago` / `weight` columns to the caller's frame.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np
import torch

from .. import _lib
from ..evaluation import RecommendationMetrics
from .base import RecModule, UserHistory, empty_rows, empty_topk, filter_csr


def _host_array(x, dtype):
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().numpy().astype(dtype, copy=False).reshape(-1)
    return np.asarray(x).astype(dtype, copy=False).reshape(-1)


class PopularityBaseline(RecModule):
    def __init__(self, n_items: Optional[int] = None, k: int = 12, time_decay: float = 0.0,
                 personalized: bool = False, **aliases):
        super().__init__()
        self.save_hyperparameters()
        # serve.py:264-268 spells the constructor PopularityBaseline(num_items=, top_k=)
        unknown = set(aliases) - {"num_items", "top_k"}
        if unknown:
            raise TypeError(f"__init__() got an unexpected keyword argument '{sorted(unknown)[0]}'")
        if "num_items" in aliases:
            if n_items is not None:
                raise TypeError("give n_items or num_items, not both")
            n_items = aliases["num_items"]
        if "top_k" in aliases:
            k = aliases["top_k"]
        if n_items is None:
            raise TypeError("__init__() missing 1 required positional argument: 'n_items'")
        self.hparams.update(n_items=n_items, k=k)
        self.n_items = self.num_items = int(n_items)
        self.k = self.top_k = int(k)
        self.time_decay = float(time_decay)
        self.personalized = bool(personalized)
        self.history: Optional[UserHistory] = None  # the model's own history (personalized)
        # No parameters and an empty state_dict, as the reference's: the fitted tables are
        # non-persistent buffers (they follow .to(device)); _anchor tells the device before a fit
        self.register_buffer("_anchor", torch.empty(0), persistent=False)
        for name in ("pop", "order", "order_val", "rank"):
            self.register_buffer(name, None, persistent=False)
        self.metrics = RecommendationMetrics(top_k=self.top_k)

    @property
    def device(self) -> torch.device:
        return self._anchor.device

    @property
    def item_popularity(self) -> Optional[List[int]]:
        """The reference's attribute: item ids, most popular first (None before a fit)."""
        return None if self.order is None else self.order.cpu().tolist()

    def _fitted(self):
        if self.order is None:
            raise RuntimeError("not fitted: call fit_popularity / fit_interactions / "
                               "set_popular_items first")

    # ------------------------------------------------------------------ fitting
    def _install(self, order: torch.Tensor, order_val: torch.Tensor, pop: torch.Tensor):
        dev = self.device
        rank = torch.full((self.num_items,), -1, dtype=torch.int32, device=dev)
        rank[order] = torch.arange(order.numel(), dtype=torch.int32, device=dev)
        self.pop, self.order, self.order_val, self.rank = pop, order, order_val, rank

    def set_popular_items(self, items, weights=None):
        """Install a given order (`serve.py:271`, `benchmark_models.py:85`): `items` most
        popular first; `weights` default to len(items) - position.  ValueError on duplicate
        or out-of-range ids."""
        it = _host_array(items, np.int64)
        if it.size and (it.min() < 0 or it.max() >= self.num_items):
            raise ValueError(f"popular items must be in [0, {self.num_items})")
        if np.unique(it).size != it.size:
            raise ValueError("popular items must be distinct")
        if weights is None:
            w = np.arange(it.size, 0, -1, dtype=np.float64)
        else:
            w = _host_array(weights, np.float64)
            if w.shape != it.shape:
                raise ValueError("weights must match items")
        dev = self.device
        order = torch.from_numpy(it).to(dev)
        wd = torch.from_numpy(w).to(dev)
        pop = torch.zeros(self.num_items, dtype=torch.float64, device=dev)
        pop[order] = wd
        self._install(order, wd.to(torch.float32), pop)
        return self

    def fit_interactions(self, item_ids, user_ids=None, days_ago=None, window_days=None, *,
                         _slab: int = 0):
        """Fit from plain arrays or tensors: one `hnm_popularity_fit_f64` call.

        pop[i] = sum over the rows of item i of exp(-time_decay * days_ago) (day weights
        `np.exp(-time_decay * np.arange(D))` in float64 on the host, D = max(days_ago) + 1 or
        `window_days`: rows older than the window are ignored); without `days_ago`, the row
        count.  Then order = items bought at least once, (pop descending, item id ascending).
        With personalized=True and `user_ids`, the interactions become the model's own
        history."""
        dev = self.device
        _lib.require_gpu(self._anchor)
        if isinstance(item_ids, torch.Tensor):
            items = item_ids.detach().to(device=dev, dtype=torch.int64).contiguous().reshape(-1)
        else:
            items = torch.from_numpy(np.ascontiguousarray(_host_array(item_ids, np.int64))).to(dev)
        n = items.numel()
        days = w = None
        D = 1
        if days_ago is not None:
            if isinstance(days_ago, torch.Tensor):
                days = days_ago.detach().to(device=dev, dtype=torch.int32).contiguous().reshape(-1)
            else:
                days = torch.from_numpy(
                    np.ascontiguousarray(_host_array(days_ago, np.int32))).to(dev)
            if days.numel() != n:
                raise ValueError("days_ago must match item_ids")
            if window_days is not None:
                D = int(window_days)
            else:
                D = int(days.max()) + 1 if n else 1
            if D < 1:
                raise ValueError("window_days (or max(days_ago) + 1) must be >= 1")
            w = torch.from_numpy(np.exp(-self.time_decay * np.arange(D))).to(dev)
        count = torch.empty(self.num_items, dtype=torch.int64, device=dev)
        pop = torch.empty(self.num_items, dtype=torch.float64, device=dev)
        _lib.call("hnm_popularity_fit_f64", _lib.ctx(dev), _lib.ptr(items), n, _lib.ptr(days),
                  _lib.ptr(w), self.num_items, D, int(_slab), _lib.ptr(count), _lib.ptr(pop))
        _lib.sync_check(dev)  # an item id outside [0, num_items): IndexError
        self.count = count
        bought = torch.nonzero(count > 0).reshape(-1)         # ascending item id
        _, perm = torch.sort(pop[bought], descending=True, stable=True)
        order = bought[perm]
        self._install(order, pop[order].to(torch.float32), pop)
        self.history = None
        if self.personalized and user_ids is not None:
            u = _host_array(user_ids, np.int64)
            num_users = int(u.max()) + 1 if u.size else 0
            self.history = UserHistory.from_interactions(u, items.cpu().numpy(), num_users,
                                                         self.num_items, dev)
        return self

    def fit_popularity(self, train_df, date_col: str = "t_dat"):
        """`baseline.py:137-165` on a duck-typed frame (`train_df[col]` -> array-like; pandas is
        not imported): columns article_idx, customer_idx and optionally `date_col` (datetimes).
        days_ago = (max date - date) in whole days when time_decay > 0 and the column exists."""
        cols = getattr(train_df, "columns", None)
        has_date = date_col in (cols if cols is not None else train_df)
        days = None
        if self.time_decay > 0 and has_date:
            dates = np.asarray(train_df[date_col]).astype("datetime64[ns]")
            if dates.size:
                days = ((dates.max() - dates) // np.timedelta64(1, "D")).astype(np.int32)
            else:
                days = np.zeros(0, np.int32)
        users = np.asarray(train_df["customer_idx"]) if self.personalized else None
        return self.fit_interactions(np.asarray(train_df["article_idx"]), users, days)

    # ------------------------------------------------------------------ answering
    def recommend_with_scores(self, user_ids, filter_items=None, k: Optional[int] = None,
                              *, _chunk: int = 0):
        """(scores [B, k] f32, items [B, k] int64): per user the first k entries of the order
        not in `filter_items` (a `{user: items}` dict or a `UserHistory`), scores = their
        popularity; rows with fewer than k entries left end in (-inf, -1).  k is clamped to
        num_items.  One `hnm_popularity_topk_f32` call."""
        self._fitted()
        k = self.top_k if k is None else k
        u, _ = self._ids(user_ids, None, flat=True)   # no user table: any id is a user
        mptr, midx = filter_csr(u, filter_items, self.num_items, u.device)
        kk = min(k, self.num_items)
        if kk <= 0:
            return empty_topk(k, u)
        B = u.numel()
        out_v, out_i = empty_rows(B, kk, u.device)
        _lib.call("hnm_popularity_topk_f32", _lib.ctx(u.device), _lib.ptr(self.order),
                  _lib.ptr(self.order_val), self.order.numel(), _lib.ptr(self.rank),
                  self.num_items, _lib.ptr(mptr), _lib.ptr(midx), B, kk, int(_chunk),
                  _lib.ptr(out_v), _lib.ptr(out_i))
        return out_v, out_i

    def forward(self, user_ids) -> torch.Tensor:
        """[B, k] int64 (`baseline.py:53-89`): every row the first k of the order; with
        personalized=True filtered by the model's own history.  -1 past the order's end."""
        self._fitted()
        hist = self.history if self.personalized else None
        with torch.no_grad():
            return self.recommend_with_scores(user_ids, filter_items=hist, k=self.top_k)[1]

    def recommend(self, user_ids, k: Optional[int] = None) -> Dict[int, List[int]]:
        """{user: [items]} (`baseline.py:167-194`), short rows trimmed."""
        self._fitted()
        k = self.top_k if k is None else k
        users = [int(x) for x in (user_ids.tolist() if isinstance(user_ids, torch.Tensor)
                                  else user_ids)]
        hist = self.history if self.personalized else None
        with torch.no_grad():
            _, top = self.recommend_with_scores(torch.tensor(users, dtype=torch.int64),
                                                filter_items=hist, k=k)
        return {u: [i for i in row if i >= 0] for u, row in zip(users, top.cpu().tolist())}

    def _validation_topk(self, batch):
        return self.forward(batch["user_ids"])
