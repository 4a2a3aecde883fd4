"""ItemCF: item-based collaborative filtering (no reference module: `GEMINI.md` stage 3 names it
among the baselines, and the reference's data analysis names "item similarity" as the answer to
its cold-start customers, but `src/models` never built it).

Three HIP entries (`csrc/itemcf.hip`, contract in `include/hnm.h`):

* `hnm_itemcf_fit_f32` -- the fit: co-occurrence counts over the device-resident `UserHistory`
  CSR, cosine similarity with shrinkage in float64 rounded once to float32, the
  `num_neighbors` best per item in (sim descending, item ascending) order.  Integer atomics
  only: the same bits on every run.
* `hnm_itemcf_scores_f32` -- dense rows (`predict_all_items`): score[i] = the fp32 sum of
  sim(j -> i) over the history items j in ascending order.
* `hnm_itemcf_topk_f32` -- the answer: one wave per row over an LDS table instead of a
  [B, num_items] matrix; a row is a user's history or, without user ids, a basket
  (`recommend_for_items`: a visitor without a user index).

Each entry has a weighted sibling (`hnm_itemcf_*_weighted_f32`: `hist_w`, an fp32 weight per
history entry -- a purchase count times a recency decay, `UserHistory.hist_w`).  `WeightedItemCF`
is the `ItemCF` that uses them: the fit counts q_ui * q_uj in fixed point (integers: still the
same bits on every run) instead of 1, a user's or basket's sum takes w_j * sim(j -> i).  A plain
`ItemCF` never calls them and refuses weights.

Top-K convention (as `PopularityBaseline`): the unmasked items with score > 0 in (score
descending, item ascending) order, rows with fewer than k of them end in (-inf, -1).  History
items are not excluded by themselves: the filter does that, as for every other model.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional

import numpy as np
import torch

from .. import _lib
from ..evaluation import RecommendationMetrics
from .base import (HistoryModel, RecModule, UserHistory, basket_csr, dense_topk, empty_rows,
                   empty_topk, filter_csr, interactions_history)

MAX_NEIGHBORS = 64   # one lane per neighbour
FUSED_MAX_K = 64     # hnm_itemcf_topk_f32; above: dense rows + dense_topk


class ItemCF(HistoryModel, RecModule):
    # WeightedItemCF: True (the hyperparameter "weighted" of its hparams)
    weighted = takes_basket_weights = False
    answers_baskets = back_fill_short_rows = True
    _NO_HISTORY = "no history: call set_history (or fit_interactions) first"

    def __init__(self, num_users: int, num_items: int, num_neighbors: int = 64,
                 shrink: float = 0.0, max_history: int = 0, top_k: int = 12):
        super().__init__()
        self.save_hyperparameters()
        if not 1 <= int(num_neighbors) <= MAX_NEIGHBORS:
            raise ValueError(f"num_neighbors must be in [1, {MAX_NEIGHBORS}]")
        if not float(shrink) >= 0.0 or not np.isfinite(shrink):
            raise ValueError("shrink must be finite and >= 0")
        if int(max_history) < 0:
            raise ValueError("max_history must be >= 0 (0 = no cap)")
        self.num_users, self.num_items = int(num_users), int(num_items)
        self.num_neighbors = int(num_neighbors)
        self.shrink, self.max_history, self.top_k = float(shrink), int(max_history), int(top_k)
        shape = (self.num_items, self.num_neighbors)
        self.register_buffer("neighbor_idx", torch.full(shape, -1, dtype=torch.int32))
        self.register_buffer("neighbor_val", torch.zeros(shape, dtype=torch.float32))
        self.register_buffer("item_count", torch.zeros(self.num_items, dtype=torch.int64))
        self._is_fitted: Optional[bool] = False   # None: unknown (a loaded state), looked up once
        self.metrics = RecommendationMetrics(top_k=self.top_k)

    @property
    def device(self) -> torch.device:
        return self.neighbor_idx.device

    def load_state_dict(self, state_dict, *args, **kwargs):
        out = super().load_state_dict(state_dict, *args, **kwargs)
        self._is_fitted = None
        return out

    def _fitted(self):
        if self._is_fitted is None:  # a loaded table is fitted when it counted anything
            self._is_fitted = bool((self.item_count > 0).any())
        if not self._is_fitted:
            raise RuntimeError("not fitted: call fit_interactions / fit_history, or load a "
                               "fitted state_dict")

    # ------------------------------------------------------------------ fitting
    def _row_weights(self, history: UserHistory):
        """The weights a history row is served with: `hist_w` for a weighted model (None when the
        history has none: served unweighted), None for a plain one."""
        return history.hist_w if self.weighted else None

    def fit_history(self, history: UserHistory, *, _window: int = 0):
        """Fit on a `UserHistory` and keep it as the model's history: one
        `hnm_itemcf_fit_f32` call (`_window`: item columns per LDS pass, for tests).  A weighted
        model needs `history.hist_w` (ValueError without) and calls
        `hnm_itemcf_fit_weighted_f32`."""
        if self.weighted and isinstance(history, UserHistory) and history.hist_w is None:
            raise ValueError("a weighted ItemCF is fitted on a history with weights "
                             "(UserHistory.from_interactions(..., weights=))")
        _lib.require_gpu(self.neighbor_idx)
        h = self.set_history(history)._need_history()
        dev = self.device
        for name, dtype in (("neighbor_idx", torch.int32), ("neighbor_val", torch.float32),
                            ("item_count", torch.int64)):
            t = getattr(self, name)
            if t.dtype != dtype or not t.is_contiguous():
                setattr(self, name, t.to(dtype).contiguous())
        _lib.call_weighted(
            "hnm_itemcf_fit_f32", 3, self._row_weights(h), _lib.ctx(dev), _lib.ptr(h.hist_ptr),
            _lib.ptr(h.hist_idx), self.num_users, self.num_items, self.num_neighbors, self.shrink,
            self.max_history, int(_window), _lib.ptr(self.neighbor_idx),
            _lib.ptr(self.neighbor_val), _lib.ptr(self.item_count))
        _lib.sync_check(dev)
        self._is_fitted = True
        return self

    def fit_interactions(self, user_ids, item_ids, *, weights=None, days_ago=None,
                         time_decay: float = 0.0, _window: int = 0):
        """Fit from (user, item) interaction arrays or tensors (duplicates allowed; ids out of
        range raise IndexError): builds the `UserHistory`, keeps it, runs the fit.

        A weighted model takes `weights` (one finite value >= 0 per transaction) and / or
        `days_ago` (whole days >= 0) with `time_decay` >= 0, by `ImplicitALS.fit_interactions`'
        rules: a transaction weighs weights * exp(-time_decay * days_ago), a pair the sum of its
        transactions; with neither a transaction weighs 1, a pair its number of purchases (pairs
        that occur once each give the unweighted table's bits).  A plain model raises ValueError
        for either."""
        if not self.weighted and (weights is not None or days_ago is not None):
            raise ValueError("this ItemCF is not weighted: build a WeightedItemCF to fit with "
                             "weights or days_ago")
        if not self.weighted:   # a weighted model validates its arguments first (fit_history asks)
            _lib.require_gpu(self.neighbor_idx)
        # a plain model has refused weights and days_ago above and reads no time_decay
        hist = interactions_history(user_ids, item_ids, self.num_users, self.num_items, self.device,
                                    weights, days_ago, time_decay if self.weighted else 0.0,
                                    unit_weights=self.weighted)
        return self.fit_history(hist, _window=_window)

    # ------------------------------------------------------------------ answering
    def _table_and_rows(self, dev, hptr, hidx):
        """The leading arguments of the scores and top-K entries, up to the history CSR."""
        return (_lib.ctx(dev), _lib.ptr(self.neighbor_idx), _lib.ptr(self.neighbor_val),
                self.num_items, self.num_neighbors, _lib.ptr(hptr), _lib.ptr(hidx))

    def _dense(self, hptr, hidx, rows: int, u: Optional[torch.Tensor], B: int,
               w: Optional[torch.Tensor] = None) -> torch.Tensor:
        """[B, num_items] scores; `w` (fp32, aligned with hidx) selects the weighted entry."""
        dev = self.device
        out = torch.empty(B, self.num_items, dtype=torch.float32, device=dev)
        _lib.call_weighted("hnm_itemcf_scores_f32", 7, w, *self._table_and_rows(dev, hptr, hidx),
                           rows, _lib.ptr(u), B, _lib.ptr(out),
                           out.stride(0) if B else self.num_items)
        return out

    def _topk(self, hptr, hidx, rows: int, u: Optional[torch.Tensor], B: int, mptr, midx, k: int,
              w: Optional[torch.Tensor] = None):
        """(scores [B, k], items [B, k]) of B history rows (u None: the CSR's own rows); `w`
        (fp32, aligned with hidx) selects the weighted entries."""
        dev = self.device
        if k <= FUSED_MAX_K:
            out_v, out_i = empty_rows(B, k, dev)
            _lib.call_weighted("hnm_itemcf_topk_f32", 7, w, *self._table_and_rows(dev, hptr, hidx),
                               rows, _lib.ptr(u), B, _lib.ptr(mptr), _lib.ptr(midx), k,
                               _lib.ptr(out_v), _lib.ptr(out_i))
            return out_v, out_i
        # k > 64: the dense rows and the row top-k kernel; slots without a positive score
        # (zero scores, masked items) become (-inf, -1)
        if B == 0:
            return empty_rows(B, k, dev)
        out_v, out_i = dense_topk(self._dense(hptr, hidx, rows, u, B, w), k, mptr, midx)
        pad = ~(out_v > 0)
        return out_v.masked_fill(pad, float("-inf")), out_i.masked_fill(pad, -1)

    def predict_all_items(self, user_ids) -> torch.Tensor:
        """[B, num_items] scores of the users' history rows."""
        self._fitted()
        u, host = self._ids(user_ids, self.num_users, flat=True)
        h = self._need_history()
        out = self._dense(h.hist_ptr, h.hist_idx, h.num_users, u, u.numel(),
                          self._row_weights(h))
        self._check(u.device, host)
        return out

    def recommend_with_scores(self, user_ids, filter_items=None, k: Optional[int] = None):
        """(scores [B, k] f32, items [B, k] int64): per user the items with score > 0 not in
        `filter_items` (a `{user: items}` dict or a `UserHistory`), best first; short rows end
        in (-inf, -1).  k is clamped to num_items."""
        self._fitted()
        k = self.top_k if k is None else k
        u, host = self._ids(user_ids, self.num_users, flat=True)
        h = self._need_history()
        mptr, midx = filter_csr(u, filter_items, self.num_items, u.device)
        kk = min(k, self.num_items)
        if kk <= 0:
            return empty_topk(k, u)
        out = self._topk(h.hist_ptr, h.hist_idx, h.num_users, u, u.numel(), mptr, midx, kk,
                         self._row_weights(h))
        self._check(u.device, host)
        return out

    def recommend(self, user_ids, filter_items=None) -> torch.Tensor:
        """[B, top_k] int64 item ids (-1 past the last item with a positive score)."""
        self._check_top_k()
        with torch.no_grad():
            return self.recommend_with_scores(user_ids, filter_items=filter_items,
                                              k=self.top_k)[1]

    def forward(self, user_ids) -> torch.Tensor:
        """`recommend` filtered by the model's own history."""
        return self.recommend(user_ids, filter_items=self.history)

    def _validation_topk(self, batch):
        # held-out purchases are scored against what the model was fitted on
        return self.forward(batch["user_ids"])

    def recommend_for_items(self, baskets, filter_seen: bool = True, k: Optional[int] = None, *,
                            weights=None):
        """(scores [n, k], items [n, k]) for n baskets of item ids -- visitors without a user
        index.  `filter_seen` removes each basket's own items from its answer.  `weights` (a
        weighted model only, else ValueError): a weight per basket entry, a repeated item's
        summed, see `basket_csr`."""
        if weights is not None and not self.weighted:
            raise ValueError("this ItemCF is not weighted: it takes no basket weights")
        self._fitted()
        _lib.require_gpu(self.neighbor_idx)
        k = self.top_k if k is None else k
        ptr, idx, n, w = basket_csr(baskets, self.num_items, self.device, weights)
        kk = min(k, self.num_items)
        if kk <= 0:
            return empty_topk(k, ptr[:n])
        mptr, midx = (ptr, idx) if filter_seen else (None, None)
        out = self._topk(ptr, idx, n, None, n, mptr, midx, kk, w)
        _lib.sync_check(self.device)   # a CSR given by the caller may hold any id
        return out

    def similar_items(self, item_ids, k: Optional[int] = None):
        """(sim [n, k] f32, items [n, k] int64): the k nearest neighbours of each item, rows of
        the fitted table (short rows end in (0.0, -1))."""
        self._fitted()
        k = self.num_neighbors if k is None else int(k)
        if not 0 <= k <= self.num_neighbors:
            raise ValueError(f"k must be in [0, num_neighbors = {self.num_neighbors}]")
        ids = torch.as_tensor(item_ids).reshape(-1).to(device=self.device, dtype=torch.int64)
        if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= self.num_items):
            raise IndexError(f"item ids must be in [0, {self.num_items})")
        return self.neighbor_val[ids, :k], self.neighbor_idx[ids, :k].to(torch.int64)

    def scoring_route(self, user_ids) -> List[str]:
        """Per user "fused" (the LDS table) or "dense" (a workspace row): what
        `hnm_itemcf_topk_f32` does with that history length.  The caller cannot choose."""
        u, _ = self._ids(user_ids, self.num_users, flat=True)
        h = self._need_history()
        lens = (h.hist_ptr[u + 1] - h.hist_ptr[u]).cpu().tolist()
        c = _lib.ctx(self.device)
        out = []
        for n in lens:
            route = C.c_int(-1)
            _lib.call("hnm_itemcf_route", c, self.num_neighbors, int(n), C.byref(route))
            out.append("dense" if route.value == 1 else "fused")
        return out


class WeightedItemCF(ItemCF):
    """`ItemCF` with the hyperparameter `weighted` = True (`hparams["weighted"]`; the buffers and
    state_dict keys are ItemCF's): fitted on `UserHistory.hist_w` by
    `hnm_itemcf_fit_weighted_f32`, a user's row weighted by the history's `hist_w`, baskets by
    the call's `weights`.  `ItemCF.__init__` keeps its parameter list, so the flag is the class;
    a checkpoint whose hyper-parameters hold `weighted: True` is built as this class
    (`serving.create_model_from_checkpoint`)."""
    weighted = takes_basket_weights = True

    def __init__(self, num_users: int, num_items: int, num_neighbors: int = 64,
                 shrink: float = 0.0, max_history: int = 0, top_k: int = 12,
                 weighted: bool = True):
        if not weighted:
            raise ValueError("a WeightedItemCF is weighted: build an ItemCF instead")
        super().__init__(num_users, num_items, num_neighbors=num_neighbors, shrink=shrink,
                         max_history=max_history, top_k=top_k)
        self.hparams["weighted"] = True
