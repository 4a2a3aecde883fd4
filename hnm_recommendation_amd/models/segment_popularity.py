"""SegmentPopularity: popular lists per user segment, for users the models have never seen.

No reference module.  The reference's data analysis (`scripts/analyze_recommendation_challenges.py`,
"COLD START STRATEGIES") names the strategy -- "Demographics -> popular items in age/gender
group", fallback global popularity -- and `src/models` never built it.  A segment is a small
integer the caller derives from the customers table (`age_segments` gives the age group;
combining it with `club_member_status` or `fashion_news_frequency` is the caller's arithmetic,
e.g. `age_group * 3 + club_status`); -1 means "unknown".

Two HIP entries (`csrc/segpop.hip`, contracts in `include/hnm.h`):

* `hnm_segpop_fit_f64` -- `PopularityBaseline`'s fit with one count table per segment: S + 1
  rows of `count` / `pop`, row S the global one, bitwise what `hnm_popularity_fit_f64` gives.
* `hnm_segpop_topk_f32` -- per request row the segment's list without the row's filter items,
  continued from the global list when it runs short (a small segment, `min_count`, a long
  history): one wave per row over the first k + h entries of the two orders.

Scores.  An entry carries the popularity of the list it came from: the segment's before the
seam, the global one after it.  A row's scores therefore are NOT monotone across the seam (each
part is); `recommend_for_segments(..., return_nseg=True)` tells where it is.  Blending the two
scales is out of scope: the lists are cascaded.

As `PopularityBaseline`: an order is (popularity descending, item id ascending); a segment's
order holds the items its users bought at least `min_count` times (inside the window), the
global order the items bought at least once; before a fit every answer raises
`RuntimeError("not fitted")`; the fitted tables are non-persistent buffers and the state_dict
is empty.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np
import torch

from .. import _lib
from ..evaluation import RecommendationMetrics
from .base import RecModule, empty_rows, empty_topk, filter_csr
from .popularity import PopularityBaseline, _host_array

_TABLES = ("count", "pop", "order_ptr", "order", "order_val", "rank", "segment_sizes",
           "user_segment", "_segment_of")


def age_segments(ages, edges=(25, 35, 45, 55, 65)) -> np.ndarray:
    """int32 age group per customer: the number of `edges` (ascending) that are <= age, so the
    default gives 0 for under 25, 1 for 25-34, ..., 5 for 65 and over; NaN or a negative age
    gives -1 ("unknown")."""
    e = np.asarray(edges, np.float64).reshape(-1)
    if e.size and not (np.isfinite(e).all() and (np.diff(e) > 0).all()):
        raise ValueError("edges must be finite and strictly ascending")
    a = np.asarray(ages, np.float64).reshape(-1)
    known = a >= 0          # False for NaN
    out = np.full(a.shape, -1, np.int32)
    out[known] = np.searchsorted(e, a[known], side="right")
    return out


class SegmentPopularity(RecModule):
    def __init__(self, n_items: int, n_segments: int, k: int = 12, time_decay: float = 0.0,
                 min_count: int = 1):
        super().__init__()
        self.save_hyperparameters()
        if int(n_items) < 0:
            raise ValueError("n_items must be >= 0")
        if int(n_segments) < 1:
            raise ValueError("n_segments must be >= 1")
        if int(min_count) < 1:
            raise ValueError("min_count must be >= 1")
        time_decay = float(time_decay)
        if not (np.isfinite(time_decay) and time_decay >= 0.0):
            raise ValueError("time_decay must be finite and >= 0")
        self.n_items = self.num_items = int(n_items)
        self.n_segments = self.num_segments = int(n_segments)
        self.k = self.top_k = int(k)
        self.time_decay = time_decay
        self.min_count = int(min_count)
        self.register_buffer("_anchor", torch.empty(0), persistent=False)
        for name in _TABLES:
            self.register_buffer(name, None, persistent=False)
        self.metrics = RecommendationMetrics(top_k=self.top_k)

    @property
    def device(self) -> torch.device:
        return self._anchor.device

    def _fitted(self):
        if self.order is None:
            raise RuntimeError("not fitted: call fit_interactions first")

    # ------------------------------------------------------------------ fitting
    def _dev(self, x, dtype, np_dtype):
        if isinstance(x, torch.Tensor):
            return x.detach().to(device=self.device, dtype=dtype).contiguous().reshape(-1)
        return torch.from_numpy(np.ascontiguousarray(_host_array(x, np_dtype))).to(self.device)

    def fit_interactions(self, item_ids, user_ids, user_segments, days_ago=None,
                         window_days=None, *, _slab: int = 0):
        """Fit from plain arrays or tensors: one `hnm_segpop_fit_f64` call, then the S + 1
        orders on the device.

        `user_segments[u]`: the segment of user u in [0, n_segments), negative = unknown (such
        a user's purchases count for the global list only); it stays on the device and answers
        `recommend_with_scores` for known users.  `days_ago` / `window_days`: as
        `PopularityBaseline.fit_interactions`.  A user id outside the segment table, a segment
        >= n_segments or an item outside [0, n_items): IndexError."""
        dev = self.device
        _lib.require_gpu(self._anchor)
        S, I = self.num_segments, self.num_items
        items = self._dev(item_ids, torch.int64, np.int64)
        users = self._dev(user_ids, torch.int64, np.int64)
        useg = self._dev(user_segments, torch.int32, np.int32)
        n = items.numel()
        if users.numel() != n:
            raise ValueError("user_ids must match item_ids")
        days = w = None
        D = 1
        if days_ago is not None:
            days = self._dev(days_ago, torch.int32, np.int32)
            if days.numel() != n:
                raise ValueError("days_ago must match item_ids")
            if window_days is not None:
                D = int(window_days)
            else:
                D = int(days.max()) + 1 if n else 1
            if D < 1:
                raise ValueError("window_days (or max(days_ago) + 1) must be >= 1")
            w = torch.from_numpy(np.exp(-self.time_decay * np.arange(D))).to(dev)
        count = torch.empty(S + 1, I, dtype=torch.int64, device=dev)
        pop = torch.empty(S + 1, I, dtype=torch.float64, device=dev)
        _lib.call("hnm_segpop_fit_f64", _lib.ctx(dev), _lib.ptr(items), _lib.ptr(users), n,
                  _lib.ptr(useg), useg.numel(), _lib.ptr(days), _lib.ptr(w), I, S, D, int(_slab),
                  _lib.ptr(count), _lib.ptr(pop))
        _lib.sync_check(dev)  # an id or a segment out of range: IndexError
        orders = []
        rank = torch.full((S + 1, I), -1, dtype=torch.int32, device=dev)
        for s in range(S + 1):
            keep = count[s] >= (self.min_count if s < S else 1)
            ids = torch.nonzero(keep).reshape(-1)              # ascending item id
            _, perm = torch.sort(pop[s][ids], descending=True, stable=True)
            o = ids[perm]
            rank[s, o] = torch.arange(o.numel(), dtype=torch.int32, device=dev)
            orders.append(o)
        lens = torch.tensor([0] + [o.numel() for o in orders], dtype=torch.int64)
        self.count, self.pop, self.rank = count, pop, rank
        self.order_ptr = torch.cumsum(lens, 0).to(dev)
        self.order = torch.cat(orders)
        self.order_val = torch.cat([pop[s][o] for s, o in enumerate(orders)]).to(torch.float32)
        self.user_segment = useg
        # the lookup of recommend_with_scores: two trailing -1 entries, so that an id clamped to
        # [-1, len] reads "unknown" when it is past the table (len) or negative (-1: the last)
        self._segment_of = torch.cat([useg, torch.full((2,), -1, dtype=torch.int32, device=dev)])
        self.segment_sizes = torch.bincount(useg[useg >= 0].to(torch.int64), minlength=S)[:S]
        return self

    def global_baseline(self) -> PopularityBaseline:
        """A `PopularityBaseline` installed from the global row: both models from one fit."""
        self._fitted()
        S = self.num_segments
        base = PopularityBaseline(self.num_items, k=self.top_k,
                                  time_decay=self.time_decay).to(self.device)
        p0, p1 = int(self.order_ptr[S]), int(self.order_ptr[S + 1])
        base._install(self.order[p0:p1].clone(), self.order_val[p0:p1].clone(),
                      self.pop[S].clone())
        base.count = self.count[S].clone()
        return base

    # ------------------------------------------------------------------ answering
    def _check_segments(self, segments) -> torch.Tensor:
        """Host int32 [B] of request segments (None = -1); ValueError outside [-1, S)."""
        seg = np.asarray([-1 if s is None else int(s) for s in segments], np.int64).reshape(-1)
        if seg.size and (seg.min() < -1 or seg.max() >= self.num_segments):
            raise ValueError(f"segments must be in [-1, {self.num_segments}), -1 or None = "
                             "unknown")
        return torch.from_numpy(seg.astype(np.int32))

    def _topk(self, seg, rows, filter_items, k, chunk=0):
        """One `hnm_segpop_topk_f32` call: `seg` int32 [B] and the mask's row keys `rows` on the
        device.  (scores, items, nseg)."""
        dev = rows.device
        mptr, midx = filter_csr(rows, filter_items, self.num_items, dev)
        B = rows.numel()
        kk = min(k, self.num_items)
        if kk <= 0:
            return (*empty_topk(k, rows), torch.zeros(B, dtype=torch.int32, device=dev))
        out_v, out_i = empty_rows(B, kk, dev)
        nseg = torch.empty(B, dtype=torch.int32, device=dev)
        _lib.call("hnm_segpop_topk_f32", _lib.ctx(dev), _lib.ptr(self.order),
                  _lib.ptr(self.order_val), _lib.ptr(self.order_ptr), _lib.ptr(self.rank),
                  self.num_items, self.num_segments, _lib.ptr(seg), _lib.ptr(mptr),
                  _lib.ptr(midx), B, kk, int(chunk), _lib.ptr(out_v), _lib.ptr(out_i),
                  _lib.ptr(nseg))
        return out_v, out_i, nseg

    def recommend_with_scores(self, user_ids, filter_items=None, k: Optional[int] = None,
                              *, _chunk: int = 0):
        """(scores [B, k] f32, items [B, k] int64) for users of the fit: a user's segment comes
        from the fitted `user_segments`; an id past that table is a user without a segment (the
        global list).  Per row the segment's order without `filter_items` (a `{user: items}`
        dict or a `UserHistory`), continued from the global order; rows with fewer than k
        entries left end in (-inf, -1).  k is clamped to num_items."""
        self._fitted()
        k = self.top_k if k is None else k
        u, _ = self._ids(user_ids, None, flat=True)   # any id is a user
        seg = self._segment_of[u.clamp(-1, self.user_segment.numel())]
        return self._topk(seg, u, filter_items, k, _chunk)[:2]

    def recommend_for_segments(self, segments, filter_items=None, k: Optional[int] = None,
                               return_nseg: bool = False):
        """The same answer for visitors without a user index: `segments[j]` in [-1, n_segments)
        (None or -1 = unknown: the global list; anything else ValueError, before any launch),
        `filter_items` a `{row position j: items}` dict.  With `return_nseg` a third result:
        int32 [B], how many leading entries of each row came from the segment's own list."""
        if isinstance(segments, torch.Tensor):
            segments = segments.detach().cpu().reshape(-1).tolist()
        seg = self._check_segments(segments)
        self._fitted()
        dev = self.device
        _lib.require_gpu(dev)
        k = self.top_k if k is None else k
        rows = torch.arange(seg.numel(), dtype=torch.int64, device=dev)
        v, i, nseg = self._topk(seg.to(dev), rows, filter_items, k)
        return (v, i, nseg) if return_nseg else (v, i)

    def forward(self, user_ids) -> torch.Tensor:
        """[B, k] int64: every user's unfiltered list, -1 past the global order's end."""
        self._fitted()
        with torch.no_grad():
            return self.recommend_with_scores(user_ids, k=self.top_k)[1]

    def recommend(self, user_ids, k: Optional[int] = None) -> Dict[int, List[int]]:
        """{user: [items]}, short rows trimmed."""
        self._fitted()
        k = self.top_k if k is None else k
        users = [int(x) for x in (user_ids.tolist() if isinstance(user_ids, torch.Tensor)
                                  else user_ids)]
        with torch.no_grad():
            _, top = self.recommend_with_scores(torch.tensor(users, dtype=torch.int64), k=k)
        return {u: [i for i in row if i >= 0] for u, row in zip(users, top.cpu().tolist())}

    def _validation_topk(self, batch):
        return self.forward(batch["user_ids"])
