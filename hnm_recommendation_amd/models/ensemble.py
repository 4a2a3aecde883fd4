"""Ensemble: several models' top-K lists fused into one on the GPU (no reference module:
`GEMINI.md` stage 5 names a "CF score ensemble", stage 7 picking the best model, and `src/models`
built neither).

Every member answers `recommend_with_scores(user_ids, filter_items, k=depth)`; the G lists land
in one [G, B, depth] pair of tensors and one HIP entry (`hnm_fuse_topk_f32`, `csrc/fuse.hip`,
contract in `include/hnm.h`) fuses them: one wave per user over an LDS table keyed by item id.
The members' items overlap, and an item's fused score depends on every list that holds it:

* `"rrf"` -- reciprocal rank fusion (Cormack, Clarke & Buettcher 2009): an item at rank r of
  member g adds w_g / (c + r), c = 60 by the paper.  Ranks need no common score scale, so a
  popularity count, a cosine sum and a dot product blend as they are.
* `"score"` -- the weighted sum of the members' scores, w_g * score; meaningful when the
  members' scores share a scale (no normalisation is applied).
* `"cascade"` -- member 0's list first, then what member 1 adds, and so on, each item with the
  score of the member that supplied it: a short list continued from the next one (what
  `serving.Recommender._back_fill` does on the host for ItemCF and the popularity list).

An item's sum runs over the members in their order, in fp32 from the first contribution, and
the selection is (fused score descending, item ascending): the same bits on every run.  Rows
with fewer than k fused items end in (-inf, -1).
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch
import torch.nn as nn

from .. import _lib
from ..evaluation import RecommendationMetrics
from .base import RecModule, basket_csr, empty_rows, empty_topk, filter_csr

MODES = {"rrf": _lib.HNM_FUSE_RANK, "score": _lib.HNM_FUSE_SCORE,
         "cascade": _lib.HNM_FUSE_CASCADE}
MAX_MEMBERS = 16      # hnm_fuse_topk_f32: G
MAX_DEPTH = 512       # ... kc
MAX_ENTRIES = 2048    # ... G * kc
MAX_K = 128           # ... k


class Ensemble(RecModule):
    takes_basket_weights = False

    def __init__(self, members, weights=None, mode: str = "rrf", rank_constant: float = 60.0,
                 depth: Optional[int] = None, top_k: int = 12):
        """`members`: an ordered `{name: model}` or a list of `(name, model)`, kept in an
        `nn.ModuleDict` (state_dict keys `members.<name>.…`); all of one `num_items`.
        `weights`: one finite value > 0 per member (default 1 each).  `mode`: "rrf", "score" or
        "cascade".  `rank_constant`: c of "rrf", finite and >= 0.  `depth`: how many candidates
        are asked of each member; the default, max(k, 4 * top_k) of the call's k clamped to
        num_items, 512 and 2,048 / len(members), is a design choice (a few times the answer's
        length, so that an item ranked low by one member and high by another still meets
        itself), not a measured optimum."""
        super().__init__()
        pairs = list(members.items()) if hasattr(members, "items") else [tuple(m) for m in members]
        names = [str(n) for n, _ in pairs]
        if not pairs:
            raise ValueError("an Ensemble needs at least one member")
        if len(pairs) > MAX_MEMBERS:
            raise ValueError(f"an Ensemble takes at most {MAX_MEMBERS} members")
        if len(set(names)) != len(names):
            raise ValueError(f"member names must be distinct, got {names}")
        if mode not in MODES:
            raise ValueError(f'mode must be one of {sorted(MODES)}, got "{mode}"')
        sizes = {int(m.num_items) for _, m in pairs}
        if len(sizes) != 1:
            raise ValueError(f"members disagree on num_items: {sorted(sizes)}")
        w = [1.0] * len(pairs) if weights is None else [float(x) for x in weights]
        if len(w) != len(pairs):
            raise ValueError(f"{len(w)} weights for {len(pairs)} members")
        if not all(math.isfinite(x) and x > 0.0 and math.isfinite(np.float32(x)) for x in w):
            raise ValueError("weights must be finite and > 0")
        rank_constant = float(rank_constant)
        if not (math.isfinite(rank_constant) and rank_constant >= 0.0):
            raise ValueError("rank_constant must be finite and >= 0")
        if depth is not None:
            depth = int(depth)
            if depth < 1:
                raise ValueError("depth must be >= 1")
            if depth > MAX_DEPTH or depth * len(pairs) > MAX_ENTRIES:
                raise ValueError(f"depth must be <= {MAX_DEPTH} and depth * members <= "
                                 f"{MAX_ENTRIES}")
        self.members = nn.ModuleDict()
        for name, m in pairs:
            try:
                self.members[name] = m
            except (KeyError, TypeError) as e:
                raise ValueError(f'"{name}" cannot name a member: {e}') from None
        self.hparams = {"members": names, "weights": w, "mode": mode,
                        "rank_constant": rank_constant, "depth": depth, "top_k": int(top_k)}
        self.num_items = sizes.pop()
        users = [int(m.num_users) for _, m in pairs if getattr(m, "num_users", None) is not None]
        self.num_users = min(users) if users else None   # None: no member has a user table
        self.weights, self.mode, self.rank_constant = w, mode, rank_constant
        self.depth, self.top_k = depth, int(top_k)
        # what serving.Recommender asks (RecModule): per instance, from the members
        self.answers_baskets = all(m.answers_baskets for _, m in pairs)
        self.back_fill_short_rows = any(m.back_fill_short_rows for _, m in pairs)
        self.metrics = RecommendationMetrics(top_k=self.top_k)

    # ------------------------------------------------------------------ members
    def _models(self):
        return list(self.members.values())

    @property
    def device(self) -> torch.device:
        return self._models()[0].device

    @property
    def history(self):
        """The first member history that is not None (a member's own, fitted or set)."""
        for m in self._models():
            h = getattr(m, "history", None)
            if h is not None:
                return h
        return None

    def set_history(self, history):
        """Forward `history` to the members that keep a history and have none."""
        for m in self._models():
            if hasattr(m, "set_history") and getattr(m, "history", None) is None:
                m.set_history(history)
        return self

    # ------------------------------------------------------------------ fusing
    def _depth(self, k: int) -> int:
        d = max(k, 4 * self.top_k) if self.depth is None else self.depth
        return max(1, min(d, self.num_items, MAX_DEPTH, MAX_ENTRIES // len(self.members)))

    def rank_weights(self, depth: Optional[int] = None) -> torch.Tensor:
        """[G, depth] float32 (host): coef[g, j] = float32(w_g) / (float32(c) + float32(j + 1)),
        every step in float32 -- the table "rrf" hands to the kernel.  `depth` defaults to the
        depth of a call with k = top_k."""
        depth = self._depth(min(self.top_k, self.num_items)) if depth is None else int(depth)
        w = np.asarray(self.weights, np.float32).reshape(-1, 1)
        ranks = np.arange(1, depth + 1, dtype=np.float32).reshape(1, -1)
        return torch.from_numpy((w / (np.float32(self.rank_constant) + ranks)).astype(np.float32))

    def _coef(self, depth: int, dev):
        if self.mode == "rrf":
            return self.rank_weights(depth).to(dev).contiguous()
        if self.mode == "score":
            return torch.tensor(self.weights, dtype=torch.float32).to(dev)
        return None

    def _fuse(self, lists, B: int, depth: int, mptr, midx, k: int, dev):
        """One `hnm_fuse_topk_f32` call over the members' (scores, items) pairs."""
        G = len(lists)
        lv = torch.empty(G, B, depth, dtype=torch.float32, device=dev)
        li = torch.empty(G, B, depth, dtype=torch.int64, device=dev)
        for g, (v, i) in enumerate(lists):
            if tuple(v.shape) != (B, depth) or tuple(i.shape) != (B, depth):
                raise RuntimeError(f"member {list(self.members)[g]} returned lists of shape "
                                   f"{tuple(i.shape)}, expected {(B, depth)}")
            lv[g].copy_(v)
            li[g].copy_(i)
        out_v, out_i = empty_rows(B, k, dev)
        coef = self._coef(depth, dev)
        _lib.call("hnm_fuse_topk_f32", _lib.ctx(dev), _lib.ptr(lv), _lib.ptr(li), B, G,
                  B * depth, depth, depth, MODES[self.mode], _lib.ptr(coef), self.num_items,
                  _lib.ptr(mptr), _lib.ptr(midx), k, _lib.ptr(out_v), _lib.ptr(out_i))
        return out_v, out_i

    def _clamp_k(self, k: Optional[int]) -> int:
        k = self.top_k if k is None else int(k)
        if min(k, self.num_items) > MAX_K:
            raise ValueError(f"an Ensemble answers at most k = {MAX_K} items per row, got {k}")
        return k

    def recommend_with_scores(self, user_ids, filter_items=None, k: Optional[int] = None):
        """(scores [B, k] f32, items [B, k] int64): each member's
        `recommend_with_scores(user_ids, filter_items, k=depth)` fused by the module's mode;
        rows with fewer than k fused items end in (-inf, -1).  k is clamped to num_items; k > 128
        raises ValueError before any launch."""
        k = self._clamp_k(k)
        ids = user_ids if isinstance(user_ids, torch.Tensor) else torch.as_tensor(user_ids)
        ids = ids.reshape(-1)
        u, _ = self._ids(ids, self.num_users)   # host ids: range-checked here, before any launch
        kk = min(k, self.num_items)
        if kk <= 0:
            return empty_topk(k, u)
        depth = self._depth(kk)
        # the members get the caller's ids: host ids stay host ids (checked on the host, no
        # sync), device ids are checked by each member's own kernels
        lists = [m.recommend_with_scores(ids, filter_items, k=depth) for m in self._models()]
        mptr, midx = filter_csr(u, filter_items, self.num_items, u.device)
        return self._fuse(lists, u.numel(), depth, mptr, midx, kk, u.device)

    def recommend(self, user_ids, filter_items=None) -> torch.Tensor:
        """[B, top_k] int64 item ids (-1 past the last fused item)."""
        self._check_top_k()
        with torch.no_grad():
            return self.recommend_with_scores(user_ids, filter_items=filter_items,
                                              k=self.top_k)[1]

    def forward(self, user_ids, filter_items=None) -> torch.Tensor:
        return self.recommend(user_ids, filter_items=filter_items)

    def predict_all_items(self, user_ids):
        raise NotImplementedError(
            "an Ensemble fuses its members' top-K lists: an item outside every list has no fused "
            "score, so there is no dense [B, num_items] row to return")

    def recommend_for_items(self, baskets, filter_seen: bool = True, k: Optional[int] = None):
        """(scores [n, k], items [n, k]) for n baskets of item ids: the members'
        `recommend_for_items(baskets, filter_seen, k=depth)` fused.  Only when every member
        answers baskets (`answers_baskets`); NotImplementedError otherwise."""
        if not self.answers_baskets:
            cannot = [n for n, m in self.members.items() if not m.answers_baskets]
            raise NotImplementedError(f"members {cannot} cannot answer from a basket of items")
        k = self._clamp_k(k)
        dev = self.device
        _lib.require_gpu(dev)
        ptr, idx, n, _ = basket_csr(baskets, self.num_items, dev)
        kk = min(k, self.num_items)
        if kk <= 0:
            return empty_topk(k, ptr[:n])
        if n == 0:
            return empty_rows(0, kk, dev)
        depth = self._depth(kk)
        lists = [m.recommend_for_items((ptr, idx), filter_seen=filter_seen, k=depth)
                 for m in self._models()]
        mptr, midx = (ptr, idx) if filter_seen else (None, None)
        return self._fuse(lists, n, depth, mptr, midx, kk, dev)
