"""Reranker: neural re-scoring of recall candidates -- two-stage serving (no reference module:
the summary of the reference's `scripts/analyze_recommendation_challenges.py` asks for "Stage 1:
candidate generation (popularity, content similarity, collaborative filtering), Stage 2: ranking
(deep learning models: NCF, Wide&Deep)", and `src/models` built the rankers for the whole
catalogue only).

Stage 1: every source answers `recommend_with_scores(user_ids, filter_items, k=depth)` -- as an
`Ensemble` asks its members, so an `Ensemble` may itself be a source.  The G lists land in one
[G, B, depth] pair of tensors and one HIP entry (`hnm_cand_union_i32`, `csrc/rerank.hip`) merges
each user's lists into one duplicate-free, ascending candidate row.

Stage 2: the ranker scores the candidates and the best k are selected, (score descending, item
ascending); the scores of the answer are the RANKER's.

* a `WideDeep` ranker takes one `hnm_widedeep_cand_topk_ex_f32` call
  (`csrc/widedeep_cand.hip`): every candidate's score is bitwise its entry of
  `predict_all_items`, and the selection rides in the same launch (k <= 64; above, the entry
  writes the scores and `hnm_cand_topk_f32` selects);
* any other ranker with the reference's pairwise `forward(user_ids, item_ids)`
  (`MatrixFactorization`, `ImplicitALS`, `NeuralCF`) scores the flattened (user, candidate) pairs
  with it -- padded positions ask for item 0 and are excluded by the row's count -- and
  `hnm_cand_topk_f32` selects.

Rows with fewer than k candidates end in (-inf, -1).
"""
from __future__ import annotations

import ctypes as C
import inspect
from typing import Optional

import torch
import torch.nn as nn

from .. import _lib
from ..evaluation import RecommendationMetrics
from .base import RecModule, empty_rows, empty_topk
from .wide_deep import WideDeep

MAX_SOURCES = 16      # hnm_cand_union_i32: G
MAX_DEPTH = 512       # ... kc
MAX_ENTRIES = 2048    # ... G * kc
MAX_K = 128           # hnm_cand_topk_f32: k
FUSED_K = 64          # hnm_widedeep_cand_topk_ex_f32: k of the fused selection

ROUTE_WIDEDEEP = "widedeep_cand_topk"          # scored and selected in one launch
ROUTE_WIDEDEEP_WIDE = "widedeep_cand_scores"   # 64 < k <= 128: scores, then hnm_cand_topk_f32
ROUTE_PAIRS = "pairwise_forward"               # ranker.forward on the pairs, then the selection


def clamp_depth(depth: Optional[int], k: int, top_k: int, num_items: int, G: int) -> int:
    """Candidates asked of each of G sources for an answer of k: `Ensemble._depth`'s rule --
    max(k, 4 * top_k) unless `depth` is given, clamped to num_items, 512 and 2,048 / G."""
    d = max(k, 4 * top_k) if depth is None else depth
    return max(1, min(d, num_items, MAX_DEPTH, MAX_ENTRIES // G))


def _pairwise_forward(ranker) -> bool:
    """Does `ranker` have the reference's forward(user_ids, item_ids)?"""
    fwd = getattr(ranker, "forward", None)
    if not callable(fwd) or getattr(type(ranker), "forward", None) is nn.Module.forward:
        return False
    try:
        params = [p for p in inspect.signature(fwd).parameters.values()
                  if p.kind in (p.POSITIONAL_ONLY, p.POSITIONAL_OR_KEYWORD)]
    except (TypeError, ValueError):
        return False
    return len(params) >= 2 and params[1].name == "item_ids"


class Reranker(RecModule):
    answers_baskets = False
    takes_basket_weights = False

    def __init__(self, ranker, sources, depth: Optional[int] = None, top_k: int = 12):
        """`ranker`: a model with the reference's pairwise `forward(user_ids, item_ids)`.
        `sources`: an ordered `{name: model}` or a list of `(name, model)`, kept in an
        `nn.ModuleDict` (state_dict keys `sources.<name>.…`, the ranker's `ranker.…`); all of the
        ranker's `num_items`.  `depth`: how many candidates are asked of each source; the
        default, max(k, 4 * top_k) of the call's k clamped to num_items, 512 and
        2,048 / len(sources), is `Ensemble`'s design choice, not a measured optimum."""
        super().__init__()
        pairs = list(sources.items()) if hasattr(sources, "items") else [tuple(s) for s in sources]
        names = [str(n) for n, _ in pairs]
        if not pairs:
            raise ValueError("a Reranker needs at least one source")
        if len(pairs) > MAX_SOURCES:
            raise ValueError(f"a Reranker takes at most {MAX_SOURCES} sources")
        if len(set(names)) != len(names):
            raise ValueError(f"source names must be distinct, got {names}")
        if not _pairwise_forward(ranker):
            raise ValueError("the ranker must score pairs: forward(user_ids, item_ids)")
        sizes = {int(m.num_items) for _, m in pairs} | {int(ranker.num_items)}
        if len(sizes) != 1:
            raise ValueError(f"sources and ranker disagree on num_items: {sorted(sizes)}")
        if depth is not None:
            depth = int(depth)
            if depth < 1:
                raise ValueError("depth must be >= 1")
            if depth > MAX_DEPTH or depth * len(pairs) > MAX_ENTRIES:
                raise ValueError(f"depth must be <= {MAX_DEPTH} and depth * sources <= "
                                 f"{MAX_ENTRIES}")
        self.ranker = ranker
        self.sources = nn.ModuleDict()
        for name, m in pairs:
            try:
                self.sources[name] = m
            except (KeyError, TypeError) as e:
                raise ValueError(f'"{name}" cannot name a source: {e}') from None
        self.hparams = {"ranker": type(ranker).__name__, "sources": names, "depth": depth,
                        "top_k": int(top_k)}
        self.num_items = sizes.pop()
        self.num_users = getattr(ranker, "num_users", None)
        self.depth, self.top_k = depth, int(top_k)
        self.back_fill_short_rows = any(m.back_fill_short_rows for _, m in pairs)
        self.metrics = RecommendationMetrics(top_k=self.top_k)

    # ------------------------------------------------------------------ parts
    def _models(self):
        return list(self.sources.values())

    @property
    def device(self) -> torch.device:
        return self.ranker.device

    @property
    def history(self):
        """The first source history that is not None (a source's own, fitted or set)."""
        for m in self._models():
            h = getattr(m, "history", None)
            if h is not None:
                return h
        return None

    def set_history(self, history):
        """Forward `history` to the sources that keep a history and have none."""
        for m in self._models():
            if hasattr(m, "set_history") and getattr(m, "history", None) is None:
                m.set_history(history)
        return self

    def _depth(self, k: int) -> int:
        return clamp_depth(self.depth, k, self.top_k, self.num_items, len(self.sources))

    def _clamp_k(self, k: Optional[int]) -> int:
        k = self.top_k if k is None else int(k)
        if min(k, self.num_items) > MAX_K:
            raise ValueError(f"a Reranker answers at most k = {MAX_K} items per row, got {k}")
        return k

    def scoring_route(self, k: Optional[int] = None) -> str:
        """The route a call with this k (default top_k) takes through the ranker."""
        kk = min(self._clamp_k(k), self.num_items)
        if isinstance(self.ranker, WideDeep):
            return ROUTE_WIDEDEEP if kk <= FUSED_K else ROUTE_WIDEDEEP_WIDE
        return ROUTE_PAIRS

    # ------------------------------------------------------------------ stage 1
    def candidates(self, user_ids, filter_items=None, depth: Optional[int] = None):
        """(cand int32 [B, G * depth], n int32 [B]): every user's distinct source items,
        ascending, -1 past the n-th (`hnm_cand_union_i32`)."""
        ids = user_ids if isinstance(user_ids, torch.Tensor) else torch.as_tensor(user_ids)
        ids = ids.reshape(-1)
        depth = self._depth(min(self.top_k, self.num_items)) if depth is None else int(depth)
        u, _ = self._ids(ids, self.num_users)
        return self._union(ids, filter_items, depth, u.numel(), u.device)

    def _union(self, ids, filter_items, depth: int, B: int, dev):
        # the sources get the caller's ids: host ids stay host ids (checked on the host, no
        # sync), device ids are checked by each source's own kernels
        lists = [m.recommend_with_scores(ids, filter_items=filter_items, k=depth)
                 for m in self._models()]
        G = len(lists)
        lv = torch.empty(G, B, depth, dtype=torch.float32, device=dev)
        li = torch.empty(G, B, depth, dtype=torch.int64, device=dev)
        for g, (v, i) in enumerate(lists):
            if tuple(v.shape) != (B, depth) or tuple(i.shape) != (B, depth):
                raise RuntimeError(f"source {list(self.sources)[g]} returned lists of shape "
                                   f"{tuple(i.shape)}, expected {(B, depth)}")
            lv[g].copy_(v)
            li[g].copy_(i)
        W = G * depth
        cand = torch.empty(B, W, dtype=torch.int32, device=dev)
        n = torch.empty(B, dtype=torch.int32, device=dev)
        _lib.call("hnm_cand_union_i32", _lib.ctx(dev), _lib.ptr(lv), _lib.ptr(li), B, G,
                  B * depth, depth, depth, self.num_items, _lib.ptr(cand), W, _lib.ptr(n))
        return cand, n

    # ------------------------------------------------------------------ stage 2
    def _select(self, scores, cand, n, k: int):
        B, W = cand.shape
        out_v, out_i = empty_rows(B, k, cand.device)
        _lib.call("hnm_cand_topk_f32", _lib.ctx(cand.device), _lib.ptr(scores), _lib.ptr(cand), W,
                  _lib.ptr(n), B, k, _lib.ptr(out_v), _lib.ptr(out_i))
        return out_v, out_i

    def _rank_widedeep(self, u, host_ids: bool, user_features, cand, n, k: int):
        m = self.ranker
        w, keep = m._weights()
        f = m._features(user_features, u)
        itf, tab, ldf = m._item_table(None, u.device, keep)
        B, W = cand.shape
        fused = k <= FUSED_K
        out_v, out_i = empty_rows(B, k, u.device) if fused else (None, None)
        scores = None if fused else torch.empty(B, W, dtype=torch.float32, device=u.device)
        _lib.call("hnm_widedeep_cand_topk_ex_f32", _lib.ctx(u.device), w, _lib.ptr(u), B,
                  _lib.ptr(f), _lib.ptr(cand), W, _lib.ptr(n), k if fused else 0,
                  _lib.ptr(out_v), _lib.ptr(out_i), _lib.ptr(scores),
                  None if itf is None else C.byref(itf), _lib.ptr(tab), ldf)
        m._check(u.device, host_ids)
        return (out_v, out_i) if fused else self._select(scores, cand, n, k)

    def _rank_pairs(self, u, cand, n, k: int):
        B, W = cand.shape
        items = cand.clamp(min=0).to(torch.int64).reshape(-1)   # padding: item 0, cut by n
        scores = self.ranker(u.repeat_interleave(W), items)
        scores = scores.reshape(B, W).to(torch.float32).contiguous()
        return self._select(scores, cand, n, k)

    def recommend_with_scores(self, user_ids, filter_items=None, k: Optional[int] = None,
                              user_features=None):
        """(scores [B, k] f32, items [B, k] int64): the sources' candidates
        (`recommend_with_scores(user_ids, filter_items, k=depth)` each), merged per user, scored
        by the ranker, best k by (ranker score descending, item ascending); rows with fewer than
        k candidates end in (-inf, -1).  `user_features`: a WideDeep ranker's batch features
        (default: its registered table).  k is clamped to num_items; k > 128 raises ValueError
        before any launch."""
        k = self._clamp_k(k)
        ids = user_ids if isinstance(user_ids, torch.Tensor) else torch.as_tensor(user_ids)
        ids = ids.reshape(-1)
        u, host_ids = self._ids(ids, self.num_users)  # host ids: range-checked before any launch
        kk = min(k, self.num_items)
        if kk <= 0:
            return empty_topk(k, u)
        if u.numel() == 0:
            return empty_rows(0, kk, u.device)
        cand, n = self._union(ids, filter_items, self._depth(kk), u.numel(), u.device)
        if isinstance(self.ranker, WideDeep):
            return self._rank_widedeep(u, host_ids, user_features, cand, n, kk)
        return self._rank_pairs(u, cand, n, kk)

    def recommend(self, user_ids, filter_items=None) -> torch.Tensor:
        """[B, top_k] int64 item ids (-1 past the last candidate)."""
        self._check_top_k()
        with torch.no_grad():
            return self.recommend_with_scores(user_ids, filter_items=filter_items,
                                              k=self.top_k)[1]

    def forward(self, user_ids, filter_items=None) -> torch.Tensor:
        return self.recommend(user_ids, filter_items=filter_items)

    def predict_all_items(self, user_ids):
        raise NotImplementedError(
            "a Reranker scores its sources' candidates only: an item outside every source's list "
            "is never shown to the ranker, so there is no dense [B, num_items] row to return "
            "(ask the ranker itself)")

    def recommend_for_items(self, baskets, filter_seen: bool = True, k: Optional[int] = None):
        raise NotImplementedError(
            "a Reranker cannot answer from a basket of items: a neural ranker has no row for a "
            "visitor without a user index")
