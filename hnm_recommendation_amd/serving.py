"""Serving core: checkpoint ingestion and batched recommendation requests.

Mirrors the model-facing half of the reference's `scripts/serve.py` `ModelServer`
 without the HTTP layer, the pandas data module and the
article-metadata tables (out of scope: SURVEY §2):

* `create_model_from_checkpoint` -- `ModelServer._create_model_from_checkpoint`
  (`serve.py:216-258`): class chosen by a substring of the checkpoint's directory name,
  `hyper_parameters` with num_users / num_items overridden, `load_state_dict`,
  `.to(device).eval()`, LightGCN gets `set_graph`; any failure -> None (logged).
* `load_checkpoints` -- `ModelServer._load_models` (`serve.py:170-209`): every
  `**/*.ckpt` under a directory, model name = parent directory name.  Files are read with
  `torch.load(..., weights_only=True)` (tensors and plain containers only; the reference's
  full unpickling load is not reproduced).
* `Recommender.get_recommendations` / `get_batch_recommendations` -- `serve.py:305-413`.
  The reference scores one user at a time: dense `predict_all_items` [1, I], `-inf` on the
  purchase history (`:350-352`), `torch.topk(num_items)` (`:355`).  Here a batch of users is
  ONE fused call (`recommend_with_scores`: scoring + in-kernel history mask + top-k on the
  GPU); per-user errors (unknown user) become `{"user_id", "error"}` entries as in the
  reference loop (`:396-411`).
* `Recommender.add_popularity_baseline` -- `_load_popularity_baseline` (`serve.py:260-280`):
  the fitted `PopularityBaseline` under "popularity_baseline", the model `"best"` falls back
  to when no checkpoint carries a `test_map` (`:415-430`).
* `Recommender.add_item_cf` / `get_recommendations_for_items` -- no reference counterpart: the
  fitted `ItemCF` under "item_cf", and the answer for a visitor without a user index (a basket
  of item ids).  ItemCF rows that run out of co-bought items are back-filled from the
  popularity baseline when one is registered.
* `Recommender.add_als` -- no reference counterpart: an `ImplicitALS` fitted on the transactions
  under "implicit_als"; it answers users like every embedding model and baskets by fold-in
  (`get_recommendations_for_items(model_name="implicit_als")`; its rows are full: no back-fill).
* `Recommender.add_ensemble` -- no reference counterpart: an `Ensemble` of registered models
  under "ensemble" (reciprocal rank fusion, weighted scores or cascade of their top-K lists, fused
  on the GPU); it answers through the same request paths as its members.
* `Recommender.add_reranker` -- no reference counterpart (its analysis script names the
  architecture): a `Reranker` of registered models under "reranker": the sources' candidates
  merged per user and re-scored by a registered neural ranker, through the same request paths.
* `Recommender.add_content_knn` -- no reference counterpart: a `ContentKNN` fitted on the
  catalogue's attribute table under "content_knn": ItemCF's table and answers (users, baskets,
  back-fill, ensemble member) for articles that have no purchases yet.
* `Recommender.add_segment_popularity` -- no reference counterpart (its analysis script names the
  strategy): a `SegmentPopularity` fitted on the transactions and the users' segments under
  "segment_popularity".  With `cold_start="segment"` an unknown user is answered by it from the
  request's `segment` (the popular list of that age / membership group, continued from the
  global list); known users reach it by name or through an ensemble.
* `Recommender.add_sequential_cf` -- no reference counterpart (its analysis script names the
  "temporal" member): a `SequentialCF` fitted on the transactions and their dates under
  "sequential_cf": ItemCF's table and answers (users, weighted baskets, back-fill, ensemble member,
  reranker source), with rows that hold what was bought AFTER an item.
"""
from __future__ import annotations

import glob
import logging
import os
from datetime import datetime
from typing import Dict, List, Optional, Sequence, Union

import torch

from .models import (ContentKNN, Ensemble, ImplicitALS, ItemCF, LightGCN, MatrixFactorization, NeuralCF,
                     PopularityBaseline, Reranker, SegmentPopularity, SequentialCF, WeightedItemCF,
                     WideDeep)
from .models.base import UserHistory

logger = logging.getLogger(__name__)

# serve.py:56: RecommendationRequest.num_items = Field(12, ge=1, le=100)
MAX_NUM_ITEMS = 100

BASELINE = "popularity_baseline"  # serve.py:273: the name the reference registers it under
ITEM_CF = "item_cf"
ALS = "implicit_als"
CONTENT_KNN = "content_knn"
ENSEMBLE = "ensemble"
RERANKER = "reranker"
SEGMENT_POP = "segment_popularity"
SEQ_CF = "sequential_cf"

# serve.py:238-248, tested in this order
_DISPATCH = (("matrix_factorization", MatrixFactorization), ("neural_cf", NeuralCF),
             ("wide_deep", WideDeep), ("lightgcn", LightGCN), (ITEM_CF, ItemCF),
             (ALS, ImplicitALS), (CONTENT_KNN, ContentKNN), (SEQ_CF, SequentialCF))


def load_checkpoint(path: str, device="cpu") -> Dict:
    """A Lightning `.ckpt` dict ({'state_dict', 'hyper_parameters', ...}); safe loader."""
    return torch.load(path, map_location=device, weights_only=True)


def create_model_from_checkpoint(model_name: str, checkpoint: Dict, num_users: int,
                                 num_items: int, device="cuda", graph=None):
    """`_create_model_from_checkpoint` (`serve.py:216-258`).  `graph` = (edge_index,
    edge_weight) for LightGCN (the data module's `get_graph()`, `:246`).  Returns the module
    in eval mode on `device`, or None when the name matches no model or anything fails."""
    try:
        state_dict = checkpoint["state_dict"]
        hparams = dict(checkpoint.get("hyper_parameters", {}))
        hparams["num_users"] = num_users
        hparams["num_items"] = num_items
        cls = next((c for key, c in _DISPATCH if key in model_name), None)
        if cls is None:
            return None
        if cls is ItemCF and hparams.pop("weighted", False):   # the hyperparameter names the class
            cls = WeightedItemCF
        model = cls(**hparams)
        if cls is LightGCN:
            if graph is None:
                raise ValueError("LightGCN checkpoint needs the interaction graph")
            edge_index, edge_weight = graph
            model.set_graph(edge_index, edge_weight)
        model.load_state_dict(state_dict)
        model.to(device)
        model.eval()
        return model
    except Exception as e:  # serve.py:255-257: log and skip the model
        logger.error("creating model from checkpoint failed: %s", e)
        return None


class Recommender:
    """The request-facing part of `ModelServer` (`serve.py:116-413`).

    models: {name: module}; model_metrics: {name: {'test_map': ...}} (what the checkpoint's
    'metrics' entry holds, `serve.py:203`); user_history: {user_idx: set(item_idx)} (the
    purchase history, `:166-168`); customer_index: optional {customer_id str: user_idx}
    (the encoder lookup, `:294-300`); article_ids: optional sequence item_idx -> article id.
    cold_start: what an unknown user gets -- "error" (the reference: ValueError / an error
    entry), "popularity" (opt-in: the unfiltered popular list of the registered
    "popularity_baseline", under that model name) or "segment" (opt-in: the unfiltered list of
    the registered "segment_popularity" for the request's `segment`, under that model name; a
    request without a segment gets that model's global list).
    """

    def __init__(self, num_users: int, num_items: int, models: Optional[Dict] = None,
                 model_metrics: Optional[Dict[str, Dict[str, float]]] = None,
                 user_history: Optional[Dict[int, set]] = None,
                 customer_index: Optional[Dict[str, int]] = None,
                 article_ids: Optional[Sequence] = None, device="cuda",
                 cold_start: str = "error"):
        if cold_start not in ("error", "popularity", "segment"):
            raise ValueError('cold_start must be "error", "popularity" or "segment"')
        self.cold_start = cold_start
        self.num_users = num_users
        self.num_items = num_items
        self.device = torch.device(device)
        self.models: Dict[str, torch.nn.Module] = {}
        self.model_metrics: Dict[str, Dict[str, float]] = {}
        self.user_history = user_history or {}
        self._history_dev: Optional[UserHistory] = None
        self.customer_index = customer_index
        self.article_ids = article_ids
        for name, m in (models or {}).items():
            self.add_model(name, m, (model_metrics or {}).get(name))

    def add_model(self, name: str, model, metrics: Optional[Dict[str, float]] = None):
        self.models[name] = model.to(self.device).eval()
        if isinstance(model, NeuralCF) and model._fused():
            model.cache_item_tables()  # a server's weights are fixed: keep the item projection
        self.model_metrics[name] = dict(metrics or {})

    def add_popularity_baseline(self, item_ids, days_ago=None, time_decay: float = 0.0,
                                window_days: Optional[int] = None) -> PopularityBaseline:
        """`_load_popularity_baseline` (`serve.py:260-280`): fit a PopularityBaseline on the
        transactions' item ids (optionally time-decayed / windowed by `days_ago`) and register
        it as "popularity_baseline".  Non-personalized: `filter_purchased` supplies the
        history, as for every other model."""
        model = PopularityBaseline(n_items=self.num_items, k=min(MAX_NUM_ITEMS, self.num_items),
                                   time_decay=time_decay).to(self.device)
        model.fit_interactions(item_ids, days_ago=days_ago, window_days=window_days)
        self.add_model(BASELINE, model)
        return model

    def add_segment_popularity(self, item_ids, user_ids, user_segments, n_segments: int,
                               days_ago=None, time_decay: float = 0.0,
                               window_days: Optional[int] = None,
                               min_count: int = 1) -> SegmentPopularity:
        """Fit a `SegmentPopularity` on the transactions and `user_segments[user]` (in
        [0, n_segments), negative = unknown; e.g. `age_segments` of the customers table) and
        register it as "segment_popularity": the answer `cold_start="segment"` gives an unknown
        user, and a recall source for known users (by name, or as an `add_ensemble` member)."""
        model = SegmentPopularity(self.num_items, n_segments,
                                  k=min(MAX_NUM_ITEMS, self.num_items), time_decay=time_decay,
                                  min_count=min_count).to(self.device)
        model.fit_interactions(item_ids, user_ids, user_segments, days_ago=days_ago,
                               window_days=window_days)
        self.add_model(SEGMENT_POP, model)
        return model

    def add_item_cf(self, user_ids, item_ids, weights=None, days_ago=None,
                    time_decay: float = 0.0, **kw) -> ItemCF:
        """Fit an `ItemCF` (keywords: num_neighbors, shrink, max_history, top_k) on the
        transactions' (user, item) pairs and register it as "item_cf".  With `weights`,
        `days_ago` or a `time_decay` > 0 it is a `WeightedItemCF` fitted on per-transaction
        weights by `add_als`' rules (quantities, a recency decay); with none of them the plain
        model and its bits.  Its history becomes the recommender's device history when the
        recommender has none."""
        if weights is not None or days_ago is not None or float(time_decay) != 0.0:
            return self._add_fitted(ITEM_CF, WeightedItemCF(self.num_users, self.num_items, **kw),
                                    user_ids, item_ids, weights=weights, days_ago=days_ago,
                                    time_decay=time_decay)
        return self._add_fitted(ITEM_CF, ItemCF(self.num_users, self.num_items, **kw),
                                user_ids, item_ids)

    def _add_fitted(self, name: str, model, user_ids, item_ids, **fit_kw):
        """Fit `model` on the transactions, register it under `name` and adopt its history as
        the recommender's device history when the recommender has none."""
        model = model.to(self.device)
        model.fit_interactions(user_ids, item_ids, **fit_kw)
        self.add_model(name, model)
        if not self.user_history and self._history_dev is None:
            self._history_dev = model.history
        return model

    def add_content_knn(self, item_attributes, column_weights=None, weighting: str = "idf",
                        **kw) -> ContentKNN:
        """Fit a `ContentKNN` (keywords: num_neighbors, top_k) on the catalogue's attribute table
        ([num_items, F] integer codes, negative = missing; `column_weights`, `weighting`: see
        `ContentKNN.fit_attributes`) and register it as "content_knn".  It reads users' rows from
        the recommender's device history when there is one; without one it still answers baskets
        (`get_recommendations_for_items(model_name="content_knn")`), and a user request raises."""
        model = ContentKNN(self.num_users, self.num_items, weighting=weighting, **kw)
        model = model.to(self.device)
        model.fit_attributes(item_attributes, column_weights=column_weights)
        hist = self._device_history()
        if hist is not None:
            model.set_history(hist)
        self.add_model(CONTENT_KNN, model)
        return model

    def add_sequential_cf(self, user_ids, item_ids, days_ago, weights=None,
                          recency_decay: float = 0.0, **kw) -> SequentialCF:
        """Fit a `SequentialCF` (keywords: num_neighbors, shrink, max_history, max_gap, gap_decay,
        repeat_buys, top_k) on the transactions' (user, item, days_ago) triples and register it as
        "sequential_cf".  `weights` / `recency_decay` shape the history a user is answered from,
        as in `SequentialCF.fit_interactions`.  Its history becomes the recommender's device
        history when the recommender has none."""
        return self._add_fitted(SEQ_CF, SequentialCF(self.num_users, self.num_items, **kw),
                                user_ids, item_ids, days_ago=days_ago, weights=weights,
                                recency_decay=recency_decay)

    def add_als(self, user_ids, item_ids, weights=None, days_ago=None, time_decay: float = 0.0,
                solver: str = "cholesky", cg_steps: int = 3, **kw) -> ImplicitALS:
        """Fit an `ImplicitALS` (keywords: embedding_dim, regularization, alpha, iterations,
        seed, top_k) on the transactions' (user, item) pairs and register it as "implicit_als".
        `weights` / `days_ago` / `time_decay`: per-transaction confidence weights, as in
        `ImplicitALS.fit_interactions` (quantities, a recency decay).  `solver` / `cg_steps` go
        to the fit, not to the model: `solver="cg"` fits by conjugate-gradient half-steps.
        Its history becomes the recommender's device history when the recommender has none."""
        return self._add_fitted(ALS, ImplicitALS(self.num_users, self.num_items, **kw), user_ids,
                                item_ids, weights=weights, days_ago=days_ago,
                                time_decay=time_decay, solver=solver, cg_steps=cg_steps)

    def add_ensemble(self, member_names, weights=None, mode: str = "rrf",
                     name: str = ENSEMBLE, **kw) -> Ensemble:
        """Build an `Ensemble` (keywords: rank_constant, depth, top_k) from registered models,
        in `member_names`' order, and register it under `name`; ValueError for a name that is
        not registered.  It carries no metrics, so `"best"` resolves as before.  Requests go
        through the existing paths: rows that run out of fused items are back-filled from the
        popularity baseline when a member's are (`back_fill_short_rows`), and a basket is
        answered when every member answers baskets."""
        names = list(member_names)
        unknown = [n for n in names if n not in self.models]
        if unknown:
            raise ValueError(f"models {unknown} are not available")
        model = Ensemble([(n, self.models[n]) for n in names], weights=weights, mode=mode, **kw)
        self.add_model(name, model)
        return model

    def add_reranker(self, ranker_name: str, source_names, name: str = RERANKER,
                     **kw) -> Reranker:
        """Build a `Reranker` (keywords: depth, top_k) from registered models -- the ranker
        `ranker_name` over the candidates of `source_names`, in that order -- and register it
        under `name`; ValueError for a name that is not registered.  It carries no metrics, so
        `"best"` resolves as before.  Requests go through the existing paths: the history filter
        reaches the sources, and rows that run out of candidates are back-filled from the
        popularity baseline when a source's are (`back_fill_short_rows`).  It answers users
        only: a basket request names it a model that cannot answer from items."""
        names = list(source_names)
        unknown = [n for n in [ranker_name, *names] if n not in self.models]
        if unknown:
            raise ValueError(f"models {unknown} are not available")
        model = Reranker(self.models[ranker_name], [(n, self.models[n]) for n in names], **kw)
        self.add_model(name, model)
        return model

    def load_checkpoints(self, checkpoint_dir: str, graph=None) -> List[str]:
        """`_load_models` (`serve.py:170-209`): every `**/*.ckpt`, name = parent dir."""
        loaded = []
        for path in sorted(glob.glob(os.path.join(checkpoint_dir, "**", "*.ckpt"),
                                     recursive=True)):
            name = os.path.basename(os.path.dirname(path))
            try:
                ckpt = load_checkpoint(path)
            except Exception as e:
                logger.error("loading %s failed: %s", path, e)
                continue
            model = create_model_from_checkpoint(name, ckpt, self.num_users, self.num_items,
                                                 self.device, graph)
            if model is not None:
                self.models[name] = model
                self.model_metrics[name] = dict(ckpt.get("metrics", {}) or {})
                loaded.append(name)
        return loaded

    def set_user_history(self, user_history: Dict[int, set]):
        """Replace the purchase history (the device copy is rebuilt on the next request)."""
        self.user_history = user_history or {}
        self._history_dev = None

    def _device_history(self) -> Optional[UserHistory]:
        """The purchase history as a device-resident CSR (built once, on first use): each
        filtered batch gathers its rows on the GPU instead of building a mask on the host."""
        if self._history_dev is None and self.user_history:
            self._history_dev = UserHistory(self.user_history, self.num_users, self.num_items,
                                            self.device)
        return self._history_dev

    # ------------------------------------------------------------------ lookups
    def get_user_idx(self, user_id: Union[int, str]) -> Optional[int]:
        """`serve.py:282-303`: ints are indices (< num_users); strings go through the
        customer-id index."""
        if isinstance(user_id, bool):
            user_id = int(user_id)
        if isinstance(user_id, int):
            return user_id if user_id < self.num_users else None
        if self.customer_index is not None:
            return self.customer_index.get(user_id)
        return None

    def _get_best_model(self) -> str:
        """`serve.py:415-430`: highest 'test_map'; without any, the popularity baseline when
        one is registered (`:421`), else the first model."""
        best, best_score = None, 0
        for name, m in self.model_metrics.items():
            if "test_map" in m and m["test_map"] > best_score:
                best, best_score = name, m["test_map"]
        if best is None:
            if not self.models:
                raise ValueError("no model loaded")
            best = BASELINE if BASELINE in self.models else next(iter(self.models))
        return best

    def _cold_start_model(self):
        if BASELINE not in self.models:
            raise ValueError('cold_start="popularity" needs a registered "popularity_baseline" '
                             "(add_popularity_baseline)")
        return self.models[BASELINE]

    def _request_segments(self, segments, n: int):
        """The `segment` / `segments` keyword of a request with n entries: None unless
        cold_start="segment"; then one int per entry (None -> -1), checked on the host against
        the registered "segment_popularity" -- ValueError before any launch."""
        if self.cold_start != "segment":
            if segments is not None and any(s is not None for s in segments):
                raise ValueError('a request segment needs cold_start="segment"')
            return None
        if SEGMENT_POP not in self.models:
            raise ValueError('cold_start="segment" needs a registered "segment_popularity" '
                             "(add_segment_popularity)")
        segs = [None] * n if segments is None else list(segments)
        if len(segs) != n:
            raise ValueError("segments must have one entry per user id")
        S = self.models[SEGMENT_POP].num_segments
        out = []
        for s in segs:
            if s is not None and (isinstance(s, bool) or not isinstance(s, int)
                                  or not -1 <= s < S):
                raise ValueError(f"segment must be None or an integer in [-1, {S}), got {s!r}")
            out.append(-1 if s is None else s)
        return out

    def _score_segments(self, segs: List[int], num_items: int):
        """Unknown users: one `SegmentPopularity.recommend_for_segments` call for all of them,
        unfiltered (they have no history)."""
        self._check_num_items(num_items)
        with torch.no_grad():
            vals, items = self.models[SEGMENT_POP].recommend_for_segments(segs, k=num_items)
        vals, items = vals.cpu().tolist(), items.cpu().tolist()
        self._trim(vals, items)
        return vals, items

    def _resolve_model(self, model_name: str):
        if model_name == "best":
            model_name = self._get_best_model()
        if model_name not in self.models:
            raise ValueError(f"model {model_name} is not available")
        return model_name, self.models[model_name]

    def _item_info(self, item_idx: int, score: Optional[float]) -> Dict:
        """`ItemInfo` (`serve.py:80-88`) without the article metadata table."""
        aid = str(item_idx)
        if self.article_ids is not None and 0 <= item_idx < len(self.article_ids):
            aid = str(self.article_ids[item_idx])
        return {"article_id": aid, "product_name": None, "product_type_name": None,
                "product_group_name": None, "colour_group_name": None,
                "department_name": None, "score": score}

    # ------------------------------------------------------------------ requests
    def _check_num_items(self, num_items):
        # serve.py:56 RecommendationRequest: num_items = Field(12, ge=1, le=100)
        hi = min(MAX_NUM_ITEMS, self.num_items)
        if isinstance(num_items, bool) or not isinstance(num_items, int) or not 1 <= num_items <= hi:
            raise ValueError(f"num_items must be an integer in [1, {hi}]")

    def _back_fill(self, vals, items, fill):
        """ItemCF rows that end in -1 (fewer than k co-bought items): continue each with the
        popularity list `fill(rows)` gives for those rows (same k, same filter), skipping what
        the row already holds -- k entries always suffice.  Filled entries carry their
        popularity as the score.  On the host: lists of at most 100 entries."""
        short = [r for r, row in enumerate(items) if row and row[-1] < 0]
        if not short or BASELINE not in self.models:
            return
        pv, pi = fill(short)
        for r, fv, fi in zip(short, pv, pi):
            n = next(j for j, it in enumerate(items[r]) if it < 0)
            have = set(items[r][:n])
            for v, it in zip(fv, fi):
                if n == len(items[r]) or it < 0:
                    break
                if it not in have:
                    vals[r][n], items[r][n] = v, it
                    n += 1

    @staticmethod
    def _trim(vals, items):
        """Drop the (-inf, -1) tail of short rows: a response lists real items only."""
        for r, row in enumerate(items):
            n = next((j for j, it in enumerate(row) if it < 0), len(row))
            vals[r], items[r] = vals[r][:n], row[:n]

    def _score_batch(self, model, idx: List[int], num_items: int, filter_purchased: bool):
        self._check_num_items(num_items)
        # host ids: range-checked on the host by the model (no device-side check / sync),
        # then one fused scoring + history-mask + top-k call; the history mask is gathered
        # on the GPU from the device-resident history (serve.py:350-352)
        users = torch.tensor(idx, dtype=torch.int64)
        hist = self._device_history() if filter_purchased else None
        if model.back_fill_short_rows and model.history is None:  # built from a checkpoint
            model.set_history(self._device_history())
        with torch.no_grad():
            vals, items = model.recommend_with_scores(users, filter_items=hist, k=num_items)
        vals, items = vals.cpu().tolist(), items.cpu().tolist()
        if model.back_fill_short_rows:
            def fill(rows):
                with torch.no_grad():
                    pv, pi = self.models[BASELINE].recommend_with_scores(
                        users[rows], filter_items=hist, k=num_items)
                return pv.cpu().tolist(), pi.cpu().tolist()
            self._back_fill(vals, items, fill)
            self._trim(vals, items)
        return vals, items

    def get_recommendations_for_items(self, item_ids, num_items: int = 12,
                                      model_name: str = ITEM_CF,
                                      include_scores: bool = False, item_weights=None) -> Dict:
        """A visitor without a user index: recommendations from a basket of item indices (the
        basket's own items are not recommended back).  `item_weights`: one finite weight >= 0
        per entry of `item_ids` ("three of these", "just viewed"; a repeated item's weights are
        summed), for an ImplicitALS or a weighted ItemCF.  ValueError for an unknown model, a
        model that cannot answer from items, an item outside [0, num_items), or weights given to
        another model."""
        self._check_num_items(num_items)
        name, model = self._resolve_model(model_name)
        if not model.answers_baskets:
            raise ValueError(f"model {name} cannot answer from a basket of items")
        if item_weights is not None and not model.takes_basket_weights:
            raise ValueError(f"model {name} takes no item weights (only {ALS} and a weighted "
                             f"{ITEM_CF} do)")
        given = [int(i) for i in item_ids]
        basket = sorted(set(given))
        if basket and not 0 <= basket[0] <= basket[-1] < self.num_items:
            raise ValueError(f"item indices must be in [0, {self.num_items})")
        with torch.no_grad():
            if item_weights is not None:
                ws = [float(x) for x in item_weights]
                if len(ws) != len(given):
                    raise ValueError("item_weights must have one entry per item id")
                vals, items = model.recommend_for_items([given], filter_seen=True, k=num_items,
                                                        weights=[ws])
            else:
                vals, items = model.recommend_for_items([basket], filter_seen=True, k=num_items)
        vals, items = vals.cpu().tolist(), items.cpu().tolist()
        if not model.back_fill_short_rows:
            # every row is full: nothing to back-fill; a basket that leaves fewer than num_items
            # items ends in masked entries at -inf (the dot top-K's convention): not listed
            n = next((j for j, v in enumerate(vals[0]) if v == float("-inf")), len(vals[0]))
            return self._result(None, name, vals[0][:n], items[0][:n], include_scores)

        def fill(rows):
            with torch.no_grad():
                pv, pi = self.models[BASELINE].recommend_with_scores(
                    torch.zeros(1, dtype=torch.int64), filter_items={0: set(basket)}, k=num_items)
            return pv.cpu().tolist(), pi.cpu().tolist()
        self._back_fill(vals, items, fill)
        self._trim(vals, items)
        return self._result(None, name, vals[0], items[0], include_scores)

    def _result(self, user_id, model_name, vals, items, include_scores):
        recs = [self._item_info(int(i), float(v) if include_scores else None)
                for v, i in zip(vals, items)]
        return {"user_id": user_id, "recommendations": recs, "model_name": model_name,
                "generated_at": datetime.now().isoformat()}

    def get_recommendations(self, user_id: Union[int, str], model_name: str = "best",
                            num_items: int = 12, filter_purchased: bool = True,
                            include_scores: bool = False, segment: Optional[int] = None) -> Dict:
        """`serve.py:305-371` (ValueError for an unknown user or model; with
        cold_start="popularity" an unknown user gets the unfiltered popular list, with
        cold_start="segment" the list of the request's `segment` -- None or -1: the global one
        -- from "segment_popularity"; a known user's `segment` is not read)."""
        segs = self._request_segments(None if segment is None else [segment], 1)
        cold = self._cold_start_model() if self.cold_start == "popularity" else None
        uidx = self.get_user_idx(user_id)
        if uidx is None:
            if segs is not None:
                vals, items = self._score_segments(segs, num_items)
                return self._result(user_id, SEGMENT_POP, vals[0], items[0], include_scores)
            if cold is not None:
                vals, items = self._score_batch(cold, [0], num_items, False)
                return self._result(user_id, BASELINE, vals[0], items[0], include_scores)
            raise ValueError(f"user {user_id} not found")
        name, model = self._resolve_model(model_name)
        vals, items = self._score_batch(model, [uidx], num_items, filter_purchased)
        return self._result(user_id, name, vals[0], items[0], include_scores)

    def get_batch_recommendations(self, user_ids: List[Union[int, str]],
                                  model_name: str = "best", num_items: int = 12,
                                  filter_purchased: bool = True,
                                  include_scores: bool = False,
                                  segments: Optional[Sequence[Optional[int]]] = None
                                  ) -> List[Dict]:
        """`serve.py:373-413`, batched: one fused scoring + mask + top-k call for all
        known users; unknown users get {'user_id', 'error'} in their slot -- or, with
        cold_start="popularity", the unfiltered popular list (one more call for all of them),
        or, with cold_start="segment", the list of their entry of `segments` (one per user id,
        None or -1: the global list) from "segment_popularity": one more call for all of them,
        whatever their segments."""
        segs = self._request_segments(segments, len(user_ids))
        cold = self._cold_start_model() if self.cold_start == "popularity" else None
        name, model = self._resolve_model(model_name)
        idx, slots, results, cold_slots = [], [], [], []
        for j, uid in enumerate(user_ids):
            u = self.get_user_idx(uid)
            if u is None and (cold is not None or segs is not None):
                results.append(None)
                cold_slots.append(j)
            elif u is None:
                results.append({"user_id": uid, "error": f"user {uid} not found"})
            elif u < 0:  # the reference's embedding lookup raises; its loop records it
                results.append({"user_id": uid, "error": "index out of range in self"})
            else:
                results.append(None)
                idx.append(u)
                slots.append(j)
        if idx:
            vals, items = self._score_batch(model, idx, num_items, filter_purchased)
            for r, j in enumerate(slots):
                results[j] = self._result(user_ids[j], name, vals[r], items[r], include_scores)
        if cold_slots and segs is not None:
            vals, items = self._score_segments([segs[j] for j in cold_slots], num_items)
            for r, j in enumerate(cold_slots):
                results[j] = self._result(user_ids[j], SEGMENT_POP, vals[r], items[r],
                                          include_scores)
        elif cold_slots:  # the same list for every unknown user: user ids play no part unfiltered
            vals, items = self._score_batch(cold, [0], num_items, False)
            for j in cold_slots:
                results[j] = self._result(user_ids[j], BASELINE, vals[0], items[0], include_scores)
        return results
