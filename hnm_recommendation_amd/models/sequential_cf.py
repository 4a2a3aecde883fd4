"""SequentialCF: "customers who bought A bought B in the following weeks" -- the directed,
time-ordered recall source (no reference module: the design note at the end of
`scripts/analyze_recommendation_challenges.py` names "Temporal" beside the short-term, long-term
and content members of its ensemble, lists "repeat buys" among the interaction features and puts
"Priority 4: Temporal/sequential models" after the neural ones; `src/models` never built it).

`ItemCF` and `WeightedItemCF` count "bought both", which is symmetric: a winter coat and gloves
point at each other.  Here row a of the table holds what was bought in the `max_gap` days AFTER
a, so the coat leads to the gloves and the gloves do not lead back.  One HIP entry
(`hnm_seqcf_fit_f32`, `csrc/seqcf.hip`, contract in `include/hnm.h`) counts the ordered pairs over
a `UserSequence` -- a pair `g` days apart weighs `exp(-gap_decay * (g - 1))` in fixed point, same-day
pairs are co-occurrence and do not count -- and keeps each item's `num_neighbors` best successors
in `ItemCF`'s table: the buffers, state_dict keys and every answering method are `ItemCF`'s,
served by the same kernels.  The fit is a counting pass in integers: no optimiser, no sampling,
the same bits on every run, bitwise a numpy restatement (tests/seqcf_oracle.py).

A user's row is served like a `WeightedItemCF`'s, score(u, i) = sum_j w_uj * sim(j -> i), from a
`UserHistory` with weights: the purchase count of (u, j), optionally decayed by recency.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib
from .base import UserHistory, interactions_history
from .item_cf import ItemCF
from .sequence import UserSequence

MAX_HISTORY = 65535      # hnm_seqcf_fit_f32: the ceiling that keeps the uint64 counters exact
MAX_GAP = 1024
GAP_ONE = 1 << 15        # the fixed point of the gap table


def gap_table(max_gap: int, gap_decay: float = 0.0) -> np.ndarray:
    """uint32 [max_gap]: entry g (a pair g + 1 days apart) = rint(32768 * exp(-gap_decay * g)) in
    float64 on the host; what `hnm_seqcf_fit_f32` takes as `gap_q`.  ValueError unless max_gap is
    an integer in [1, 1024] and gap_decay finite and >= 0."""
    if isinstance(max_gap, bool) or int(max_gap) != max_gap or not 1 <= int(max_gap) <= MAX_GAP:
        raise ValueError(f"max_gap must be an integer in [1, {MAX_GAP}]")
    gap_decay = float(gap_decay)
    if not gap_decay >= 0.0 or not np.isfinite(gap_decay):
        raise ValueError("gap_decay must be finite and >= 0")
    g = np.arange(int(max_gap), dtype=np.float64)
    return np.rint(float(GAP_ONE) * np.exp(-gap_decay * g)).astype(np.uint32)


class SequentialCF(ItemCF):
    """`ItemCF`'s table and answers, fitted on the order of purchases (`fit_sequence`,
    `fit_interactions`).  `max_history` = 0: the entry's ceiling, 65,535 events a user."""
    weighted = takes_basket_weights = True

    def __init__(self, num_users: int, num_items: int, num_neighbors: int = 64,
                 shrink: float = 0.0, max_history: int = 0, max_gap: int = 28,
                 gap_decay: float = 0.0, repeat_buys: bool = False, top_k: int = 12):
        if not 0 <= int(max_history) <= MAX_HISTORY:
            raise ValueError(f"max_history must be in [0, {MAX_HISTORY}] (0 = {MAX_HISTORY})")
        gap_table(max_gap, gap_decay)                  # validates both
        super().__init__(num_users, num_items, num_neighbors=num_neighbors, shrink=shrink,
                         max_history=max_history, top_k=top_k)
        self.max_gap, self.gap_decay = int(max_gap), float(gap_decay)
        self.repeat_buys = bool(repeat_buys)
        self.hparams = {"num_users": num_users, "num_items": num_items,
                        "num_neighbors": num_neighbors, "shrink": shrink,
                        "max_history": max_history, "max_gap": max_gap, "gap_decay": gap_decay,
                        "repeat_buys": repeat_buys, "top_k": top_k}

    def _fitted(self):
        if self._is_fitted is None:
            self._is_fitted = bool((self.item_count > 0).any())
        if not self._is_fitted:
            raise RuntimeError("not fitted: call fit_interactions / fit_sequence, or load a "
                               "fitted state_dict")

    def fit_sequence(self, sequence: UserSequence, history: UserHistory, *, _window: int = 0):
        """Fit on a `UserSequence` -- one `hnm_seqcf_fit_f32` call (`_window`: item columns per
        LDS pass, for tests) -- and keep `history`, a `UserHistory` with `hist_w`, as the model's
        history (ValueError without weights): the rows users are answered from."""
        if not isinstance(sequence, UserSequence):
            raise TypeError("sequence must be a UserSequence")
        if isinstance(history, UserHistory) and history.hist_w is None:
            raise ValueError("a SequentialCF serves a history with weights "
                             "(UserHistory.from_interactions(..., weights=))")
        if sequence.num_users != self.num_users or sequence.num_items != self.num_items:
            raise ValueError(f"sequence built for {sequence.num_users} users x "
                             f"{sequence.num_items} items, model has {self.num_users} x "
                             f"{self.num_items}")
        _lib.require_gpu(self.neighbor_idx)
        self.set_history(history)._need_history()
        dev = self.device
        if sequence.device != dev:
            raise ValueError(f"sequence lives on {sequence.device}, the model on {dev}")
        for name, dtype in (("neighbor_idx", torch.int32), ("neighbor_val", torch.float32),
                            ("item_count", torch.int64)):
            t = getattr(self, name)
            if t.dtype != dtype or not t.is_contiguous():
                setattr(self, name, t.to(dtype).contiguous())
        # uint32 travels as its int32 bit pattern
        q = torch.from_numpy(gap_table(self.max_gap, self.gap_decay).view(np.int32)).to(dev)
        _lib.call("hnm_seqcf_fit_f32", _lib.ctx(dev), _lib.ptr(sequence.seq_ptr),
                  _lib.ptr(sequence.seq_item), _lib.ptr(sequence.seq_day), self.num_users,
                  self.num_items, self.num_neighbors, self.shrink,
                  self.max_history or MAX_HISTORY, self.max_gap, _lib.ptr(q),
                  int(self.repeat_buys), int(_window), _lib.ptr(self.neighbor_idx),
                  _lib.ptr(self.neighbor_val), _lib.ptr(self.item_count))
        _lib.sync_check(dev)
        self._is_fitted = True
        return self

    def fit_interactions(self, user_ids, item_ids, days_ago, *, weights=None,
                         recency_decay: float = 0.0, _window: int = 0):
        """Fit from (user, item, days_ago) transaction arrays or tensors (`UserSequence.
        from_interactions`' rules).  The served history is `interactions_history(..., weights,
        days_ago, recency_decay, unit_weights=True)`: a user's item weighs the sum over its
        transactions of weights * exp(-recency_decay * days_ago) -- with no decay and no weights,
        the purchase count.  `recency_decay` shapes what a user is answered from; the table's own
        decay over the gap between two purchases is the hyperparameter `gap_decay`."""
        seq = UserSequence.from_interactions(user_ids, item_ids, days_ago, self.num_users,
                                             self.num_items, self.device)
        hist = interactions_history(user_ids, item_ids, self.num_users, self.num_items,
                                    self.device, weights, days_ago, recency_decay,
                                    unit_weights=True)
        return self.fit_sequence(seq, hist, _window=_window)

    def fit_history(self, *args, **kwargs):
        raise TypeError("a SequentialCF is fitted on the order of purchases: call "
                        "fit_interactions(user_ids, item_ids, days_ago) or "
                        "fit_sequence(UserSequence, UserHistory)")
