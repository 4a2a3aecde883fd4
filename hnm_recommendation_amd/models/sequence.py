"""The time-ordered side of the fitted models: `UserSequence`, a device-resident CSR of every
user's purchase events oldest first.  `UserHistory` (models/history.py) drops the dates; a
`SequentialCF` is fitted on this layout instead and still serves from a `UserHistory`.
`models/base.py` re-exports the public name.
"""
from __future__ import annotations

import numpy as np
import torch

from .history import _host, interaction_weights

MAX_DAYS = 32768     # days_ago < 2^15: a day difference indexes hnm_seqcf_fit_f32's gap table


class UserSequence:
    """Per-user purchase events in time order (CSR over user ids), built ONCE on the host.

    An event is a distinct (user, day, item): repeated transactions of one triple count once.
    A user's events are sorted by (`days_ago` descending, item ascending), so the oldest comes
    first.  `seq_ptr` int64 [num_users + 1]; `seq_item` int32; `seq_day` int32 =
    `max_days_ago - days_ago` (a later event has a larger day; `max_days_ago` is the largest
    value given); `nnz` events in all, `max_len` the longest row.  `seq_item` / `seq_day` hold
    one padding element when nothing is stored."""

    @classmethod
    def from_interactions(cls, user_ids, item_ids, days_ago, num_users: int, num_items: int,
                          device):
        """From (user, item, days_ago) transaction arrays or tensors.  `days_ago`: whole days >= 0
        and < 32768 by `interaction_weights`' rule for days (fractional, negative and non-finite
        values raise ValueError); ids out of range raise IndexError.  One lexicographic
        `np.unique` over (user, day, item): a permutation of the transactions gives the same
        arrays."""
        u = _host(user_ids).reshape(-1).astype(np.int64)
        i = _host(item_ids).reshape(-1).astype(np.int64)
        if u.shape != i.shape:
            raise ValueError("user_ids and item_ids must have the same shape")
        if days_ago is None:
            raise ValueError("days_ago must have one entry per interaction")
        interaction_weights(u.shape[0], None, days_ago, 0.0)      # the rule for days
        d = _host(days_ago).reshape(-1)
        if d.size and d.max() >= MAX_DAYS:
            raise ValueError(f"days_ago must be < {MAX_DAYS}")
        d = d.astype(np.int64)
        num_users, num_items = int(num_users), int(num_items)
        if u.size and (u.min() < 0 or u.max() >= num_users or i.min() < 0 or i.max() >= num_items):
            raise IndexError("interaction ids out of range")
        max_days_ago = int(d.max()) if d.size else 0
        span = max_days_ago + 1
        if num_users * span * max(num_items, 1) >= 2 ** 63:
            raise ValueError("num_users * days * num_items exceeds the int64 key of the sort")
        key = np.unique((u * span + (max_days_ago - d)) * num_items + i)   # (user, day, item)
        rest, items = np.divmod(key, max(num_items, 1))
        r, day = np.divmod(rest, span)
        ptr = np.zeros(num_users + 1, np.int64)
        np.cumsum(np.bincount(r, minlength=num_users), out=ptr[1:])
        obj = cls.__new__(cls)
        obj._set(ptr, items.astype(np.int32), day.astype(np.int32), num_users, num_items,
                 max_days_ago, device)
        return obj

    def _set(self, ptr, item, day, num_users, num_items, max_days_ago, device):
        self.num_users, self.num_items = int(num_users), int(num_items)
        self.max_days_ago = int(max_days_ago)
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        lens = np.diff(ptr)
        self.max_len = int(lens.max()) if lens.size else 0
        self.nnz = int(ptr[-1])
        pad = np.zeros(1, np.int32)
        self.seq_ptr = torch.from_numpy(ptr).to(dev)
        self.seq_item = torch.from_numpy(item if item.size else pad).to(dev)
        self.seq_day = torch.from_numpy(day if day.size else pad).to(dev)
