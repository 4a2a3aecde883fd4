"""Shared host logic of the drop-in model modules.

The reference models are `pytorch_lightning.LightningModule`s (e.g. `neural_cf.py:9`);
Lightning is not part of the scoring hot path and is not installed here, so the mirror
modules are plain `nn.Module`s that keep what the serving/eval callers rely on:
constructor kwargs, `hparams` (what `save_hyperparameters()` records and `serve.py:228`
reads back from `.ckpt` files), submodule names (state_dict keys), `eval()/to()`.
"""
from __future__ import annotations

import inspect

import torch
import torch.nn as nn

from .. import _lib
from .history import (HistoryModel, UserHistory, _history_arrays, basket_csr,  # noqa: F401
                      filter_csr, interaction_weights, interactions_history)
from .sequence import UserSequence  # noqa: F401


class RecModule(nn.Module):
    """nn.Module + the LightningModule bits the hot path's callers use."""
    # what `serving.Recommender` asks a model before a request
    answers_baskets = False        # has recommend_for_items (a visitor without a user index)
    takes_basket_weights = False   # ... which takes per-item `weights`
    back_fill_short_rows = False   # rows read from the model's history may run out of items:
    #                                continued from the popularity list, the rest trimmed

    def save_hyperparameters(self):
        frame = inspect.currentframe().f_back
        info = inspect.getargvalues(frame)
        self.hparams = {k: info.locals[k] for k in info.args if k != "self"}

    def log(self, name, value, *args, **kwargs):
        """LightningModule.log stand-in: the last value per name lands in `logged_metrics`
        (what a Trainer's callback_metrics would hold)."""
        if not hasattr(self, "logged_metrics"):
            self.logged_metrics = {}
        self.logged_metrics[name] = value

    # ------------------------------------------------------ Lightning evaluation hooks
    # The reference's offline-evaluation stack (`trainer.validate` / `trainer.test(ckpt_path=
    # "best")`, scripts/train.py:252): validation_step -> predict_all_items -> torch.topk ->
    # metrics.update, then on_*_epoch_end logs metrics.compute() and resets (neural_cf.py:235-272,
    # lightgcn.py:267-294, wide_deep.py:314-342, matrix_factorization.py:158-185).  Here the
    # dense score matrix + torch.topk is the fused top-K (`recommend_with_scores`, same
    # (score desc, item asc) order), so a step never materialises the [B, num_items] scores.
    def _validation_topk(self, batch):
        return self.recommend_with_scores(batch["user_ids"], k=self.top_k)[1]

    def validation_step(self, batch, batch_idx):
        """batch: {'user_ids': [B], 'ground_truth': [B, T] item ids (negative = padding) or a
        list of id lists}."""
        self._check_top_k()  # torch.topk(scores, self.top_k) raises for top_k > num_items
        with torch.no_grad():
            top = self._validation_topk(batch)
        self.metrics.update(top, batch["ground_truth"])

    def _epoch_end(self, prefix, **kw):
        metrics = self.metrics.compute()
        self.metrics.reset()
        for name, value in metrics.items():
            self.log(f"{prefix}_{name}", value, **kw)
        return metrics

    def on_validation_epoch_end(self):
        return self._epoch_end("val", prog_bar=True)

    def test_step(self, batch, batch_idx):
        self.validation_step(batch, batch_idx)

    def on_test_epoch_end(self):
        return self._epoch_end("test")

    # ------------------------------------------------------------------ helpers
    @property
    def device(self) -> torch.device:
        return next(self.parameters()).device

    def _ids(self, ids: torch.Tensor, bound, what: str = "user_ids", flat: bool = False):
        """(int64 contiguous ids on the module device, host_checked).  Host ids are
        range-checked here for free (IndexError before any launch), so the call needs no
        device-side check; device ids are checked by the kernels' error word, which costs a
        stream sync after the call (`_check`).  `bound` None: no range (a model without a user
        table); `flat`: any shape is flattened, not only a 0-d id."""
        if not isinstance(ids, torch.Tensor):
            ids = torch.as_tensor(ids)
        if flat or ids.dim() == 0:
            ids = ids.reshape(-1)
        dev = self.device
        _lib.require_gpu(dev)
        host = not ids.is_cuda
        if host and bound is not None and ids.numel() > 0:
            lo, hi = int(ids.min()), int(ids.max())
            if lo < 0 or hi >= bound:
                raise IndexError(f"index out of range in self ({what} must be in [0, {bound}))")
        return ids.to(device=dev, dtype=torch.int64).contiguous(), host

    def _check_top_k(self):
        """`recommend()` ends in `torch.topk(scores, self.top_k, dim=1)` (e.g. neural_cf.py:324),
        which raises for top_k outside [0, num_items]; so does the mirror, before any launch.
        `recommend_with_scores(k=...)` (the serve path's per-request k) clamps k instead."""
        if not 0 <= self.top_k <= self.num_items:
            raise RuntimeError("selected index k out of range")

    @staticmethod
    def _check(device, *host_checked):
        """Raise IndexError for out-of-range device ids (syncs the stream) -- skipped when
        every id of the call was range-checked on the host."""
        if not all(host_checked):
            _lib.sync_check(device)


def empty_topk(k: int, u: torch.Tensor):
    """torch.topk's k = 0 result ([B, 0] scores and ids); k < 0 raises as torch.topk does."""
    if k < 0:
        raise RuntimeError("selected index k out of range")
    return empty_rows(u.numel(), 0, u.device)


def empty_rows(B: int, k: int, device):
    """Uninitialised (scores [B, k] f32, items [B, k] int64): the outputs of a top-K entry."""
    return (torch.empty(B, k, dtype=torch.float32, device=device),
            torch.empty(B, k, dtype=torch.int64, device=device))


def dense_topk(scores: torch.Tensor, k: int, mptr=None, midx=None):
    """torch.topk(scores, k) with the CSR mask, on the HIP row top-k kernel."""
    B, I = scores.shape
    k = min(k, I)
    out_v, out_i = empty_rows(B, k, scores.device)
    _lib.call("hnm_topk_rows_f32", _lib.ctx(scores.device), _lib.ptr(scores), scores.stride(0),
              B, I, _lib.ptr(mptr), _lib.ptr(midx), k, _lib.ptr(out_v), _lib.ptr(out_i))
    return out_v, out_i


def f32c(t: torch.Tensor) -> torch.Tensor:
    """fp32 contiguous view (no copy when already so)."""
    return t.detach().to(torch.float32).contiguous()
