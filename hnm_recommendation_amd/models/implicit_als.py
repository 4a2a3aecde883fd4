"""ImplicitALS: matrix-factorization embeddings fitted on the GPU by alternating least squares
for implicit feedback (Hu, Koren & Volinsky 2008).  No reference module: `GEMINI.md` stage 3
names "Matrix Factorization (e.g. ALS ...)" beside the baselines, `src/models` never built it.

    L(X, Y) = sum_{u,i} c_ui (p_ui - x_u . y_i)^2 + reg (|X|^2 + |Y|^2)
    p_ui = 1, c_ui = 1 + alpha w_ui for (u, i) in the history; p_ui = 0, c_ui = 1 otherwise

w_ui is the pair's weight in the history (`UserHistory.hist_w`: summed purchase counts, a recency
decay, ...; the caller applies any log or other transform first), and 1 when the history carries
no weights -- the model this module has always fitted, through the same entry and to the same
bits.

Three HIP entries (`csrc/als.hip`, contract in `include/hnm.h`):

* `hnm_als_gram_f32` -- G = T^T T of a factor table, fixed-order chunked summation;
* `hnm_als_solve_rows_f32` -- one half-step: per CSR row the d x d system
  (G + alpha sum t t^T + reg I) x = (1 + alpha) sum t, by Cholesky in LDS.  The user step, the
  item step (over the transposed history), fold-in of a basket (`user_factors`) and
  `refresh_users` are this one entry, so they agree bit for bit;
* `hnm_als_solve_rows_weighted_f32` -- the same half-step with a weight per stored entry:
  (G + alpha sum w t t^T + reg I) x = sum (1 + alpha w) t.  A history with `hist_w` takes it in
  the fit (the transpose carries the weights) and in `refresh_users`; `user_factors` and
  `recommend_for_items` take it when the call gives `weights`;
* `hnm_als_cg_rows_f32` / `hnm_als_cg_rows_weighted_f32` (`csrc/als_cg.hip`) -- the same
  systems, bit for bit, taken a few conjugate-gradient steps from the previous sweep's row
  instead of solved exactly (Takacs, Pilaszy & Tikk 2011): `fit_history(..., solver="cg",
  cg_steps=3)`.  An option of a fit only: fold-in, `refresh_users` and the cached item Gram stay
  on the exact Cholesky entry, so after a CG fit the stored user rows are the approximate ones
  the sweeps left and a refreshed row is the exact one.

A fit is `iterations` sweeps (user step, then item step): no optimizer, no sampling, no
learning rate.  The module IS a `MatrixFactorization` with zero biases: the same parameters and
state_dict keys, served by the same certified dot-product top-K; a saved ImplicitALS loads as a
MatrixFactorization and the reverse.
"""
from __future__ import annotations

from typing import List, Optional

import numpy as np
import torch

from .. import _lib
from .base import (HistoryModel, UserHistory, basket_csr, dense_topk, empty_rows, empty_topk, f32c,
                   interaction_weights, interactions_history)
from .matrix_factorization import MatrixFactorization

LOSS_PAIR_CHUNK = 1 << 20   # history pairs per float64 pass of loss()
SOLVERS = ("cholesky", "cg")
MAX_CG_STEPS = 32           # hnm.h: hnm_als_cg_rows_f32 takes steps in [1, 32]


def supported_dim(d: int) -> bool:
    return 16 <= d <= 128 and d % 16 == 0


def check_solver(solver, cg_steps):
    """The validated (solver, cg_steps) of a fit: ("cholesky", None) or ("cg", steps)."""
    if solver not in SOLVERS:
        raise ValueError(f"solver must be one of {SOLVERS}, not {solver!r}")
    if isinstance(cg_steps, bool) or int(cg_steps) != cg_steps \
            or not 1 <= int(cg_steps) <= MAX_CG_STEPS:
        raise ValueError(f"cg_steps must be an integer in [1, {MAX_CG_STEPS}]")
    return (solver, int(cg_steps)) if solver == "cg" else (solver, None)


class ImplicitALS(HistoryModel, MatrixFactorization):
    answers_baskets = takes_basket_weights = True   # by fold-in; its rows are full

    def __init__(self, num_users: int, num_items: int, embedding_dim: int = 64,
                 regularization: float = 0.01, alpha: float = 40.0, iterations: int = 15,
                 seed: int = 0, top_k: int = 12):
        if not supported_dim(int(embedding_dim)):
            raise ValueError("embedding_dim must be a multiple of 16 in [16, 128]")
        if not float(regularization) > 0.0 or not np.isfinite(regularization):
            raise ValueError("regularization must be finite and > 0")
        if not float(alpha) >= 0.0 or not np.isfinite(alpha):
            raise ValueError("alpha must be finite and >= 0")
        if int(iterations) < 0:
            raise ValueError("iterations must be >= 0")
        super().__init__(int(num_users), int(num_items), embedding_dim=int(embedding_dim),
                         top_k=int(top_k), sparse=False)
        self.save_hyperparameters()
        self.regularization, self.alpha = float(regularization), float(alpha)
        self.iterations, self.seed = int(iterations), int(seed)
        self.loss_history: List[float] = []
        self.fit_solver = ("cholesky", None)   # what the last fit ran: a fit's option, for logs
        self._gram: Optional[torch.Tensor] = None   # Y^T Y of the fitted item table (fold-in)
        with torch.no_grad():
            self.user_embeddings.weight.zero_()
            self._init_items()

    def _init_items(self):
        """Y ~ N(0, 0.01^2) from a CPU generator: the starting bits do not depend on the device."""
        g = torch.Generator(device="cpu").manual_seed(self.seed)
        y = torch.empty(self.num_items, self.embedding_dim, dtype=torch.float32)
        y.normal_(0.0, 0.01, generator=g)
        w = self.item_embeddings.weight
        w.data.copy_(y.to(w.device))

    def load_state_dict(self, state_dict, *args, **kwargs):
        out = super().load_state_dict(state_dict, *args, **kwargs)
        self._gram = None
        return out

    # ------------------------------------------------------------------ the entries
    def _tables(self):
        """(X, Y): the embedding tables themselves as fp32 contiguous device tensors."""
        for emb in (self.user_embeddings, self.item_embeddings):
            w = emb.weight
            if w.dtype != torch.float32 or not w.is_contiguous():
                w.data = w.data.to(torch.float32).contiguous()
        X, Y = self.user_embeddings.weight.data, self.item_embeddings.weight.data
        _lib.require_gpu(X, Y)
        return X, Y

    def _gram_of(self, tab: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        d = self.embedding_dim
        if out is None:
            out = torch.empty(d, d, dtype=torch.float32, device=tab.device)
        _lib.call("hnm_als_gram_f32", _lib.ctx(tab.device), _lib.ptr(tab), tab.shape[0],
                  tab.stride(0), d, _lib.ptr(out))
        return out

    def _solve(self, ptr, idx, n_rows: int, tab, gram, row_ids, B: int, out, w=None):
        """One half-step; `w` (fp32, aligned with idx) selects the weighted entry."""
        _lib.call_weighted(
            "hnm_als_solve_rows_f32", 3, w, _lib.ctx(tab.device), _lib.ptr(ptr), _lib.ptr(idx),
            n_rows, _lib.ptr(tab), tab.shape[0], tab.stride(0), self.embedding_dim, _lib.ptr(gram),
            self.alpha, self.regularization, _lib.ptr(row_ids), B, _lib.ptr(out),
            out.stride(0) if B else self.embedding_dim)
        return out

    def _cg(self, ptr, idx, n_rows: int, tab, gram, x, steps: int, w=None):
        """One CG half-step for every row, in place on `x` (its rows are the start vectors)."""
        _lib.call_weighted(
            "hnm_als_cg_rows_f32", 3, w, _lib.ctx(tab.device), _lib.ptr(ptr), _lib.ptr(idx),
            n_rows, _lib.ptr(tab), tab.shape[0], tab.stride(0), self.embedding_dim, _lib.ptr(gram),
            self.alpha, self.regularization, None, n_rows, _lib.ptr(x), x.stride(0), steps)
        return x

    def _item_gram(self) -> torch.Tensor:
        _, Y = self._tables()
        if self._gram is None or self._gram.device != Y.device:
            self._gram = self._gram_of(Y)
        return self._gram

    # ------------------------------------------------------------------ fitting
    @staticmethod
    def _transpose(history: UserHistory):
        """(tptr int64 [I + 1], tusers int32, tw fp32 or None): the item -> user CSR, rows
        ascending by user id (a stable sort by item id of pairs that are stored user-major); the
        history's weights, when it has them, go through the same permutation."""
        dev, nnz = history.device, history.nnz
        lens = history.hist_ptr[1:] - history.hist_ptr[:-1]
        users = torch.repeat_interleave(torch.arange(history.num_users, device=dev), lens)
        items = history.hist_idx[:nnz].to(torch.int64)
        order = torch.sort(items, stable=True).indices
        tptr = torch.zeros(history.num_items + 1, dtype=torch.int64, device=dev)
        tptr[1:] = torch.cumsum(torch.bincount(items, minlength=history.num_items), 0)
        tusers = users[order].to(torch.int32)
        if nnz == 0:
            tusers = torch.zeros(1, dtype=torch.int32, device=dev)
        tw = None
        if history.hist_w is not None:
            tw = history.hist_w[:nnz][order].contiguous()
            if nnz == 0:
                tw = torch.zeros(1, dtype=torch.float32, device=dev)
        return tptr, tusers.contiguous(), tw

    def fit_history(self, history: UserHistory, *, iterations: Optional[int] = None,
                    track_loss: bool = False, solver: str = "cholesky", cg_steps: int = 3):
        """Fit on a `UserHistory` and keep it as the model's history: `iterations` sweeps of
        (user step, item step) from the seeded Y.  A history with weights (`hist_w`) is fitted
        with c_ui = 1 + alpha w_ui through the weighted entry, one without through the unweighted
        one.  `track_loss`: `loss()` after every sweep in `self.loss_history` (a monitoring pass
        in float64 per sweep).

        `solver="cg"`: both half-steps of every sweep take `cg_steps` (1..32) conjugate-gradient
        steps from the row's value of the previous sweep instead of the exact Cholesky solve,
        in place on X and Y (X starts at zeros, Y at the seeded table).  The sweeps still lower
        the loss; the tables are not the exact-solve fit's.  `self.fit_solver` keeps what ran.
        Fold-in (`user_factors`, `recommend_for_items`) and `refresh_users` stay exact."""
        chosen = check_solver(solver, cg_steps)
        _lib.require_gpu(self.item_embeddings.weight)
        iters = self.iterations if iterations is None else int(iterations)
        if iters < 0:
            raise ValueError("iterations must be >= 0")
        history = self.set_history(history)._need_history()
        X, Y = self._tables()
        dev = X.device
        with torch.no_grad():
            self._init_items()
            X.zero_()
            self.user_bias.weight.zero_()
            self.item_bias.weight.zero_()
            self.global_bias.zero_()
        self._gram = None
        self.loss_history = []
        self.fit_solver = chosen
        tptr, tusers, tw = self._transpose(history)
        U, I = self.num_users, self.num_items
        gram = torch.empty(self.embedding_dim, self.embedding_dim, dtype=torch.float32, device=dev)
        for _ in range(iters):
            self._gram_of(Y, gram)
            if chosen[0] == "cg":
                self._cg(history.hist_ptr, history.hist_idx, U, Y, gram, X, chosen[1],
                         history.hist_w)
            else:
                self._solve(history.hist_ptr, history.hist_idx, U, Y, gram, None, U, X,
                            history.hist_w)
            self._gram_of(X, gram)
            if chosen[0] == "cg":
                self._cg(tptr, tusers, I, X, gram, Y, chosen[1], tw)
            else:
                self._solve(tptr, tusers, I, X, gram, None, I, Y, tw)
            if track_loss:
                self.loss_history.append(self.loss())
        _lib.sync_check(dev)
        return self

    _interaction_weights = staticmethod(interaction_weights)   # the old name; now in history.py

    def fit_interactions(self, user_ids, item_ids, *, weights=None, days_ago=None,
                         time_decay: float = 0.0, iterations: Optional[int] = None,
                         track_loss: bool = False, solver: str = "cholesky", cg_steps: int = 3):
        """Fit from (user, item) interaction arrays or tensors (duplicates allowed; ids out of
        range raise IndexError): builds the `UserHistory`, keeps it, runs the sweeps.

        `weights` (one finite value >= 0 per transaction) and/or `days_ago` (whole days >= 0)
        with `time_decay` >= 0 make it a weighted fit: a transaction weighs
        weights * exp(-time_decay * days_ago) (float64 on the host), a pair the sum of its
        transactions (`UserHistory.from_interactions`).  With neither, this is the unweighted
        fit and its bits.  `solver` / `cg_steps`: as in `fit_history`."""
        check_solver(solver, cg_steps)
        _lib.require_gpu(self.item_embeddings.weight)
        hist = interactions_history(user_ids, item_ids, self.num_users, self.num_items,
                                    self.device, weights, days_ago, time_decay)
        return self.fit_history(hist, iterations=iterations, track_loss=track_loss, solver=solver,
                                cg_steps=cg_steps)

    def loss(self) -> float:
        """L(X, Y) over the model's history in float64, without a [U, I] matrix:
        sum_{u,i} (x_u . y_i)^2 = tr((X^T X)(Y^T Y)); each history pair then trades its s^2 for
        (1 + alpha w)(1 - s)^2 (w = 1 without weights); plus the regulariser."""
        X, Y = self._tables()
        h = self._need_history()
        X64, Y64 = X.to(torch.float64), Y.to(torch.float64)
        total = ((X64.T @ X64) * (Y64.T @ Y64)).sum()
        lens = h.hist_ptr[1:] - h.hist_ptr[:-1]
        users = torch.repeat_interleave(torch.arange(h.num_users, device=X.device), lens)
        items = h.hist_idx[:h.nnz].to(torch.int64)
        for p0 in range(0, h.nnz, LOSS_PAIR_CHUNK):
            s = (X64[users[p0:p0 + LOSS_PAIR_CHUNK]] * Y64[items[p0:p0 + LOSS_PAIR_CHUNK]]).sum(1)
            c = 1.0 + self.alpha
            if h.hist_w is not None:
                c = 1.0 + self.alpha * h.hist_w[p0:min(p0 + LOSS_PAIR_CHUNK, h.nnz)].to(torch.float64)
            total = total + (c * (1.0 - s) ** 2 - s ** 2).sum()
        total = total + self.regularization * ((X64 ** 2).sum() + (Y64 ** 2).sum())
        return float(total)

    # ------------------------------------------------------------------ fold-in
    def user_factors(self, baskets, weights=None) -> torch.Tensor:
        """[n, d] fold-in vectors of n baskets (a list of item-id iterables, or a (ptr, idx) CSR
        with ascending unique rows): the user half-step against the fitted Y.  `weights`: a
        weight per basket item ("three of these", "just viewed"), see `basket_csr`.  Always the
        exact (Cholesky) entry, whichever solver the fit used."""
        gram = self._item_gram()
        _, Y = self._tables()
        ptr, idx, n, w = basket_csr(baskets, self.num_items, Y.device, weights)
        out = torch.empty(n, self.embedding_dim, dtype=torch.float32, device=Y.device)
        self._solve(ptr, idx, n, Y, gram, None, n, out, w)
        _lib.sync_check(Y.device)   # a CSR given by the caller may hold any id
        return out

    def recommend_for_items(self, baskets, filter_seen: bool = True, k: Optional[int] = None, *,
                            weights=None):
        """(scores [n, k], items [n, k]) for n baskets of item ids -- visitors without a user
        index: the fold-in vectors (`user_factors(baskets, weights)`) are the user table of the
        dot-product top-K.  `filter_seen` removes each basket's own items from its answer.  The
        fold-in is the exact (Cholesky) entry, whichever solver the fit used."""
        k = self.top_k if k is None else k
        gram = self._item_gram()
        _, Y = self._tables()
        dev, d = Y.device, self.embedding_dim
        ptr, idx, n, w = basket_csr(baskets, self.num_items, Y.device, weights)
        kk = min(k, self.num_items)
        if kk <= 0:
            return empty_topk(k, ptr[:n])
        if n == 0:
            return empty_rows(0, kk, dev)
        F = torch.empty(n, d, dtype=torch.float32, device=dev)
        self._solve(ptr, idx, n, Y, gram, None, n, F, w)
        rows = torch.arange(n, dtype=torch.int64, device=dev)
        ub = torch.zeros(n, dtype=torch.float32, device=dev)
        ib, gb = f32c(self.item_bias.weight).reshape(-1), f32c(self.global_bias)
        mptr, midx = (ptr, idx) if filter_seen else (None, None)
        c = _lib.ctx(dev)
        if kk > 64:
            s = torch.empty(n, self.num_items, dtype=torch.float32, device=dev)
            _lib.call("hnm_dot_scores_f32", c, _lib.ptr(F), n, d, _lib.ptr(rows), n, _lib.ptr(Y),
                      self.num_items, d, d, _lib.ptr(ub), _lib.ptr(ib), _lib.ptr(gb), _lib.ptr(s),
                      s.stride(0))
            out = dense_topk(s, kk, mptr, midx)
        else:
            out = empty_rows(n, kk, dev)
            _lib.call("hnm_dot_topk_f32", c, _lib.ptr(F), n, d, _lib.ptr(rows), n, _lib.ptr(Y),
                      self.num_items, d, d, _lib.ptr(ub), _lib.ptr(ib), _lib.ptr(gb),
                      _lib.ptr(mptr), _lib.ptr(midx), kk, _lib.ptr(out[0]), _lib.ptr(out[1]))
        _lib.sync_check(dev)
        return out

    def refresh_users(self, user_ids, history: Optional[UserHistory] = None):
        """Recompute the stored factors of `user_ids` from `history` (default: the model's own)
        against the fitted Y -- a customer who bought something since the fit, without a refit.
        A history with weights takes the weighted entry, as in the fit.  Always the exact
        (Cholesky) entry: after a `solver="cg"` fit the stored rows are the approximate ones the
        sweeps left, and a refreshed row is the exact one."""
        h = self._need_history(history)
        u, _ = self._ids(user_ids, self.num_users)
        gram = self._item_gram()
        X, Y = self._tables()
        out = torch.empty(u.numel(), self.embedding_dim, dtype=torch.float32, device=Y.device)
        self._solve(h.hist_ptr, h.hist_idx, self.num_users, Y, gram, u, u.numel(), out, h.hist_w)
        _lib.sync_check(Y.device)
        X[u] = out
        return self
