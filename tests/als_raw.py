"""What test_gpu_als.py and test_gpu_wals.py share on the GPU side: device buffers, the raw
unweighted half-step, the error measure against the float64 oracles (als_oracle.py,
wals_oracle.py) and the module of the fit tests."""
import numpy as np
import torch

from hnm_recommendation_amd import ImplicitALS, _lib

DEV = torch.device("cuda", 0)
FU, FI = 300, 200
ALPHA, REG = 40.0, 0.01


def bits(a):
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a).view(np.int32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def strided(a, ld):
    """A device [rows, ld] buffer (NaN in the padding) whose first columns hold `a`."""
    buf = torch.full((a.shape[0], ld), float("nan"), dtype=torch.float32, device=DEV)
    buf[:, :a.shape[1]] = dev(a)
    return buf


def raw_solve(ptr, idx, n_rows, buf, tab_rows, d, gram, alpha, reg, row_ids, B, ldo=None):
    ldo = d if ldo is None else ldo
    out = torch.full((max(B, 1), ldo), 7.0, dtype=torch.float32, device=DEV)
    st = _lib.fn("hnm_als_solve_rows_f32")(
        _lib.ctx(DEV), _lib.ptr(ptr), _lib.ptr(idx), n_rows, _lib.ptr(buf), tab_rows,
        buf.stride(0), d, _lib.ptr(gram), alpha, reg, _lib.ptr(row_ids), B, _lib.ptr(out), ldo)
    return st, out


def rel_err(x, x64):
    nz = np.abs(x64).max(1) > 0
    return float((np.abs(x[nz] - x64[nz]).max(1) / np.abs(x64[nz]).max(1)).max())


def new_model(d, seed=0, **kw):
    return ImplicitALS(FU, FI, embedding_dim=d, regularization=REG, alpha=ALPHA, seed=seed,
                       **kw).to(DEV)


def tables(m):
    return (m.user_embeddings.weight.detach().cpu().numpy(),
            m.item_embeddings.weight.detach().cpu().numpy())
