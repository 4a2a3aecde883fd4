"""Wide&Deep recommend (top-12) of a B-user batch over the full H&M catalogue, with and without
item features: what the item-feature fold (csrc/widedeep_features.hip) adds to a step.

Synthetic weights, the default tower (512, 256, 128), d = 64.  The feature counts are
ASSUMPTIONS (Fu = 6, Fi = 24): the reference's data module is not part of its snapshot, so its
real counts are unknown.  Host clock around synchronised steps (tools/deep_probe.py); the fold
kernel's own time comes from a kernel trace of this script.  Features are N(0, scale^2); the
default scale 0.01 is about the spread of the init embedding tables -- unit-variance features
dwarf those, the certified bound then exceeds the score spread and every row takes the exact
kernel (the `fallback rows` column shows it: `scale` = 1 gives a ~1.4 s step with or without
item features).
    python tools/wd_itemfeat_probe.py [B] [steps] [Fi] [Fu] [scale]
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/wd_itemfeat_probe.py 4096 3"""
import os
import sys
import time

import numpy as np
import torch

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
from hnm_recommendation_amd import WideDeep, _lib  # noqa: E402
from hnm_recommendation_amd import synthetic as syn  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
FI = int(sys.argv[3]) if len(sys.argv) > 3 else 24
FU = int(sys.argv[4]) if len(sys.argv) > 4 else 6
SCALE = float(sys.argv[5]) if len(sys.argv) > 5 else 0.01
DEV = torch.device("cuda", 0)
torch.cuda.set_device(0)
U, I, D, LAYERS = 20_000, syn.HM_ITEMS, 64, (512, 256, 128)
rng = np.random.Generator(np.random.PCG64(7))
users = torch.from_numpy(syn.user_batch(U, B, seed=1)).to(DEV)
for fu, fi in ((0, 0), (0, FI), (FU, 0), (FU, FI)):
    sd = syn.widedeep_state_dict(U, I, D, LAYERS, num_user_features=fu, num_item_features=fi,
                                 seed=0)  # bench.py's weights (--weights init)
    m = WideDeep(U, I, num_user_features=fu, num_item_features=fi, embedding_dim=D,
                 deep_layers=list(LAYERS))
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    m = m.to(DEV).eval()
    if fu:
        m.set_user_features((SCALE * rng.standard_normal((U, fu))).astype(np.float32))
    if fi:
        m.set_item_features((SCALE * rng.standard_normal((I, fi))).astype(np.float32))
    with torch.no_grad():
        m.recommend_with_scores(users)  # warm-up
        torch.cuda.synchronize()
        ts = []
        for _ in range(STEPS):
            t0 = time.perf_counter()
            m.recommend_with_scores(users)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        _lib.prefilter_stats(DEV, reset=True)  # one more, untimed step with the counters on
        _lib.set_option(DEV, _lib.HNM_OPT_STATS, 1)
        m.recommend_with_scores(users)
        _lib.set_option(DEV, _lib.HNM_OPT_STATS, 0)
        rows, cands, fb = _lib.prefilter_stats(DEV, reset=True)
    print(f"B {B} Fu {fu} Fi {fi}: median {np.median(ts):8.2f} ms/step  min {min(ts):8.2f}  "
          f"max {max(ts):8.2f}  ({STEPS} steps; {fb} fallback rows of {rows})", flush=True)
    del m
    torch.cuda.empty_cache()
