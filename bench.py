"""Headline benchmark: recommendations/sec (batched users, K=12) on the reference's
configs (BASELINE.json), MI355X-native HIP path.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload ncf|lightgcn|lightgcn128|widedeep|mf|ncf_deep]
                    [--dump-outputs DIR] [--full]

Default workload = BASELINE.json configs[1]: NeuralCF mf 64, mlp [128,64,32], full H&M
shape (1,371,980 users x 105,542 items), batch 4096 users per rank per step, K=12,
synthetic PCG64 weights with the reference init distributions.  A step = one
`recommend()` of the batch: per-user + per-item layer-1 projections, the fused
pair-MLP + top-K kernel, the partition merge (and at N>1 the item-sharded exchange:
all_gather of user ids + all_to_all of candidates + merge).  Inputs (user-id batches) are
resident in HBM before timing.

N>1 (torchrun, one rank per GPU): items are row-sharded across ranks; every rank brings
4096 users and scores all N*4096 users against its I/N items (weak scaling).

A plain run sets up, warms up, times the K steps, writes the last timed step's outputs
(--dump-outputs DIR: DIR/scores.npy float32 [B, 12] and DIR/items.npy float64 [B, 12], the
arrays `recommend()` returned; the inputs are seeded, so two builds compare output for output)
and prints ONE JSON line: metric, value, ms_per_step, dtype and
  roofline     -- dominant kernel (NCF: ncf16_scan_kernel, the certified f16 scan; with
                  --exact the fp32 ncf32_kernel) algorithmic FLOPs per launch / its
                  average duration (HIP events on the ctx stream, measured live here),
                  vs the MFMA peak of the kernel's dtype; `traffic` from the committed
                  rocprofv3 PMC summary (profiles/) when present for this workload.
With --full the same line also carries the legs measured after the timed region (exact_fp32,
filtered, module_surface, pipelined_3_streams, prefilter counters, ...), and the default NCF
run adds every other workload's line, the pruning-robustness lines and the B = 1 serve
latencies, each from a child process:
  exact_fp32   -- the same step with the pre-filter off (every pair in exact fp32).
  cpu_baseline -- the reference's PyTorch-CPU path (oracle/torch_cpu.py: its torch ops
                  restated, pinned to the reference goldens) on a bounded user sample,
                  on the host's cores, rank 0 at N=1 only.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch
import torch.distributed as dist

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

from hnm_recommendation_amd import LightGCN, MatrixFactorization, NeuralCF, UserHistory, WideDeep  # noqa: E402
from hnm_recommendation_amd import _lib  # noqa: E402
from hnm_recommendation_amd import sharding as S  # noqa: E402
from hnm_recommendation_amd import synthetic as syn  # noqa: E402

METRIC = "recommendations/sec (batched users, K=12) at 1/2/4/8 MI355X; % HBM roofline"
FP32_MFMA_PEAK_TFLOPS = 157.3   # MI355X_MICROARCH.md: fp32 matrix (= vector) peak
# f16 dense MFMA: v_mfma_f32_32x32x16_f16 = 32 cycles/SIMD -> 1024 FLOP/clk/SIMD x 4 x 256 CUs
# x 2.4 GHz (MI355X_MICROARCH.md "Peak BF16/FP16 MFMA ~2.5 PF dense")
F16_MFMA_PEAK_TFLOPS = 2516.6
HBM_PEAK_GBS = 8000.0           # MI355X_MICROARCH.md: HBM3E spec peak
# random 256-B row gathers measured on MI355X (tools/gather_probe.hip, profiles/r4x_gather_probe.txt,
# 4 loads in flight per 16-lane group): an L2-resident 4 MB table 23.0 TB/s -- the ceiling of a
# gather with perfect L2 locality; uniformly random rows of the LightGCN tables themselves:
# 27 MB (the item table at d=64) 8.5 TB/s, 351 MB (the user table) 7.1 TB/s
L2_GATHER_TBPS = 23.0
ITEM_TABLE_GATHER_TBPS = 8.5
USER_TABLE_GATHER_TBPS = 7.1
K = 12
# trained-like weight sets (synthetic.stress_state_dict; the certified bounds' stress cases of
# tests/test_gpu_bound_stress.py): embedding rows at norms 50-200 / Student-t(3) weights and biases
STRESS_WEIGHTS = ("norms", "student_t")


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def launch_ranks(n_gpus):
    """`bench.py --gpus N` (N > 1) started without a launcher: run N ranks through
    torch.distributed.run as a CHILD process and return its exit code.  This process has
    not touched the GPU (no HIP call before this point), and it does not exec."""
    import socket
    import subprocess
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           f"--nproc-per-node={n_gpus}", "--master-addr=127.0.0.1", f"--master-port={port}",
           os.path.abspath(__file__), *sys.argv[1:]]
    log(f"launching {n_gpus} ranks: {' '.join(cmd)}")
    return subprocess.call(cmd, env=env)


def setup_dist(n_gpus):
    """One process per GPU; backend "nccl" (= RCCL over xGMI).  HNM_DIST_BACKEND=gloo
    rehearses the sharded path on fewer GPUs than ranks (collectives staged through host)."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != n_gpus:
        raise SystemExit(f"bench.py --gpus {n_gpus} but WORLD_SIZE={world}: launch one rank "
                         "per GPU (torch.distributed.run --nproc-per-node N)")
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1:
        backend = os.environ.get("HNM_DIST_BACKEND", "nccl")
        ndev = torch.cuda.device_count()
        dev = local if backend == "nccl" else local % max(ndev, 1)
        torch.cuda.set_device(dev)
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", dev))
        else:
            dist.init_process_group(backend)
        return rank, world, torch.device("cuda", dev)
    torch.cuda.set_device(0)
    return rank, world, torch.device("cuda", 0)


def load(m, sd, device):
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return m.to(device).eval()


def build_workload(name, rank, world, device, batch, exact=False, weights="init"):
    """Returns (step_fn(users) -> (vals, idx), flops_or_bytes_per_launch, bound, info)."""
    U, I = syn.HM_USERS, syn.HM_ITEMS
    lo, hi = S.shard_range(I, rank, world)
    info = {}
    if name == "ncf":
        kw = (dict(bias_scale=0.05, emb_scale=20.0) if weights == "personal" else
              dict(bias_scale=0.05) if weights in STRESS_WEIGHTS else {})
        sd = syn.ncf_state_dict(U, I, 64, (128, 64, 32), seed=0, **kw)
        if weights in STRESS_WEIGHTS:
            sd = syn.stress_state_dict(sd, weights, syn.NCF_EMB_KEYS, "mlp_item_embedding.weight")
        m = load(NeuralCF(U, I), sd, device)
        local = S.ncf_shard_topk(m, lo, hi, K)
        info["_filtered"] = lambda hist: S.ItemShardedRecommender(
            S.ncf_shard_topk(m, lo, hi, K, hist), S.hip_merge, K, lo, rank, world).recommend
        info["_module"] = m
        info["_user_sharded"] = lambda: S.ncf_shard_topk(m, 0, I, K)
        per_launch = 4352.0 * batch * world * (hi - lo)   # 4,352 FLOP / pair
        info.update({"model": "NeuralCF", "mf_dim": 64, "mlp_dims": [128, 64, 32], "weights": weights,
                     "scan": "exact fp32" if exact else
                             "certified f16 pre-filter + exact fp32 re-scoring (ncf_cert.hip)"})
        bound, kernel = "mfma", ("ncf32_kernel" if exact else "ncf16_scan_kernel")
        cpu = ("ncf", sd)
    elif name in ("lightgcn", "lightgcn128"):
        d = 64 if name == "lightgcn" else 128
        sd = syn.lightgcn_state_dict(U, I, d, seed=0)
        m = LightGCN(U, I, embedding_dim=d, num_layers=3)
        edges = syn.bipartite_edge_index(U, I, syn.HM_INTERACTIONS, seed=2)
        m.set_graph(torch.from_numpy(edges))
        m = load(m, sd, device)
        g = m._device_graph()
        # the reference recomputes the propagation inside every recommend() call
        # (lightgcn.py:197 predict_all_items -> self.forward()): so does the step, restricted
        # to the rows that call reads (LightGCN.propagate_for: outputs identical)
        # world > 1: the propagation's item rows are sharded too (restricted SpMM plans, one
        # all_gather of the [I, d] item rows after layers 1 and 2; bitwise the same outputs)
        ex = S.ItemRowExchange(U, I, rank, world) if world > 1 else None
        rec = S.ItemShardedRecommender(S.lightgcn_shard_topk(m, lo, hi, K, exchange=ex),
                                       S.hip_merge, K, lo, rank, world)

        def full_step(users):  # whole-graph propagation per call, for comparison
            F = m.propagate(g)
            return S.ItemShardedRecommender(S.dot_shard_topk(F[:U], F[U:], lo, hi, K),
                                            S.hip_merge, K, lo, rank, world).recommend(users)

        N = U + I
        # per whole-graph propagation layer: CSR (col int32 + val fp32 per nnz, rowptr int64),
        # X read once, Y written once, item-row accumulators read + written (layers 1..L-1;
        # the restricted last layer is not timed)
        per_launch = g.nnz * 8.0 + (N + 1) * 8.0 + 2.0 * N * d * 4 + 2.0 * I * d * 4
        gathered = g.nnz * d * 4.0
        if ex is not None:
            # a rank's layer 1..L-1: the user rows + its item shard (restricted plan), X read
            # once, its rows written, its items' accumulators read + written
            rp = g.rowptr.cpu()
            kept = int(rp[U]) + int(rp[U + hi]) - int(rp[U + lo])
            per_launch = (kept * 8.0 + (N + 1) * 8.0 + N * d * 4.0 + (U + hi - lo) * d * 4.0
                          + 2.0 * (hi - lo) * d * 4)
            gathered = kept * d * 4.0
            info["item_row_exchange"] = {
                "all_gathers_per_step": 2, "bytes_received_per_rank": ex.bytes_per_call(d),
                "note": "propagation item rows sharded: every rank computes all user rows of "
                        "layers 1-2 and its own item rows (hnm_spmm_plan_restrict), one "
                        "all_gather of the [I, d] item rows after each of those layers, the "
                        "last layer on its own items; roofline prices the rank's restricted layer"}
        info["_filtered"] = lambda hist: S.ItemShardedRecommender(
            S.lightgcn_shard_topk(m, lo, hi, K, hist, exchange=ex), S.hip_merge, K, lo, rank,
            world).recommend
        info["_module"] = m
        info.update({"model": "LightGCN", "embedding_dim": d, "num_layers": 3,
                "interactions": syn.HM_INTERACTIONS, "nnz_with_self_loops": g.nnz,
                "step": "3-layer propagation restricted to what recommend() reads (layers 1-2 "
                        "whole graph, layer 3 on item rows + the step's users; outputs "
                        "identical to forward()) + certified top-K scan of the batch"})
        info["_serving"] = lambda: (lambda F: S.ItemShardedRecommender(
            S.dot_shard_topk(F[:U], F[U:], lo, hi, K), S.hip_merge, K, lo, rank,
            world).recommend)(m.propagate(g))
        info["_full_step"] = full_step
        info["_user_sharded"] = lambda: S.lightgcn_shard_topk(m, 0, I, K)
        ret = dict(step=rec.recommend, per_launch=per_launch, bound="hbm",
                   kernel="spmm layer (spmm_swalk_kernel short rows + spmm_walk_kernel long rows + spmm_walk_finish_kernel), whole-graph layers",
                   timing=_lib.TIME_SPMM, gathered=gathered)
        return ret, info, ("lightgcn", (sd, edges, d))
    elif name == "widedeep":
        sd = syn.widedeep_state_dict(U, I, 64, (512, 256, 128), seed=0)
        m = load(WideDeep(U, I), sd, device)
        local = S.widedeep_shard_topk(m, lo, hi, K)
        info["_user_sharded"] = lambda: S.widedeep_shard_topk(m, 0, I, K)
        per_launch = 328450.0 * batch * world * (hi - lo)   # 328,450 FLOP / pair
        info.update({"model": "WideDeep", "embedding_dim": 64, "deep_layers": [512, 256, 128]})
        bound, kernel = "mfma", ("widedeep_score_kernel" if exact else "wdc_scan_kernel")
        info["scan"] = ("exact fp32" if exact else
                        "certified f16 (layers 2 and 3: one W_hi.x_hi MFMA pass each; weight and activation residuals bounded exactly, the layer-2 bound terms on the matrix pipe) pre-filter + exact fp32 re-scoring")
        cpu = ("widedeep", None)
    elif name == "ncf_deep":
        # a NeuralCF tower other than the default two-layer one (VERDICT r4 missing #1): the
        # reference builds any depth (neural_cf.py:75-90); [128, 64, 32, 16] with mf 64
        kw = (dict(bias_scale=0.05, emb_scale=20.0) if weights == "personal" else
              dict(bias_scale=0.05) if weights in STRESS_WEIGHTS else {})
        sd = syn.ncf_state_dict(U, I, 64, (128, 64, 32, 16), seed=0, **kw)
        if weights in STRESS_WEIGHTS:
            sd = syn.stress_state_dict(sd, weights, syn.NCF_EMB_KEYS, "mlp_item_embedding.weight")
        m = load(NeuralCF(U, I, mlp_dims=[128, 64, 32, 16]), sd, device)
        local = S.ncf_shard_topk(m, lo, hi, K)  # -> ncf_deep_shard_topk (single-phase exchange)
        info["_module"] = m
        info["_per_pair_route"] = True
        # useful fp32 MACs a pair after the per-row first layer: GMF 64, layers 64x32 and
        # 32x16, prediction 16
        per_launch = 2.0 * (64 + 64 * 32 + 32 * 16 + 16) * batch * (hi - lo)
        info.update({"model": "NeuralCF", "mf_dim": 64, "mlp_dims": [128, 64, 32, 16],
                     "weights": weights,
                     "scan": "exact fp32: f32-MFMA layer chains over 32-item tiles (bitwise the "
                             "fmaf chain) with fused per-partition top-k lists (ncf_deep.hip)"})
        info["_deep_cert"] = True
        bound, kernel = "mfma", "ncf_deep_mfma_kernel"
        cpu = ("ncf", sd)
    elif name == "mf":
        if weights == "personal":
            raise SystemExit("--weights personal: NCF only (MF's init best items are already "
                             "user-specific)")
        sd = syn.mf_state_dict(U, I, 64, seed=0, bias_scale=0.05 if weights in STRESS_WEIGHTS else 0.0)
        if weights in STRESS_WEIGHTS:
            sd = syn.stress_state_dict(sd, weights, syn.MF_EMB_KEYS, "item_embeddings.weight")
        m = load(MatrixFactorization(U, I, sparse=False), sd, device)
        local = S.dot_shard_topk(m.user_embeddings.weight.detach(), m.item_embeddings.weight.detach(),
                                 lo, hi, K, user_bias=m.user_bias.weight.detach(),
                                 item_bias=m.item_bias.weight.detach(),
                                 const_bias=m.global_bias.detach())
        per_launch = 2.0 * 64 * batch * world * (hi - lo)
        info["_module"] = m
        info["_user_sharded"] = lambda: S.dot_shard_topk(
            m.user_embeddings.weight.detach(), m.item_embeddings.weight.detach(), 0, I, K,
            user_bias=m.user_bias.weight.detach(), item_bias=m.item_bias.weight.detach(),
            const_bias=m.global_bias.detach())
        info.update({"model": "MatrixFactorization", "embedding_dim": 64, "weights": weights})
        bound, kernel = "mfma", ("dot_score_kernel" if exact else "dot16_scan_kernel")
        cpu = ("mf", sd)
    else:
        raise SystemExit(f"unknown workload {name}")
    rec = S.ItemShardedRecommender(local, S.hip_merge, K, lo, rank, world)
    ret = dict(step=rec.recommend, per_launch=per_launch, bound=bound, kernel=kernel,
               timing=_lib.TIME_SCORE)
    return ret, info, cpu


def dump_outputs(path, out, rank):
    """--dump-outputs: the (scores, items) pair the last timed step returned, as float32 /
    float64 .npy files (item ids are exact in float64); a few hundred KB at the default batch."""
    vals, idx = out
    os.makedirs(path, exist_ok=True)
    tag = "" if rank == 0 else f"_rank{rank}"
    np.save(os.path.join(path, f"scores{tag}.npy"), vals.detach().float().cpu().numpy())
    np.save(os.path.join(path, f"items{tag}.npy"), idx.detach().cpu().numpy().astype(np.float64))


def timed_rate(fn, batches, steps, world, B):
    """users/s of `steps` calls of fn over the resident batches (one warm call first),
    bracketed like the headline loop (sync + barrier on both sides, max over ranks)."""
    fn(batches[0])
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for j in range(steps):
        fn(batches[j % len(batches)])
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    el = time.perf_counter() - t0
    if world > 1:
        on_host = dist.get_backend() == "gloo"
        t = torch.tensor([el], dtype=torch.float64, device="cpu" if on_host else "cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        el = float(t[0])
    return B * world * steps / el


def pipelined_rate(fn, batches, steps, B, nstreams=3):
    """users/s with `nstreams` independent batches in flight: one worker thread per torch
    stream (hence one hnm_ctx each), batches dealt round-robin, every call complete (nothing
    shared across calls, no work skipped); the outputs are compared bitwise with the
    sequential answers of the same batches.  3 streams, not 2: with GPU_MAX_HW_QUEUES = 4 two
    pool streams can land on one hardware queue and serialize."""
    import threading
    ref = [fn(b) for b in batches]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in range(nstreams)]
    outs = [None] * steps
    errs = []
    start = threading.Barrier(nstreams + 1)
    dev = torch.cuda.current_device()

    def work(w):
        try:
            torch.cuda.set_device(dev)
            with torch.cuda.stream(streams[w]):
                fn(batches[w % len(batches)])  # this thread's ctx + workspace
                torch.cuda.current_stream().synchronize()
                start.wait()
                for j in range(w, steps, nstreams):
                    outs[j] = fn(batches[j % len(batches)])
                torch.cuda.current_stream().synchronize()
        except BaseException as e:  # reported below
            errs.append(e)
            start.abort()

    ts = [threading.Thread(target=work, args=(w,)) for w in range(nstreams)]
    for t in ts:
        t.start()
    try:
        start.wait()
    except threading.BrokenBarrierError:
        pass
    t0 = time.perf_counter()
    for t in ts:
        t.join()
    el = time.perf_counter() - t0
    if errs:
        raise errs[0]
    same = all(torch.equal(outs[j][1], ref[j % len(batches)][1]) and
               torch.equal(outs[j][0].view(torch.int32), ref[j % len(batches)][0].view(torch.int32))
               for j in range(steps))
    return B * steps / el, same


def _median_rate(fn, users, runs, budget_s):
    """users/s of fn(users): median of up to `runs` timed calls within ~budget_s."""
    times = []
    t_start = time.perf_counter()
    while len(times) < runs and (not times or time.perf_counter() - t_start < budget_s):
        t0 = time.perf_counter()
        fn(users)
        times.append(time.perf_counter() - t0)
    return len(users) / float(np.median(times)), len(times)


def cpu_baseline(cpu):
    """The reference's PyTorch-CPU path (oracle/torch_cpu.py: the reference's torch ops
    restated, checked against the reference-produced goldens) on a bounded user sample,
    on this host's cores (the box's CPU share = OMP_NUM_THREADS)."""
    if cpu is None:
        return None
    from oracle import torch_cpu as T  # baseline leg only
    kind, payload = cpu
    cores = int(os.environ.get("OMP_NUM_THREADS", os.cpu_count() or 1))
    torch.set_num_threads(cores)
    U, I = syn.HM_USERS, syn.HM_ITEMS
    out = {"unit": "users/s", "cores": cores, "kind": "port"}
    if kind == "ncf":
        sd = T.as_torch(payload)
        users = torch.from_numpy(syn.user_batch(U, 64, seed=7))
        T.ncf_recommend(sd, users[:8])  # warm-up
        v, n = _median_rate(lambda u: T.ncf_recommend(sd, u), users, 3, 20.0)
        out["sample"] = (f"torch restatement of NeuralCF.recommend (neural_cf.py:143-208,300-326: "
                         f"gathers, expand+cat in 1000-item chunks, Linear/ReLU, topk), B=64 x "
                         f"{I} items, median of {n}")
    elif kind == "mf":
        sd = T.as_torch(payload)
        users = torch.from_numpy(syn.user_batch(U, 4096, seed=7))
        T.mf_recommend(sd, users[:64])
        v, n = _median_rate(lambda u: T.mf_recommend(sd, u), users, 3, 20.0)
        out["sample"] = (f"torch restatement of MatrixFactorization.recommend "
                         f"(matrix_factorization.py:108-131,220-246), B=4096 x {I} items, "
                         f"median of {n}")
    elif kind == "lightgcn":
        sd, edges, d = payload
        t0 = time.perf_counter()
        graph = T.lightgcn_graph(torch.from_numpy(edges), U + I)
        t_graph = time.perf_counter() - t0
        w = torch.from_numpy(sd["embeddings.weight"])
        t0 = time.perf_counter()
        fu, fi = T.lightgcn_forward(w, graph, U)
        t_prop = time.perf_counter() - t0
        users = torch.from_numpy(syn.user_batch(U, 4096, seed=7))
        T.lightgcn_recommend(fu, fi, users[:64])
        r_score, n = _median_rate(lambda u: T.lightgcn_recommend(fu, fi, u), users, 3, 10.0)
        # the reference's recommend() re-propagates on every call (lightgcn.py:197)
        v = 4096 / (t_prop + 4096 / r_score)
        out["scoring_only_users_per_s"] = round(r_score, 2)
        out["propagation_s"] = round(t_prop, 3)
        out["sample"] = (f"torch restatement of LightGCN.recommend: 3-layer propagation "
                         f"(lightgcn.py:136-164, torch.sparse.mm on CSR; set_graph {t_graph:.1f}s "
                         f"not counted) + F_U[ids] @ F_I^T + topk (:188-204), B=4096 x {I} "
                         f"items, d={d}, one propagation + median of {n} scorings")
    elif kind == "widedeep":
        # full U is infeasible on the reference path (one-hot [500, U+I] per user per
        # chunk): timed at U=10,000 with the full item catalogue, one user
        Uc = 10_000
        sd = T.as_torch(syn.widedeep_state_dict(Uc, I, 64, (512, 256, 128), seed=0))
        users = torch.from_numpy(syn.user_batch(Uc, 1, seed=7))
        v, n = _median_rate(lambda u: T.widedeep_recommend(sd, u), users, 1, 0.0)
        out["sample"] = (f"torch restatement of WideDeep.recommend (wide_deep.py:157-285,405-435: "
                         f"one-hot wide input, deep tower, 500-item chunks) at U=10,000 (full U "
                         f"infeasible on the reference path), B=1 x {I} items, one run")
    else:
        return None
    out["value"] = round(v, 3)
    return out


def serve_latency(args, device):
    """Serve-path latency (serve.py:340-357): ONE user per request, 23-item purchase
    history masked, top-k with scores copied back to the host, for k = 12 and 100.
    NCF on the full H&M shape; LightGCN with its propagated tables cached (what a server
    holding the module sees after the first request).  p50/p99 over `--steps` requests,
    certified path (default) and exact fp32 scan."""
    U, I = syn.HM_USERS, syn.HM_ITEMS
    if args.workload == "ncf":
        m = load(NeuralCF(U, I), syn.ncf_state_dict(U, I, 64, (128, 64, 32), seed=0), device)
        if not os.environ.get("HNM_BENCH_NO_ITEM_CACHE"):
            m.cache_item_tables()  # what serving.Recommender does with a server's fixed weights
    elif args.workload in ("lightgcn", "lightgcn128"):
        d = 64 if args.workload == "lightgcn" else 128
        m = LightGCN(U, I, embedding_dim=d, num_layers=3)
        m.set_graph(torch.from_numpy(syn.bipartite_edge_index(U, I, syn.HM_INTERACTIONS, seed=2)))
        m = load(m, syn.lightgcn_state_dict(U, I, d, seed=0), device)
        m.forward()
    elif args.workload == "mf":
        m = load(MatrixFactorization(U, I, sparse=False), syn.mf_state_dict(U, I, 64, seed=0), device)
    else:
        raise SystemExit("--latency: ncf, lightgcn, lightgcn128 or mf")
    users = syn.user_batch(U, max(args.steps, 8), seed=300)
    hist = syn.filter_dict(users, I, per_user=23, seed=301)
    out = {"metric": "serve latency (B=1 recommend_with_scores, 23-item history mask, "
                     "scores to host)", "unit": "ms", "workload": args.workload,
           "higher_is_better": False, "requests": len(users)}
    for mode in ("certified", "exact"):
        _lib.set_prefilter(device, mode == "certified")
        for k in (12, 100):
            def one(u):
                ut = torch.tensor([int(u)], dtype=torch.int64, device=device)
                v, i = m.recommend_with_scores(ut, filter_items={int(u): hist[int(u)]}, k=k)
                return v.cpu().tolist(), i.cpu().tolist()
            for u in users[:5]:
                one(u)
            lat = []
            for u in users:
                t0 = time.perf_counter()
                one(u)
                lat.append((time.perf_counter() - t0) * 1e3)
            out[f"{mode}_k{k}"] = {"p50": round(float(np.percentile(lat, 50)), 4),
                                   "p99": round(float(np.percentile(lat, 99)), 4),
                                   "mean": round(float(np.mean(lat)), 4)}
    _lib.set_prefilter(device, True)
    print(json.dumps(out), flush=True)


# algorithmic FLOP per (user, item) pair and the f16 MFMA FLOP the certified
# scans issue per pair: NCF 4,096 layer 2 + 1,024 16x16x32 epilogue (64 useful) + 128 GMF;
# W&D one W_hi x_hi pass of layer 2 (262,144), its two bound MFMAs (16x16x32 against x_hi and
# |x_lo|: 32,768) and one pass of layer 3 (65,536); dot d = 64: 128
ALG_FLOP_PER_PAIR = {"ncf": 4352.0, "widedeep": 328450.0, "mf": 128.0, "ncf_deep": 5280.0}
# ncf_deep (the certified deep scan): layer 2 4,096 + layer 3 on 16x16x32 tiles whose A rows zero
# the other item half's k-groups 2,048 + the 16x16x16 prediction 512 + GMF 128
ISSUED_F16_FLOP_PER_PAIR = {"ncf": 5248.0, "widedeep": 360448.0, "mf": 128.0, "ncf_deep": 6784.0}
RANDOM_DATA_F16_TFLOPS = 1235.0  # bare f16 MFMA loop, random operands: 1,190-1,291 TF/s


def pmc_traffic(workload):
    """HBM bytes per launch of the dominant kernel from the committed rocprofv3 PMC summary."""
    p = os.path.join(REPO, "profiles", f"pmc_{workload}.json")
    if not os.path.exists(p):
        return None
    try:
        return json.load(open(p)).get("hbm_bytes_per_launch")
    except Exception:
        return None


# the other BASELINE configs, run by the default (NCF, N = 1) invocation as child processes so
# that the driver's record carries every workload line (configs[2] lightgcn, configs[3]
# widedeep, configs[4]'s per-GPU work lightgcn128; mf is the MatrixFactorization extension)
EXTRA_WORKLOADS = (("lightgcn", "configs[2]: LightGCN 3-layer dim=64, full H&M adjacency"),
                   ("widedeep", "configs[3]: Wide&Deep dim=64, 512-256-128 tower"),
                   ("lightgcn128", "configs[4] per-GPU work at N=1: LightGCN dim=128"),
                   ("mf", "MatrixFactorization dim=64 (SURVEY §8(f))"),
                   ("ncf_deep", "NeuralCF [128,64,32,16] tower (neural_cf.py:75-90 any depth)"))


def run_child(argv, timeout):
    """One bench.py child process; returns its JSON line (None on failure, logged)."""
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    cmd = [sys.executable, os.path.abspath(__file__), *argv]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env)
    except subprocess.TimeoutExpired:
        log(f"child {' '.join(argv)} timed out")
        return None
    lines = [ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")]
    if r.returncode != 0 or not lines:
        log(f"child {' '.join(argv)} failed rc={r.returncode}: {r.stderr[-800:]}")
        return None
    return json.loads(lines[-1])


def gather_ceiling(gathered_bytes, avg_kernel_ms):
    """The SpMM layer's gathered rows (half from each table) against the measured 256-B
    row-gather rates: perfect L2 locality (`frac`) and the same gathers in uniformly random
    order (`vs_uniform_random`: what the walks' column order buys)."""
    ach = gathered_bytes / (avg_kernel_ms * 1e-3) / 1e12                      # TB/s
    uni = 1.0 / (0.5 / ITEM_TABLE_GATHER_TBPS + 0.5 / USER_TABLE_GATHER_TBPS)  # TB/s
    return {"bytes": gathered_bytes, "achieved_TBps": round(ach, 3),
            "l2_rate_TBps": L2_GATHER_TBPS, "uniform_random_TBps": round(uni, 3),
            "ms": round(gathered_bytes / (L2_GATHER_TBPS * 1e12) * 1e3, 4),
            "frac": round(ach / L2_GATHER_TBPS, 4),
            "vs_uniform_random": round(ach / uni, 4),
            "source": "tools/gather_probe.hip, profiles/r4x_gather_probe.txt"}


def compact_line(line):
    """The fields of a workload's line that the headline line repeats under `other_configs`
    (its full line is printed on its own stdout line before the headline): small enough that
    the headline JSON line with every workload fits a driver's 8 KB output tail."""
    r = line.get("roofline") or {}
    out = {"value": line["value"], "ms_per_step": line["ms_per_step"], "steps": line["steps"],
           "dtype": line["dtype"], "baseline_config": line["config"].get("baseline_config"),
           "roofline": {k: r.get(k) for k in ("bound", "kernel", "achieved", "peak", "unit",
                                              "frac", "avg_kernel_ms", "launches",
                                              "algorithmic_per_launch", "traffic")}}
    if r.get("gather_ceiling"):
        out["roofline"]["gather_ceiling"] = {k: r["gather_ceiling"].get(k)
                                             for k in ("bytes", "ms", "frac", "vs_uniform_random")}
    for k in ("cpu_baseline", "exact_fp32", "filtered", "serving_cached_propagation",
              "pipelined_3_streams", "full_propagation_step", "per_pair_lds_route"):
        if line.get(k):
            out[k] = line[k]["value"]
    if line.get("prefilter"):
        out["candidates_per_row"] = line["prefilter"]["candidates_per_row"]
        out["fallback_rows"] = line["prefilter"]["fallback_rows"]
    return out


# workloads whose step is a fraction of a millisecond (MF: ~0.18 ms): 20 steps time ~4 ms,
# where one host hiccup moved a whole line by 60 % (gpurun_out/r11x); their extra lines time
# at least 200 steps
SHORT_STEP_WORKLOADS = ("mf",)
# a headline timed over thousands of steps does not lengthen the child lines with it (ncf_deep:
# 24 ms a step): each times at most this many, and reports its own `steps`
EXTRA_MAX_STEPS = 1000


def run_extras(args):
    """Every other workload's bench line and the B = 1 serve latencies, measured by child
    processes after the headline line's timed region (one process per workload: each
    holds only its own tables).  Each full line is printed on stdout as
    `workload_line <name> {...}` (the headline stays the one line that starts with "{");
    configs[2] (lightgcn) last, right above the headline, so a tail of the output keeps it."""
    out, lat, full = {}, {}, {}
    for w, what in EXTRA_WORKLOADS:
        steps, warmup = ((5, 1) if w == "widedeep" else
                         (min(args.steps, EXTRA_MAX_STEPS), args.warmup))
        if w in SHORT_STEP_WORKLOADS:  # sub-ms steps: a longer timed region (host jitter)
            steps, warmup = max(steps, 200), max(warmup, 20)
        argv = ["--workload", w, "--steps", str(steps), "--warmup", str(warmup), "--full",
                "--no-extras"]
        if args.no_cpu_baseline:
            argv.append("--no-cpu-baseline")
        t0 = time.perf_counter()
        line = run_child(argv, 900)
        log(f"extra workload {w}: {time.perf_counter() - t0:.1f}s")
        if line is not None:
            line["config"]["baseline_config"] = what
            full[w] = line
            out[w] = compact_line(line)
    # pruning robustness: the certified NCF / MF steps on weights less
    # favourable to the pruning than the init -- NCF "personal" (user-specific best items) and
    # the trained-like stress sets; step time, candidates re-scored per row, fallback rows
    rob = {}
    for w, ws in (("ncf", ("personal", "norms", "student_t", "norms+strided")),
                  ("mf", ("norms", "student_t")), ("ncf_deep", ("norms",))):
        for wt in ws:
            wname, _, opt = wt.partition("+")
            st, wu = min(args.steps, EXTRA_MAX_STEPS), args.warmup
            if w in SHORT_STEP_WORKLOADS:
                st, wu = max(st, 200), max(wu, 20)
            line = run_child(["--workload", w, "--weights", wname, "--steps", str(st),
                              "--warmup", str(wu), "--profile-only"]
                             + (["--" + opt] if opt else []), 600)
            log(f"robustness {w} {wt} done")
            if line is not None:
                pf = line.get("prefilter") or {}
                rob.setdefault(w, {})[wt] = {
                    "value": line["value"], "ms_per_step": line["ms_per_step"],
                    "candidates_per_row": pf.get("candidates_per_row"),
                    "fallback_rows": pf.get("fallback_rows"),
                    "strided_sample_rows": pf.get("strided_sample_rows"),
                    "scan_ms": (line.get("roofline") or {}).get("avg_kernel_ms")}
    out["pruning_robustness"] = rob
    for w in ("ncf", "lightgcn"):
        line = run_child(["--latency", "--workload", w, "--steps", "200", "--no-extras"], 600)
        log(f"serve latency {w} done")
        if line is not None:
            print("serve_latency_line " + json.dumps(line), flush=True)
            lat[w] = {k: v["p50"] for k, v in line.items() if isinstance(v, dict) and "p50" in v}
    for w in sorted(full, key=lambda w: w == "lightgcn"):
        print(f"workload_line {w} " + json.dumps(full[w]), flush=True)
    return out, lat


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--workload", default="ncf")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--latency", action="store_true",
                    help="serve-path B=1 latency (p50/p99) instead of the throughput line")
    ap.add_argument("--weights", default="init", choices=["init", "personal", *STRESS_WEIGHTS],
                    help="init: reference init distributions; personal: NCF weights whose "
                         "best items are user-specific (emb_scale 20, biases); norms / "
                         "student_t: trained-like weights (NCF, MF: embedding rows at norms "
                         "50-200 / Student-t(3) weights and biases)")
    ap.add_argument("--strided", action="store_true",
                    help="NCF: HNM_OPT_STRIDED=1, the gated per-user strided sample beside the "
                         "champion sample (pays off on weights whose best items are "
                         "user-specific; costs ~2 %% of the init-weight step)")
    ap.add_argument("--exact", action="store_true",
                    help="exact fp32 scan of every item instead of the certified f16 pre-filter")
    ap.add_argument("--profile-only", action="store_true",
                    help="the headline timed loop only (no exact / filtered / module-surface / "
                         "pipelined / baseline legs): what the rocprofv3 kernel stats in "
                         "profiles/ are collected over, so their averages match `roofline`")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also measure everything else the benchmark "
                         "reports: exact fp32 / filtered / module-surface / pipelined legs, the "
                         "pre-filter counters, the CPU baseline and (default NCF run) the other "
                         "workloads, pruning robustness and B=1 serve latencies.  Without it: "
                         "set up, warm up, time --steps steps, print the result line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned as DIR/scores.npy (float32) "
                         "and DIR/items.npy (float64), [batch, 12] each (rank r > 0 of a "
                         "multi-GPU run: scores_rank<r>.npy / items_rank<r>.npy)")
    ap.add_argument("--no-extras", action="store_true",
                    help="--full, default NCF run only: skip the other workloads' lines and the B=1 "
                         "serve latencies (otherwise measured after the headline, N=1 only)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(args.gpus))

    rank, world, device = setup_dist(args.gpus)
    if args.latency:
        serve_latency(args, device)
        return
    B = args.batch
    t_setup = time.perf_counter()
    if args.exact:
        _lib.set_prefilter(device, False)
    if args.strided:
        _lib.set_option(device, _lib.HNM_OPT_STRIDED, 1)
    wl, info, cpu = build_workload(args.workload, rank, world, device, B, args.exact,
                                   args.weights)
    if args.strided:
        info["strided_sample"] = True
    step, per_launch, bound, kernel = wl["step"], wl["per_launch"], wl["bound"], wl["kernel"]
    # resident user batches: rank-specific, distinct ids
    nb = 4
    batches = [torch.from_numpy(syn.user_batch(syn.HM_USERS, B, seed=100 + 17 * rank + j)).to(device)
               for j in range(nb)]
    torch.cuda.synchronize()
    log(f"[rank {rank}] setup {time.perf_counter() - t_setup:.1f}s")

    for j in range(args.warmup):
        step(batches[j % nb])
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    _lib.enable_timing(device, wl["timing"])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    last = None
    for j in range(args.steps):
        last = step(batches[j % nb])
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    ktime_ms, launches = _lib.kernel_timing(device)
    _lib.enable_timing(device, False)
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, last, rank)
    del last
    # the legs measured beside the headline: --full only, and never with --profile-only
    legs = args.full and not args.profile_only
    pf_rows = pf_cands = pf_fallback = pf_sampled = 0
    if args.full or args.profile_only or info.get("_deep_cert"):
        # pre-filter counters from one extra, untimed step (counting uses atomics); a plain run
        # takes it only for the deep tower, whose kernel and dtype fields depend on it
        _lib.prefilter_stats(device, reset=True)
        _lib.set_option(device, _lib.HNM_OPT_STATS, 1)
        step(batches[0])
        _lib.set_option(device, _lib.HNM_OPT_STATS, 0)
        pf_rows, pf_cands, pf_fallback, pf_sampled = _lib.prefilter_stats(device, reset=True,
                                                                          extended=True)
    exact_rate = None
    if info.get("_deep_cert") and pf_rows and pf_fallback < pf_rows:
        # round 6: the deep tower's certified f16 pre-filter pruned (trained-like weights): the
        # timed kernel is the deep f16 scan; at the init weights the proxy rows predict that its
        # bound cannot prune and the call runs the exact f32-MFMA kernel (every row "fallback")
        kernel = "ncf16_scan_kernel"
        info["scan"] = ("certified f16 pre-filter (the two-layer scan with layer 3 on the matrix "
                        "pipe; bound through |wp3|^T|W3||W2|) + exact deep re-scoring (ncf_cert.hip)")
    elif info.get("_deep_cert") and pf_rows:
        info["scan"] += ("; certified pre-filter tried: its proxy rows predict no pruning at these "
                         "weights (worst-case bound wider than the score spread), exact kernels ran")
    if not legs:
        args.no_extras = args.no_cpu_baseline = True
    per_pair = None
    if info.get("_per_pair_route") and legs:
        # the same step through the per-pair LDS kernel + dense rows + row top-k
        # (HNM_OPT_DEEP_MFMA = 0, bitwise the same lists), reported beside `value`
        _lib.set_option(device, _lib.HNM_OPT_DEEP_MFMA, 0)
        step(batches[0])
        torch.cuda.synchronize()
        tp = time.perf_counter()
        for j in range(2):
            step(batches[j % nb])
        torch.cuda.synchronize()
        per_pair = B * 2 / (time.perf_counter() - tp)
        _lib.set_option(device, _lib.HNM_OPT_DEEP_MFMA, 1)
    if legs and not args.exact and not info.get("_per_pair_route"):
        # the like-for-like fp32 path (HNM_OPT_PREFILTER=0: every pair scored in exact fp32
        # arithmetic), timed the same way on the same batches, reported beside `value`
        _lib.set_prefilter(device, False)
        nexact = min(args.steps, 3 if args.workload == "widedeep" else 10)
        step(batches[0])
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        te = time.perf_counter()
        for j in range(nexact):
            step(batches[j % nb])
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        exact_rate = (time.perf_counter() - te, nexact)
        _lib.set_prefilter(device, True)
    if world > 1:
        on_host = dist.get_backend() == "gloo"
        t = torch.tensor([elapsed, ktime_ms / max(launches, 1)], dtype=torch.float64,
                         device="cpu" if on_host else device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed, avg_kernel_ms = float(t[0]), float(t[1])
    else:
        avg_kernel_ms = ktime_ms / max(launches, 1)

    users_total = B * world * args.steps
    value = users_total / elapsed
    if exact_rate is not None and world > 1:
        on_host = dist.get_backend() == "gloo"
        t = torch.tensor([exact_rate[0]], dtype=torch.float64, device="cpu" if on_host else device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        exact_rate = (float(t[0]), exact_rate[1])
    f16 = kernel in ("ncf16_scan_kernel", "dot16_scan_kernel", "wdc_scan_kernel")
    if bound == "hbm":
        achieved = per_launch / (avg_kernel_ms * 1e-3) / 1e9
        peak, punit = HBM_PEAK_GBS, "GB/s"
    else:
        achieved = per_launch / (avg_kernel_ms * 1e-3) / 1e12
        peak, punit = (F16_MFMA_PEAK_TFLOPS if f16 else FP32_MFMA_PEAK_TFLOPS), "TFLOP/s"
    line = {
        "metric": METRIC,
        "value": round(value, 2),
        "unit": "users/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(elapsed / args.steps * 1e3, 4),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": ("f32" if args.exact or not (f16 or bound == "hbm") else
                  "f16+f32"),
        "data": ("synthetic (PCG64 weights with reference init distributions; H&M shape)"
                 if args.weights == "init" else
                 f"synthetic (PCG64 weights, '{args.weights}' set: bench.py --weights; H&M shape)"),
        "config": {"workload": f"{args.workload}: BASELINE configs[1] NeuralCF dim=64, full H&M "
                               f"shape, batch={B} users/rank, K=12" if args.workload == "ncf"
                   else args.workload,
                   "users": syn.HM_USERS, "items": syn.HM_ITEMS, "batch_per_rank": B, "k": K,
                   "parallelism": f"item-shard{world}" if world > 1 else "single",
                   **{k: v for k, v in info.items() if not k.startswith("_")}},
        "roofline": {"bound": bound, "kernel": kernel,
                     "achieved": round(achieved, 3), "peak": peak, "unit": punit,
                     "frac": round(achieved / peak, 4),
                     "avg_kernel_ms": round(avg_kernel_ms, 4), "launches": launches,
                     "algorithmic_per_launch": per_launch,
                     "traffic": pmc_traffic(args.workload)},
        "cpu_baseline": None,
    }
    if per_pair is not None:
        line["per_pair_lds_route"] = {
            "value": round(per_pair, 2), "unit": "users/s", "vs_value": round(per_pair / value, 4),
            "note": "HNM_OPT_DEEP_MFMA=0: per-pair LDS kernel (dense rows) + row top-k, the round-4 "
                    "deep-tower path; identical lists"}
    issued = ISSUED_F16_FLOP_PER_PAIR.get(args.workload)
    if f16 and issued and not args.exact:
        # f16 MFMA FLOP the scan actually issues per pair (epilogue / split passes included)
        # against the rate a bare f16 MFMA loop sustains on random data at this occupancy:
        # the chip's power limit, not the nominal peak, caps an MFMA-dense scan
        rate = issued * per_launch / ALG_FLOP_PER_PAIR[args.workload] / (avg_kernel_ms * 1e-3) / 1e12
        line["roofline"]["issued"] = {
            "flop_per_pair": issued, "tflops": round(rate, 1),
            "random_data_mfma_rate": RANDOM_DATA_F16_TFLOPS,
            "frac_of_random_data_rate": round(rate / RANDOM_DATA_F16_TFLOPS, 3),
            "source": "tools/mfma_shape_probe.hip, profiles/r2_mfma_shape_probe.txt"}
    if wl.get("gathered"):
        # gather-aware ceiling beside the algorithmic one: every CSR entry gathers one whole
        # d-float row (half of them from each table); measured 256-B row-gather rates above:
        # `frac` against perfect L2 locality, `vs_uniform_random` against the same gathers in
        # random order (what the walks' column order buys)
        line["roofline"]["gather_ceiling"] = gather_ceiling(wl["gathered"], avg_kernel_ms)
    if "_serving" in info and rank == 0 and world == 1 and legs:
        # serving rate with the propagation computed once (weights unchanged between calls);
        # reported beside `value`, never as it
        serve = info["_serving"]()
        torch.cuda.synchronize()
        ts = time.perf_counter()
        for j in range(args.steps):
            serve(batches[j % nb])
        torch.cuda.synchronize()
        line["serving_cached_propagation"] = {
            "value": round(B * args.steps / (time.perf_counter() - ts), 2), "unit": "users/s",
            "note": "top-K scan only, propagation computed once outside the timed loop"}
    if exact_rate is not None:
        line["exact_fp32"] = {
            "value": round(B * world * exact_rate[1] / exact_rate[0], 2), "unit": "users/s",
            "steps": exact_rate[1],
            "note": "same step with HNM_OPT_PREFILTER=0: every (user, item) pair in exact fp32"}
    if "_filtered" in info and not args.exact and legs:
        # purchase-history filter (the reference's filter_items / serve.py:350-352): every
        # user's history = its interactions in the synthetic H&M transactions (the LightGCN
        # graph's edges, mean 23.2 items), held on the device as a UserHistory; each step
        # gathers the batch's rows on the GPU (hnm_mask_gather_csr) and masks them in-kernel
        tH = time.perf_counter()
        hu, hi_ = syn.interactions(syn.HM_USERS, syn.HM_ITEMS, syn.HM_INTERACTIONS, seed=2)
        hist = UserHistory.from_interactions(hu, hi_, syn.HM_USERS, syn.HM_ITEMS, device)
        del hu, hi_
        t_hist = time.perf_counter() - tH
        fstep = info["_filtered"](hist)
        nf = min(args.steps, 10 if args.workload == "lightgcn128" else 20)
        rate = timed_rate(fstep, batches, nf, world, B)
        per_row = float((hist.hist_ptr[batches[0] + 1] - hist.hist_ptr[batches[0]]).float().mean())
        line["filtered"] = {
            "value": round(rate, 2), "unit": "users/s", "steps": nf,
            "vs_unfiltered": round(rate / value, 4),
            "history_items_per_user": round(per_row, 2),
            "history": f"device-resident CSR of all {syn.HM_USERS} users' interactions "
                       f"({hist.nnz} unique items; built once in {t_hist:.1f}s, outside timing)",
            "note": "same step with each user's purchase history masked (-inf) in-kernel; "
                    "mask rows gathered on the GPU per step"}
        if "_module" in info and world == 1:
            m = info["_module"]
            host = [b.cpu() for b in batches]
            ms = {}
            ms["recommend_with_scores_device_ids"] = timed_rate(
                lambda u: m.recommend_with_scores(u), batches, nf, world, B)
            ms["recommend_host_ids"] = timed_rate(
                lambda j: m.recommend(host[j]), list(range(len(host))), nf, world, B)
            ms["recommend_with_scores_history_filter"] = timed_rate(
                lambda u: m.recommend_with_scores(u, filter_items=hist), batches, nf, world, B)
            out = {k: round(v, 2) for k, v in ms.items()}
            out["vs_value"] = {k: round(v / value, 4) for k, v in ms.items()}
            out["note"] = (
                "the reference's own module surface (model.recommend / recommend_with_scores, what "
                "serve.py and evaluation call) timed on the same batches: device ids are range-"
                "checked by the kernels' error word (one stream sync per call, IndexError raised "
                "at the call); host ids are checked on the host (no sync; includes the 32 KB "
                "H2D copy of the ids)" + (
                    "; LightGCN's module caches forward() (propagation once, reused while the "
                    "weights are unchanged), so these rates exclude the per-call propagation "
                    "`value` includes" if args.workload.startswith("lightgcn") else ""))
            line["module_surface"] = out
        del hist
    if (world == 1 and args.workload in ("ncf", "mf", "lightgcn") and not args.exact
            and legs):
        # serving throughput with independent batches overlapped on 3 HIP streams (the small
        # per-call kernels and re-scoring of one batch run beside another batch's scan);
        # reported beside `value` (one batch in flight), never as it
        try:
            np_ = min(args.steps * 2, 60)
            prate, same = pipelined_rate(step, batches, np_, B)
            line["pipelined_3_streams"] = {
                "value": round(prate, 2), "unit": "users/s", "steps": np_,
                "vs_value": round(prate / value, 4), "bitwise_equal_to_sequential": same,
                "note": "3 worker threads, each with its own torch stream and hnm_ctx, full "
                        "recommend() calls on independent batches; what a threaded server gets"}
        except Exception as e:  # reported, never fatal
            log(f"pipelined leg failed: {e!r}")
    if world > 1 and "_user_sharded" in info and legs:
        # SURVEY §8(e)'s comparison layout: every rank holds the whole catalogue and scores
        # only its own B users (no collective); the same batches, clock and max over ranks
        try:
            us = info["_user_sharded"]()
            urate = timed_rate(us, batches, min(args.steps, 20), world, B)
            line["user_sharded_layout"] = {
                "value": round(urate, 2), "unit": "users/s", "vs_value": round(urate / value, 4),
                "note": "replicated item tables, each rank its own 4,096 users over all items, no "
                        "exchange: SURVEY §8(e)'s upper-bound layout, reported beside the "
                        "item-sharded `value`"}
            del us
        except Exception as e:  # reported, never fatal
            log(f"user-sharded leg failed: {e!r}")
    if "_full_step" in info and legs:
        full = info["_full_step"]
        full(batches[0])
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        tf = time.perf_counter()
        nfull = min(args.steps, 10)
        for j in range(nfull):
            full(batches[j % nb])
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        line["full_propagation_step"] = {
            "value": round(B * world * nfull / (time.perf_counter() - tf), 2), "unit": "users/s",
            "note": "same step with the whole-graph 3-layer propagation (all 1.48M rows per layer)"}
    if pf_rows:
        line["prefilter"] = {"rows": pf_rows, "candidates_per_row": round(
            pf_cands / max(pf_rows - pf_fallback, 1), 1), "fallback_rows": pf_fallback,
            "strided_sample_rows": pf_sampled,
            "outputs": "bit-identical to the exact fp32 scan (tests/test_gpu_prefilter.py)"}
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        try:
            line["cpu_baseline"] = cpu_baseline(cpu)
        except Exception as e:  # baseline is reported, never fatal
            log(f"cpu baseline failed: {e!r}")
    if (rank == 0 and world == 1 and args.workload == "ncf" and not args.no_extras
            and not args.exact and args.weights == "init"):
        others, lat = run_extras(args)
        line["other_configs"] = others
        line["serve_latency_b1_p50_ms"] = lat
        # the headline's own explanatory notes stay in its full line (printed above): the
        # line the driver parses must fit its output tail together with every workload
        print("workload_line ncf " + json.dumps(line), flush=True)
        for v in line.values():
            if isinstance(v, dict):
                v.pop("note", None)
                v.pop("history", None)
                v.pop("source", None)
        if isinstance(line.get("cpu_baseline"), dict):
            line["cpu_baseline"]["sample"] = line["cpu_baseline"]["sample"][:90]
    if rank == 0:
        print(json.dumps(line), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
