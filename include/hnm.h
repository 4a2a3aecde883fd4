/* libhnm_mi355x — C ABI of the MI355X-native top-N scoring hot path.
 *
 * Drop-in boundary for hyunlord/hnm_recommendation @ 2025-07-25 (reference paths below are
 * relative to that repo).  The reference has no FFI: its boundary is the PyTorch module
 * surface `NeuralCF` / `LightGCN` / `WideDeep` / `MatrixFactorization` with `forward`,
 * `predict_all_items`, `recommend` and `set_graph`.  Each entry point
 * below replaces the ATen / torch_sparse work one of those methods does; the Python
 * mirror in `hnm_recommendation_amd/models/` binds them with ctypes.
 *
 * Conventions
 *  - Every pointer argument is a DEVICE pointer owned by the caller (the torch caching
 *    allocator); the library never frees caller memory.  Shapes are row-major, fp32
 *    tables with an explicit leading dimension, int64 ids.  An empty batch (B == 0 or
 *    n == 0) is a no-op whose per-row pointers (ids, outputs, bounds) may be NULL -- what
 *    torch hands over for an empty tensor.
 *  - Calls are asynchronous and stream-ordered on the ctx stream (hnm_ctx_set_stream:
 *    torch's current stream).  A ctx is not re-entrant: use one per (device, thread)
 *    (the Python layer does: one per thread, destroyed when the thread exits).  Switching
 *    a ctx to another stream queues the new stream behind the work already issued on the
 *    old one (an event recorded on the old stream, waited on by the new one; no host sync),
 *    so the ctx workspace is never reused while a kernel on the previous stream still reads
 *    it.  A stream handed to hnm_ctx_set_stream must therefore stay alive until the ctx has
 *    been switched away from it (torch's pooled streams always do; a caller-owned
 *    hipStream_t / torch.cuda.ExternalStream must outlive that switch).
 *  - Device binding: a ctx belongs to the device it was created on.  Every entry that takes
 *    a ctx switches the calling thread to ctx->device for its duration (workspace allocation,
 *    events, launches, the null stream when no stream was set) and restores the caller's
 *    current device before returning; hnm_ctx_create leaves the current device unchanged.  So
 *    one host thread may drive ctxs of several GPUs; the pointers passed to a call must live on
 *    that ctx's device, and a stream set with hnm_ctx_set_stream must belong to it.
 *  - Status: 0 on success, negative on error; hnm_last_error() holds a thread-local
 *    message.  No C++ exception crosses the ABI.
 *  - Out-of-range user/item ids never fault: the row is skipped (index -1 / NaN) and the
 *    ctx error word records it; hnm_ctx_check() synchronizes and returns HNM_EOOB, which
 *    the Python layer raises as IndexError (reference: nn.Embedding IndexError).
 *  - Top-K order is (score desc, item index asc); -inf (filtered) items rank last and are
 *    returned only when fewer than k finite scores exist (torch.topk semantics).
 */
#ifndef HNM_H_
#define HNM_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HNM_ABI_VERSION 1

typedef int32_t hnm_status;
enum {
  HNM_OK = 0,
  HNM_EINVAL = -1,       /* bad argument / shape */
  HNM_EOOB = -2,         /* an id was out of range (reported by hnm_ctx_check) */
  HNM_EHIP = -3,         /* HIP runtime error */
  HNM_ENOMEM = -4,       /* workspace allocation failed */
  HNM_EUNSUPPORTED = -5, /* shape outside what the kernels are built for */
  HNM_ECOLL = -6         /* RCCL error (hnm_ctx_rccl_init, hnm_topk_allgather_merge_f32) */
};

typedef struct hnm_ctx hnm_ctx;
typedef struct hnm_spmm_plan hnm_spmm_plan;

int hnm_abi_version(void);
const char* hnm_last_error(void);

/* ---- context ------------------------------------------------------------------------ */
hnm_status hnm_ctx_create(int device, hnm_ctx** out);
hnm_status hnm_ctx_destroy(hnm_ctx* ctx);
hnm_status hnm_ctx_set_stream(hnm_ctx* ctx, void* hip_stream);
hnm_status hnm_ctx_reserve(hnm_ctx* ctx, size_t bytes);   /* pre-grow workspace */
hnm_status hnm_ctx_check(hnm_ctx* ctx);                   /* sync; HNM_EOOB if flagged */
hnm_status hnm_ctx_num_cus(hnm_ctx* ctx, int* out);
/* Close an open two-phase top-K call (hnm_*_topk_begin_f32 without its _finish), e.g.
 * after a failed cross-shard exchange; the begin phase's tables are discarded. */
hnm_status hnm_ctx_abort_pending(hnm_ctx* ctx);
/* Options.  HNM_OPT_PREFILTER (default 1): NCF and dot-product top-K scan the catalogue
 * with the certified f16 pre-filter and re-score the surviving candidates in exact fp32
 * (results identical to the fp32 scan); 0 = exact fp32 scan of every item.  Calls outside
 * the pre-filter's range take the exact scan whatever the option: fewer than 8,192 items or
 * than 64 k, k > 64, the dot path with d > 128 or with an f16 item copy of 2 GiB or more
 * (16.7M items at d <= 64, 8.3M at d <= 128), NCF layer widths beyond 64 / 32 or 33.5M items. */
enum { HNM_OPT_PREFILTER = 1,
       HNM_OPT_STATS = 3,      /* 1: count pre-filter candidates / fallback rows (diagnostics) */
       HNM_OPT_STRIDED = 4,    /* NeuralCF certified top-K: 1 = the gated per-user strided
                                  sample may run (weights whose best items are user-specific:
                                  bench "norms" 3.68 -> 3.09 ms a step); 0 (default) = the
                                  champion sample alone (the gate costs ~2 % of the init-weight
                                  step) */
       HNM_OPT_DEEP_MFMA = 5   /* deep NeuralCF towers (hnm_ncf_deep_*): 1 (default) = the
                                  fp32-MFMA tile kernel where the tower fits it (widths <= 128,
                                  mf <= 128, weight image + tiles within a CU's 160 KB of
                                  LDS); 0 = the per-pair LDS kernel everywhere (same scores
                                  bitwise: the A/B and parity switch).  hnm_ncf_deep_route
                                  tells which one a tower takes */,
       HNM_OPT_LINEAR_MFMA = 6 /* hnm_linear_rows_f32 (every per-call layer-1 projection): 1
                                  (default) = the fp32-MFMA kernel where K % 32 == 0 (exact fp32
                                  fma chain in k order: bitwise the VALU kernel); 0 = the VALU
                                  kernel everywhere (the A/B and parity switch) */ };
/* NeuralCF certified top-K, two-layer towers up to 64 wide with h0 a multiple of 32 and 16-B
 * aligned tables: 1 (default) = one launch builds the per-call tables (P_u, wp * g_u, Q_i) and
 * the bound statistics of their rows; 0 = the separate projection, gather and statistics
 * launches (same tables and results bitwise: the A/B and parity switch) */
#define HNM_OPT_NCF_TABLES 7
/* NeuralCF certified top-K, two-layer towers: the f16 scan's layer 2 and GMF on
 * v_mfma_f32_16x16x32_f16 (1, default) or on v_mfma_f32_32x32x16_f16 (0).  Both layouts satisfy
 * the same certified bound, so every returned id and score is bitwise the same (the A/B and
 * parity switch); the deep towers' scan ignores it. */
#define HNM_OPT_SCAN_SHAPE 8
/* NeuralCF certified top-K, two-layer towers on the 16x16x32 layout (HNM_OPT_SCAN_SHAPE 1): the
 * threshold pass of the f16 scan runs its user-pair loop software-pipelined by hand -- the next
 * pair's P~ reads and B operands formed under this pair's layer-2 MFMAs, that block at a raised
 * wave priority -- (1, default) or as the compiler schedules the plain loop (0).  The same MFMAs on the same operands in the same chains, so every
 * returned id and score is bitwise the same (the A/B and parity switch); layout 0 and the deep
 * towers' scan ignore it. */
#define HNM_OPT_SCAN_PIPE 9
/* NeuralCF certified top-K, two-layer towers on the 16x16x32 layout (HNM_OPT_SCAN_SHAPE 1): the
 * f16 scan's epilogue wm . relu(H~) runs as 2 v_smfmac_f32_16x16x64_f16 a user pair and tile --
 * the converted accumulators of the pair's two users interleaved into one B operand of K = 64, wm
 * as an A operand with exact 2:4 structured sparsity -- (1, default) or as the 4 dense
 * v_mfma_f32_16x16x32_f16 (0).  The same products accumulated in fp32 in another order,
 * within the same certified bound, so every returned id and score is bitwise the same (the A/B
 * and parity switch); candidate counts may differ by a test value next to a threshold.  Layout 0
 * and the deep towers' scan ignore it. */
#define HNM_OPT_SCAN_SPARSE 10
/* NeuralCF certified top-K, two-layer towers on the 16x16x32 layout with the sparse epilogue
 * (HNM_OPT_SCAN_SHAPE 1 and HNM_OPT_SCAN_SPARSE 1), every pass of a call alike: the epilogue's A
 * operand holds wm in rows 0, 4, 8 and 12 (row 4 (2 user + item half)), so the pair's 64 test
 * values lie in one accumulator register of all 64 lanes, lane 32 user + item, and the threshold
 * test is one compare whose result is the pass mask (1, default), or in rows 0-3, the values in
 * four registers of lanes 0-15 and the test four compares (0).  The same products in the same
 * order: test values, candidate buffers and every returned id and score are bitwise the same (the
 * A/B and parity switch).  Ignored where either of the two options above is 0 and by the deep
 * towers' scan. */
#define HNM_OPT_SCAN_ROW0 11
hnm_status hnm_ctx_set_option(hnm_ctx* ctx, int option, int64_t value);
/* Pre-filter counters since the last reset (counted only while HNM_OPT_STATS is 1): out[0]
 * rows scored, out[1] candidates re-scored in fp32, out[2] rows that took the exact fallback
 * scan.  The sample-threshold path of hnm_dot_topk_f32 (pre-filter off, >= 8,192 items) counts
 * the same way: its rows, the candidates its select kernel ranks, the rows whose candidate buffer
 * overflowed (or held fewer than k) and took the LIST fallback.  Synchronizes the whole DEVICE (not the ctx stream), so it may be called on a ctx
 * another thread owns; counts of calls that thread issues while this runs may land before or
 * after a reset (totals are exact for threads that are idle meanwhile). */
hnm_status hnm_ctx_prefilter_stats(hnm_ctx* ctx, int64_t* out, int reset);
/* The same counters, the first n of 7: out[3] = rows whose bound also used the per-user strided
 * sample (NeuralCF: gated on when it is predicted to save re-scoring); out[4] / out[5] = the
 * last NeuralCF call's gate inputs: candidates its proxy rows would re-score with the champion
 * bound alone / with the strided sample's bound too (diagnostics); out[6] = Wide&Deep rows whose
 * certified cascade refined best first in two phases (more survivors than its first phase
 * takes). */
hnm_status hnm_ctx_prefilter_stats_ex(hnm_ctx* ctx, int64_t* out, int n, int reset);
/* Dominant-kernel timer: while on, calls record HIP events on the ctx stream around their
 * main kernel; `mask` selects the class: 1 = the scoring / scan kernel of every top-K or
 * dense call, 2 = each LightGCN propagation layer (SpMM), 3 = both.  hnm_ctx_timing()
 * syncs, returns the summed kernel time and the number of timed launches, and resets.
 * Enabling creates 1,024 event pairs up front (more are created only past that many timed
 * launches), so a timed loop records without creating events.  (bench.py's live roofline
 * figures.) */
hnm_status hnm_ctx_enable_timing(hnm_ctx* ctx, int mask);
hnm_status hnm_ctx_timing(hnm_ctx* ctx, double* total_ms, int64_t* launches);

/* ---- a1: embedding row gather ------------------------------------------------------
 * out[b, :d] = table[ids[b], :d].  Replaces nn.Embedding.__call__ at
 * neural_cf.py:155-156, lightgcn.py:199, wide_deep.py:207. */
hnm_status hnm_gather_rows_f32(hnm_ctx* ctx, const float* table, int64_t rows, int64_t ld,
                               int d, const int64_t* ids, int64_t n, float* out,
                               int64_t ldo);

/* ---- per-row projection used to decompose the first MLP layer --------------------
 * Y[r, c(n)] = sum_k X[x(r), k] * W[n, k] (+ bias[n]),  n < N, k < K.
 * x(r) = ids ? ids[r] : r (ids bounded by x_rows);  c(n) = n, or with pair_permute
 * c(n) = (n & 1) * (ldy / 2) + (n >> 1) — the lane-half layout the MFMA kernels read.
 * W has leading dimension ldw (a column slice of a Linear weight, e.g. the user or the
 * item half of mlp_layers.0.weight, neural_cf.py:85-87 / wide_deep.py:128). */
hnm_status hnm_linear_rows_f32(hnm_ctx* ctx, const float* X, int64_t ldx, const int64_t* ids,
                               int64_t x_rows, int64_t M, int K, const float* W,
                               int64_t ldw, const float* bias, int N, float* Y, int64_t ldy,
                               int pair_permute);

/* ---- a7 + a11 + a12: dot-product scoring fused with filter and top-K ---------------
 * s[b, i] = user_tab[user_ids[b]] . item_tab[i] (+ user_bias[user_ids[b]]) (+ item_bias[i])
 *           (+ const_bias[0]); masked (b, i) -> -inf; top-k per row.
 * LightGCN.predict_all_items + recommend (lightgcn.py:188-204, 332-358) and
 * MatrixFactorization (matrix_factorization.py:108-131, 220-246).
 * mask: CSR over the batch rows (mask_ptr[B+1], mask_idx sorted ascending per row) or NULL.
 * d <= 128, d % 4 == 0, 16-B aligned tables.  Fused path: k <= 64 (larger k: dense
 * scores + hnm_topk_rows_f32). */
hnm_status hnm_dot_topk_f32(hnm_ctx* ctx, const float* user_tab, int64_t num_users,
                            int64_t ldu, const int64_t* user_ids, int64_t B,
                            const float* item_tab, int64_t num_items, int64_t ldi, int d,
                            const float* user_bias, const float* item_bias,
                            const float* const_bias, const int64_t* mask_ptr,
                            const int32_t* mask_idx, int k, float* out_val,
                            int64_t* out_idx);
/* Two-phase hnm_dot_topk_f32 for item-sharded serving: as hnm_ncf_topk_begin_f32 /
 * _finish_f32 (lower bounds in real score units, biases included). */
hnm_status hnm_dot_topk_begin_f32(hnm_ctx* ctx, const float* user_tab, int64_t num_users,
                                  int64_t ldu, const int64_t* user_ids, int64_t B,
                                  const float* item_tab, int64_t num_items, int64_t ldi, int d,
                                  const float* user_bias, const float* item_bias,
                                  const float* const_bias, const int64_t* mask_ptr,
                                  const int32_t* mask_idx, int k, float* lower_bound);
/* The begin phase with each row's k best certified sample lower bounds [B, k] (distinct
 * items, real units, descending, -inf padded; as hnm_ncf_topk_begin_lists_f32): the caller
 * all-gathers them over the item shards and passes the k-th best of the union to finish. */
hnm_status hnm_dot_topk_begin_lists_f32(hnm_ctx* ctx, const float* user_tab, int64_t num_users,
                                        int64_t ldu, const int64_t* user_ids, int64_t B,
                                        const float* item_tab, int64_t num_items, int64_t ldi,
                                        int d, const float* user_bias, const float* item_bias,
                                        const float* const_bias, const int64_t* mask_ptr,
                                        const int32_t* mask_idx, int k, float* lower_lists);
hnm_status hnm_dot_topk_finish_f32(hnm_ctx* ctx, const float* user_tab, int64_t num_users,
                                   int64_t ldu, const int64_t* user_ids, int64_t B,
                                   const float* item_tab, int64_t num_items, int64_t ldi, int d,
                                   const float* user_bias, const float* item_bias,
                                   const float* const_bias, const int64_t* mask_ptr,
                                   const int32_t* mask_idx, int k, const float* lower_bound,
                                   int short_ok, float* out_val, int64_t* out_idx);
/* Diagnostics of the certified f16 pre-filter of hnm_dot_topk_f32 (no reference
 * counterpart): approx[b, i] = the f16 scan's score (biases included), bound[b] = the
 * row's error bound; |approx - exact| <= bound for every item (tests check it). */
hnm_status hnm_dot_prefilter_debug_f32(hnm_ctx* ctx, const float* user_tab, int64_t num_users,
                                       int64_t ldu, const int64_t* user_ids, int64_t B,
                                       const float* item_tab, int64_t num_items, int64_t ldi,
                                       int d, const float* user_bias, const float* item_bias,
                                       const float* const_bias, float* approx, int64_t lda,
                                       float* bound);
/* Dense variant: out[b, i] (ldo >= num_items), the predict_all_items matrix. */
hnm_status hnm_dot_scores_f32(hnm_ctx* ctx, const float* user_tab, int64_t num_users,
                              int64_t ldu, const int64_t* user_ids, int64_t B,
                              const float* item_tab, int64_t num_items, int64_t ldi, int d,
                              const float* user_bias, const float* item_bias,
                              const float* const_bias, float* out, int64_t ldo);

/* Pairwise variant: out[n] = user_tab[user_ids[n]] . item_tab[item_ids[n]] + biases
 * (LightGCN.predict lightgcn.py:166-186, MatrixFactorization.forward :80-106). */
hnm_status hnm_pair_dot_f32(hnm_ctx* ctx, const float* user_tab, int64_t num_users,
                            int64_t ldu, const float* item_tab, int64_t num_items, int64_t ldi,
                            int d, const int64_t* user_ids, const int64_t* item_ids, int64_t n,
                            const float* user_bias, const float* item_bias,
                            const float* const_bias, float* out);

/* ---- a3 + a4: NeuralCF --------------------------------------------------------------
 * Reference layout (state_dict of neural_cf.py:56-67):  mlp_dims = [2*h0, h1, h2].
 *   s = wp[:mf].(g_u * g_i) + wp[mf:].relu(W2 relu(W1 [m_u; m_i] + b1) + b2) + bp
 * Requires mf <= 128, h1 <= 128, h2 <= 32 (the default 64 / [128,64,32] config). */
typedef struct {
  const float* gmf_user;   /* [num_users, mf] */
  const float* gmf_item;   /* [num_items, mf] */
  const float* mlp_user;   /* [num_users, h0] */
  const float* mlp_item;   /* [num_items, h0] */
  const float* w1;         /* [h1, 2*h0]  mlp_layers.0.weight */
  const float* b1;         /* [h1] */
  const float* w2;         /* [h2, h1]    mlp_layers.3.weight */
  const float* b2;         /* [h2] */
  const float* wp;         /* [mf + h2]   prediction_layer.weight */
  const float* bp;         /* [1]         prediction_layer.bias */
  int64_t num_users;
  int64_t num_items;
  int32_t mf;
  int32_t h0;
  int32_t h1;
  int32_t h2;
  /* Optional (NULL: computed per call; ZERO-INITIALISE the struct so an unset field is NULL --
   * a non-NULL pointer is used as the table, and one that is not 16-B aligned is refused with
   * HNM_EINVAL): the item half of layer 1 for THESE num_items rows,
   * W1[:, h0:] m_i pair-permuted, [num_items, 64] (h1 <= 64 and mf <= 64) or [num_items, 128],
   * as hnm_ncf_item_proj_f32 writes it -- for callers whose item tables and W1 stay fixed
   * between calls (a server); a row shard points at its first row. */
  const float* item_proj;
} hnm_ncf_weights;

/* out = the item projection hnm_ncf_weights.item_proj takes (zero padded columns). */
hnm_status hnm_ncf_item_proj_f32(hnm_ctx* ctx, const hnm_ncf_weights* w, float* out);

hnm_status hnm_ncf_topk_f32(hnm_ctx* ctx, const hnm_ncf_weights* w, const int64_t* user_ids,
                            int64_t B, const int64_t* mask_ptr, const int32_t* mask_idx,
                            int k, float* out_val, int64_t* out_idx);
/* Two-phase hnm_ncf_topk_f32 for item-sharded serving (no reference counterpart: the
 * reference is single-device).  begin: per-call tables + each row's
 * certified lower bound of its exact k-th best score over this call's items, lower_bound[B]
 * (real score units; -inf when unknown, e.g. with the pre-filter off).  The caller may
 * replace the bounds by any valid lower bounds -- the max over the item shards of a node --
 * then finish completes the fused top-k with them; short_ok = 1 lets a row keep fewer than
 * k entries (padded with -inf / -1: another shard holds its better items): the row is then a
 * prefix of its exact top-k that holds every item scoring at or above the row's bound, and (when
 * out_val is given) nothing below it unless the row took the exact fallback scan.  Nothing else may
 * use the ctx between begin and finish (HNM_EINVAL otherwise). */
hnm_status hnm_ncf_topk_begin_f32(hnm_ctx* ctx, const hnm_ncf_weights* w,
                                  const int64_t* user_ids, int64_t B, const int64_t* mask_ptr,
                                  const int32_t* mask_idx, int k, float* lower_bound);
/* As hnm_ncf_topk_begin_f32, but for each row the k best certified lower bounds of the
 * sample's items, lower_lists[B, k] (real units, descending, -inf padded; all -inf when
 * unknown): bounds of k DISTINCT items' exact scores, so the k-th best of the union of every
 * item shard's lists is a lower bound of the row's global k-th best -- as tight as a
 * single-device call's -- where the max of the shards' single bounds is only each shard's own
 * k-th.  finish then takes that merged bound. */
hnm_status hnm_ncf_topk_begin_lists_f32(hnm_ctx* ctx, const hnm_ncf_weights* w,
                                        const int64_t* user_ids, int64_t B,
                                        const int64_t* mask_ptr, const int32_t* mask_idx, int k,
                                        float* lower_lists);
hnm_status hnm_ncf_topk_finish_f32(hnm_ctx* ctx, const hnm_ncf_weights* w,
                                   const int64_t* user_ids, int64_t B, const int64_t* mask_ptr,
                                   const int32_t* mask_idx, int k, const float* lower_bound,
                                   int short_ok, float* out_val, int64_t* out_idx);
hnm_status hnm_ncf_scores_f32(hnm_ctx* ctx, const hnm_ncf_weights* w,
                              const int64_t* user_ids, int64_t B, float* out, int64_t ldo);
/* Diagnostics of the certified pre-filter (no reference counterpart): approx[b, i] = the
 * f16 scan's score of item i without the output bias bp, bound[b, i] = the pair's error
 * bound (both [B, lda]); |approx + bp - exact| <= bound holds for every pair (tests check
 * it on the full catalogue). */
hnm_status hnm_ncf_prefilter_debug_f32(hnm_ctx* ctx, const hnm_ncf_weights* w,
                                       const int64_t* user_ids, int64_t B, float* approx,
                                       int64_t lda, float* bound);
/* NeuralCF.forward(user_ids, item_ids) (neural_cf.py:112-141): out[n]. */
hnm_status hnm_ncf_pair_scores_f32(hnm_ctx* ctx, const hnm_ncf_weights* w,
                                   const int64_t* user_ids, const int64_t* item_ids,
                                   int64_t n, float* out);

/* NeuralCF with an MLP tower of any depth (neural_cf.py:75-90: one Linear -> ReLU per
 * consecutive pair of mlp_dims, any length >= 2), exact fp32 -- the path for towers the fused
 * kernels above do not cover (they take the default two-layer tower).  w[l] / b[l] =
 * mlp_layers.{3l}.weight [dims[l+1], dims[l]] / bias; dims[0] = 2 x the MLP embedding width;
 * widths dims[1..nl] <= 512, nl <= 8.
 * item_ids NULL: dense scores out[b * ldo + i] for every item (ldo >= num_items:
 * predict_all_items; recommend = hnm_ncf_deep_topk_f32).  item_ids set: pair scores
 * out[n] = s(user_ids[n], item_ids[n]), n < B (forward).  Out-of-range ids flag HNM_EOOB
 * (hnm_ctx_check) and score NaN. */
typedef struct {
  const float* gmf_user;   /* [num_users, mf] */
  const float* gmf_item;   /* [num_items, mf] */
  const float* mlp_user;   /* [num_users, dims[0] / 2] */
  const float* mlp_item;   /* [num_items, dims[0] / 2] */
  const float* w[8];
  const float* b[8];
  const float* wp;         /* [mf + dims[nl]] prediction_layer.weight */
  const float* bp;         /* [1] */
  int64_t num_users;
  int64_t num_items;
  int32_t mf;
  int32_t nl;              /* Linear layers = len(mlp_dims) - 1 */
  int32_t dims[9];
} hnm_ncf_deep_weights;

hnm_status hnm_ncf_deep_scores_f32(hnm_ctx* ctx, const hnm_ncf_deep_weights* w,
                                   const int64_t* user_ids, int64_t B, const int64_t* item_ids,
                                   float* out, int64_t ldo);
/* Fused top-k of a deep tower (NeuralCF.recommend, neural_cf.py:300-326, with the -inf filter
 * and torch.topk of neural_cf.py:316-324): (score desc, item asc), scores bitwise those of
 * hnm_ncf_deep_scores_f32, 1 <= k <= 64, mask as hnm_ncf_topk_f32.  Three-layer towers
 * [2 h0, h1 <= 64, h2 <= 32, h3 <= 16] with mf <= 64 (a multiple of 4) take the certified f16
 * pre-filter when HNM_OPT_PREFILTER is on and the call is in its range (B >= 16, >= 8,192 items,
 * >= 64 k): the two-layer tower's f16 scan with a third layer on the matrix pipe, its worst-case
 * bound carried through |wp3|^T |W3| |W2|, exact fp32 re-scoring of the survivors by the deep
 * chain (outputs bitwise the exact path's); rows the bound cannot serve take the exact scan
 * (their count is read back: the call synchronizes its stream).  Otherwise towers with every
 * width dims[1..nl] <= 128 and mf <= 128 take the fp32-MFMA scan that keeps per-partition top-k
 * lists (no [B, I] score matrix); wider towers (and towers whose packed weights do not fit a
 * CU's LDS, e.g. three 128 x 128 layers) score dense rows per user chunk in the workspace and
 * take the row top-k kernel. */
hnm_status hnm_ncf_deep_topk_f32(hnm_ctx* ctx, const hnm_ncf_deep_weights* w,
                                 const int64_t* user_ids, int64_t B, const int64_t* mask_ptr,
                                 const int32_t* mask_idx, int k, float* out_val,
                                 int64_t* out_idx);
/* Which exact-path kernel hnm_ncf_deep_scores_f32 (dense) / hnm_ncf_deep_topk_f32 take for this
 * tower on this ctx: 0 = per-pair LDS kernel (+ dense-chunk row top-k), 1 = fp32-MFMA tile kernel
 * (+ fused partition lists).  Honours HNM_OPT_DEEP_MFMA.  No launch, no sync. */
hnm_status hnm_ncf_deep_route(hnm_ctx* ctx, const hnm_ncf_deep_weights* w, int* route);
/* Diagnostics of that pre-filter (no reference counterpart): approx[b, i] = the f16 scan's score
 * of item i without bp, bound[b, i] its certified bound ([B, lda], real units); |approx + bp -
 * exact| <= bound for every pair (tests check it on the full catalogue). */
hnm_status hnm_ncf_deep_prefilter_debug_f32(hnm_ctx* ctx, const hnm_ncf_deep_weights* w,
                                            const int64_t* user_ids, int64_t B, float* approx,
                                            int64_t lda, float* bound);

/* ---- a9 + a10: Wide&Deep ------------------------------------------------------------
 * Reference layout (wide_deep.py:92-134): deep tower Linear -> ReLU -> BatchNorm1d (eval:
 * running stats, eps) per layer; final_layer over [wide (one-hot u, one-hot i, wide user
 * features) ; deep].  wide_user/item_embedding are unused by the reference forward.
 *   s = wide_user[u] + wide_item[i] (+ wide_user_features(f_u) . wide_feat)
 *       + final_deep . deep(u, i) + final_b
 * where wide_user / wide_item / wide_feat / final_deep are the segments [0, U), [U, U+I),
 * [U+I, U+I+F) and [wide_dim, ...) of final_layer.weight[0] (item rows may be a shard).
 * Towers of 2 (w3 == NULL, l3 == 0) or 3 layers, widths <= 512 / 256 / 128; deep input
 * [e_u; e_i] (+ deep_user_features(f_u) when num_user_features > 0) (+ deep_item_features(f_i):
 * the _ex entries below). */
typedef struct {
  const float* deep_user;  /* [num_users, d] */
  const float* deep_item;  /* [num_items, d] */
  const float* w1;         /* [l1, l1_in]  deep_network.0 */
  const float* b1;
  const float* bn1_w;      /* deep_network.2 weight / bias / running_mean / running_var */
  const float* bn1_b;
  const float* bn1_mean;
  const float* bn1_var;
  const float* w2;         /* [l2, l1]  deep_network.4 */
  const float* b2;
  const float* bn2_w;
  const float* bn2_b;
  const float* bn2_mean;
  const float* bn2_var;
  const float* w3;         /* [l3, l2]  deep_network.8 (NULL for a two-layer tower) */
  const float* b3;
  const float* bn3_w;
  const float* bn3_b;
  const float* bn3_mean;
  const float* bn3_var;
  const float* wide_user;  /* final_layer.weight[0, 0:U] */
  const float* wide_item;  /* final_layer.weight[0, U:U+I] */
  const float* wide_feat;  /* final_layer.weight[0, U+I:U+I+F] or NULL */
  const float* final_deep; /* final_layer.weight[0, wide_dim:] (last hidden width) */
  const float* final_b;    /* [1] */
  const float* duf_w;      /* [d, F] deep_user_features or NULL */
  const float* duf_b;
  const float* wuf_w;      /* [F, F] wide_user_features or NULL */
  const float* wuf_b;
  int64_t num_users;
  int64_t num_items;
  int32_t d;
  int32_t l1_in;
  int32_t l1;
  int32_t l2;
  int32_t l3;
  int32_t num_user_features;
  float eps;
} hnm_widedeep_weights;

hnm_status hnm_widedeep_topk_f32(hnm_ctx* ctx, const hnm_widedeep_weights* w,
                                 const int64_t* user_ids, int64_t B, const float* user_features,
                                 const int64_t* mask_ptr, const int32_t* mask_idx, int k,
                                 float* out_val, int64_t* out_idx);
hnm_status hnm_widedeep_scores_f32(hnm_ctx* ctx, const hnm_widedeep_weights* w,
                                   const int64_t* user_ids, int64_t B, const float* user_features,
                                   float* out, int64_t ldo);
/* WideDeep.forward(user_ids, item_ids, user_features) (wide_deep.py:157-230): out[n]. */
hnm_status hnm_widedeep_pair_scores_f32(hnm_ctx* ctx, const hnm_widedeep_weights* w,
                                        const int64_t* user_ids, const int64_t* item_ids,
                                        const float* user_features, int64_t n, float* out);
/* Item-side feature weights of WideDeep(num_item_features > 0) (wide_deep.py:101-103,
 * 116-117): deep_item_features [d, Fi] + bias, wide_item_features [Fi, Fi] + bias (NULL
 * when use_wide_features=False) and its slice of final_layer.weight. */
typedef struct {
  const float* dif_w;
  const float* dif_b;
  const float* wif_w;
  const float* wif_b;
  const float* wide_feat;
  int32_t num_item_features;
} hnm_widedeep_item_features;
/* WideDeep.forward(user_ids, item_ids, user_features, item_features): pairwise scores with
 * per-pair item features [n, Fi] (wide_deep.py:190-195, 214-217).  itf may be NULL (no
 * item features).  A NULL w->wide_user / w->wide_item means use_wide_user_item=False. */
hnm_status hnm_widedeep_pair_scores_ex_f32(hnm_ctx* ctx, const hnm_widedeep_weights* w,
                                           const hnm_widedeep_item_features* itf,
                                           const int64_t* user_ids, const int64_t* item_ids,
                                           const float* user_features, const float* item_features,
                                           int64_t n, float* out);
/* Catalogue scoring of a model with item features: hnm_widedeep_topk_f32 /
 * hnm_widedeep_scores_f32 plus the item-feature weights and the item-feature TABLE
 * item_features [w->num_items, Fi] (fp32, device, leading dimension ldf >= Fi; row i = the
 * features of item row i of this call's tables -- a row shard points at its first row, as for
 * deep_item / wide_item).  The features are per item, so they fold into the per-item layer-1
 * table and the per-item wide term before the scan:
 *   Q_i  = W1[:, d:2d] e_i + W1[:, c:c+d] (dif_w f_i + dif_b),  c = (2 + [Fu > 0]) d
 *   wI_i = wide_item[i] + wide_feat . (wif_w f_i + wif_b)
 * (the reference passes item_features=None in predict_all_items, wide_deep.py:275, and cannot
 * score such a model; this is its forward over every (user, item) pair).  w->l1_in must be
 * (2 + [Fu > 0] + 1) d; item_features, dif_w and dif_b must not be NULL (HNM_EINVAL); wif_w /
 * wide_feat may be NULL (use_wide_features=False: no wide item-feature term).  itf == NULL or
 * itf->num_item_features == 0: exactly the entries without _ex. */
hnm_status hnm_widedeep_topk_ex_f32(hnm_ctx* ctx, const hnm_widedeep_weights* w,
                                    const int64_t* user_ids, int64_t B, const float* user_features,
                                    const int64_t* mask_ptr, const int32_t* mask_idx, int k,
                                    float* out_val, int64_t* out_idx,
                                    const hnm_widedeep_item_features* itf,
                                    const float* item_features, int64_t ldf);
hnm_status hnm_widedeep_scores_ex_f32(hnm_ctx* ctx, const hnm_widedeep_weights* w,
                                      const int64_t* user_ids, int64_t B,
                                      const float* user_features, float* out, int64_t ldo,
                                      const hnm_widedeep_item_features* itf,
                                      const float* item_features, int64_t ldf);

/* ---- top-K merge (item partitions, item shards across GPUs) ------------------------
 * Candidates of row b: for g < G: cand[g*gstride + b*bstride + j], j < kc (value, global
 * item index; index < 0 = empty).  out: the best k of them per row, sorted. */
hnm_status hnm_topk_merge_f32(hnm_ctx* ctx, const float* cand_val, const int64_t* cand_idx,
                              int64_t B, int64_t G, int64_t gstride, int64_t bstride,
                              int kc, int k, float* out_val, int64_t* out_idx);

/* ---- (e) item-sharded exchange from the C ABI, over RCCL (SURVEY §8(b) hnm_topk_allgather_merge)
 * Every rank scores the SAME B users against its own item shard (global item ids) into [B, k]
 * lists; hnm_topk_allgather_merge_f32 all-gathers the lists of the communicator's ranks on the
 * ctx stream and merges them into the global top-k (score desc, item asc), identical on every
 * rank.  Every rank must call it (B and k equal on all).  The communicator: hnm_rccl_unique_id
 * on one rank (size >= 128 bytes), the bytes shared by the host, hnm_ctx_rccl_init on every
 * rank (owned by the ctx); or hnm_ctx_set_rccl_comm with the host's own ncclComm_t (borrowed;
 * NULL detaches).  The Python mirror's exchange (sharding.py, torch.distributed) adds a
 * certified bound exchange before the shard scans; this is the single-phase form. */
hnm_status hnm_rccl_unique_id(void* out, int64_t size);
hnm_status hnm_ctx_rccl_init(hnm_ctx* ctx, int world, int rank, const void* unique_id,
                             int64_t size);
hnm_status hnm_ctx_set_rccl_comm(hnm_ctx* ctx, void* comm);
/* Abort the ctx's own communicator (ncclCommAbort; a borrowed one is only detached).  When
 * hnm_topk_allgather_merge_f32 returns an error on one rank (argument check, open two-phase
 * call, workspace ENOMEM -- all checked before the collective), that rank never entered the
 * collective its peers are waiting in: the host aborts the communicator on every rank and
 * creates a new one (hnm_ctx_rccl_init). */
hnm_status hnm_ctx_rccl_abort(hnm_ctx* ctx);
hnm_status hnm_topk_allgather_merge_f32(hnm_ctx* ctx, const float* local_val,
                                        const int64_t* local_idx, int64_t B, int k,
                                        float* out_val, int64_t* out_idx);

/* The item-shard exchange's candidate lists as int32 pairs (one all_to_all): pairs[2e] = the
 * bits of val[e], pairs[2e+1] = idx[e] + offset (idx < 0 stays; global ids < 2^31); pairs
 * 8-byte aligned. */
hnm_status hnm_pack_candidates_i32(hnm_ctx* ctx, const float* val, const int64_t* idx, int64_t n,
                                   int64_t offset, int32_t* pairs);
/* Merge of received pairs [G][B][kc][2] (G <= 16), each list sorted in the top-K order (score
 * desc, id asc; id < 0 = empty, at the tail) -> out [B, k] sorted, empty slots (-inf, -1):
 * the same result as hnm_topk_merge_f32 over the unpacked candidates. */
hnm_status hnm_topk_merge_sorted_pairs_i32(hnm_ctx* ctx, const int32_t* pairs, int64_t B,
                                           int64_t G, int kc, int k, float* out_val,
                                           int64_t* out_idx);
/* The item-shard bound exchange's merge: lists[g*B*kc + b*kc + j] (g < G <= 16, j < kc), each
 * row of each list in descending order (hnm_{ncf,dot}_topk_begin_lists_f32's output,
 * all-gathered); out[b] = the k-th best value of row b's union of the G lists (k <= G*kc).
 * New (the reference has no multi-GPU path): sharding.py's exchange calls it. */
hnm_status hnm_topk_lists_kth_f32(hnm_ctx* ctx, const float* lists, int64_t B, int64_t G,
                                  int kc, int k, float* out);

/* Diagnostics of the certified split-f16 pre-filter of hnm_widedeep_topk_f32 (no reference
 * counterpart): approx[b, i] = the scan's score, bound[b, i] = its certified error bound;
 * |approx - exact| <= bound for every pair (tests check it on the full catalogue). */
hnm_status hnm_widedeep_prefilter_debug_f32(hnm_ctx* ctx, const hnm_widedeep_weights* w,
                                            const int64_t* user_ids, int64_t B,
                                            const float* user_features, float* approx,
                                            int64_t lda, float* bound);
/* The re-scoring cascade's refining stage (round 5) over the WHOLE catalogue: approx[b*lda + i]
 * = the three-pass split-f16 score of (user b, item i), bound[b*lda + i] its certified bound
 * (|approx - exact| <= bound, exact = hnm_widedeep_pair_scores_f32's arithmetic); the top-K path
 * runs it only on the scan's survivors.  Diagnostics / tests; B * num_items < 2^31. */
hnm_status hnm_widedeep_refine_debug_f32(hnm_ctx* ctx, const hnm_widedeep_weights* w,
                                         const int64_t* user_ids, int64_t B,
                                         const float* user_features, float* approx, int64_t lda,
                                         float* bound);
/* Both diagnostics for a model with item features (see hnm_widedeep_topk_ex_f32). */
hnm_status hnm_widedeep_prefilter_debug_ex_f32(hnm_ctx* ctx, const hnm_widedeep_weights* w,
                                               const int64_t* user_ids, int64_t B,
                                               const float* user_features, float* approx,
                                               int64_t lda, float* bound,
                                               const hnm_widedeep_item_features* itf,
                                               const float* item_features, int64_t ldf);
hnm_status hnm_widedeep_refine_debug_ex_f32(hnm_ctx* ctx, const hnm_widedeep_weights* w,
                                            const int64_t* user_ids, int64_t B,
                                            const float* user_features, float* approx,
                                            int64_t lda, float* bound,
                                            const hnm_widedeep_item_features* itf,
                                            const float* item_features, int64_t ldf);

/* ---- a11: batch mask from a device-resident history CSR --------------------------------
 * The purchase-history filter (serve.py:350-352; the filter_items loop of every recommend,
 * neural_cf.py:316-321) without a host round trip: hist_ptr[num_users + 1] / hist_idx (per
 * user, sorted ascending, unique, in [0, num_items)) stay on the device; for a batch of
 * user_ids[B] this writes the CSR mask the top-K entry points take: mask_ptr[B + 1] and
 * mask_idx[mask_ptr[B]] with row b = the history ids i of user_ids[b] with
 * item_lo <= i < item_hi, as i - item_lo (an item shard's local ids; pass 0 / INT64_MAX for
 * the whole catalogue).  Users outside [0, num_users) get empty rows (the scoring call flags
 * them).  capacity = the mask_idx length (B x the longest history always suffices); beyond
 * it rows are truncated and hnm_ctx_check() returns HNM_EINVAL.  Asynchronous, two launches. */
hnm_status hnm_mask_gather_csr(hnm_ctx* ctx, const int64_t* hist_ptr, const int32_t* hist_idx,
                               int64_t num_users, const int64_t* user_ids, int64_t B,
                               int64_t item_lo, int64_t item_hi, int64_t capacity,
                               int64_t* mask_ptr, int32_t* mask_idx);

/* ---- torch.topk over a dense score matrix (serve.py:350-355, k up to 100) ----------
 * Row top-k of scores[b, :I] (leading dim ld) with the optional CSR -inf mask, 1 <= k <= I
 * (torch.topk's range).  k <= 128: row-select kernels; larger k: a stable segmented radix
 * sort of whole rows in chunks (same (score desc, item asc) order; workspace ~512 MB). */
hnm_status hnm_topk_rows_f32(hnm_ctx* ctx, const float* scores, int64_t ld, int64_t B,
                             int64_t I, const int64_t* mask_ptr, const int32_t* mask_idx,
                             int k, float* out_val, int64_t* out_idx);

/* ---- a5: LightGCN.set_graph ----------------------------------------------------------
 * A_hat = D^-1/2 (A + I) D^-1/2 (lightgcn.py:81-134) as CSR with E + N entries:
 * self-loops appended, deg = row sums of the weights (edge_weight NULL -> 1), deg^-1/2
 * with inf -> 0, val = dinv[row] * w * dinv[col]; duplicates kept (summed by the SpMM). */
hnm_status hnm_csr_build_norm(hnm_ctx* ctx, const int64_t* edge_index, const float* edge_weight,
                              int64_t E, int64_t N, int64_t* rowptr, int32_t* col, float* val);

/* ---- a6: LightGCN.forward propagation -----------------------------------------------
 * Y = A_hat X (graph @ all_embeddings, lightgcn.py:152), with the layer combine fused:
 * acc_out = acc_in + alpha * Y (lightgcn.py:156-158).  Y and acc_out may be NULL.
 * d in {4, 8, 16, 32, 64, 128, 256}.  With a plan on a graph of N <= 2^22 nodes (the "walk
 * plan"; rowptr[0] == 0): every row's entries are summed in (col, CSR position) order -- rows
 * of at most 128 entries (the user rows) as one fp32 fma chain each by the column-ordered short
 * walk; longer rows (the item rows: ~300 neighbours each, power-law up to ~1e6) by the
 * user-ordered walk: cut into pieces of at most `cap` entries (piece j = sorted entries
 * j, j + n, ...), each piece one fp32 fma chain, several pieces summed in 256/(d/4)
 * interleaved slices and a fixed pairwise tree -- deterministic.  Larger graphs: short rows one
 * 16-lane group each, long rows one wave, rows over 2,048 entries in 2,048-entry segments + a
 * fixed tree, all in CSR order.  Without a plan: one wave per row, CSR order (deterministic,
 * slower on power-law rows).
 * BINDING: a plan is bound to the col / val pointers of its first prepare / SpMM /
 * rows_combine call and snapshots their values then (a walk plan keeps a sorted copy and
 * per-d schedules); a later call with other col / val pointers fails with HNM_EINVAL, and
 * values changed in place behind the same pointers are NOT seen -- create a new plan.
 * PREPARATION: binding and the first use of each d do one-time host work that synchronizes the
 * ctx stream (a D2H copy of col / val, host sorts, synchronous uploads of ~8 B per entry per
 * schedule; seconds on the 65M-entry H&M graph) and cannot be captured in a hipGraph: call
 * hnm_spmm_plan_prepare(ctx, plan, col, val, d) up front (d = 0: bind only).  After it every
 * SpMM / rows_combine call is asynchronous; an SpMM over split rows needs n_part * d * 4 bytes
 * of ctx workspace (a few MB; hnm_ctx_reserve covers it).
 * ROW RANGES: a range call launches only the short-walk blocks holding rows of the range, but
 * the whole long-row walk whenever one of its rows is in the range (outputs restricted to the
 * range): chunking [0, N) into many ranges repeats the item half's gathers per chunk. */
hnm_status hnm_spmm_plan_create(hnm_ctx* ctx, int64_t N, const int64_t* rowptr,
                                hnm_spmm_plan** out);
hnm_status hnm_spmm_plan_prepare(hnm_ctx* ctx, hnm_spmm_plan* plan, const int32_t* col,
                                 const float* val, int d);
hnm_status hnm_spmm_plan_destroy(hnm_spmm_plan* plan);
/* A row-restricted copy of a BOUND plan (no reference counterpart: the item-sharded LightGCN
 * propagation of SURVEY §8(e)).  The new plan computes only the rows inside the n_ranges host
 * ranges [ranges[2j], ranges[2j+1]) (ascending, disjoint, within [0, N)); SpMM calls on it never
 * write other rows of Y or acc.  Every kept row is summed exactly as the base plan sums it (same
 * pieces and order: bitwise equal rows), and a walk plan's schedules hold only the kept rows'
 * entries, so a layer costs what its kept rows cost (one rank: all user rows + its item shard).
 * The copy is bound to the base's col / val, owns its own sorted copy and schedules (destroy it
 * separately; its per-d schedules are built on first use / prepare as for any plan);
 * rows_combine on it equals rows_combine on the base.  The base itself must not be restricted. */
hnm_status hnm_spmm_plan_restrict(hnm_ctx* ctx, const hnm_spmm_plan* base, const int64_t* ranges,
                                  int n_ranges, hnm_spmm_plan** out);
hnm_status hnm_spmm_csr_f32(hnm_ctx* ctx, const hnm_spmm_plan* plan, int64_t N,
                            const int64_t* rowptr, const int32_t* col, const float* val,
                            const float* X, int d, float* Y, float alpha,
                            const float* acc_in, float* acc_out);
/* Row-range form: rows [row_begin, row_end) only.  Accumulators exist for rows >= acc_row0
 * and are stored from there on (acc[(r - acc_row0) * d]); acc_in NULL means beta * X[r]
 * (the alpha_0 * E_0 term folded into layer 1: acc_out = fma(alpha, Y, beta * X)).
 * hnm_spmm_csr_f32 == range [0, N), acc_row0 0, beta 0. */
hnm_status hnm_spmm_csr_range_f32(hnm_ctx* ctx, const hnm_spmm_plan* plan, int64_t N,
                                  const int64_t* rowptr, const int32_t* col, const float* val,
                                  const float* X, int d, float* Y, float alpha,
                                  const float* acc_in, float* acc_out, float beta,
                                  int64_t row_begin, int64_t row_end, int64_t acc_row0);
/* Final embeddings of `n` listed rows (ids < N) after L layers, given the layer inputs
 * E_0 .. E_{L-1} (host array `layers` of L device pointers, each [N, d]) and alphas[0..L]
 * (host): out[b] = sum_l alphas[l] E_l[rows[b]] with E_L[r] = (A_hat E_{L-1})[r] computed
 * for the listed rows only -- the last layer of LightGCN.forward restricted to the users a
 * recommend() call reads (lightgcn.py:197-199).  Same operations and order as the fused
 * combine of hnm_spmm_csr_f32 with the same plan (bitwise equal: every row is summed in the
 * order that plan's SpMM uses for it; plan NULL: the plan-less SpMM's order).  An id out of
 * range flags HNM_EOOB and writes NaN.  1 <= L <= 8. */
hnm_status hnm_spmm_rows_combine_f32(hnm_ctx* ctx, const hnm_spmm_plan* plan, int64_t N,
                                     const int64_t* rowptr,
                                     const int32_t* col, const float* val, const int64_t* rows,
                                     int64_t n, int d, const float* const* layers,
                                     const float* alphas, int L, float* out);
/* out = alpha * x + beta * y (y may be NULL): the alpha_0 * E_0 term of the combine. */
hnm_status hnm_axpby_f32(hnm_ctx* ctx, int64_t n, float alpha, const float* x, float beta,
                         const float* y, float* out);

/* ---- (f)4: ranking metrics over top-K lists (src/evaluation/metrics.py) ---------------
 * Per user r: predicted ids pred[r*ldp + j], j < min(pred_len ? pred_len[r] : ldp, k);
 * truth ids either CSR (truth_ptr[B+1] non-NULL: truth_idx[truth_ptr[r] .. truth_ptr[r+1]))
 * or dense rows truth_idx[r*ldt + j], j < ldt, kept where truth_mask == NULL ||
 * truth_mask[r*ldt + j] != 0 (the torchmetrics classes' `target[i][mask[i]]`).
 * n_true = the kept-entry count (pass unique ids for evaluate_recommendations' set
 * semantics, metrics.py:212).  inv_log2[i] = 1.0 / np.log2(i + 2), i < k (device, float64).
 * per_user[r*4 + 0..3] = AP@k, Recall@k, Precision@k, NDCG@k: the reference's float64
 * formulas in its summation order (evaluate_recommendations :218-247, MeanAveragePrecision
 * :49-62, RecallAtK :95-100, PrecisionAtK :133-137, NDCGAtK :176-186), zero denominators
 * -> 0.0.  sums[0..3] = sum over all rows of each metric, sums[4..7] = the same over rows
 * with n_true > 0, sums[8] = that row count (deterministic fixed-order reduction).
 * per_user, n_true and sums may each be NULL (not all three).  k <= 128. */
hnm_status hnm_rank_metrics_f64(hnm_ctx* ctx, const int64_t* pred, int64_t B, int64_t ldp,
                                const int64_t* pred_len, int k, const int64_t* truth_ptr,
                                const int64_t* truth_idx, int64_t ldt, const uint8_t* truth_mask,
                                const double* inv_log2, double* per_user, int64_t* n_true,
                                double* sums);

/* ---- PopularityBaseline (src/models/baseline.py) ----------------------------------------
 * Fit (baseline.py:137-165).  item_ids int64[n]; days_ago int32[n] or NULL; day_weight
 * f64[num_days] or NULL (= all 1.0).  With cnt[i, d] = the number of rows with item i and
 * day d:
 *   count[i] = sum_d cnt[i, d]                                         (int64[num_items])
 *   pop[i]   = ((0 + cnt[i,0] * w[0]) + cnt[i,1] * w[1]) + ...         (f64[num_items])
 * in ascending d, each product and each add rounded to float64 once (no fma), so pop is the
 * same bits on every run and equals that loop on the host.  days_ago == NULL: num_days = 1,
 * w = {1.0}, pop == count.  Rows whose day is outside [0, num_days) are ignored (the window
 * of get_popular_items(k, period)); item ids outside [0, num_items) raise the ctx error word
 * (HNM_EOOB from hnm_ctx_check) and are skipped.  The counts sit in an int32 [slab, num_items]
 * table in the ctx workspace (integer atomics), folded into pop one ascending slab of days at
 * a time; slab = 0 picks the slab from a 256 MiB table cap (slab > 0: days per pass, for
 * tests).  A cell must stay below 2^31 rows.  num_days > 65,536: HNM_EUNSUPPORTED. */
hnm_status hnm_popularity_fit_f64(hnm_ctx* ctx, const int64_t* item_ids, int64_t n,
                                  const int32_t* days_ago, const double* day_weight,
                                  int64_t num_items, int64_t num_days, int64_t slab,
                                  int64_t* count, double* pop);
/* Per-user top-K of a popularity order (baseline.py:78-85, 183-187).  order int64[R]: item
 * ids, most popular first; order_val f32[R]; rank int32[num_items]: position in order, -1 for
 * items not in it; mask_ptr int64[B+1] / mask_idx int32: the CSR mask of the other top-K
 * entries (both may be NULL; rows need not be sorted or de-duplicated).  Row b of out_val /
 * out_idx [B, k] holds the first k entries of order whose item is not in row b of the mask,
 * in order; slots past the last available entry hold (-inf, -1).  One wave per user over the
 * window min(R, k + h_b) of the order (h_b = the row's mask length), `chunk` ranks per LDS
 * bitmap pass (0 = default 8,192; else a multiple of 64 in [64, 8192]).  mask_idx entries
 * outside [0, num_items) raise the error word.  k = 0 or B = 0: HNM_OK, nothing launched. */
hnm_status hnm_popularity_topk_f32(hnm_ctx* ctx, const int64_t* order, const float* order_val,
                                   int64_t R, const int32_t* rank, int64_t num_items,
                                   const int64_t* mask_ptr, const int32_t* mask_idx, int64_t B,
                                   int k, int chunk, float* out_val, int64_t* out_idx);

/* ---- SegmentPopularity: popular lists per user segment (no reference module; the reference's
 * analysis names the strategy: "Demographics -> popular items in age/gender group") ---------
 * Fit: hnm_popularity_fit_f64 with one count table per segment.  item_ids / user_ids int64[n];
 * user_segment int32[num_users]: a user's segment in [0, num_segments), negative = unknown;
 * days_ago, day_weight, num_days, slab: as hnm_popularity_fit_f64.  S = num_segments >= 1
 * (else HNM_EINVAL).  count int64 / pop f64 are [S + 1, num_items]; row S is the global row.
 * A transaction increments row S and, when s = user_segment[user] >= 0, row s; per row
 *   count[s, i] = sum_d cnt[d, s, i]
 *   pop[s, i]   = ((0 + cnt[0,s,i] * w[0]) + cnt[1,s,i] * w[1]) + ...
 * in ascending d, each product and each add rounded to float64 once (no fma): the same bits on
 * every run and for every slab, and row S is bitwise hnm_popularity_fit_f64's result.  An item
 * outside [0, num_items), a user outside [0, num_users) or a segment >= S raises the ctx error
 * word (HNM_EOOB from hnm_ctx_check), and that transaction is skipped entirely.  The counts sit
 * in an int32 [slab, S + 1, num_items] table in the ctx workspace; slab = 0 picks the days per
 * pass from the 256 MiB table cap.  One day's table above the cap, or num_days > 65,536:
 * HNM_EUNSUPPORTED. */
hnm_status hnm_segpop_fit_f64(hnm_ctx* ctx, const int64_t* item_ids, const int64_t* user_ids,
                              int64_t n, const int32_t* user_segment, int64_t num_users,
                              const int32_t* days_ago, const double* day_weight,
                              int64_t num_items, int64_t num_segments, int64_t num_days,
                              int64_t slab, int64_t* count, double* pop);
/* Per-row top-K: a segment's list, continued from the global one.  The S + 1 orders are
 * concatenated in order int64 / order_val f32 at the device offsets order_ptr int64[S + 2]
 * (order S = the global one); rank int32[S + 1, num_items]: position in each order, -1 = not in
 * it.  seg int32[B]: the row's segment, negative = none (NULL: none for every row); seg >= S
 * raises the error word and the row is answered as one without a segment.  mask_ptr / mask_idx,
 * k, chunk: as hnm_popularity_topk_f32.  With hist = row b of the mask and s = seg[b]:
 *   seg_part = [x for x in order[s] if x not in hist][:k]                  (empty when s < 0)
 *   rest     = [x for x in order[S] if x not in hist and x not in seg_part][:k - len(seg_part)]
 * row b of out_val / out_idx [B, k] = seg_part + rest, then (-inf, -1); out_nseg[b] (int32, may
 * be NULL) = len(seg_part).  Each entry carries the score of the list it came from: the
 * segment's popularity before position out_nseg[b], the global popularity from there on, so the
 * scores of a row are NOT monotone across that seam (each part is).  With every row at a
 * negative segment the result is bitwise hnm_popularity_topk_f32's over order S.  One wave per
 * row, two phases over windows min(R, k + h_b) of the two orders; phase 2 also marks what phase
 * 1 emitted.  order == NULL: every order is empty.  k = 0: out_nseg = 0, nothing launched. */
hnm_status hnm_segpop_topk_f32(hnm_ctx* ctx, const int64_t* order, const float* order_val,
                               const int64_t* order_ptr, const int32_t* rank, int64_t num_items,
                               int64_t num_segments, const int32_t* seg, const int64_t* mask_ptr,
                               const int32_t* mask_idx, int64_t B, int k, int chunk,
                               float* out_val, int64_t* out_idx, int32_t* out_nseg);

/* ---- ItemCF: item-based collaborative filtering (no reference counterpart) ---------------
 * Fit.  hist_ptr int64[num_users + 1] / hist_idx int32: the de-duplicated user -> item CSR
 * (rows ascending and unique: UserHistory's layout).  A user with more than max_history items
 * is dropped (0 = no cap).  Over the kept users, n[i] = users holding i, C[i, j] = users
 * holding both i and j (i != j), and for C[i, j] > 0
 *   sim[i, j] = (float)( (double)C / ( sqrt((double)n_i * (double)n_j) + shrink ) )
 * in float64 with one rounding per operation and no fma, rounded once to float32.  Row i of
 * nbr_idx int32[num_items, N] / nbr_val f32[num_items, N] holds the N largest entries in
 * (sim descending, j ascending) order, padded with (-1, 0.0f); item_count int64[num_items] =
 * n.  1 <= N <= 64.  Integer atomics only: the same bits on every run.  `window`: item columns
 * counted per LDS pass (0 = default 16,384; else a multiple of 64 in [64, 16384]).  The item ->
 * user transpose lives in the ctx workspace; the call reads the CSR's last offset back (one
 * stream sync).  Item ids outside [0, num_items) and rows outside the CSR raise the ctx error
 * word (HNM_EOOB from hnm_ctx_check) and are skipped.  History entries and users: < 2^31. */
hnm_status hnm_itemcf_fit_f32(hnm_ctx* ctx, const int64_t* hist_ptr, const int32_t* hist_idx,
                              int64_t num_users, int64_t num_items, int N, double shrink,
                              int64_t max_history, int window, int32_t* nbr_idx, float* nbr_val,
                              int64_t* item_count);
/* Dense scores of B history rows: out[b, i] (row stride ld >= num_items) = the fp32 sum of
 * nbr_val(j -> i) over the items j of the row in ascending order, plain adds from the first
 * term; 0.0f where no j points to i.  Row b is the history of user_ids[b], or row b of the CSR
 * itself when user_ids is NULL (then B <= num_users: a CSR of baskets).  A user id outside
 * [0, num_users) raises the error word and scores as an empty history. */
hnm_status hnm_itemcf_scores_f32(hnm_ctx* ctx, const int32_t* nbr_idx, const float* nbr_val,
                                 int64_t num_items, int N, const int64_t* hist_ptr,
                                 const int32_t* hist_idx, int64_t num_users,
                                 const int64_t* user_ids, int64_t B, float* out, int64_t ld);
/* Fused top-K of the same scores, 0 <= k <= 64: row b of out_val / out_idx [B, k] holds the
 * items with score > 0 that are not in row b of the CSR mask (mask_ptr int64[B + 1] / mask_idx
 * int32, rows ascending; both may be NULL), in (score descending, item ascending) order; slots
 * past the last such item hold (-inf, -1).  History items are not excluded by themselves.  One
 * wave per row over an LDS table sized from h_b * N (h_b = the row's history length); rows with
 * h_b * N > 4,096 take the dense route (a workspace row, the same additions in the same order,
 * the same selection: the same bits) -- hnm_itemcf_route tells which.  B = 0 or k = 0: HNM_OK,
 * nothing launched. */
hnm_status hnm_itemcf_topk_f32(hnm_ctx* ctx, const int32_t* nbr_idx, const float* nbr_val,
                               int64_t num_items, int N, const int64_t* hist_ptr,
                               const int32_t* hist_idx, int64_t num_users,
                               const int64_t* user_ids, int64_t B, const int64_t* mask_ptr,
                               const int32_t* mask_idx, int k, float* out_val, int64_t* out_idx);
/* *route = 0: a row of history_len items takes the fused LDS route of hnm_itemcf_topk_f32 with
 * N neighbours per item; 1: the dense route.  No launch, no sync. */
hnm_status hnm_itemcf_route(hnm_ctx* ctx, int N, int64_t history_len, int* route);
/* The weighted siblings: hist_w f32, aligned with hist_idx (hist_w[p] is the weight of entry
 * hist_idx[p]: a purchase count, a recency decay, their product -- UserHistory.hist_w), finite
 * and >= 0; every other argument, status and rule is the unweighted entry's, and hist_w == NULL
 * IS the unweighted entry, bit for bit.  hnm_itemcf_route serves both.
 *
 * Fit.  The counts stay integers by counting in fixed point.  max_history counts entries, not
 * weights.  With w_max = the largest weight among the kept users' entries,
 *   s = 32768.0 / (double)w_max            q = (uint32) rint((double)w * s)      (ties to even)
 * in float64, so w_max maps to exactly 2^15.  Over the kept users, in uint64,
 *   n_w[i] = sum_u q_ui^2                  C_w[i, j] = sum_u q_ui * q_uj   (i != j)
 * (a product <= 2^30, fewer than 2^31 users: < 2^61, nothing overflows; integer sums are
 * order-free, so a run gives the same bits every time), and for C_w[i, j] > 0
 *   sim[i, j] = (float)( (double)C_w / ( sqrt((double)n_i * (double)n_j) + (shrink * s) * s ) )
 * one rounding per operation, no fma: shrink is in the caller's weight units squared, and with
 * unit weights it is the unweighted shrink.  Selection, order and padding are
 * hnm_itemcf_fit_f32's.  Entries with q == 0 are left out: item_count[i] = kept users holding i
 * with q > 0.  w_max == 0 (or no kept entry) behaves as an empty history: every row padded,
 * item_count zero.  A negative or non-finite weight raises its own bit of the ctx error word
 * (HNM_EINVAL from hnm_ctx_check; HNM_EOOB is named first when both were seen) and counts as 0.
 * Two identities hold bit for bit: every weight 1.0f gives hnm_itemcf_fit_f32's nbr_idx,
 * nbr_val and item_count for any shrink and max_history (a power-of-two scale commutes with
 * every rounding); every weight equal to any one constant does at shrink = 0.  `window`: uint64
 * counters per LDS pass (0 = default 16,384 = 128 KiB of LDS, one workgroup a CU; else a multiple
 * of 64 in [64, 16384]; up to 8,192 = 64 KiB two workgroups share a CU).  Workspace: the unweighted fit's plus 8 bytes per history entry
 * and 8 per item. */
hnm_status hnm_itemcf_fit_weighted_f32(hnm_ctx* ctx, const int64_t* hist_ptr,
                                       const int32_t* hist_idx, const float* hist_w,
                                       int64_t num_users, int64_t num_items, int N, double shrink,
                                       int64_t max_history, int window, int32_t* nbr_idx,
                                       float* nbr_val, int64_t* item_count);
/* Scores.  out[b, i] = the fp32 sum over the row's items j in ascending order of
 * fl(w_j * nbr_val(j -> i)): the product is rounded to fp32 first, then a plain add (no fma);
 * w_j is the row's raw fp32 weight, not the quantised one.  A weight of 0 contributes nothing.  A
 * negative or non-finite weight raises the weight bit of the error word and counts as 0. */
hnm_status hnm_itemcf_scores_weighted_f32(hnm_ctx* ctx, const int32_t* nbr_idx,
                                          const float* nbr_val, int64_t num_items, int N,
                                          const int64_t* hist_ptr, const int32_t* hist_idx,
                                          const float* hist_w, int64_t num_users,
                                          const int64_t* user_ids, int64_t B, float* out,
                                          int64_t ld);
/* Fused top-K of the weighted scores: score > 0, the mask, the (score descending, item
 * ascending) order, the (-inf, -1) padding and the h_b * N <= 4,096 route rule are
 * hnm_itemcf_topk_f32's; both routes give the same bits. */
hnm_status hnm_itemcf_topk_weighted_f32(hnm_ctx* ctx, const int32_t* nbr_idx,
                                        const float* nbr_val, int64_t num_items, int N,
                                        const int64_t* hist_ptr, const int32_t* hist_idx,
                                        const float* hist_w, int64_t num_users,
                                        const int64_t* user_ids, int64_t B,
                                        const int64_t* mask_ptr, const int32_t* mask_idx, int k,
                                        float* out_val, int64_t* out_idx);

/* ---- ContentKNN: item-attribute similarity (no reference counterpart) ----------------------
 * The fit of a neighbour table from the catalogue's categorical attributes instead of purchases:
 * an item nobody has bought yet still has a row.  The table is hnm_itemcf_fit_f32's (selection,
 * order, padding), so hnm_itemcf_scores_f32 / hnm_itemcf_topk_f32 serve it unchanged.
 *
 * attrs int32[num_items, F], row-major, 1 <= F <= 16: column f holds the item's code in that
 * column's own vocabulary [0, V_f), V_f = code_ptr[f + 1] - code_ptr[f] (code_ptr int64[F + 1],
 * ascending from an offset >= 0; device memory like every other pointer).  A negative code is
 * missing and matches nothing.  A code >= V_f raises the ctx error word (HNM_EOOB from
 * hnm_ctx_check) and counts as missing; so does every code when code_ptr does not ascend.
 * code_q uint32[code_ptr[F]]: the fixed-point weight of code v of column f is
 * code_q[code_ptr[f] + v] <= 2^20; a larger one raises its own bit of the error word (HNM_EINVAL
 * from hnm_ctx_check; HNM_EOOB is named first when both were seen) and counts as 0.  The weight
 * belongs to the (column, code) pair: two items that match in a column carry the same weight
 * there, so S below is symmetric.  With q_if = that weight, or 0 for a missing code,
 *   n_i = sum_f q_if  (<= 2^24)        item_count[i] = the number of columns with q_if > 0
 *   S_ij = sum_f [a_if == a_jf and a_if >= 0] * q_if          (i != j, an exact integer)
 * and for S_ij > 0
 *   sim[i, j] = (float)( (double)S / sqrt((double)n_i * (double)n_j) )
 * in float64 with one rounding per operation and no fma (n_i * n_j < 2^48 is exact), rounded
 * once to float32: hnm_itemcf_fit_f32's rule.  Row i of nbr_idx int32[num_items, N] / nbr_val
 * f32[num_items, N], 1 <= N <= 64, holds the N largest entries in (float32 sim descending, j
 * ascending) order, padded with (-1, 0.0f).  An item with n_i = 0 has an empty row and is
 * nobody's neighbour.  The order is the rounded float32 value's: sims that differ in float64 and
 * collapse in float32 are ordered by j.  Integers up to the float64 expression: the same bits on
 * every run, and on every `tile`.
 *
 * A dense num_items^2 scan (a wave keeps a few rows' codes in scalar registers and streams the
 * column items in LDS tiles); the float64 expression is evaluated only for pairs that pass a
 * conservative fp32 upper bound of sim against the row's current N-th value (csrc/content.hip
 * argues the bound).  `tile`: column items per LDS tile (0 = default 512; else a multiple of 64
 * in [64, 512]).  Workspace: 8 F + 8 bytes per item.  No stream sync.  num_items = 0: HNM_OK,
 * nothing launched.  num_items < 2^31. */
hnm_status hnm_content_fit_f32(hnm_ctx* ctx, const int32_t* attrs, int64_t num_items, int F,
                               const int64_t* code_ptr, const uint32_t* code_q, int N, int tile,
                               int32_t* nbr_idx, float* nbr_val, int64_t* item_count);

/* ---- SequentialCF: directed next-purchase transitions (no reference counterpart) ------------
 * The fit of a neighbour table from the ORDER of purchases: row a holds what customers bought in
 * the days AFTER a.  The table is hnm_itemcf_fit_f32's (selection, order, padding), and row a
 * -> b is the direction hnm_itemcf_scores_f32 / hnm_itemcf_topk_f32 read (val(j -> i) over the
 * history items j), so they serve it unchanged: score(u, i) = sum_j w_uj * sim(j -> i).
 *
 * seq_ptr int64[num_users + 1] / seq_item int32 / seq_day int32: the user -> event CSR
 * (UserSequence's layout).  An event is a distinct (user, day, item); a user's events are sorted
 * by (day ascending, item ascending), a later purchase has a larger day.  gap_q uint32[max_gap]
 * (device memory like every other pointer): gap_q[g - 1] is the fixed-point weight of a pair g
 * days apart, <= 32768 = 2^15 (the weight 1.0).
 *
 * Users with more than max_history events are dropped, as in ItemCF's fit; the counts below run
 * over the kept users.  n[a] = the number of events of item a: item_count int64[num_items].
 * T[a, b] = the sum of gap_q[t - s - 1] over all ordered pairs of events of one user, the first
 * (a, day s), the second (b, day t), with 1 <= t - s <= max_gap; a != b is required unless
 * repeat_buys is set; same-day pairs are co-occurrence, which is ItemCF's, and do not count.  For
 * T[a, b] > 0
 *   sim(a -> b) = (float)( (double)T / ( 32768.0 * ( sqrt((double)n_a * (double)n_b) + shrink ) ) )
 * in float64 with one rounding per operation and no fma, rounded once to float32: the form of
 * hnm_itemcf_fit_f32.  Row a of nbr_idx int32[num_items, N] / nbr_val f32[num_items, N] keeps its
 * N best in (sim descending, b ascending) order and is padded with (-1, 0.0f).
 *
 * Exactness.  T is an integer in uint64.  With e_u(x) = the events of item x of user u, T[a, b] <=
 * 2^15 * sum_u e_u(a) * e_u(b), and e_u(a) + e_u(b) <= max_history <= 65535 gives e_u(a) * e_u(b)
 * <= (65535 / 4) * (e_u(a) + e_u(b)), so T <= 2^15 * (65535 / 4) * E for a sequence of E events.
 * The entry refuses E >= 2^31 (HNM_EUNSUPPORTED), so T < 2^60 (a -> a under repeat_buys: e (e - 1)
 * / 2 pairs a user, T < 2^61): nothing overflows, integer sums are order-free, and the result is the same bits on every run and at every `window`.  That bound is
 * why max_history has a ceiling here and not in ItemCF, whose counters add at most 2^30 a user.
 *
 * Ranges, checked before anything is launched (HNM_EINVAL, outputs untouched): 1 <= N <= 64;
 * shrink finite and >= 0; 1 <= max_history <= 65535; 1 <= max_gap <= 1024; every gap_q entry <=
 * 32768 (the table is read back: one stream sync, shared with the CSR's last offset);
 * repeat_buys 0 or 1; `window`, below.  An item id outside [0, num_items) and a row outside the
 * CSR raise the ctx error word (HNM_EOOB from hnm_ctx_check) and are skipped.  Days that do not
 * ascend inside a row give an unspecified table; nothing outside the outputs is written.
 *
 * Two routes, the same T and so the same bits.  A row a whose events are followed, inside max_gap
 * days, by at most 1,024 later events in all (same-item and zero-weight ones included: an upper
 * bound of its distinct successors) is counted in an LDS hash table keyed by b.  Any other row
 * walks the catalogue in windows of uint64 LDS counters and re-reads its ranges once a window:
 * `window` = counters per pass, 0 = default 16,384 (128 KiB of LDS and the gap table: one
 * workgroup a CU), else a multiple of 64 in [64, 16384].  Workspace: 12 bytes per event and 16 per
 * item.  num_items = 0: HNM_OK, nothing launched.  Users and num_items: < 2^31. */
hnm_status hnm_seqcf_fit_f32(hnm_ctx* ctx, const int64_t* seq_ptr, const int32_t* seq_item,
                             const int32_t* seq_day, int64_t num_users, int64_t num_items, int N,
                             double shrink, int64_t max_history, int max_gap,
                             const uint32_t* gap_q, int repeat_buys, int window, int32_t* nbr_idx,
                             float* nbr_val, int64_t* item_count);

/* ---- Fusion of overlapping top-K lists: an ensemble of models (no reference counterpart) ----
 * hnm_topk_merge_f32 merges lists whose items are disjoint.  Here G models each give a list per
 * row, the same item may stand in several of them, and its fused score depends on every list
 * that holds it.
 *
 * Input.  Entry j (j < kc) of list g (g < G) of row b (b < B) sits at
 * list_val / list_idx[g * gstride + b * bstride + j]: hnm_topk_merge_f32's layout.  Position j is
 * rank j + 1.  An entry is EMPTY when idx < 0 or val is not finite (the (-inf, -1) tails of
 * ItemCF and the popularity baseline, the -inf tails of the dot top-K): it contributes nothing.
 * An entry with idx >= num_items raises the ctx error word (HNM_EOOB from hnm_ctx_check) and is
 * skipped like an empty one.  The non-empty items of one list of one row must be distinct (every
 * top-K entry of this library guarantees it); if they are not, that row's result is unspecified,
 * and nothing outside the row's outputs is written.
 *
 * A non-empty entry (g, j) contributes
 *   HNM_FUSE_RANK   coef[g * kc + j]     coef f32[G * kc]: the host's table, any rank discount
 *                                        (reciprocal rank fusion: w_g / (c + j + 1)); no division
 *                                        on the device
 *   HNM_FUSE_SCORE  fl(coef[g] * val)    coef f32[G]: one fp32 rounding of the product
 * and an item's fused score is the fp32 sum of its contributions in ascending g: it starts from
 * the first contribution itself and continues with plain adds, never an fma.  coef is finite.
 *
 * Output, RANK and SCORE.  Row b of out_val / out_idx [B, k] holds the items that occur in at
 * least one list of the row and are not in row b of the CSR mask (mask_ptr int64[B + 1] /
 * mask_idx int32, rows ascending; both may be NULL), in (fused score descending, item
 * ascending) order with their fused scores; slots past the last such item hold (-inf, -1).
 * There is no score > 0 condition: dot-product scores may be negative.
 *
 * HNM_FUSE_CASCADE.  coef is ignored and may be NULL.  An item's key is (g*, j*): the lowest g
 * whose list holds it, then its position there.  The output is the unmasked items in ascending
 * key, each with the val of that first occurrence: list 0 first, then what list 1 adds, and so
 * on -- a short list continued from the next one.
 *
 * Limits: 1 <= G <= 16, 1 <= kc <= 512, G * kc <= 2,048, 0 <= k <= 128; anything outside is
 * HNM_EUNSUPPORTED (nothing is written).  A mode outside the three, or coef NULL in RANK or
 * SCORE: HNM_EINVAL.  B = 0 or k = 0: HNM_OK, nothing launched.  One wave per row over an LDS
 * table of the power of two >= 2 * G * kc slots (at most 32 KiB); no workspace, no float
 * atomics: the sum's order is fixed by g, not by which lane arrives first, so the result is the
 * same bits on every run. */
#define HNM_FUSE_RANK 0
#define HNM_FUSE_SCORE 1
#define HNM_FUSE_CASCADE 2
hnm_status hnm_fuse_topk_f32(hnm_ctx* ctx, const float* list_val, const int64_t* list_idx,
                             int64_t B, int64_t G, int64_t gstride, int64_t bstride, int kc,
                             int mode, const float* coef, int64_t num_items,
                             const int64_t* mask_ptr, const int32_t* mask_idx, int k,
                             float* out_val, int64_t* out_idx);

/* ---- Two-stage serving: candidate rows for a ranker (no reference counterpart; the reference's
 * design note asks for "Stage 1: candidate generation, Stage 2: ranking") --------------------
 * Candidate union.  G recall sources each give a list per row; the ranker wants every item of a
 * row once.
 *
 * Input.  list_val / list_idx, B, G, gstride, bstride, kc: hnm_fuse_topk_f32's layout, and its
 * definition of an EMPTY entry: idx < 0, or list_val given (it may be NULL) and the value not
 * finite.  An entry with idx >= num_items raises the ctx error word (HNM_EOOB from
 * hnm_ctx_check) and is skipped like an empty one.  An item may stand in several lists of a row,
 * and more than once in one list.
 *
 * Output.  Row b of out_cand int32[B, ldc] holds the distinct non-empty item ids of the row's G
 * lists in ASCENDING order, out_n[b] of them; positions out_n[b] .. ldc hold -1.
 * ldc >= G * kc (else HNM_EINVAL).
 *
 * Limits: 1 <= G <= 16, 1 <= kc <= 512, G * kc <= 2,048; anything outside is HNM_EUNSUPPORTED
 * (nothing is written).  B = 0: HNM_OK, nothing launched.  One wave per row: the ids sorted in
 * LDS by a bitonic network (at most 8 KiB a wave), then compacted with ballot + popcount; no
 * workspace, no atomics: the same bits on every run.  No stream sync. */
hnm_status hnm_cand_union_i32(hnm_ctx* ctx, const float* list_val, const int64_t* list_idx,
                              int64_t B, int64_t G, int64_t gstride, int64_t bstride, int kc,
                              int64_t num_items, int32_t* out_cand, int64_t ldc, int32_t* out_n);

/* Selection from scored candidate rows.  Row b considers entries j < cand_n[b] (clamped to
 * [0, ldc]) of scores f32[B, ldc] / cand int32[B, ldc]; an entry with cand < 0, or whose score is
 * NaN or -inf, is dropped.  Row b of out_val / out_idx [B, k] holds the best k of the rest in
 * (score descending, item id ascending) order -- the library's total order -- and (-inf, -1)
 * past the last one.  The candidates of a row must be distinct; if they are not, that row's
 * result is unspecified, and nothing outside the row's outputs is written.  1 <= k <= 128
 * (else HNM_EUNSUPPORTED, nothing written).  B = 0: HNM_OK.  One wave per row; no workspace,
 * no stream sync. */
hnm_status hnm_cand_topk_f32(hnm_ctx* ctx, const float* scores, const int32_t* cand, int64_t ldc,
                             const int32_t* cand_n, int64_t B, int k, float* out_val,
                             int64_t* out_idx);

/* Wide&Deep over candidate rows: score and select in one launch.  w, user_ids, user_features,
 * itf, item_features, ldf: as hnm_widedeep_topk_ex_f32, and the same per-call preparation
 * (folded weights, the layer-1 tables of the batch rows and of the WHOLE catalogue, the
 * item-feature fold): the catalogue's layer-1 table is rebuilt on every call, as in every
 * Wide&Deep entry.  cand int32[B, ldc] / cand_n int32[B]: row b's candidates are entries
 * j < cand_n[b] (clamped to [0, ldc]); hnm_cand_union_i32's output.
 *
 * The score of (b, item) is BITWISE row b, column item of hnm_widedeep_scores_ex_f32: the same
 * device function on the same operands in the same order.  A candidate < 0 is skipped; one
 * >= w->num_items raises the ctx error word (HNM_EOOB from hnm_ctx_check) and is skipped.
 * Out-of-range user_ids behave as in hnm_widedeep_topk_ex_f32.
 *
 * Output.  Row b of out_val / out_idx [B, k]: the row's candidates whose score is neither NaN
 * nor -inf, best k in (score descending, item ascending) order, (-inf, -1) past the last one.
 * out_scores f32[B, ldc] (may be NULL): the score of cand[b, j], -inf for skipped candidates
 * and for positions cand_n[b] .. ldc.  k = 0 with out_scores: only the scores are written
 * (out_val / out_idx may be NULL); k = 0 without: HNM_EINVAL.  The candidates of a row must be
 * distinct; if they are not, that row's selection is unspecified, and nothing outside that
 * row's outputs is written.  There is no mask: the sources of the candidates applied it.
 *
 * Limits: 0 <= k <= 64, ldc <= 2,048, and the tower shapes of hnm_widedeep_topk_ex_f32; else
 * HNM_EUNSUPPORTED (nothing is written).  B = 0: HNM_OK.  One wave per user, walking its list in
 * tiles of 32.  No stream sync.  hnm_ctx_enable_timing (scoring class) times the candidate
 * kernel alone, without the preparation. */
hnm_status hnm_widedeep_cand_topk_ex_f32(hnm_ctx* ctx, const hnm_widedeep_weights* w,
                                         const int64_t* user_ids, int64_t B,
                                         const float* user_features, const int32_t* cand,
                                         int64_t ldc, const int32_t* cand_n, int k,
                                         float* out_val, int64_t* out_idx, float* out_scores,
                                         const hnm_widedeep_item_features* itf,
                                         const float* item_features, int64_t ldf);

/* ---- ImplicitALS: alternating least squares for implicit feedback (Hu, Koren & Volinsky
 * 2008; no reference counterpart) ----------------------------------------------------------
 * Gram matrix.  out f32[d, d] (contiguous) = tab^T tab over the first `rows` rows of tab (row
 * stride ld >= d), all in fp32: rows are taken in chunks of 2,048; inside a chunk entry (i, j)
 * is the fmaf chain acc = fmaf(t_r[i], t_r[j], acc) over the chunk's rows r in ascending order
 * from 0.0f; the chunk partials are added in ascending chunk order from the first partial.
 * Chunk size and order are compile-time constants, so the result is the same bits on every run
 * and does not depend on the grid or the CU count; out is exactly symmetric.  rows = 0: zeros.
 * Workspace: cdiv(rows, 2048) * d * d floats of the ctx workspace (22 MB for 1,371,980 rows at
 * d = 64, 88 MB at d = 128).  d: a multiple of 16 in [16, 128], else HNM_EUNSUPPORTED. */
hnm_status hnm_als_gram_f32(hnm_ctx* ctx, const float* tab, int64_t rows, int64_t ld, int64_t d,
                            float* out);
/* One ALS half-step for B rows of a CSR.  ptr int64[n_rows + 1] / idx int32: the CSR (rows of
 * UserHistory's layout, or of its transpose); tab f32[tab_rows, d] (row stride ld >= d): the
 * table the rows index; gram f32[d, d]: hnm_als_gram_f32 of tab.  Output row b (out + b * ldo,
 * ldo >= d) is the solution for CSR row row_ids[b] (int64[B]), or for row b when row_ids is
 * NULL (then B <= n_rows).  For a row with entries j_0, j_1, ... (stored order), in fp32:
 *   S[i][c] = fmaf chain over m of t_{j_m}[i] * t_{j_m}[c], from 0.0f
 *   b0[c]   = ((0 + t_{j_0}[c]) + t_{j_1}[c]) + ...
 *   A[i][c] = fmaf(alpha, S[i][c], gram[i][c]) (+ reg when i == c),  c <= i
 *   b[c]    = (1.0f + alpha) * b0[c]
 *   out     = A^-1 b by a right-looking Cholesky A = L L^T (l_kk = sqrtf(a_kk), l_ik = a_ik /
 *             l_kk, a_ij = fmaf(-l_ik, l_jk, a_ij)), b carried as an extra row (L y = b), then
 *             L^T x = y from the last entry up (x_k = y_k / l_kk, y_i = fmaf(-l_ki, x_k, y_i)).
 * Only the lower triangle of gram is read.  A row without entries gives exact zeros.  One
 * definition serves the fit and fold-in, and one workgroup owns a row whatever its length (a
 * long row is the same loop run longer: there is no length threshold and no second route), so a
 * row's bits depend on its inputs alone -- not on B, on the other rows or on the run.  No
 * floating-point atomics.  An idx entry outside [0, tab_rows) or a row_ids entry outside
 * [0, n_rows) raises the ctx error word (HNM_EOOB from hnm_ctx_check) and that output row is
 * NaN; the other rows are unaffected.  d: a multiple of 16 in [16, 128], else
 * HNM_EUNSUPPORTED; reg <= 0, alpha < 0 or a non-finite value: HNM_EINVAL.  B = 0 or
 * n_rows = 0: HNM_OK, nothing launched.  Workspace: none (the systems live in LDS). */
hnm_status hnm_als_solve_rows_f32(hnm_ctx* ctx, const int64_t* ptr, const int32_t* idx,
                                  int64_t n_rows, const float* tab, int64_t tab_rows, int64_t ld,
                                  int64_t d, const float* gram, float alpha, float reg,
                                  const int64_t* row_ids, int64_t B, float* out, int64_t ldo);
/* The same half-step with a confidence weight per stored entry: c_m = 1 + alpha * w_m, p = 1
 * (Hu, Koren & Volinsky's c_ui = 1 + alpha r_ui; r = a purchase count, a recency decay, ...).
 * w f32, aligned with idx (w[p] is the weight of entry idx[p]); every other argument is
 * hnm_als_solve_rows_f32's.  For a row with entries j_0, j_1, ... and weights w_0, w_1, ... in
 * stored order, in fp32:
 *   S[i][c] = fmaf chain over m of fl(w_m * t_{j_m}[i]) * t_{j_m}[c], from 0.0f      (c <= i)
 *   b0[c]   = ((0 + t_{j_0}[c]) + t_{j_1}[c]) + ...
 *   bw[c]   = fmaf chain over m: acc = fmaf(w_m, t_{j_m}[c], acc), from 0.0f
 *   A[i][c] = fmaf(alpha, S[i][c], gram[i][c]) (+ reg when i == c)
 *   b[c]    = fmaf(alpha, bw[c], b0[c])
 *   out     = A^-1 b   -- the Cholesky and back-substitution above, word for word
 * (the weight scales the factor indexed by the output ROW i).  Two identities hold bit for bit
 * whenever 1.0f + alpha' is exact in fp32 for the unweighted alpha' named: every weight 1.0f
 * gives hnm_als_solve_rows_f32's bits at alpha' = alpha; every weight 2^e gives its bits at
 * alpha' = 2^e * alpha.  A weight of 0 is legal: the entry then counts in b0 (and in nothing
 * else).  A negative or non-finite weight raises its own bit of the ctx error word (HNM_EINVAL
 * from hnm_ctx_check) and that output row is NaN; the other rows are unaffected, and an id out
 * of range still reports HNM_EOOB (which hnm_ctx_check names first when both were seen).
 * w == NULL with work to do: HNM_EINVAL.  Every other status, the B = 0 / n_rows = 0 rule, one
 * workgroup per row, no floating-point atomics and "a row's bits depend on its inputs alone"
 * are hnm_als_solve_rows_f32's. */
hnm_status hnm_als_solve_rows_weighted_f32(hnm_ctx* ctx, const int64_t* ptr, const int32_t* idx,
                                           const float* w, int64_t n_rows, const float* tab,
                                           int64_t tab_rows, int64_t ld, int64_t d,
                                           const float* gram, float alpha, float reg,
                                           const int64_t* row_ids, int64_t B, float* out,
                                           int64_t ldo);
/* The half-step by conjugate gradients (Takacs, Pilaszy & Tikk 2011): `steps` CG steps on the
 * row's system from a start vector, instead of the exact solve.  The arguments are
 * hnm_als_solve_rows_f32's, except that out / ldo become the in/out x / ldx (ldx >= d): on entry
 * row b of x (x + b * ldx) holds the start vector x0 for CSR row row_ids[b] (or row b), on return
 * the result; and `steps` in [1, 32] is added.  A fit calls it with the table of the previous
 * sweep as x (a warm start).  The system -- S, b0, A (its lower triangle, taken as the symmetric
 * matrix) and b -- is hnm_als_solve_rows_f32's, bit for bit.  Then, in fp32:
 *   x = x0;  r_i = b_i - (A x)_i;  p = r;  rs = r.r
 *   repeat `steps` times:
 *     if !(rs > 0) stop
 *     q = A p;  pq = p.q
 *     if !(pq > 0) stop
 *     a = rs / pq;  x_i = fmaf(a, p_i, x_i);  r_i = fmaf(-a, q_i, r_i)
 *     rn = r.r;  p_i = fmaf(rn / rs, p_i, r_i);  rs = rn
 * Summation order, fixed at compile time and a function of d alone:
 *   (A v)_i = ((P_0 + P_1) + P_2) + P_3,  P_w = the chain acc = fmaf(A_ij, v_j, acc) over
 *             j = w d / 4, ..., (w + 1) d / 4 - 1 ascending, from 0.0f
 *   u.v     = the butterfly sum over 64 slots l of z_l = fmaf(u_{l+64}, v_{l+64}, fl(u_l * v_l))
 *             (d <= 64: z_l = fl(u_l * v_l)), elements >= d being zero: z <- z_l + z_{l ^ 32},
 *             then ^ 16, 8, 4, 2, 1.
 * No floating-point atomics: a row's bits depend on that row's inputs (its x0 included) and on
 * `steps` -- not on B, on the other rows or on the run.  The row rules are
 * hnm_als_solve_rows_f32's: a row without entries gives exact +0.0 (x0 is ignored); an idx entry
 * or a row_ids entry out of range gives a NaN row and HNM_EOOB from hnm_ctx_check; the other rows
 * are untouched; one workgroup owns a row whatever its length.  A non-finite x0 is the caller's
 * problem: that row comes back non-finite, without an error.  steps outside [1, 32], x == NULL
 * with work to do, reg <= 0, alpha < 0 or a non-finite value: HNM_EINVAL; d not a multiple of 16
 * in [16, 128]: HNM_EUNSUPPORTED; B = 0 or n_rows = 0: HNM_OK, nothing launched, x untouched.
 * Workspace: none. */
hnm_status hnm_als_cg_rows_f32(hnm_ctx* ctx, const int64_t* ptr, const int32_t* idx,
                               int64_t n_rows, const float* tab, int64_t tab_rows, int64_t ld,
                               int64_t d, const float* gram, float alpha, float reg,
                               const int64_t* row_ids, int64_t B, float* x, int64_t ldx, int steps);
/* hnm_als_cg_rows_f32 on the weighted system: w f32, aligned with idx, right after it; S, b0,
 * bw, A and b are hnm_als_solve_rows_weighted_f32's bit for bit, the recurrence and its
 * summation order are the ones above.  With every weight 1.0f (or 2^e) the result is
 * hnm_als_cg_rows_f32's bits at alpha (or at 2^e alpha) whenever 1.0f + that alpha is exact.  A
 * negative or non-finite weight gives a NaN row and HNM_EINVAL from hnm_ctx_check; w == NULL
 * with work to do: HNM_EINVAL.  Everything else is hnm_als_cg_rows_f32's. */
hnm_status hnm_als_cg_rows_weighted_f32(hnm_ctx* ctx, const int64_t* ptr, const int32_t* idx,
                                        const float* w, int64_t n_rows, const float* tab,
                                        int64_t tab_rows, int64_t ld, int64_t d,
                                        const float* gram, float alpha, float reg,
                                        const int64_t* row_ids, int64_t B, float* x, int64_t ldx,
                                        int steps);

#ifdef __cplusplus
}
#endif
#endif /* HNM_H_ */
