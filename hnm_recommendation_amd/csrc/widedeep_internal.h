// Shared between widedeep.hip (weight folding, exact fp32 kernels, entry points),
// widedeep_cert.hip (certified split-f16 scan) and widedeep_rescore.hip (refine / best-first /
// re-score cascade).
#pragma once
#include <type_traits>

#include "hnm_device.h"
#include "hnm_internal.h"

// ------------------------------------------------------------------ folded weights, exact tile
struct WdPrep {
  int K1P;     // layer-1 width padded to a multiple of 8
  int RB2;     // layer-2 row blocks of 32
  int OB;      // layer-3 row blocks of 32 (0: two-layer tower)
  float4* W2f; // [RB2][K1P/8][64] float4
  float4* W3f; // [OB][RB2][4][64] float4
  float* b2p;  // [RB2*32] folded layer-2 bias
  float* b3p;  // [OB*32]  folded layer-3 bias
  float* wdp;  // [32*max(OB,RB2)] folded final weights on the last hidden layer
  float* bias; // [1] folded final bias
};

// Per-call preparation shared by the exact and the certified paths: folded weights,
// layer-1 projections P (batch rows) / Q (all items), per-user constants.  `extra` bytes of
// caller scratch follow in the same workspace carve.
struct WdSetup {
  WdPrep pr;
  int K1P;
  float* Pu;
  float* Qi;
  float* cu;
  const float* wI;  // [I] per-item wide term: w->wide_item, or the item-feature fold's output
  char* extra;
};

// The item-feature table of an _ex call: weights, [I, Fi] features (row stride ldf).  on():
// the call has item features (itf == NULL or Fi == 0: the plain entries' behaviour).
struct WdItemFeat {
  const hnm_widedeep_item_features* itf = nullptr;
  const float* f = nullptr;
  int64_t ldf = 0;
  bool on() const { return itf && itf->num_item_features > 0; }
};

__device__ __forceinline__ float bn_a(const float* g, const float* v, int i, float eps) {
  return g[i] / sqrtf(v[i] + eps);
}
__device__ __forceinline__ float bn_c(const float* g, const float* b, const float* m,
                                      const float* v, int i, float eps) {
  return b[i] - m[i] * bn_a(g, v, i, eps);
}

// One wave's exact fp32 deep score for its user against a 32-item tile (the per-pair
// arithmetic of widedeep_score_kernel, shared with the certified path's re-scoring kernel
// so both produce bitwise the same values).  prow / qrow: the user's / lane item's
// pair-permuted layer-1 rows offset by h * K1P / 2 (LDS or global); returns the lane's
// half of w_d' . relu(layer 3) (the caller adds the other half with one shfl_xor 32).
template <int RB2, int OB>
__device__ __forceinline__ float wd_tile_fp32(const float* __restrict__ prow,
                                              const float* __restrict__ qrow, int S4,
                                              const float4* __restrict__ W2f,
                                              const float4* __restrict__ W3f,
                                              const float* __restrict__ cb2,
                                              const float* __restrict__ cb3,
                                              const float* __restrict__ cwd, int lane, int h) {
  constexpr int G2 = RB2 < 4 ? RB2 : 4;  // layer-2 row blocks per pass
  f32x16 acc3[OB > 0 ? OB : 1];
  float fin = 0.f;
#pragma unroll
  for (int ob = 0; ob < (OB > 0 ? OB : 1); ++ob)
    acc3[ob] = f32x16{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

#pragma unroll
  for (int g = 0; g < RB2 / G2; ++g) {
    f32x16 acc2[G2];
#pragma unroll
    for (int gi = 0; gi < G2; ++gi)
      acc2[gi] = f32x16{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    // ---- layer 2 for row blocks g*G2 .. g*G2+G2-1
    float4 af[G2];
#pragma unroll
    for (int gi = 0; gi < G2; ++gi) af[gi] = W2f[((int64_t)(g * G2 + gi) * S4 + 0) * 64 + lane];
    for (int s4 = 0; s4 < S4; ++s4) {
      float4 an[G2];
      const int sn = s4 + 1 < S4 ? s4 + 1 : s4;
#pragma unroll
      for (int gi = 0; gi < G2; ++gi) an[gi] = W2f[((int64_t)(g * G2 + gi) * S4 + sn) * 64 + lane];
      const float4 pv = *reinterpret_cast<const float4*>(prow + 4 * s4);
      const float4 qv = *reinterpret_cast<const float4*>(qrow + 4 * s4);
      const float x0 = fmaxf(pv.x + qv.x, 0.f), x1 = fmaxf(pv.y + qv.y, 0.f);
      const float x2 = fmaxf(pv.z + qv.z, 0.f), x3 = fmaxf(pv.w + qv.w, 0.f);
#pragma unroll
      for (int gi = 0; gi < G2; ++gi) acc2[gi] = mfma32x32x2(af[gi].x, x0, acc2[gi]);
#pragma unroll
      for (int gi = 0; gi < G2; ++gi) acc2[gi] = mfma32x32x2(af[gi].y, x1, acc2[gi]);
#pragma unroll
      for (int gi = 0; gi < G2; ++gi) acc2[gi] = mfma32x32x2(af[gi].z, x2, acc2[gi]);
#pragma unroll
      for (int gi = 0; gi < G2; ++gi) acc2[gi] = mfma32x32x2(af[gi].w, x3, acc2[gi]);
#pragma unroll
      for (int gi = 0; gi < G2; ++gi) af[gi] = an[gi];
    }
    // ---- relu(D2 + b2') feeds layer 3 (or the final dot for a two-layer tower).
    // Layer-3 A fragments are streamed one (gi, r4) step ahead; the scheduling barrier
    // keeps hipcc from hoisting all of them (which spills).
    float4 a3c[OB > 0 ? OB : 1], a3n[OB > 0 ? OB : 1];
    if (OB > 0) {
#pragma unroll
      for (int ob = 0; ob < (OB > 0 ? OB : 1); ++ob)
        a3c[ob] = W3f[((int64_t)(ob * RB2 + g * G2) * 4 + 0) * 64 + lane];
    }
#pragma unroll
    for (int gi = 0; gi < G2; ++gi) {
      const int rb = g * G2 + gi;
      float hv[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) hv[r] = fmaxf(acc2[gi][r] + cb2[rb * 32 + mfma32_row(r, h)], 0.f);
      if (OB > 0) {
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          const int st = gi * 4 + r4;
          if (st + 1 < G2 * 4) {
            const int gn = (st + 1) >> 2, rn = (st + 1) & 3;
#pragma unroll
            for (int ob = 0; ob < (OB > 0 ? OB : 1); ++ob)
              a3n[ob] = W3f[((int64_t)(ob * RB2 + g * G2 + gn) * 4 + rn) * 64 + lane];
          }
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int ob = 0; ob < (OB > 0 ? OB : 1); ++ob) {
            acc3[ob] = mfma32x32x2(a3c[ob].x, hv[4 * r4 + 0], acc3[ob]);
            acc3[ob] = mfma32x32x2(a3c[ob].y, hv[4 * r4 + 1], acc3[ob]);
            acc3[ob] = mfma32x32x2(a3c[ob].z, hv[4 * r4 + 2], acc3[ob]);
            acc3[ob] = mfma32x32x2(a3c[ob].w, hv[4 * r4 + 3], acc3[ob]);
          }
#pragma unroll
          for (int ob = 0; ob < (OB > 0 ? OB : 1); ++ob) a3c[ob] = a3n[ob];
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) fin = fmaf(hv[r], cwd[rb * 32 + mfma32_row(r, h)], fin);
      }
    }
  }
  if (OB > 0) {
#pragma unroll
    for (int ob = 0; ob < (OB > 0 ? OB : 1); ++ob) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int o = ob * 32 + mfma32_row(r, h);
        fin = fmaf(fmaxf(acc3[ob][r] + cb3[o], 0.f), cwd[o], fin);
      }
    }
  }
  return fin;
}

// pair-permuted position t of a layer-1 row -> layer-1 unit (hnm_linear_rows_f32 layout)
__device__ __forceinline__ int wd_korig(int t, int K1P) {
  const int half = K1P >> 1;
  return t < half ? 2 * t : 2 * (t - half) + 1;
}

// ------------------------------------------------------------------ instantiated tower shapes
// X(RB2, OB, CERT): the exact kernel is instantiated for every entry, the certified scan, refine
// and re-score kernels for those with CERT = 1.  This is the only list of shapes: wd_shape,
// wdc_eligible and every launch go through wd_dispatch.
#define WD_SHAPES(X)                                     \
  X(8, 4, 1) X(4, 2, 1) X(2, 1, 1) X(1, 0, 1) X(2, 0, 1) \
  X(4, 0, 0) X(8, 0, 0) X(1, 1, 1) X(4, 4, 0) X(8, 2, 0)

// f(RB2, OB) as integral constants for the table's entry of (rb2, ob) -- with CERT, a certified
// one.  false: there is no such entry and f was not called.
template <bool CERT, class F>
static bool wd_dispatch(int rb2, int ob, F&& f) {
#define WD_X(R, O, C)                                                        \
  if constexpr (C || !CERT)                                                  \
    if (rb2 == R && ob == O) {                                               \
      f(std::integral_constant<int, R>{}, std::integral_constant<int, O>{}); \
      return true;                                                           \
    }
  WD_SHAPES(WD_X)
#undef WD_X
  return false;
}
// a launch whose wd_dispatch found no entry (wd_shape / wdc_eligible admit table entries only)
static inline hnm_status wd_not_instantiated(const WdPrep& pr) {
  hnm_set_error("widedeep: %d/%d row blocks not instantiated", pr.RB2, pr.OB);
  return HNM_EUNSUPPORTED;
}

enum { WDC_THRESH, WDC_DEBUG };  // the scan's MODE: lower-bound lists + segments / per-item output
#define WDC_G2 8  // layer-2 row blocks per pass over k (the x operands are formed once per pass)
// users per wave of the certified scan: 2 for the wide default tower (weight-fragment reuse)
constexpr int wdc_upw(int RB2, int OB) { return RB2 == 8 && OB == 4 ? 2 : 1; }
constexpr int wdc_g2(int RB2, int OB) { return RB2 < WDC_G2 ? RB2 : WDC_G2; }

// ------------------------------------------------------------------ certified path: f16 helpers
typedef _Float16 wh8 __attribute__((ext_vector_type(8)));

// one 16-B fragment per lane from a buffer: a uniform byte offset (SGPR) + lane * 16, so a
// fragment costs one scalar add instead of a 64-bit per-lane address (8 of those held across
// the k loop were spilled and reloaded every step, each reload's vmcnt wait also waiting for
// the prefetched fragments)
// Fragments are held as 4 x 32-bit registers and viewed as 8 f16 only at the MFMA: arrays of
// wh8 were merged into one <64 x half> value whose lane moves the backend emitted as
// v_bfi_b32 "copies" of freshly loaded fragments, each waiting for its load (the prefetch
// distance dropped to zero)
typedef unsigned wfr __attribute__((ext_vector_type(4)));
__device__ __forceinline__ wh8 wd_h(wfr f) { return __builtin_bit_cast(wh8, f); }
__device__ __forceinline__ wfr wd_frag(__amdgpu_buffer_rsrc_t rs, int lane, int byte_off) {
  return __builtin_bit_cast(wfr, __builtin_amdgcn_raw_buffer_load_b128(rs, lane * 16, byte_off, 0));
}

__device__ __forceinline__ f32x16 wd_mfma16(wh8 a, wh8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}

// Split 8 fp32 values into f16 hi / lo halves: hi = f16(x), lo = f16(x - hi) (RNE; the
// remainder is exact in fp32).
__device__ __forceinline__ void wd_split8(const float* x, wh8& hi, wh8& lo) {
  typedef _Float16 wh2 __attribute__((ext_vector_type(2)));
#pragma unroll
  for (int e = 0; e < 8; e += 2) {
    wh2 hp;
    hp[0] = (_Float16)x[e];
    hp[1] = (_Float16)x[e + 1];
    hi[e] = hp[0];
    hi[e + 1] = hp[1];
    lo[e] = (_Float16)__builtin_fmaf((float)hp[0], -1.f, x[e]);
    lo[e + 1] = (_Float16)__builtin_fmaf((float)hp[1], -1.f, x[e + 1]);
  }
}

struct WdCertParams {
  unsigned mx[2];       // max|P| over the batch rows, max|Q| over the items (float bits)
  float s1, sw2, s2, sw3;  // f16 operand scales (powers of two)
  float c2, c3;            // layer-2 accumulator -> x2 scale, layer-3 accumulator -> real
  float inv_s2;
  float g1, g2, g3, g4, cb, absb, rho;
  float sb, inv_sb;        // scale of the bound A rows (one-pass layer 2, WD_BOUND_MFMA)
  int bad;                 // bound unusable: every row takes the exact path
};

struct WdScanArgs {
  const float* Pu;  // [B, K1P]  pair-permuted layer-1 user part (+ b1)
  const float* Qi;  // [I, K1P]  pair-permuted layer-1 item part
  int K1P;
  const wh8* W2hl;
  const wh8* W3hl;
  const wh8* WBf;    // [KB * 2 * 64] bound A fragments (WD_BOUND_MFMA)
  const float* v1;   // [K1P]
  const float* v1o;  // [K1P] v1 without the dropped-pass terms (one-pass layer 2)
  const float* v2;   // [RB2*32]
  const float* b2s;  // [RB2*32] b2' s2
  const float* b3p;  // [OB*32]
  const float* wdp;  // [NL*32]
  const float* cu;   // [B] per-user constant
  const float* wI;   // [I] wide item weight
  const WdCertParams* prm;
  int64_t B, I, ipp;
  int NP;
  const int64_t* mptr;
  const int32_t* midx;
  int K;
  float* lbv;    // [B, NP, K] lower-bound lists
  int32_t* lbi;
  int32_t* segi;  // [B, NP, cap] appended items
  float* segu;    // [B, NP, cap] their upper bounds
  int* cnt;       // [B, NP]
  int cap;
  float* dbg_a;   // DEBUG: [B, lda] approx score, bound
  float* dbg_e;
  int64_t lda;
};

struct WdRescoreArgs {
  const float* Pu;
  const float* Qi;
  int K1P;
  const float4* W2f;
  const float4* W3f;
  const float* b2p;
  const float* b3p;
  const float* wdp;
  const float* cu;
  const float* wI;
  const WdCertParams* prm;
  int64_t B;
  int NP, K, cap;
  const float* Lk;   // [B, K] merged lower-bound lists (slot K-1 = L_u)
  int32_t* segi;     // [B, NP * cap] the scan's segments; wdc_collect compacts each row's
  float* segu;       //   survivors to its front (items, then the refined upper bounds)
  float* segl;       // [B, NP * cap] the survivors' refined lower bounds
  const int* cnt;
  int* ns;           // [B] survivors of each row; -1: the row takes the exact kernel
  int* toff;         // [B + 1] exclusive prefix of the rows' refining tiles (toff[B] = total)
  int32_t* fbrows;   // rows that take the exact kernel
  int* nfb;
  float* ov;
  int64_t* oi;
  unsigned long long* stats;  // HNM_OPT_STATS: rows, candidates re-scored in fp32, fallback rows;
                              // stats[6]: rows that ran the best-first second phase
  // the refining stage (three-pass split-f16 tile, wd_tile_f16x3)
  const wh8* W2hl;
  const wh8* W3hl;
  const float* v1p;  // [K1P] plain v1 (no dropped-pass terms)
  const float* v2p;  // [RB2*32] plain v2
  const float* b2s;  // [RB2*32] b2' s2
  int64_t rstride;   // row stride of segi / segu / segl (NP * cap)
  float* segs;       // [B, NP * cap] the survivors' SCAN upper bounds, compacted by wdc_collect
  const int* rstart; // refining stage: row b's tiles start at position rstart[b] (nullptr: 0)
  float* dbg_a;      // hnm_widedeep_refine_debug_f32: refined score / bound per item, [B, lda]
  float* dbg_e;
  int64_t lda;
};

struct WdcWs {
  WdCertParams* prm;
  wh8* W2hl;
  wh8* W3hl;
  wh8* WBf;
  float* v1;
  float* v1o;
  float* v2o;
  float* v2;
  float* b2s;
  float* part;
  float* lbv;
  int32_t* lbi;
  float* Lv;
  int64_t* Li;
  int32_t* segi;
  float* segu;
  int* cnt;
  float* segl;
  float* segs;
  int32_t* cli;
  int* nA;
  float* tv;
  int* tg;
  int* ns;
  int* toff;
  int32_t* fbrows;
  int* nfb;
  float* fcv;
  int32_t* fci;
  float* fov;
  int64_t* foi;
  int64_t np, ipp;
  int cap;
};

// ------------------------------------------------------------------ widedeep.hip
// validates the weights, fills pr's K1P / RB2 / OB; HNM_EUNSUPPORTED: shape not in WD_SHAPES
hnm_status wd_shape(const hnm_widedeep_weights* w, WdPrep* pr, const WdItemFeat& itf = {});
// Per-call preparation (see WdSetup); S->pr holds wd_shape's result.  With item features the
// fold kernel adds their layer-1 part to Q and writes the wide term wI (wd_fold_item_features).
hnm_status wd_setup(hnm_ctx* ctx, const hnm_widedeep_weights* w, const int64_t* ids, int64_t B,
                    const float* ufeat, size_t extra, WdSetup* S, const WdItemFeat& itf = {});
// item partitions for blocks of upb users: about two workgroups per CU, >= 4 tiles each
void wd_partition(const hnm_ctx* ctx, int64_t B, int64_t I, int64_t* np, int64_t* ipp,
                  int upb = 4);
// Exact fp32 pass: dense scores (dense != nullptr) or the per-partition top-K lists +
// merge for the rows rows[0, n) (rows == nullptr: batch rows 0 .. n).  cv/ci: list scratch
// (values / int32 items, each hnm_align(n * np * K * 4) bytes with wd_partition(n)'s np);
// outputs at the compact row index.
hnm_status wd_exact(hnm_ctx* ctx, const hnm_widedeep_weights* w, const WdSetup& S, int64_t n,
                    const int64_t* mptr, const int32_t* midx, int K, const int32_t* rows,
                    float* cv, int32_t* ci, float* ov, int64_t* oi, float* dense, int64_t ldo,
                    bool timed);

// ------------------------------------------------------------------ widedeep_features.hip
#define WDF_MAX_D 256  // embedding width and feature count the fold's LDS staging covers
#define WDF_MAX_F 256
// Q_i += W1[:, c:c+d] (dif_w f_i + dif_b) in place (pair-permuted, row stride K1P) and, with a
// wide item-feature term, wI_i = wide_item[i] + wide_feat . (wif_w f_i + wif_b)
hnm_status wd_fold_item_features(hnm_ctx* ctx, const hnm_widedeep_weights* w,
                                 const WdItemFeat& itf, int K1P, float* Qi, float* wI);

// ------------------------------------------------------------------ widedeep_cert.hip
bool wdc_eligible(const hnm_ctx* ctx, const WdPrep& pr, int64_t I, int K, bool debug);
// carves the certified path's scratch from base (nullptr: sizes only); returns its bytes
size_t wdc_carve(const hnm_ctx* ctx, const WdPrep& pr, int64_t B, int64_t I, int K, char* base,
                 WdcWs* c);
// bound vectors, scales and the split-f16 weight fragments of this call
hnm_status wdc_prepare(hnm_ctx* ctx, const hnm_widedeep_weights* w, const WdSetup& S, int64_t B,
                       const WdcWs& c);
hnm_status wdc_scan(hnm_ctx* ctx, const hnm_widedeep_weights* w, const WdSetup& S, int64_t B,
                    const int64_t* mptr, const int32_t* midx, int K, const WdcWs& c, int mode,
                    float* dbg_a, float* dbg_e, int64_t lda);

// ------------------------------------------------------------------ widedeep_rescore.hip
// the certified top-K: prepare, scan, merge, cascade, exact fallback rows
hnm_status wdc_topk(hnm_ctx* ctx, const hnm_widedeep_weights* w, const WdSetup& S, int64_t B,
                    const int64_t* mptr, const int32_t* midx, int K, const WdcWs& c, float* ov,
                    int64_t* oi);
