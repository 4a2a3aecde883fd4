// Shared between the units of the certified NeuralCF path: ncf_cert.hip (the entry unit: the
// derivation of the bound, the sampling side, the plan and the orchestration),
// ncf_cert_params.hip (per-call tables, bound statistics, scales, f16 copies), ncf_cert_scan.hip
// (the f16 scan) and ncf_cert_rescore.hip (exact re-scoring).  Kernels stay private to their
// unit; only the host launchers declared at the end cross units.
#pragma once
#include "hnm_device.h"
#include "ncf_internal.h"

constexpr int64_t CERT_MIN_ITEMS = 8192;  // below this the exact LIST kernel is cheaper
constexpr float CERT_RHO = 0.0029296875f; // 6 u16 = 3 * 2^-10
// Deep towers [2 h0, h1, h2, h3] (round 6): the same scan with a third layer; the bound keeps
// its separable form with v = |wp3|^T |W3| |W2| and a factor 7.03 u < 8 u = 2^-8 (derivation at
// cert_scales_kernel's deep branch, ncf_cert_params.hip)
constexpr float CERT_RHO_DEEP = 0.00390625f;
constexpr int CERT_MAX_NP = 64;           // item partitions (candidate segments per row)
constexpr int CERT_PROXY_USERS = 8;       // batch rows that pick the champion sample
#ifndef CERT_CHAMPIONS_AB  // A/B builds only (tools/build_variant.sh)
#define CERT_CHAMPIONS_AB 2048
#endif
constexpr int64_t CERT_CHAMPIONS = CERT_CHAMPIONS_AB;  // champion sample size (item groups), at most
constexpr int64_t CERT_GROUP_MIN = 48;    // items per champion group, at least
// Gated per-user strided sample (round 5).  The champion sample is tight when the rows' best
// items are shared (init weights at the H&M shape: ~70 candidates a row) and degrades to a
// ~1/52 random sample when they are user-specific (trained-like weights: 600+ candidates and
// overflowing segments).  A sample pass over one 32-item tile in CERT_STRIDE for every row gives
// a second lower bound (the larger of the two is used) at ~1/CERT_STRIDE of the scan's cost.
// Whether it pays is predicted on the proxy rows, whose every item the proxy pass scored:
// cert_gate_kernel takes each proxy's K-th over its LEAVE-ONE-OUT champions (picked by the
// other proxies: what a non-proxy row sees) and over the strided tiles, and counts, per proxy,
// the items the main scan would append under each bound (approx + e_i >= tau, tau = kv - 2 Eu:
// cert_tau_kernel); the pass runs when it saves more than CERT_GATE_GAIN
// candidates a row on average -- re-scoring ~250 candidates costs about what the 1/8 pass does
// (bench step: 65 us for 4,096 x 70 candidates against 1/8 of a 1.85 ms scan).  Gated off, the
// pass and its K-th exit at launch.
// Opt-in (HNM_OPT_STRIDED = 1; round 5, A/B on one box: init weights 2.002 -> 2.046 ms a step,
// the gate and the gated-off launches; "norms" weights 3.683 -> 3.092 ms).
constexpr int CERT_STRIDE = 8;
constexpr int64_t CERT_GATE_GAIN = 150;  // (the proxies under-predict the saving: 235 predicted
                                         // for 468 measured on "norms" batch 1)
// scan workgroups per CU (LDS 51.7 KB each; the scan's 168 VGPRs fit three waves per SIMD)
#define HNM_SCAN_OCC 3
constexpr int CERT_WG_PER_CU = HNM_SCAN_OCC;

enum { CM_P, CM_Q, CM_WG, CM_G, CM_B, CM_D, CM_N };

struct CertParams {
  unsigned mx[CM_N];  // float bits of non-negative maxima (reduced from per-block partials)
  float s1, sw, sm, sgu, sgi;
  float s3;           // deep towers: the layer-3 weight scale (1 otherwise)
  float unit, cg;     // scaled score unit; GMF accumulator -> score unit
  float rho;          // the bound's relative factor (CERT_RHO; deep towers CERT_RHO_DEEP)
  float c0, absb, Bmax, Dmax;
  int bad;            // bound not usable: every row takes the exact fallback
};

// layer-1 unit stored at pair-permuted position t (x[h*32+s] = x[2s+h])
__device__ __forceinline__ int korig(int t) { return 2 * (t & 31) + (t >> 5); }

// The scratch region of a call (cert_carve, ncf_cert.hip)
struct CertWs {
  CertParams* prm;
  float *Au, *Cu, *Bi, *Di, *tau, *Eu, *b2s, *kthv, *lb, *pdense, *cdense, *part;
  float *Bs, *Cs;  // Bi, Cu in the scan's test units (cert_convert_kernel)
  int32_t* sidx;  // champion items
  int32_t* sloo;  // [CERT_PROXY_USERS, nch] leave-one-out champions (gate)
  int32_t* sidx2; // [ns] strided sample items
  float* sdense;  // [B, ns] strided sample values (gated)
  float* kth2;    // [B, K] its K best
  int* gate;
  unsigned long long* gcnt;  // [4] gate counters
  int64_t* kthi;
  int *cnt, *flag;
  int32_t *buf, *ovf_cnt, *ovf_rows;
  float* bufd;  // the appended candidates' test values
  _Float16 *P16, *WG16, *Q16, *G16, *W2h, *wmh;
  _Float16 *W3h, *wph;  // deep towers: layer 3 and the prediction weights (f16, scaled)
  float *b3s, *u;       // deep towers: layer-3 bias (scaled); |wp3|^T |W3| (bound statistics)
  float* cv;
  int32_t* ci;
};

struct CertShape {
  int64_t nch, gsz;  // champion sample: nch groups of gsz items
  int64_t ns;        // strided sample: items of tiles 0, S, 2S, ... (CERT_STRIDE)
  Partition part;    // of the main scan
  int capp;          // candidate slots per (row, partition)
};

// Blocks of the statistics launch (item blocks first), whose partials cert_scales_kernel
// reduces: at most 1,024 + 256, the slots of CertWs::part.  fused: ncf_tables_kernel (64-row
// tiles).
struct StatBlocks {
  int items, users;
};

// ------------------------------------------------------------------ f16 scan kernel
// SAMPLE: dense[b][n] = approx - e_i (scanned item n = sidx[n] if set), e_i = the per-item part
//         of the bound, 6u unit (B_i + C_u D_i);
// THRESH: append item n to segment (b, partition) when approx + e_i >= tau_b;
// DEBUG:  dense[b][n] = approx, dense2[b][n] = Eu_b + e_i (the whole bound), scaled units.
enum { SCAN_SAMPLE = 0, SCAN_THRESH = 1, SCAN_DEBUG = 2 };

struct ScanArgs {
  const _Float16* P16;   // [B, 64]
  const _Float16* WG16;  // [B, 64]
  const _Float16* Q16;   // [Itot, 64]
  const _Float16* G16;   // [Itot, 64]
  const _Float16* W2h;   // [32, 64]
  const _Float16* wmh;   // [32]
  const float* b2s;      // [32]
  const _Float16* W3h;   // DEEP: [16, 32] layer-3 weights x s3 (unit, hidden)
  const _Float16* wph;   // DEEP: [16] prediction weights of the layer-3 units x sm
  const float* b3s;      // DEEP: [16] layer-3 bias x s1 sw s3
  const float* Bi;       // [Itot] per-item bound terms (x rho * unit: test units)
  const float* Di;
  const float* Cu;       // [B] per-user bound terms (x rho * unit)
  const float* Eu;       // [B] user-constant part of the bound, scaled (DEBUG)
  const CertParams* prm;
  int64_t B;
  int64_t I;        // scanned items (sample count for the sample pass)
  const int32_t* sidx;  // SAMPLE: scanned item n is item sidx[n] (gather map), if set
  int64_t ipp;
  int NP;
  int upw;  // users per wave (32; fewer for the 8-row proxy pass: every wave gets a pair)
  const int64_t* mptr;
  const int32_t* midx;
  const float* tau;  // [B] scaled thresholds (THRESH)
  int* cnt;          // [B, NP] appended counts (THRESH)
  int32_t* buf;      // [B, NP, capp] appended item ids (THRESH)
  float* segd;       // [B, NP, capp] their test values approx + e_i - tau (THRESH)
  int capp;
  float* dense;      // [B, ldo]
  float* dense2;     // [B, ldo] (DEBUG)
  int64_t ldo;
  const int* gate;   // SAMPLE: *gate == 0 -> the launch does nothing (gated strided sample)
};

// ------------------------------------------------------------------ host launchers across units
// ncf_cert.hip: the shape of a call and its carved scratch (every phase of a call recomputes the
// same plan from the same arguments)
struct CertPlan {
  CertShape sh;
  CertWs ws;
};
CertShape cert_shape(int64_t B, int64_t I, int K, int num_cus);
CertPlan cert_plan(const hnm_ctx* ctx, int64_t B, int64_t I, int K, void* scratch, bool strided);

// ncf_cert_params.hip: bound statistics (unless t.stats: ncf_cert_tables left them), CertParams
// and the f16 operand tables of a call
hnm_status cert_prepare(hnm_ctx* ctx, const hnm_ncf_weights* w, const NcfTabs& t, int64_t B,
                        const CertWs& x, const CertDeep* dp);

// ncf_cert_scan.hip: ncf16_scan_kernel<mode> on ctx->stream -- the deep scan when a.W3h is set,
// else the layout HNM_OPT_SCAN_SHAPE selects
void cert_launch_scan(hnm_ctx* ctx, int mode, dim3 grid, const ScanArgs& a);

// ncf_cert_rescore.hip: exact re-scoring + top-K of the appended candidates (dp: the deep tower's
// chain); rows that need the exact scan are queued at x.ovf_rows[0 .. *x.ovf_cnt)
void cert_launch_rescore(hnm_ctx* ctx, const hnm_ncf_weights* w, const NcfTabs& t, int64_t B,
                         const CertPlan& pl, int K, int short_ok, float* ov, int64_t* oi,
                         const CertDeep* dp);
