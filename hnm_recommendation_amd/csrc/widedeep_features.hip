// Wide&Deep item features for catalogue scoring (the _ex entries of widedeep.hip).
//
// WideDeep.forward (wide_deep.py:190-195, 214-217) feeds per-pair item features into both
// parts: deep input [e_u; e_i; (x_u;) x_i] with x_i = deep_item_features(f_i), and the wide
// cross final_w[feat] . wide_item_features(f_i).  Over a catalogue both depend on the item
// alone, so they fold into the per-item tables every scoring kernel already reads:
//   Q_i  += W1[:, c:c+d] x_i          c = (2 + [Fu > 0]) d; pair-permuted, row stride K1P
//   wI_i  = wide_item[i] + wide_feat . (wif_w f_i + wif_b)
// One kernel, in place over Q (one read and one write of it; no [I, K1P] temporary).  Every
// output is one fp32 fma chain over k = 0 .. d-1 from 0, added once to the stored Q value, so
// the result does not depend on the grid.
//
// A block takes 32-item tiles.  The tile's features are staged in LDS and x of the tile is
// formed there (k-major, so a k step reads the 32 items as eight 16-B broadcasts); the wide term's
// Fi x Fi products are spread over the block (reading them in one thread per item made that
// thread's dependent loads the whole kernel's time).  Thread t owns pair-permuted column cg + t
// of the tile's 32 rows (32 accumulators), and the W1 chunk is staged through LDS 16 k at a
// time, transposed so the threads' reads are conflict free.  Q reads and writes are 1 KB runs
// of a row.
#include <algorithm>

#include "widedeep_internal.h"

#define WDF_TI 32        // items per tile
#define WDF_KC 16        // k per staged W1 chunk
#define WDF_WS (256 + 1) // row stride of the staged chunk (floats)

struct WdFoldArgs {
  const float* W1c;  // w1 + c: [l1, d] with row stride ldw
  int ldw, l1, d, K1P, Fi;
  const float* feat;  // [I, Fi], row stride ldf
  int64_t ldf;
  const float* dif_w;  // [d, Fi]
  const float* dif_b;
  const float* wif_w;  // [Fi, Fi] (wI != nullptr)
  const float* wif_b;
  const float* wide_feat;
  const float* wide_item;
  int64_t I;
  float* Qi;
  float* wI;  // nullptr: no wide item-feature term
};

__global__ __launch_bounds__(256) void wd_item_feature_fold_kernel(WdFoldArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* xs = smem;                  // [d][WDF_TI]
  float* ws = smem + a.d * WDF_TI;   // [WDF_KC][WDF_WS]
  float* red = ws + WDF_KC * WDF_WS;  // [8][WDF_TI] partial wide terms
  float* fs = red + 256;              // [WDF_TI][FS] the tile's features
  const int FS = a.Fi | 1;            // odd row stride: the 32 items' rows spread over the banks
  const int tid = threadIdx.x;
  const int d = a.d, Fi = a.Fi, K1P = a.K1P;
  const int64_t ntiles = hnm_cdiv(a.I, WDF_TI);
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t base = tile * WDF_TI;
    __syncthreads();  // the previous tile's reads of xs / fs / red are done
    // the tile's features (rows past the catalogue: zero)
    for (int e = tid; e < WDF_TI * Fi; e += 256) {
      const int it = e / Fi, q = e % Fi;
      fs[it * FS + q] = base + it < a.I ? a.feat[(base + it) * a.ldf + q] : 0.f;
    }
    __syncthreads();
    // x_i = dif_w f_i + dif_b (hnm_linear_rows_f32's order: the chain, then the bias)
    for (int e = tid; e < d * WDF_TI; e += 256) {
      const int k = e / WDF_TI, it = e % WDF_TI;
      const float* f = fs + it * FS;
      const float* wr = a.dif_w + (int64_t)k * Fi;
      float s = 0.f;
#pragma unroll 8
      for (int q = 0; q < Fi; ++q) s = fmaf(f[q], wr[q], s);
      xs[k * WDF_TI + it] = base + it < a.I ? s + a.dif_b[k] : 0.f;
    }
    if (a.wI) {
      // thread (it, gp): the rows g = gp, gp + 8, .. of wide_item_features, each one chain in q,
      // weighted into a partial sum; the eight partial sums are added in gp order
      const int it = tid & (WDF_TI - 1), gp = tid / WDF_TI;
      const float* f = fs + it * FS;
      float part = 0.f;
      for (int g = gp; g < Fi; g += 256 / WDF_TI) {
        const float* wr = a.wif_w + (int64_t)g * Fi;
        float s = 0.f;
#pragma unroll 8
        for (int q = 0; q < Fi; ++q) s = fmaf(f[q], wr[q], s);
        if (a.wif_b) s += a.wif_b[g];
        part = fmaf(s, a.wide_feat[g], part);
      }
      red[gp * WDF_TI + it] = part;
      __syncthreads();
      if (tid < WDF_TI && base + tid < a.I) {
        float acc = red[tid];
        for (int g = 1; g < 256 / WDF_TI; ++g) acc += red[g * WDF_TI + tid];
        a.wI[base + tid] = a.wide_item[base + tid] + acc;
      }
    }
    for (int cg = 0; cg < K1P; cg += 256) {
      const int p = cg + tid;
      const bool valid = p < K1P && wd_korig(p, K1P) < a.l1;  // padded columns stay zero
      float acc[WDF_TI];
#pragma unroll
      for (int it = 0; it < WDF_TI; ++it) acc[it] = 0.f;
      for (int k0 = 0; k0 < d; k0 += WDF_KC) {
        __syncthreads();  // xs is written; the previous chunk's reads of ws are done
        for (int e = tid; e < 256 * WDF_KC; e += 256) {
          const int pp = e / WDF_KC, kk = e % WDF_KC;
          const int col = cg + pp, k = k0 + kk;
          float v = 0.f;
          if (col < K1P && k < d) {
            const int n = wd_korig(col, K1P);
            if (n < a.l1) v = a.W1c[(int64_t)n * a.ldw + k];
          }
          ws[kk * WDF_WS + pp] = v;
        }
        __syncthreads();
        const int kend = std::min(WDF_KC, d - k0);
        for (int kk = 0; kk < kend; ++kk) {
          const float wv = ws[kk * WDF_WS + tid];
          const float4* xr = reinterpret_cast<const float4*>(xs + (k0 + kk) * WDF_TI);
#pragma unroll
          for (int j = 0; j < WDF_TI / 4; ++j) {
            const float4 x = xr[j];
            acc[4 * j + 0] = fmaf(wv, x.x, acc[4 * j + 0]);
            acc[4 * j + 1] = fmaf(wv, x.y, acc[4 * j + 1]);
            acc[4 * j + 2] = fmaf(wv, x.z, acc[4 * j + 2]);
            acc[4 * j + 3] = fmaf(wv, x.w, acc[4 * j + 3]);
          }
        }
      }
      if (valid) {
        float* q = a.Qi + base * K1P + p;
        const int nrows = (int)std::min<int64_t>(WDF_TI, a.I - base);
#pragma unroll
        for (int it = 0; it < WDF_TI; ++it)
          if (it < nrows) q[it * K1P] += acc[it];
      }
    }
  }
}

hnm_status wd_fold_item_features(hnm_ctx* ctx, const hnm_widedeep_weights* w,
                                 const WdItemFeat& F, int K1P, float* Qi, float* wI) {
  const hnm_widedeep_item_features* itf = F.itf;
  WdFoldArgs a;
  a.W1c = w->w1 + (int64_t)(2 + (w->num_user_features > 0 ? 1 : 0)) * w->d;
  a.ldw = w->l1_in;
  a.l1 = w->l1;
  a.d = w->d;
  a.K1P = K1P;
  a.Fi = itf->num_item_features;
  a.feat = F.f;
  a.ldf = F.ldf;
  a.dif_w = itf->dif_w;
  a.dif_b = itf->dif_b;
  a.wif_w = itf->wif_w;
  a.wif_b = itf->wif_b;
  a.wide_feat = itf->wide_feat;
  a.wide_item = w->wide_item;
  a.I = w->num_items;
  a.Qi = Qi;
  a.wI = wI;
  // <= 81.2 KB (d <= WDF_MAX_D, Fi <= WDF_MAX_F) of the CU's 160 KB; 28.2 KB at d = 64, Fi = 24
  const size_t lds = (size_t)(w->d * WDF_TI + WDF_KC * WDF_WS + 256 + WDF_TI * (a.Fi | 1)) * 4;
  (void)hipFuncSetAttribute((const void*)wd_item_feature_fold_kernel,
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  const int64_t ntiles = hnm_cdiv(a.I, WDF_TI);
  const unsigned grid = (unsigned)std::min<int64_t>(ntiles, 8 * (int64_t)ctx->num_cus);
  hipLaunchKernelGGL(wd_item_feature_fold_kernel, dim3(grid), dim3(256), lds, ctx->stream, a);
  HNM_LAUNCH_CHECK();
  return HNM_OK;
}
