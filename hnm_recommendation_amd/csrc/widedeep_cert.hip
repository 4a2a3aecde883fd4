// ------------------------------------------------------------------ certified f16x3 scan
// Wide&Deep top-K with a CERTIFIED split-f16 pre-filter and exact fp32 re-scoring.
//
// The fp32 MFMA rate is 1/16 of the f16 rate.  A plain f16 scan cannot prune W&D: its
// rigorous error bound (f16 rounding of every operand, propagated through |W3||W2|) spans
// a third of the score spread.  Split operands can: every f16 operand is x = x_hi + x_lo
// (x_hi = f16(x), x_lo = f16(x - x_hi)); layer 2 runs the f16 MFMA passes W_hi x_hi + W_hi x_lo,
// layer 3 W_hi x_hi only (WD_SPLIT_PASSES / WD_SPLIT_PASSES3), with fp32 accumulation: the
// activation's split error is 2^-22 (x_lo kept) or 2^-11 |x| (dropped), and the weights'
// residual R = W - W_hi (known, fixed per call) enters the bound exactly: (|R|^T v) . x.
// Nothing the scan computes is returned: it only prunes; every returned score is recomputed
// by wd_tile_fp32 (the fp32 kernel's own arithmetic), so outputs are bitwise those of the
// exact fp32 path (tests/test_gpu_prefilter.py).
//
// Bound (per pair, real units).  Let x1 = relu(P_u + Q_i) (the fp32 layer-1 values both
// paths read), x2 = relu(D2 + b2'), x3 = relu(D3 + b3') (this scan's values), and
// v3 = |w_d'|, v2 = |W3'|^T v3, v1 = |W2'|^T v2 (for a two-layer tower v2 = |w_d'|).
// The fp32 path's K-term fma chain errs by <= K u sum|terms| (u = 2^-24); the split path's
// MFMA chain by <= 6u (sum|terms| + |acc|) per MFMA (measured <= 3.4u:
// profiles/r1_mfma_semantics_probe.txt (c)) plus 3 * 2^-22 for the split operands; ReLU is
// 1-Lipschitz and errors propagate through |W|, so
//   |approx - exact| <= rho (g1 v1.x1 + g2 v2.x2 + g3 v3.x3 + g4 (|fin| + |c_u| + |w_I|)
//                            + cb) + absb
// and for the dropped passes v1 += (|R2|^T v2) / g1, v2 += (|R3|^T v3) / g2 (W_lo x_hi), and
// v2 *= 1 + 2^-11 / g2 for layer 3's dropped W_hi x_lo (wdc_params_kernel).
// with g1 = (2.125 K1 + 22)u, g2 = (2.125 n2 + 22)u (layer 3) or (32 RB2 + 12)u (final dot
// of a two-layer tower), g3 = (32 NOB + 10)u, g4 = 10u, cb the bias-add roundings, absb the
// f16 subnormal slack (2^-25 per rounding, scaled back), rho = 1 + 2^-6.  The v.x terms are
// three dot products per pair computed next to the MFMAs.
//
// Selection.  Each (user, item partition) keeps a wave-resident top-K of lower bounds
// lb = approx - e: its K-th is a lower bound of the exact K-th score at every moment, so an
// item is appended to the (user, partition) segment when ub = approx + e reaches it (every
// exact top-K item does).  The K-th of the merged lower-bound lists, L_u, filters the
// segments; the survivors (a few hundred per user) are re-scored in fp32.  Rows with an
// unusable bound, fewer than K finite items or an overflowing segment take the exact kernel.
// (This unit: bound parameters, split-f16 operands, scan; the cascade: widedeep_rescore.hip.)
#include <algorithm>

#include "widedeep_internal.h"

// f16 MFMA passes per split layer: 3 = W_hi x_hi + W_hi x_lo + W_lo x_hi; 2 drops W_lo x_hi
// and bounds it explicitly: the dropped term of layer 2 is R2 x1 with R2 = W2' - W2'_hi the
// known residual of the f16 weights, so the bound adds (|R2|^T v2) . x1 (and (|R3|^T v3) . x2
// for layer 3), folded into v1 / v2 by wdc_params_kernel -- a per-element residual, about
// 2^-12.5 |W| on average instead of the 2^-11 worst case.
// Measured (random-init bench weights, 4,096 users x 105,542 items): 3/3 passes 392 ms (51
// candidates a row), 2/2 295 ms (360), **2/1 272-275 ms (393)**, 3/2 375 ms (56), 2/3 314 ms
// (349); one pass on layer 2 with x_lo bounded by 2^-11 |x| overflows every row's segments,
// with the per-pair exact x_lo term (v1o . |x - x_hi|, WD_SPLIT_PASSES = 1) it holds (788
// candidates a row) but runs 283 ms: at half the MFMAs the k loop's operand VALU bounds it.
// Round 3: one pass on layer 2 with the bound's layer-2 terms on the matrix pipe
// (WD_BOUND_MFMA below) and packed operand formation: 232 ms (1,145 candidates a row; their
// exact fp32 re-scoring ~14 ms) vs 2 passes 262-267 ms (393) -- W&D 15.1 k -> 16.5 k users/s
// (profiles/r3g_widedeep_ab.txt).
// The product (round 5: the alternatives above and below are gone from the source; git
// history and DESIGN.md §4 keep them): layer 2 and layer 3 one W_hi x_hi pass each, the
// layer-2 bound terms on the matrix pipe, the k loop in register-set pairs with the weight
// fragments two steps ahead, the accumulators pinned by asm.
// One-pass layer 2 (WD_SPLIT_PASSES = 1) with the bound's layer-2 terms on the matrix pipe: per k
// step and user two v_mfma_f32_16x16x32_f16 whose A rows 0 / 1 carry sb v1 (B = x_hi) and
// sb (v1 + 1.001 v1o / g1) (B = |x_lo|) for the items c / c + 16 of the 32x32 operand layout,
// rounded UP to f16 (wdc_boundfrag_kernel), accumulated over the first row-block pass only:
//   g1 v1.x + 1.001 v1o.|x - x_hi|  <=  g1 (v1.x_hi + (v1 + 1.001 v1o / g1).|x_lo|)
// (x = x_hi + x_lo exactly, |x_lo| rounded to f16 costs 2^-10 relative, in the A rows).  This
// replaces the 16 VALU fmas per user and k step that bound the VALU-bound one-pass kernel.
// (Measured and dropped, round 3: |x_lo| := 0 where z < 0 -- 789 instead of 1,145 candidates
// a row but a 5.7 ms slower scan, the same step; weight fragments three steps ahead.)

// One pass over k with every layer-2 row block (G2 = RB2 = 8, two users: 256 accumulator
// registers = the whole AGPR file).  Every other accumulator is pinned by inline asm so the
// compiler keeps layer 2's in place (left to it, it moved ~140 accumulator registers per k step
// between the files): the bound MFMAs' in VGPRs ("+v"), layer 3's in the AGPRs layer 2 has
// released ("=a" / "+a").  Layer 2's own MFMAs stay builtins: as asm they were issued in one
// block, with no vector work between them (a step then costs MFMA + VALU time, not the max).
// Wait states (nothing is padded inside an asm string): NOP = 2 states before an MFMA whose
// B operand a VALU instruction may just have written; an accumulate chain (C = the previous
// MFMA's D, same shape) needs none; the results -> any other reader: the s_nop fences after
// each loop.
// (As builtins the bound MFMAs cost 128 accumulator moves a step, measured.)
template <bool NOP>
__device__ __forceinline__ void wd_mfma16x_accv(f32x4& c, const wh8& a, const wh8& b) {
  if (NOP)
    asm volatile("s_nop 1\n\tv_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(c) : "v"(a), "v"(b));
  else
    asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(c) : "v"(a), "v"(b));
}
// D = a b (C = 0), D in accumulator registers
template <bool NOP>
__device__ __forceinline__ void wd_mfma_acc0(f32x16& d, const wh8& a, const wh8& b) {
  if (NOP)
    asm volatile("s_nop 1\n\tv_mfma_f32_32x32x16_f16 %0, %1, %2, 0" : "=a"(d) : "v"(a), "v"(b));
  else
    asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, 0" : "=a"(d) : "v"(a), "v"(b));
}
// c += a b in place, c in accumulator registers
template <bool NOP>
__device__ __forceinline__ void wd_mfma_acc(f32x16& c, const wh8& a, const wh8& b) {
  if (NOP)
    asm volatile("s_nop 1\n\tv_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+a"(c) : "v"(a), "v"(b));
  else
    asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+a"(c) : "v"(a), "v"(b));
}

// c - (float)h for the low (SEL = 0) or high (SEL = 1) f16 half of a packed register: one
// v_fma_mix_f32 instead of a convert and a subtract (the split operand's remainder, exact)
template <int SEL>
__device__ __forceinline__ float wd_sub_half(unsigned packed, float c) {
  float d;
  if (SEL == 0)
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(d) : "v"(packed), "v"(c));
  else
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(d) : "v"(packed), "v"(c));
  return d;
}

// One-pass layer 2 operands from the unclamped layer-1 sums z (WD_BOUND_MFMA): per pair of
// elements one packed fma (z = q s1 + p), one RNE convert, one packed max: x_hi = relu(z)_hi
// (= max(f16(z), 0): rounding is monotonic), and |x_lo| = |f16(z - f16(z))| by v_fma_mix{lo,hi}
// (exact difference, one RNE rounding) + one and.  For z < 0 the true x_lo is 0, so |x_lo| here
// only over-estimates the bound term it feeds.  6 VALU per 2 elements instead of 9.
typedef _Float16 wh2 __attribute__((ext_vector_type(2)));
typedef float wf2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void wd_split_relu2(wf2 z, wh2& hi, unsigned& alo) {
  const wh2 hu = __builtin_convertvector(z, wh2);
  hi = __builtin_elementwise_max(hu, (wh2){(_Float16)0.f, (_Float16)0.f});
  const unsigned hub = __builtin_bit_cast(unsigned, hu);
  unsigned d;  // both halves written by the pair (no initialising move)
  asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]\n\t"
      "v_fma_mixhi_f16 %0, %1, -1.0, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]"
      : "=&v"(d) : "v"(hub), "v"(z.x), "v"(z.y));
  alo = d & 0x7fff7fffu;
}

__device__ __forceinline__ float wd_pow2_below_inv(float m) {  // largest 2^e with m 2^e <= 1
  int e;
  (void)frexpf(m, &e);
  return ldexpf(1.f, -e);
}

__device__ __forceinline__ float wd_nmax(float a, float b) { return (b > a || b != b) ? b : a; }

// per-block maxima of |P| (rows [0, B)) and |Q| (items) -> part[blk * 2 + {0, 1}]
__global__ __launch_bounds__(256) void wdc_stats_kernel(const float* __restrict__ Pu,
                                                        int64_t nP, const float* __restrict__ Qi,
                                                        int64_t nQ, float* __restrict__ part) {
  __shared__ float red[2][4];
  float mp = 0.f, mq = 0.f;
  const int64_t stride = (int64_t)gridDim.x * 256 * 4;
  for (int64_t e = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; e < nP; e += stride) {
    const float4 v = *reinterpret_cast<const float4*>(Pu + e);
    mp = wd_nmax(mp, wd_nmax(wd_nmax(fabsf(v.x), fabsf(v.y)), wd_nmax(fabsf(v.z), fabsf(v.w))));
  }
  for (int64_t e = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; e < nQ; e += stride) {
    const float4 v = *reinterpret_cast<const float4*>(Qi + e);
    mq = wd_nmax(mq, wd_nmax(wd_nmax(fabsf(v.x), fabsf(v.y)), wd_nmax(fabsf(v.z), fabsf(v.w))));
  }
  for (int o = 32; o >= 1; o >>= 1) {
    mp = wd_nmax(mp, __shfl_xor(mp, o));
    mq = wd_nmax(mq, __shfl_xor(mq, o));
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    red[0][wave] = mp;
    red[1][wave] = mq;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    float m = red[threadIdx.x][0];
    for (int w = 1; w < 4; ++w) m = wd_nmax(m, red[threadIdx.x][w]);
    part[blockIdx.x * 2 + threadIdx.x] = m;
  }
}

// One block: bound vectors v1 (pair-permuted positions), v2, scales, coefficients.
__global__ __launch_bounds__(256) void wdc_params_kernel(hnm_widedeep_weights w, WdPrep p,
                                                         const float* __restrict__ part, int nblk,
                                                         float* __restrict__ v1,
                                                         float* __restrict__ v2,
                                                         float* __restrict__ b2s,
                                                         WdCertParams* prm,
                                                         float* __restrict__ v1o,
                                                         float* __restrict__ v2o) {
  __shared__ float sv2[256];
  __shared__ float red[8][4];
  __shared__ float bc[8];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K1P = p.K1P, n2 = p.RB2 * 32, NOB = p.OB > 0 ? p.OB : 1;
  const int l1 = w.l1, l2 = w.l2, l3 = w.l3;
  float mp = 0.f, mq = 0.f;
  for (int b = tid; b < nblk; b += 256) {
    mp = wd_nmax(mp, part[2 * b]);
    mq = wd_nmax(mq, part[2 * b + 1]);
  }
  // v2 (layer-2 rows): OB > 0: sum_m |W3'_mj| |wd'_m|; two-layer tower: |wd'_j|
  float mW3 = 0.f, sv2b = 0.f, swdb3 = 0.f, sumwd = 0.f;
  for (int jx = tid; jx < n2; jx += 256) {
    float v = 0.f;
    if (jx < l2) {
      if (p.OB > 0) {
        const float a2 = bn_a(w.bn2_w, w.bn2_var, jx, w.eps);
        for (int m = 0; m < l3; ++m) {
          const float wv = fabsf(w.w3[(int64_t)m * l2 + jx] * a2);
          mW3 = wd_nmax(mW3, wv);
          v = fmaf(wv, fabsf(p.wdp[m]), v);
        }
      } else {
        v = fabsf(p.wdp[jx]);
      }
    }
    sv2[jx] = v;
    v2[jx] = v;
    v2o[jx] = v;  // before the dropped-pass terms (the re-scoring cascade's three-pass tile)
    sv2b = fmaf(v, fabsf(p.b2p[jx]), sv2b);
  }
  for (int m = tid; m < NOB * 32; m += 256) {
    if (p.OB > 0) swdb3 = fmaf(fabsf(p.wdp[m]), fabsf(p.b3p[m]), swdb3);
    sumwd += fabsf(p.wdp[m]);
  }
  __syncthreads();
  // v1 (pair-permuted positions) and layer-2 row statistics
  float mW2 = 0.f, sv1 = 0.f;
  for (int t = tid; t < K1P; t += 256) {
    const int k = wd_korig(t, K1P);
    float v = 0.f;
    if (k < l1) {
      const float a1 = bn_a(w.bn1_w, w.bn1_var, k, w.eps);
      for (int jx = 0; jx < l2; ++jx) {
        const float wv = fabsf(w.w2[(int64_t)jx * l1 + k] * a1);
        mW2 = wd_nmax(mW2, wv);
        v = fmaf(wv, sv2[jx], v);
      }
    }
    v1[t] = v;
    v1o[t] = v;  // before the dropped-pass terms: the per-pair x_lo term of a one-pass layer 2
    sv1 += v;
  }
  const float zmax = mp + mq;
  float m2 = 0.f, sumv2 = 0.f;  // max_j (zmax sum_k |W2'_jk| + |b2'_j|)
  for (int jx = tid; jx < l2; jx += 256) {
    float rs = 0.f;
    for (int k = 0; k < l1; ++k)
      rs += fabsf(w.w2[(int64_t)jx * l1 + k] * bn_a(w.bn1_w, w.bn1_var, k, w.eps));
    m2 = wd_nmax(m2, fmaf(zmax, rs, fabsf(p.b2p[jx])));
    sumv2 += sv2[jx];
  }
  float vals[8] = {mp, mq, mW2, mW3, m2, sv1, sv2b, swdb3};
  for (int q = 0; q < 8; ++q) {
    float x = vals[q];
    for (int o = 32; o >= 1; o >>= 1) {
      const float y = __shfl_xor(x, o);
      x = q < 5 ? wd_nmax(x, y) : x + y;
    }
    if (lane == 0) red[q][wave] = x;
  }
  float sums2[2] = {sumv2, sumwd};
  for (int q = 0; q < 2; ++q)
    for (int o = 32; o >= 1; o >>= 1) sums2[q] += __shfl_xor(sums2[q], o);
  __shared__ float red2[2][4];
  if (lane == 0) {
    red2[0][wave] = sums2[0];
    red2[1][wave] = sums2[1];
  }
  __syncthreads();
  if (tid < 8) {
    float x = red[tid][0];
    for (int wv = 1; wv < 4; ++wv) x = tid < 5 ? wd_nmax(x, red[tid][wv]) : x + red[tid][wv];
    bc[tid] = x;
  }
  __syncthreads();
  const float M2 = bc[4];
  const float lim = 1.0e30f;
  bool bad = (K1P & 15) != 0;
  for (int q = 0; q < 8; ++q) bad |= !(bc[q] <= lim);
  const float F16R = 16384.f;  // scaled operand magnitudes <= 2^14
  const float s1 = bc[0] + bc[1] > 0.f ? F16R * wd_pow2_below_inv(bc[0] + bc[1]) : 1.f;
  const float sw2 = bc[2] > 0.f ? F16R * wd_pow2_below_inv(bc[2]) : 1.f;
  const float s2 = M2 > 0.f ? F16R * wd_pow2_below_inv(M2) : 1.f;
  const float sw3 = bc[3] > 0.f ? F16R * wd_pow2_below_inv(bc[3]) : 1.f;
  for (float sc : {s1, sw2, s2, sw3}) bad |= !(sc >= 1e-25f && sc <= 1e25f);
  // b2' in x2 units
  for (int jx = tid; jx < n2; jx += 256) b2s[jx] = p.b2p[jx] * s2;
  if (!bad) {
    // the dropped W_lo x_hi passes: v1 += (|R2|^T v2) / g1 and, with a
    // third layer, v2 += (|R3|^T v3) / g2, R = W' - f16(W' sw) / sw exactly as wdc_convert_kernel
    // rounds it; 1 + 2^-10 covers |x_hi| <= (1 + 2^-11)|x| and the fp32 sums.  Each thread
    // updates the entries it wrote above (same t / jx mapping).
    const float uu = 5.9604645e-08f;
    const float g1c = (2.125f * K1P + 22.f) * uu;
    const float g2c = (2.125f * n2 + 22.f) * uu;
    const float fr = 1.0009765625f;
    // one pass on layer 3 also drops W_hi x_lo: |x_lo| <= 2^-11 |x| (RNE), i.e. v2 += 2^-11 v2 /
    // g2; a one-pass layer 2 bounds its x_lo term per pair instead (scan: v1o . |x - x_hi|)
    const float xl1 = 0.f;
    const float xl3 = 4.8828125e-4f;
    for (int t = tid; t < K1P; t += 256) {
      const int k = wd_korig(t, K1P);
      if (k >= l1) continue;
      float r = 0.f;
      for (int jx = 0; jx < l2; ++jx) {
        float v = w.w2[(int64_t)jx * l1 + k] * bn_a(w.bn1_w, w.bn1_var, k, w.eps);
        v *= sw2;
        r = fmaf(fabsf(v - (float)(_Float16)v), sv2[jx], r);
      }
      v1[t] = v1[t] * (1.f + fr * xl1 / g1c) + fr * (r / sw2) / g1c;
    }
    if (p.OB > 0) {
      for (int jx = tid; jx < l2; jx += 256) {
        float r = 0.f;
        for (int m = 0; m < l3; ++m) {
          float v = w.w3[(int64_t)m * l2 + jx] * bn_a(w.bn2_w, w.bn2_var, jx, w.eps);
          v *= sw3;
          r = fmaf(fabsf(v - (float)(_Float16)v), fabsf(p.wdp[m]), r);
        }
        v2[jx] = v2[jx] * (1.f + fr * xl3 / g2c) + fr * (r / sw3) / g2c;
      }
    }
  }
  // scale of the bound A rows: max over k of v1 + (1.001 / g1) v1o, the larger row
  __shared__ float ared[4];
  __syncthreads();  // every thread's v1 / v1o entries are written
  float amax = 0.f;
  {
    const float g1c = (2.125f * K1P + 22.f) * 5.9604645e-08f;
    for (int t = tid; t < K1P; t += 256) amax = wd_nmax(amax, v1[t] + (1.0009765625f / g1c) * v1o[t]);
  }
  for (int o = 32; o >= 1; o >>= 1) amax = wd_nmax(amax, __shfl_xor(amax, o));
  if (lane == 0) ared[wave] = amax;
  __syncthreads();
  if (tid != 0) return;
  amax = wd_nmax(wd_nmax(ared[0], ared[1]), wd_nmax(ared[2], ared[3]));
  const float u = 5.9604645e-08f;  // 2^-24
  const float phi = 2.98023224e-08f;  // 2^-25: half the f16 subnormal spacing
  const float sumv2t = red2[0][0] + red2[0][1] + red2[0][2] + red2[0][3];
  const float sumwdt = red2[1][0] + red2[1][1] + red2[1][2] + red2[1][3];
  WdCertParams c;
  c.mx[0] = __float_as_uint(bc[0]);
  c.mx[1] = __float_as_uint(bc[1]);
  c.s1 = s1;
  c.sw2 = sw2;
  c.s2 = s2;
  c.sw3 = sw3;
  c.c2 = s2 / (s1 * sw2);
  c.c3 = 1.f / (s2 * sw3);
  c.inv_s2 = 1.f / s2;
  c.g1 = (2.125f * K1P + 22.f) * u;
  c.g2 = (p.OB > 0 ? 2.125f * n2 + 22.f : 32.f * p.RB2 + 12.f) * u;
  c.g3 = p.OB > 0 ? (32.f * NOB + 10.f) * u : 0.f;
  c.g4 = 10.f * u;
  c.cb = 4.f * u * (bc[6] + bc[7]);
  // subnormal slack: x1 / W2 / x2 / W3 roundings, 2 per operand (hi and lo), doubled
  c.absb = 4.f * phi *
           (bc[5] / s1 + sumv2t * K1P * (bc[0] + bc[1]) / sw2 + sumv2t / s2 +
            (p.OB > 0 ? sumwdt * n2 * M2 / sw3 : 0.f));
  c.rho = 1.015625f;
  c.sb = amax > 0.f ? 16384.f * wd_pow2_below_inv(amax * 1.01f) : 1.f;
  c.inv_sb = 1.f / c.sb;
  bad |= !(amax <= lim) || !(c.sb >= 1e-30f && c.sb <= 1e30f);
  bad |= !(c.absb <= lim) || !(c.c2 > 0.f && c.c2 <= lim) || !(c.c3 > 0.f && c.c3 <= lim);
  c.bad = bad;
  *prm = c;
}

// Split-f16 A operands.  W2hl[((rb * KB + kb) * 2 + hl) * 64 + lane][t]: row rb*32 +
// (lane & 31), pair-permuted position 16 kb + 8 (lane >> 5) + t; W3hl[((ob * 2 RB2 + kb3) *
// 2 + hl) * 64 + lane][t]: row ob*32 + (lane & 31), layer-2 row (kb3 >> 1) * 32 +
// mfma32_row(8 (kb3 & 1) + t, lane >> 5) -- the order in which layer 2's accumulator
// registers become layer 3's B operand.
__global__ __launch_bounds__(256) void wdc_convert_kernel(hnm_widedeep_weights w, WdPrep p,
                                                          const WdCertParams* __restrict__ prm,
                                                          wh8* __restrict__ W2hl,
                                                          wh8* __restrict__ W3hl) {
  const int K1P = p.K1P, KB = K1P / 16;
  const float sw2 = prm->sw2, sw3 = prm->sw3;
  const int64_t n2 = (int64_t)p.RB2 * KB * 64, n3 = (int64_t)p.OB * 2 * p.RB2 * 64;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n2 + n3;
       e += (int64_t)gridDim.x * 256) {
    const int lane = (int)(e & 63), h = lane >> 5, r = lane & 31;
    wh8 hi, lo;
    if (e < n2) {
      const int64_t q = e >> 6;
      const int kb = (int)(q % KB), rb = (int)(q / KB);
      const int o = rb * 32 + r;
      for (int t = 0; t < 8; ++t) {
        const int k = wd_korig(16 * kb + 8 * h + t, K1P);
        float v = 0.f;
        if (o < w.l2 && k < w.l1) v = w.w2[(int64_t)o * w.l1 + k] * bn_a(w.bn1_w, w.bn1_var, k, w.eps);
        v *= sw2;
        const _Float16 vh = (_Float16)v;
        hi[t] = vh;
        lo[t] = (_Float16)(v - (float)vh);
      }
      W2hl[(q * 2 + 0) * 64 + lane] = hi;
      W2hl[(q * 2 + 1) * 64 + lane] = lo;
    } else {
      const int64_t q = (e - n2) >> 6;
      const int kb3 = (int)(q % (2 * p.RB2)), ob = (int)(q / (2 * p.RB2));
      const int o = ob * 32 + r;
      for (int t = 0; t < 8; ++t) {
        const int jx = (kb3 >> 1) * 32 + mfma32_row(8 * (kb3 & 1) + t, h);
        float v = 0.f;
        if (o < w.l3 && jx < w.l2) v = w.w3[(int64_t)o * w.l2 + jx] * bn_a(w.bn2_w, w.bn2_var, jx, w.eps);
        v *= sw3;
        const _Float16 vh = (_Float16)v;
        hi[t] = vh;
        lo[t] = (_Float16)(v - (float)vh);
      }
      W3hl[(q * 2 + 0) * 64 + lane] = hi;
      W3hl[(q * 2 + 1) * 64 + lane] = lo;
    }
  }
}

// f16 rounded toward +inf (for v >= 0: every bound operand is nonnegative)
__device__ __forceinline__ _Float16 wd_f16_up(float v) {
  _Float16 h = (_Float16)v;
  if ((float)h < v) h = __builtin_bit_cast(_Float16, (unsigned short)(__builtin_bit_cast(unsigned short, h) + 1));
  return h;
}

// Bound A fragments of the one-pass layer 2 (WD_BOUND_MFMA): WBf[(typ * KB + kb) * 64 + lane], the
// 16x16x32 A operand (lane l holds A[l & 15][8 (l >> 4) + t]).  Row 0 takes the k-groups of items
// c (lane groups 0 / 2 of the 32x32 B layout: k = 16 kb + 8 (g >> 1) + t), row 1 those of items
// c + 16 (groups 1 / 3); every other entry is 0.  typ 0 multiplies x_hi: sb v1; typ 1 multiplies
// |x_lo|: sb (v1 + 1.001 v1o / g1) (1 + 2^-10) -- the 2^-10 covers |x_lo|'s f16 rounding, the
// 2^-20 the fp32 evaluation; rounded up.
__global__ __launch_bounds__(256) void wdc_boundfrag_kernel(const WdCertParams* __restrict__ prm,
                                                            const float* __restrict__ v1,
                                                            const float* __restrict__ v1o, int K1P,
                                                            wh8* __restrict__ WBf) {
  const int KB = K1P / 16;
  const float sb = prm->sb;
  const float c1 = 1.0009765625f / ((2.125f * K1P + 22.f) * 5.9604645e-08f);
  for (int e = blockIdx.x * 256 + threadIdx.x; e < KB * 2 * 64; e += gridDim.x * 256) {
    const int lane = e & 63, q = e >> 6, kb = q % KB, typ = q / KB;
    const int row = lane & 15, g = lane >> 4;
    wh8 out = {};
    if (row == (g & 1)) {
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        const int k = 16 * kb + 8 * (g >> 1) + t;
        const float v = typ == 0 ? v1[k] : (v1[k] + c1 * v1o[k]) * (1.0009765625f * 1.00000095367f);
        out[t] = wd_f16_up(v * sb);
      }
    }
    WBf[e] = out;
  }
}

#define WDC_VPM 4  // VALU instructions scheduled per MFMA in the k loop's interleave
#ifndef WD_STAMPS  // diagnostic builds only: per-phase s_memtime cycle sums (tools/wd_stamps.py)
#define WD_STAMPS 0
#endif
#if WD_STAMPS
__device__ unsigned long long wd_stamp_acc[4];  // k loop, layer-2 epilogue + layer 3, final, tiles
extern "C" int hnm_debug_wd_stamps(unsigned long long* out) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(wd_stamp_acc), sizeof(wd_stamp_acc));
}
extern "C" int hnm_debug_wd_stamps_reset() {
  const unsigned long long z[4] = {0, 0, 0, 0};
  return (int)hipMemcpyToSymbol(HIP_SYMBOL(wd_stamp_acc), z, sizeof(z));
}
#endif

// Block = 4 waves x UPW users each (rows blockIdx.x * 4 UPW + wave * UPW + v) x item
// partition blockIdx.y; the Q tile (32 items, fp32) is shared through LDS.  Per tile a wave
// runs layer 2 as RB2 x K1P/16 f16 MFMAs per user (one W_hi x_hi pass; G2 row blocks per pass
// over k, the next layer fed from the accumulators as each pass completes), layer 3 as
// OB x 2 RB2, then the bound.  UPW = 2: every weight fragment loaded from
// L2 feeds two users' MFMAs -- the fragment stream is what bounds the one-user variant
// (tools/wd_ablation.sh: no weight loads = -19% time).  Round 3 product: G2 = RB2 = 8, one
// pass over k (the x operands, most of the k loop's vector work, formed once per tile instead
// of once per pass: 217 -> 160-164 ms), layer 2's 256 accumulators in the AGPR file, layer 3
// after all of layer 2 (ASMACC below).
template <int RB2, int OB, int G2, int MODE, int UPW>
__global__ __launch_bounds__(256, UPW == 1 ? 2 : 1) void wdc_scan_kernel(WdScanArgs A) {
  constexpr int NOB = OB > 0 ? OB : 1;
  constexpr int NL = OB > 0 ? OB : RB2;
  constexpr int NU = 4 * UPW;  // users per block
  constexpr bool ASMACC = G2 == RB2;  // accumulators pinned by asm (the 8 x 4 product shape)
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int K1P = A.K1P, KB = K1P / 16, QRS = K1P + 4;
  float* qs = smem;               // [32][QRS]
  float* ps = qs + 32 * QRS;      // [NU][K1P]
  float* b2l = ps + NU * K1P;     // [RB2*32]
  float* v2l = b2l + RB2 * 32;    // [RB2*32]
  float* b3l = v2l + RB2 * 32;    // [NOB*32]
  float* wdl = b3l + NOB * 32;    // [NL*32]
  // qs / qn (offset qn_off): the Q tile being scored and the next one, filled during its k loop
  const int qn_off = (int)(wdl + NL * 32 - smem);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, j = lane & 31;
  const __amdgpu_buffer_rsrc_t w2rs =
      __builtin_amdgcn_make_buffer_rsrc((void*)A.W2hl, 0, RB2 * KB * 2 * 1024, 0x00020000);
  const __amdgpu_buffer_rsrc_t wbrs =
      __builtin_amdgcn_make_buffer_rsrc((void*)A.WBf, 0, KB * 2 * 1024, 0x00020000);
  const __amdgpu_buffer_rsrc_t w3rs =
      __builtin_amdgcn_make_buffer_rsrc((void*)A.W3hl, 0, NOB * 2 * RB2 * 2 * 1024, 0x00020000);
  const int64_t ublk = (int64_t)blockIdx.x * NU;
  const int p = blockIdx.y;
  const int64_t part_start = (int64_t)p * A.ipp;
  const int64_t part_end = std::min<int64_t>(A.I, part_start + A.ipp);
  // P and Q are staged pre-scaled by s1 (a power of two: relu(s1 p + s1 q) = s1 relu(p + q)
  // exactly), so the k loop forms the f16 operands without a multiply
  const float s1 = A.prm->s1, inv_s1 = 1.f / s1;
  for (int e = tid; e < NU * K1P / 4; e += 256) {
    const int r = e / (K1P / 4), c = e % (K1P / 4);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ublk + r < A.B) v = *reinterpret_cast<const float4*>(A.Pu + (ublk + r) * K1P + 4 * c);
    v.x *= s1; v.y *= s1; v.z *= s1; v.w *= s1;
    *reinterpret_cast<float4*>(ps + r * K1P + 4 * c) = v;
  }
  for (int e = tid; e < RB2 * 32; e += 256) {
    b2l[e] = A.b2s[e];
    v2l[e] = A.v2[e];
  }
  for (int e = tid; e < NOB * 32; e += 256) b3l[e] = OB > 0 ? A.b3p[e] : 0.f;
  for (int e = tid; e < NL * 32; e += 256) wdl[e] = A.wdp[e];
  const float c2 = A.prm->c2, c3 = A.prm->c3, inv_s2 = A.prm->inv_s2;
  const float g1 = A.prm->g1, g2 = A.prm->g2, g3 = A.prm->g3, g4 = A.prm->g4;
  const float cbd = A.prm->cb, absb = A.prm->absb, rho = A.prm->rho;

  int64_t bu[UPW];
  bool act[UPW];
  float cub[UPW];
  WaveTopK<1> L[UPW];
  int nm[UPW], mpos[UPW], mend[UPW], count[UPW];
#pragma unroll
  for (int v = 0; v < UPW; ++v) {
    bu[v] = ublk + wave * UPW + v;
    act[v] = bu[v] < A.B;
    cub[v] = act[v] ? A.cu[bu[v]] : 0.f;
    L[v].init();
    nm[v] = INT_BIG;
    mpos[v] = mend[v] = count[v] = 0;
    if (A.mptr && act[v]) {
      int64_t lo = A.mptr[bu[v]], hi = A.mptr[bu[v] + 1];
      while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (A.midx[mid] < part_start) lo = mid + 1;
        else hi = mid;
      }
      mpos[v] = (int)lo;
      mend[v] = (int)A.mptr[bu[v] + 1];
      nm[v] = mpos[v] < mend[v] ? A.midx[mpos[v]] : INT_BIG;
    }
  }

  const int64_t ntiles = part_end > part_start ? hnm_cdiv(part_end - part_start, TILE) : 0;
  // Q tiles are double-buffered: tile t + 1 is copied into the other buffer while tile t is
  // scored, one 8-column slice of its 32 rows per k step (K1P / 8 = NG KB / QPS steps; a
  // thread moves one dword of row tid / 8): step s writes the slice loaded during step s - 1
  // and loads slice s + 1 -- no exposed load latency, one barrier a tile, no branches in the
  // k loop (kernel 270 -> 261 ms; the tile load + barrier it replaces cost 6 %).  The loads are
  // buffer loads over the next tile's valid rows (a scalar column offset; rows past the
  // partition, and the slice after the last, read as 0 by the bounds check).  Q is staged
  // unscaled: the k loop forms s1 x1 = fma(q, s1, p s1), which rounds exactly like s1 (p + q)
  // (s1 is a power of two; scaling in the copy instead, one more VALU a step: 275 ms).
  constexpr int NG = RB2 / G2, QPS = 2 / NG;
  static_assert(NG * QPS == 2, "one tile's copy spans the tile's k steps");
  const int qrow_t = tid >> 3, qcol_t = tid & 7;
  const int qvoff = (qrow_t * K1P + qcol_t) * 4;
  auto qrsrc = [&](int64_t nb) {  // the tile at nb: its rows inside the partition
    const int64_t rows = std::max<int64_t>(0, std::min<int64_t>(TILE, part_end - nb));
    const float* src = A.Qi + std::min<int64_t>(nb, part_end - 1) * K1P;
    return __builtin_amdgcn_make_buffer_rsrc((void*)src, 0, (int)(rows * K1P * 4), 0x00020000);
  };
  auto qload = [&](__amdgpu_buffer_rsrc_t rs, int c) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, qvoff, c * 4, 0));
  };
  if (ntiles > 0) {
    const __amdgpu_buffer_rsrc_t rs = qrsrc(part_start);
    for (int c = 0; c < K1P; c += 8) smem[qrow_t * QRS + qcol_t + c] = qload(rs, c);
  }
  unsigned long long st_acc[4] = {0, 0, 0, 0}, st_t0 = 0, st_t1 = 0;
  for (int64_t t = 0; t < ntiles; ++t) {
    if (WD_STAMPS) st_t0 = __builtin_amdgcn_s_memtime();
    const int64_t base = part_start + t * TILE;
    const int cur_off = (t & 1) ? qn_off : 0, nxt_off = (t & 1) ? 0 : qn_off;
    const __amdgpu_buffer_rsrc_t qrs = qrsrc(base + TILE);
    float* const qdst = smem + nxt_off + qrow_t * QRS + qcol_t;
    __syncthreads();
    if (!act[0]) {  // users are assigned in order: the wave has none, it only copies
      for (int c = 0; c < K1P; c += 8) qdst[c] = qload(qrs, c);
      continue;
    }
    float qv[QPS];
#pragma unroll
    for (int e = 0; e < QPS; ++e) qv[e] = qload(qrs, 8 * e);

    const float* qrow = smem + cur_off + j * QRS + 8 * h;
    f32x16 acc3[UPW][NOB];
    float fin[UPW], bx2[UPW], bx3[UPW];
#pragma unroll
    for (int v = 0; v < UPW; ++v) fin[v] = bx2[v] = bx3[v] = 0.f;
    // the bound's layer-2 terms on the matrix pipe: 16x16 accumulators, rows 0 / 1
    // of lanes 0-15 = items c / c + 16
    f32x4 accb[UPW];
#pragma unroll
    for (int v = 0; v < UPW; ++v) accb[v] = f32x4{0.f, 0.f, 0.f, 0.f};
    // one pass over k per G2 row blocks (NG passes); the bound MFMAs: with NG = 2 pass 0 takes
    // the x_hi rows, pass 1 the |x_lo| rows (one 16x16x32 MFMA per user and k step each); NG = 1
    // both.  One loop body for every pass: duplicating it for the passes spilled 300+ registers
    constexpr int NG2 = RB2 / G2;
    static_assert(NG2 <= 2, "bound MFMA split assumes at most two row-block passes");
#pragma unroll 1
    for (int g = 0; g < NG2; ++g) {
      f32x16 acc2[UPW][G2];
#pragma unroll
      for (int v = 0; v < UPW; ++v)
#pragma unroll
        for (int gi = 0; gi < G2; ++gi)
          acc2[v][gi] = f32x16{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      // k loop, software-pipelined: the f16 operands of step kb + 1 (LDS reads, relu, split:
      // ~45 VALU per user) are formed while step kb's 3 G2 UPW MFMAs run -- one wave per
      // SIMD issues ~5 VALU per 32-cycle MFMA gap nearly for free (MI355X_MICROARCH.md,
      // cycle constants), so a step costs its MFMAs instead of VALU + MFMA.  hi weight
      // fragments are prefetched one step ahead, lo fragments at the top of their step (first
      // used 2 G2 UPW MFMAs later).
      auto frag = [&](int gi, int kk, int hl) {
        const int q = ((g * G2 + gi) * KB + kk) * 2;
        return wd_frag(w2rs, lane, (q + hl) * 1024);
      };
      // x_hi and |x_lo| of step kk (the layer-2 MFMAs' and the bound MFMAs' B operands), packed
      auto form = [&](int kk, wh8* oh, wh8* ol) {
        const float4 q0 = *reinterpret_cast<const float4*>(qrow + 16 * kk);
        const float4 q1 = *reinterpret_cast<const float4*>(qrow + 16 * kk + 4);
#pragma unroll
        for (int v = 0; v < UPW; ++v) {
          const float* prow = ps + (wave * UPW + v) * K1P + 8 * h + 16 * kk;
          const float4 p0 = *reinterpret_cast<const float4*>(prow);
          const float4 p1 = *reinterpret_cast<const float4*>(prow + 4);
          {
            const wf2 s2v = {s1, s1};
            const wf2 zq[4] = {{q0.x, q0.y}, {q0.z, q0.w}, {q1.x, q1.y}, {q1.z, q1.w}};
            const wf2 zp[4] = {{p0.x, p0.y}, {p0.z, p0.w}, {p1.x, p1.y}, {p1.z, p1.w}};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              wh2 hi;
              unsigned alo;
              wd_split_relu2(__builtin_elementwise_fma(zq[e], s2v, zp[e]), hi, alo);
              const wh2 lo2 = __builtin_bit_cast(wh2, alo);
              oh[v][2 * e] = hi[0];
              oh[v][2 * e + 1] = hi[1];
              ol[v][2 * e] = lo2[0];
              ol[v][2 * e + 1] = lo2[1];
            }
          }
        }
      };
      // the weight and bound fragments of step kb + 2 are loaded into the registers step kb's
      // MFMAs have just read -- a two-step prefetch distance with two register sets (the
      // one-pass step is half as long as a two-pass one, so one step ahead left its MFMAs
      // waiting on L2)
      auto stepd = [&](int kb, wfr (&a)[G2], const wh8 (&xh)[UPW], const wh8 (&xl)[UPW],
                       wh8 (&nxh)[UPW], wh8 (&nxl)[UPW], wfr (&bq)[2]) {
        const bool more = kb + 1 < KB;
        const int kn = more ? kb + 1 : kb;
        const int kf = kb + 2 < KB ? kb + 2 : KB - 1;
#pragma unroll
        for (int gi = 0; gi < G2; ++gi)
#pragma unroll
          for (int v = 0; v < UPW; ++v) {
            acc2[v][gi] = wd_mfma16(wd_h(a[gi]), xh[v], acc2[v][gi]);
          }
#pragma unroll
        for (int v = 0; v < UPW; ++v) {
          if constexpr (ASMACC && NG2 == 1) {
            wd_mfma16x_accv<true>(accb[v], wd_h(bq[0]), xh[v]);
            wd_mfma16x_accv<true>(accb[v], wd_h(bq[1]), xl[v]);
          } else if (NG2 == 1) {
            accb[v] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wd_h(bq[0]), xh[v], accb[v], 0, 0, 0);
            accb[v] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wd_h(bq[1]), xl[v], accb[v], 0, 0, 0);
          } else {
            const wh8 bop = g == 0 ? xh[v] : xl[v];
            accb[v] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wd_h(bq[0]), bop, accb[v], 0, 0, 0);
          }
        }
#pragma unroll
        for (int gi = 0; gi < G2; ++gi) a[gi] = frag(gi, kf, 0);
        bq[0] = wd_frag(wbrs, lane, (int)(((NG2 == 1 ? 0 : g) * KB + kf)) * 1024);
        if (NG2 == 1) bq[1] = wd_frag(wbrs, lane, (int)((KB + kf)) * 1024);
        form(kn, nxh, nxl);
#pragma unroll
        for (int e = 0; e < QPS; ++e) {
          const int c = 8 * ((g * KB + kb) * QPS + e);
          qdst[c] = qv[e];
          qv[e] = qload(qrs, c + 8 * QPS);
        }
        // the next step's LDS reads first, then one MFMA + WDC_VPM VALU at a time (2+1 passes:
        // 268-272 ms; 2, 3, 5, 6, 8 VALU per MFMA 305-315 ms, compiler order 331 ms)
        __builtin_amdgcn_sched_group_barrier(0x100, 4 + 2 * UPW, 0);
#pragma unroll
        for (int i = 0; i < G2 * UPW + (3 - NG2) * UPW; ++i) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x002, WDC_VPM, 0);
        }
      };
      wfr fa[G2], fb[G2], ba[2], bb[2];
      wh8 xha[UPW], xla[UPW], xhb[UPW], xlb[UPW];
      form(0, xha, xla);
#pragma unroll
      for (int gi = 0; gi < G2; ++gi) fa[gi] = frag(gi, 0, 0);
      {
        const int k1 = KB > 1 ? 1 : 0;
#pragma unroll
        for (int gi = 0; gi < G2; ++gi) fb[gi] = frag(gi, k1, 0);
        const int bo = (NG2 == 1 ? 0 : g) * KB;
        ba[0] = wd_frag(wbrs, lane, (int)(bo) * 1024);
        bb[0] = wd_frag(wbrs, lane, (int)((bo + k1)) * 1024);
        if (NG2 == 1) {
          ba[1] = wd_frag(wbrs, lane, (int)(KB) * 1024);
          bb[1] = wd_frag(wbrs, lane, (int)((KB + k1)) * 1024);
        }
      }
      {
        // steps in pairs with the two register sets swapped (the one-pass kernel is issue-bound:
        // copying one set into the other was 28 v_mov per step)
        int kb = 0;
        for (; kb + 1 < KB; kb += 2) {
          stepd(kb, fa, xha, xla, xhb, xlb, ba);
          stepd(kb + 1, fb, xhb, xlb, xha, xla, bb);
        }
        if (kb < KB) stepd(kb, fa, xha, xla, xhb, xlb, ba);
      }
      if constexpr (ASMACC) {
        // the last MFMAs' results -> any reader: 8-pass XDL, 12+ wait states; the fence names
        // every accumulator so no read is scheduled above it
        asm volatile("s_nop 7\n\ts_nop 7");
#pragma unroll
        for (int v = 0; v < UPW; ++v)
#pragma unroll
          for (int gi = 0; gi < G2; ++gi) asm volatile("" : "+a"(acc2[v][gi]));
#pragma unroll
        for (int v = 0; v < UPW; ++v) asm volatile("" : "+v"(accb[v]));
        if (WD_STAMPS) {
          st_t1 = __builtin_amdgcn_s_memtime();
          st_acc[0] += st_t1 - st_t0;
        }
      }
      if (G2 < RB2 && g == 0) {  // zeroed after the k loop (G2 = RB2: by the first MFMA's C = 0)
#pragma unroll
        for (int v = 0; v < UPW; ++v)
#pragma unroll
          for (int ob = 0; ob < NOB; ++ob)
            acc3[v][ob] = f32x16{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      }
      // One pass over k (G2 = RB2) with a layer 3: every row block's x2 first (its f16 B operand
      // kept in 8 registers per row block and user, its bound term summed), then layer 3 -- so
      // layer 3's accumulators take the registers of layer 2's, which are all dead by then
      // (one phase per row block kept both sets live and spilled).
      if constexpr (G2 == RB2 && OB > 0) {
        // in halves of RH row blocks: x2 of the half's blocks (their f16 B operands, their
        // bound terms), then their layer-3 MFMAs -- layer 3's accumulators take the registers of
        // the first half's layer-2 ones (all 256 accumulator registers hold layer 2 until then)
        constexpr int RH = RB2 >= 2 ? RB2 / 2 : 1;
        // the bias / bound rows are loop-invariant LDS reads: an opaque offset per tile keeps
        // them from being hoisted out of the tile loop (256 registers held across it: spilled)
        int lz = 0;
        asm volatile("" : "+v"(lz));
        const float* b2t = b2l + lz;
        const float* v2t = v2l + lz;
        const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        // layer 3's weight fragments, W3D row-block halves (kb3 steps) ahead of their MFMAs: the
        // first ones are in flight while layer 2's accumulators are converted
        constexpr int W3D = 2, NK3 = 2 * RB2;
        wfr w3b[W3D + 1][NOB];
        auto w3load = [&](int kb3) {
#pragma unroll
          for (int ob = 0; ob < NOB; ++ob) {
            const int q = (ob * 2 * RB2 + kb3) * 2;
            w3b[kb3 % (W3D + 1)][ob] = wd_frag(w3rs, lane, q * 1024);
          }
        };
#pragma unroll
        for (int k3 = 0; k3 < W3D && k3 < NK3; ++k3) w3load(k3);
#pragma unroll
        for (int r0 = 0; r0 < RB2; r0 += RH) {
          wh8 yh_h[UPW][RH][2];
#pragma unroll
          for (int rr = 0; rr < RH; ++rr) {
            // one row block at a time: hoisting every block's accumulator reads needs 256 VGPRs
            __builtin_amdgcn_sched_barrier(0);
            const int rb = r0 + rr;
            float bias16[16], vv16[16];
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4) {
              const float4 bb = *reinterpret_cast<const float4*>(b2t + rb * 32 + 8 * r4 + 4 * h);
              const float4 vq = *reinterpret_cast<const float4*>(v2t + rb * 32 + 8 * r4 + 4 * h);
              bias16[4 * r4] = bb.x; bias16[4 * r4 + 1] = bb.y; bias16[4 * r4 + 2] = bb.z; bias16[4 * r4 + 3] = bb.w;
              vv16[4 * r4] = vq.x; vv16[4 * r4 + 1] = vq.y; vv16[4 * r4 + 2] = vq.z; vv16[4 * r4 + 3] = vq.w;
            }
#pragma unroll
            for (int v = 0; v < UPW; ++v) {
              // four independent chains (a nonnegative sum: its rounding is inside rho in any
              // order) instead of one 16-deep dependent chain per row block
              float part[4] = {bx2[v], 0.f, 0.f, 0.f};
#pragma unroll
              for (int r = 0; r < 16; ++r) {
                const float y = fmaxf(fmaf(acc2[v][rb][r], c2, bias16[r]), 0.f);
                part[r & 3] = fmaf(vv16[r], y, part[r & 3]);
                yh_h[v][rr][r >> 3][r & 7] = (_Float16)y;
              }
              bx2[v] = (part[0] + part[1]) + (part[2] + part[3]);
              // the bound sum is due here: otherwise it is sunk to its use after layer 3,
              // holding every fp32 x2 value live (spilled)
              asm volatile("" : "+v"(bx2[v]));
            }
          }
#pragma unroll
          for (int rr = 0; rr < RH; ++rr) {
#pragma unroll
            for (int half2 = 0; half2 < 2; ++half2) {
              __builtin_amdgcn_sched_barrier(0);
              const int kb3 = 2 * (r0 + rr) + half2;
              if (kb3 + W3D < NK3) w3load(kb3 + W3D);
              const wfr* bh = w3b[kb3 % (W3D + 1)];
              const bool first = r0 == 0 && rr == 0 && half2 == 0;
#pragma unroll
              for (int ob = 0; ob < NOB; ++ob)
#pragma unroll
                for (int v = 0; v < UPW; ++v) {
                  if constexpr (ASMACC) {
                    if (first) {
                      if (ob == 0) wd_mfma_acc0<true>(acc3[v][ob], wd_h(bh[ob]), yh_h[v][rr][half2]);
                      else wd_mfma_acc0<false>(acc3[v][ob], wd_h(bh[ob]), yh_h[v][rr][half2]);
                    } else {
                      if (ob == 0) wd_mfma_acc<true>(acc3[v][ob], wd_h(bh[ob]), yh_h[v][rr][half2]);
                      else wd_mfma_acc<false>(acc3[v][ob], wd_h(bh[ob]), yh_h[v][rr][half2]);
                    }
                  } else {
                    acc3[v][ob] = wd_mfma16(wd_h(bh[ob]), yh_h[v][rr][half2], first ? zero16 : acc3[v][ob]);
                  }
                }
            }
          }
        }
        if constexpr (ASMACC) {  // layer 3's results -> the VALU readers below
          asm volatile("s_nop 7\n\ts_nop 7");
#pragma unroll
          for (int v = 0; v < UPW; ++v)
#pragma unroll
            for (int ob = 0; ob < NOB; ++ob) asm volatile("" : "+a"(acc3[v][ob]));
        }
        if (WD_STAMPS) {
          const unsigned long long t2 = __builtin_amdgcn_s_memtime();
          st_acc[1] += t2 - st_t1;
          st_t1 = t2;
        }
        continue;
      }
      // x2 = relu(D2 + b2') in s2 units feeds layer 3 (or the final dot)
#pragma unroll
      for (int gi = 0; gi < G2; ++gi) {
        // fence: keeps the scheduler from hoisting every row block's layer-3 fragment loads
        // (G2 = 8: 64 x 16 B a lane) above the first block's MFMAs
        if (G2 == RB2) __builtin_amdgcn_sched_barrier(0);
        const int rb = g * G2 + gi;
        float y[UPW][16];
        float bias16[16], vv16[16];
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {  // rows 8 r4 + 4 h + 0..3: one 16-B read each
          const float4 bb = *reinterpret_cast<const float4*>(b2l + rb * 32 + 8 * r4 + 4 * h);
          const float4 vq = *reinterpret_cast<const float4*>(v2l + rb * 32 + 8 * r4 + 4 * h);
          bias16[4 * r4] = bb.x; bias16[4 * r4 + 1] = bb.y; bias16[4 * r4 + 2] = bb.z; bias16[4 * r4 + 3] = bb.w;
          vv16[4 * r4] = vq.x; vv16[4 * r4 + 1] = vq.y; vv16[4 * r4 + 2] = vq.z; vv16[4 * r4 + 3] = vq.w;
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = rb * 32 + mfma32_row(r, h);
          const float bias = bias16[r], vv = vv16[r], wv = wdl[OB == 0 ? row : 0];
#pragma unroll
          for (int v = 0; v < UPW; ++v) {
            y[v][r] = fmaxf(fmaf(acc2[v][gi][r], c2, bias), 0.f);
            bx2[v] = fmaf(vv, y[v][r], bx2[v]);
            if (OB == 0) fin[v] = fmaf(y[v][r], wv, fin[v]);
          }
        }
        if (OB > 0) {
#pragma unroll
          for (int half2 = 0; half2 < 2; ++half2) {
            wh8 yh[UPW], yl[UPW];
#pragma unroll
            for (int v = 0; v < UPW; ++v) wd_split8(&y[v][8 * half2], yh[v], yl[v]);
            const int kb3 = 2 * rb + half2;
            wh8 bh[NOB];
#pragma unroll
            for (int ob = 0; ob < NOB; ++ob) {
              const int q = (ob * 2 * RB2 + kb3) * 2;
              bh[ob] = wd_h(wd_frag(w3rs, lane, q * 1024));
            }
            // G2 = RB2: the chain starts at the first row block with C = 0 (an inline constant),
            // so acc3 becomes live only as acc2's registers are consumed
            const bool first = G2 == RB2 && gi == 0 && half2 == 0;
            const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ob = 0; ob < NOB; ++ob)
#pragma unroll
              for (int v = 0; v < UPW; ++v)
                acc3[v][ob] = wd_mfma16(bh[ob], yh[v], first ? zero16 : acc3[v][ob]);

          }
        }
      }
    }
    const int64_t item = base + j;
    const bool ivalid = lane < 32 && item < part_end;
    const float wi = ivalid ? A.wI[item] : 0.f;
    const int64_t tile_end = std::min<int64_t>(base + TILE, part_end);
#pragma unroll
    for (int v = 0; v < UPW; ++v) {
      if (OB > 0) {
        // four independent chains each (at most 16 NOB + 3 roundings on any path, within the
        // 32 NOB of g3) instead of two 16 NOB-deep dependent chains
        float fp[4] = {fin[v], 0.f, 0.f, 0.f}, bp[4] = {bx3[v], 0.f, 0.f, 0.f};
#pragma unroll
        for (int ob = 0; ob < NOB; ++ob) {
#pragma unroll
          for (int r4 = 0; r4 < 4; ++r4) {
            const float4 b3 = *reinterpret_cast<const float4*>(b3l + ob * 32 + 8 * r4 + 4 * h);
            const float4 w4 = *reinterpret_cast<const float4*>(wdl + ob * 32 + 8 * r4 + 4 * h);
            const float bq[4] = {b3.x, b3.y, b3.z, b3.w}, wq[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float z = fmaxf(fmaf(acc3[v][ob][4 * r4 + e], c3, bq[e]), 0.f);
              fp[e] = fmaf(z, wq[e], fp[e]);
              bp[e] = fmaf(fabsf(wq[e]), z, bp[e]);
            }
          }
        }
        fin[v] = (fp[0] + fp[1]) + (fp[2] + fp[3]);
        bx3[v] = (bp[0] + bp[1]) + (bp[2] + bp[3]);
      } else {
        fin[v] *= inv_s2;
      }
      const float fv = hnm_sum_halves(fin[v]);
      // item j's row of the bound accumulators: lane j (< 16) row 0, lane j - 16 row 1; the
      // layer-2 x_lo term is inside (the A rows of the |x_lo| operand)
      const float d0 = __shfl(accb[v][0], lane & 15), d1 = __shfl(accb[v][1], lane & 15);
      const float b1 = ((lane & 31) < 16 ? d0 : d1) * (A.prm->inv_sb * inv_s1);
      const float bl1 = 0.f;
      const float b2 = hnm_sum_halves(bx2[v]);
      const float b3 = hnm_sum_halves(bx3[v]);
      const float score = fv + cub[v] + wi;
      const float e = rho * (g1 * b1 + bl1 + g2 * (b2 * inv_s2) + g3 * b3 +
                             g4 * (fabsf(fv) + fabsf(cub[v]) + fabsf(wi)) + cbd) + absb;
      bool masked = false;
      while (nm[v] < tile_end) {
        if (item == nm[v]) masked = true;
        ++mpos[v];
        nm[v] = mpos[v] < mend[v] ? A.midx[mpos[v]] : INT_BIG;
      }
      if (!act[v]) continue;
      if (MODE == WDC_DEBUG) {
        if (ivalid) {
          A.dbg_a[bu[v] * A.lda + item] = score;
          A.dbg_e[bu[v] * A.lda + item] = e;
        }
        continue;
      }
      const bool ok = ivalid && !masked;
      const float lb = score - e, ub = score + e;
      L[v].offer(lb, (int)item, ok, A.K);
      const bool app = ok && ub >= L[v].thr_v;
      const uint64_t m = __ballot(app);
      const int pos = count[v] + __popcll(m & ((1ull << lane) - 1));
      const int64_t seg = (bu[v] * A.NP + p) * (int64_t)A.cap;
      if (app && pos < A.cap) {
        A.segi[seg + pos] = (int32_t)item;
        A.segu[seg + pos] = ub;
      }
      count[v] += __popcll(m);
    }
    if (WD_STAMPS) {
      const unsigned long long t3 = __builtin_amdgcn_s_memtime();
      st_acc[2] += t3 - st_t1;
      st_acc[3] += t3 - st_t0;
    }
  }
  if (WD_STAMPS && lane == 0) {
#if WD_STAMPS
#pragma unroll
    for (int i = 0; i < 4; ++i) atomicAdd(&wd_stamp_acc[i], st_acc[i]);
#endif
  }
  if (MODE == WDC_THRESH) {
#pragma unroll
    for (int v = 0; v < UPW; ++v) {
      if (!act[v]) continue;
      L[v].store(A.lbv + (bu[v] * A.NP + p) * A.K, A.lbi + (bu[v] * A.NP + p) * A.K, A.K);
      if (lane == 0) A.cnt[bu[v] * A.NP + p] = count[v];
    }
  }
}

// ------------------------------------------------------------------ certified path host
#define WDC_CAP 4096  // appended candidates per (user, partition) segment

bool wdc_eligible(const hnm_ctx* ctx, const WdPrep& pr, int64_t I, int K, bool debug) {
  return (debug || (ctx->prefilter && I >= 4096)) && K <= 64 && pr.K1P % 16 == 0 &&
         wd_dispatch<true>(pr.RB2, pr.OB, [](auto, auto) {});
}

constexpr int WDC_STAT_BLOCKS = 1024;

size_t wdc_carve(const hnm_ctx* ctx, const WdPrep& pr, int64_t B, int64_t I, int K, char* base,
                 WdcWs* c) {
  int64_t np, ipp;
  wd_partition(ctx, B, I, &np, &ipp, 4 * wdc_upw(pr.RB2, pr.OB));
  const int cap = (int)std::min<int64_t>(WDC_CAP, ipp);
  const int K1P = pr.K1P, KB = K1P / 16;
  const int64_t fbn = 8 * (int64_t)ctx->num_cus + 4 + B;  // bound on n * np(n) over n <= B
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* p = base ? base + off : nullptr;
    off += hnm_align(bytes);
    return p;
  };
  WdcWs t;
  t.prm = (WdCertParams*)take(sizeof(WdCertParams));
  t.W2hl = (wh8*)take((size_t)pr.RB2 * KB * 2 * 64 * 16);
  t.W3hl = (wh8*)take((size_t)std::max(pr.OB, 1) * 2 * pr.RB2 * 2 * 64 * 16);
  t.WBf = (wh8*)take((size_t)KB * 2 * 64 * 16);
  t.v1 = (float*)take((size_t)K1P * 4);
  t.v1o = (float*)take((size_t)K1P * 4);
  t.v2 = (float*)take((size_t)pr.RB2 * 32 * 4);
  t.v2o = (float*)take((size_t)pr.RB2 * 32 * 4);
  t.b2s = (float*)take((size_t)pr.RB2 * 32 * 4);
  t.part = (float*)take((size_t)WDC_STAT_BLOCKS * 2 * 4);
  t.lbv = (float*)take((size_t)B * np * K * 4);
  t.lbi = (int32_t*)take((size_t)B * np * K * 4);
  t.Lv = (float*)take((size_t)B * K * 4);
  t.Li = (int64_t*)take((size_t)B * K * 8);
  t.segi = (int32_t*)take((size_t)B * np * cap * 4);
  t.segu = (float*)take((size_t)B * np * cap * 4);
  t.cnt = (int*)take((size_t)B * np * 4);
  t.segl = (float*)take((size_t)B * np * cap * 4);
  t.segs = (float*)take((size_t)B * np * cap * 4);
  t.cli = (int32_t*)take((size_t)B * np * cap * 4);
  t.nA = (int*)take((size_t)B * 4);
  t.tv = (float*)take((size_t)B * 4);
  t.tg = (int*)take((size_t)B * 4);
  t.ns = (int*)take((size_t)B * 4);
  t.toff = (int*)take((size_t)(B + 1) * 4);
  t.fbrows = (int32_t*)take((size_t)B * 4);
  t.nfb = (int*)take(4);
  t.fcv = (float*)take((size_t)fbn * K * 4);
  t.fci = (int32_t*)take((size_t)fbn * K * 4);
  t.fov = (float*)take((size_t)B * K * 4);
  t.foi = (int64_t*)take((size_t)B * K * 8);
  t.np = np;
  t.ipp = ipp;
  t.cap = cap;
  if (c) *c = t;
  return off;
}

hnm_status wdc_prepare(hnm_ctx* ctx, const hnm_widedeep_weights* w, const WdSetup& S, int64_t B,
                       const WdcWs& c) {
  hipStream_t s = ctx->stream;
  const int64_t I = w->num_items;
  hipLaunchKernelGGL(wdc_stats_kernel, dim3(WDC_STAT_BLOCKS), dim3(256), 0, s, S.Pu,
                     B * S.K1P, S.Qi, I * S.K1P, c.part);
  hipLaunchKernelGGL(wdc_params_kernel, dim3(1), dim3(256), 0, s, *w, S.pr, c.part,
                     WDC_STAT_BLOCKS, c.v1, c.v2, c.b2s, c.prm, c.v1o, c.v2o);
  hipLaunchKernelGGL(wdc_convert_kernel, dim3(256), dim3(256), 0, s, *w, S.pr, c.prm, c.W2hl,
                     c.W3hl);
  hipLaunchKernelGGL(wdc_boundfrag_kernel, dim3((unsigned)hnm_cdiv(S.K1P / 16 * 2 * 64, 256)),
                       dim3(256), 0, s, c.prm, c.v1, c.v1o, S.K1P, c.WBf);
  HNM_LAUNCH_CHECK();
  return HNM_OK;
}

hnm_status wdc_scan(hnm_ctx* ctx, const hnm_widedeep_weights* w, const WdSetup& S, int64_t B,
                    const int64_t* mptr, const int32_t* midx, int K, const WdcWs& c, int mode,
                    float* dbg_a, float* dbg_e, int64_t lda) {
  const WdPrep& pr = S.pr;
  const int NOB = pr.OB > 0 ? pr.OB : 1, NL = pr.OB > 0 ? pr.OB : pr.RB2;
  WdScanArgs a;
  a.Pu = S.Pu;
  a.Qi = S.Qi;
  a.K1P = S.K1P;
  a.W2hl = c.W2hl;
  a.W3hl = c.W3hl;
  a.WBf = c.WBf;
  a.v1 = c.v1;
  a.v1o = c.v1o;
  a.v2 = c.v2;
  a.b2s = c.b2s;
  a.b3p = pr.b3p;
  a.wdp = pr.wdp;
  a.cu = S.cu;
  a.wI = S.wI;
  a.prm = c.prm;
  a.B = B;
  a.I = w->num_items;
  a.ipp = c.ipp;
  a.NP = (int)c.np;
  a.mptr = mptr;
  a.midx = midx;
  a.K = K;
  a.lbv = c.lbv;
  a.lbi = c.lbi;
  a.segi = c.segi;
  a.segu = c.segu;
  a.cnt = c.cnt;
  a.cap = c.cap;
  a.dbg_a = dbg_a;
  a.dbg_e = dbg_e;
  a.lda = lda;
  const int upb = 4 * wdc_upw(pr.RB2, pr.OB);
  const size_t lds =
      (size_t)(2 * 32 * (S.K1P + 4) + upb * S.K1P + 2 * pr.RB2 * 32 + NOB * 32 + NL * 32) * 4;
  dim3 grid((unsigned)hnm_cdiv(B, upb), (unsigned)c.np);
  if (mode == WDC_THRESH) hnm_timer_begin(ctx, HNM_TIME_SCORE);
  auto launch = [&](auto kern) {
    (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kern, grid, dim3(256), lds, ctx->stream, a);
  };
  const bool found = wd_dispatch<true>(pr.RB2, pr.OB, [&](auto R, auto O) {
    constexpr int G2 = wdc_g2(R(), O()), UPW = wdc_upw(R(), O());
    if (mode == WDC_THRESH) launch(wdc_scan_kernel<R(), O(), G2, WDC_THRESH, UPW>);
    else launch(wdc_scan_kernel<R(), O(), G2, WDC_DEBUG, UPW>);
  });
  if (mode == WDC_THRESH) hnm_timer_end(ctx, HNM_TIME_SCORE);
  if (!found) return wd_not_instantiated(pr);
  HNM_LAUNCH_CHECK();
  return HNM_OK;
}

extern "C" hnm_status hnm_widedeep_prefilter_debug_ex_f32(
    hnm_ctx* ctx, const hnm_widedeep_weights* w, const int64_t* user_ids, int64_t B,
    const float* user_features, float* approx, int64_t lda, float* bound,
    const hnm_widedeep_item_features* itf, const float* item_features, int64_t ldf) {
  HNM_CTX_DEVICE(ctx);
  HNM_REQUIRE(ctx && user_ids && approx && bound && w && lda >= w->num_items, HNM_EINVAL,
              "widedeep_prefilter_debug: bad argument");
  WdItemFeat F;
  F.itf = itf;
  F.f = item_features;
  F.ldf = ldf;
  WdSetup S;
  hnm_status st = wd_shape(w, &S.pr, F);
  if (st) return st;
  HNM_REQUIRE(wdc_eligible(ctx, S.pr, w->num_items, 1, true), HNM_EUNSUPPORTED,
              "widedeep_prefilter_debug: tower shape not covered by the certified scan");
  if (B <= 0) return HNM_OK;
  const int64_t I = w->num_items;
  const size_t extra = wdc_carve(ctx, S.pr, B, I, 1, nullptr, nullptr);
  st = wd_setup(ctx, w, user_ids, B, user_features, extra, &S, F);
  if (st) return st;
  WdcWs c;
  wdc_carve(ctx, S.pr, B, I, 1, S.extra, &c);
  st = wdc_prepare(ctx, w, S, B, c);
  if (st) return st;
  return wdc_scan(ctx, w, S, B, nullptr, nullptr, 1, c, WDC_DEBUG, approx, bound, lda);
}

extern "C" hnm_status hnm_widedeep_prefilter_debug_f32(hnm_ctx* ctx,
                                                       const hnm_widedeep_weights* w,
                                                       const int64_t* user_ids, int64_t B,
                                                       const float* user_features,
                                                       float* approx, int64_t lda,
                                                       float* bound) {
  return hnm_widedeep_prefilter_debug_ex_f32(ctx, w, user_ids, B, user_features, approx, lda,
                                             bound, nullptr, nullptr, 0);
}
