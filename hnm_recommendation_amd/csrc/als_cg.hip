// ImplicitALS: the conjugate-gradient half-step (hnm_als_cg_rows_f32 and its weighted sibling;
// Takacs, Pilaszy & Tikk 2011).  Contract in include/hnm.h, float64 restatement in
// tests/cg_oracle.py.
//
// Stages 1 and 2 are als_solve_kernel's (als_internal.h): the row's A (lower triangle) and b stand
// in LDS exactly as the Cholesky entries form them.  AlsCg::run replaces stages 3 and 4: from the
// row's start vector x0 (the output row itself) it takes `steps` CG steps on A x = b in fp32
//   x = x0;  r = b - A x;  p = r;  rs = r.r
//   repeat: q = A p;  a = rs / (p.q);  x += a p;  r -= a q;  rn = r.r;  p = r + (rn / rs) p;  rs = rn
// and stops early when rs or p.q is not > 0 (converged to the last bit, or a non-finite x0).
//
// Shape.  Every wave keeps x, r and p whole in registers -- lane l holds elements l and l + 64 --
// so the four waves run the same vector arithmetic on the same values and agree bit for bit; the
// dot products are wave_sum (a fixed butterfly) and need no barrier.  The matvec is split over the
// waves by column: wave w owns columns j in [w d / 4, (w + 1) d / 4), takes p_j from the owning
// lane (v_readlane) and adds A_ij p_j into its partial q_i, a lane per row i.  Only the stored
// lower triangle is read: A[i][j] for j <= i is a row walk over the lanes (stride LD, odd),
// A[j][i] for j > i a column walk (stride 1) -- both conflict-free.  The four partials go to LDS,
// one barrier, and every wave adds them in wave order.  The partial buffer is double-buffered, so
// that barrier is the only one of a step: steps + 1 barriers a row (the first matvec is A x0)
// against the factorisation's 2 d.
//
// Summation order, a function of d alone: q_i = ((P0 + P1) + P2) + P3 with Pw = the fmaf chain
// acc = fmaf(A_ij, p_j, acc) over wave w's columns j ascending, from 0.0f; a dot product u.v is
// wave_sum over lanes l of fmaf(u_{l+64}, v_{l+64}, u_l * v_l) (d <= 64: of u_l * v_l), elements
// >= d being zero.
// LDS: the matrix plus 2 x 4 x 32 NT floats of partials (4 KB at d = 128, where two workgroups a
// CU still fit).
#include "als_internal.h"

namespace {

struct AlsCg {
  template <int NT>
  static __device__ __forceinline__ void run(float* As, int d, float* __restrict__ xrow, int steps) {
    constexpr int DP = 32 * NT, LD = DP + 1;
    constexpr int NS = NT > 2 ? 2 : 1;  // elements a lane: i = lane + 64 s
    __shared__ float part[2][4][DP];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int jw = d >> 2, j0 = wave * jw;  // this wave's columns (d is a multiple of 16)
    int buf = 0;
    // q = A v, v whole in this wave's registers
    auto matvec = [&](const float (&v)[NS], float (&q)[NS]) {
      float acc[NS];
#pragma unroll
      for (int s = 0; s < NS; ++s) acc[s] = 0.f;
      for (int jb = j0; jb < j0 + jw; jb += 4) {  // jw is a multiple of 4; j is uniform over the wave
#pragma unroll
        for (int u = 0; u < 4; ++u) {  // four independent LDS reads in flight a lane
          const int j = jb + u;
          float vj;
          if constexpr (NS == 2)
            vj = __uint_as_float(
                __builtin_amdgcn_readlane(__float_as_uint(j < 64 ? v[0] : v[1]), j & 63));
          else
            vj = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(v[0]), j));
#pragma unroll
          for (int s = 0; s < NS; ++s) {
            const int i = lane + 64 * s;
            if (i < d) acc[s] = fmaf(As[j <= i ? i * LD + j : j * LD + i], vj, acc[s]);
          }
        }
      }
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const int i = lane + 64 * s;
        if (i < d) part[buf][wave][i] = acc[s];
      }
      __syncthreads();
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const int i = lane + 64 * s;
        q[s] = i < d ? ((part[buf][0][i] + part[buf][1][i]) + part[buf][2][i]) + part[buf][3][i]
                     : 0.f;
      }
      buf ^= 1;
    };
    auto dot = [&](const float (&u)[NS], const float (&v)[NS]) {
      float z = __fmul_rn(u[0], v[0]);  // never contracted into the butterfly's first add
      if constexpr (NS == 2) z = fmaf(u[1], v[1], z);
      // every lane of every wave holds the same sum; taking lane 0's makes it a scalar, and the
      // loop's exits uniform branches around the matvec's barrier
      return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(wave_sum(z))));
    };
    float x[NS], r[NS], p[NS], q[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const int i = lane + 64 * s;
      x[s] = i < d ? xrow[i] : 0.f;
    }
    matvec(x, q);
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const int i = lane + 64 * s;
      r[s] = i < d ? As[d * LD + i] - q[s] : 0.f;
      p[s] = r[s];
    }
    float rs = dot(r, r);
    for (int k = 0; k < steps; ++k) {
      if (!(rs > 0.f)) break;  // every wave holds the same rs: uniform over the workgroup
      matvec(p, q);
      const float pq = dot(p, q);
      if (!(pq > 0.f)) break;
      const float a = rs / pq;
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        x[s] = fmaf(a, p[s], x[s]);
        r[s] = fmaf(-a, q[s], r[s]);
      }
      const float rn = dot(r, r);
      const float beta = rn / rs;
#pragma unroll
      for (int s = 0; s < NS; ++s) p[s] = fmaf(beta, p[s], r[s]);
      rs = rn;
    }
    if (wave == 0) {
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const int i = lane + 64 * s;
        if (i < d) xrow[i] = x[s];
      }
    }
  }
};

// The two CG entries: w == NULL and weighted == false is hnm_als_cg_rows_f32.
hnm_status als_cg_rows(hnm_ctx* ctx, const int64_t* ptr, const int32_t* idx, const float* w,
                       bool weighted, int64_t n_rows, const float* tab, int64_t tab_rows,
                       int64_t ld, int64_t d, const float* gram, float alpha, float reg,
                       const int64_t* row_ids, int64_t B, float* x, int64_t ldx, int steps) {
  HNM_CTX_DEVICE(ctx);
  HNM_REQUIRE(ctx, HNM_EINVAL, "als_cg_rows: ctx is NULL");
  HNM_REQUIRE(als_dim_ok(d), HNM_EUNSUPPORTED,
              "als_cg_rows: d = %lld (multiples of 16 in [16, 128] supported)", (long long)d);
  HNM_REQUIRE(std::isfinite(reg) && reg > 0.f, HNM_EINVAL,
              "als_cg_rows: reg must be finite and > 0");
  HNM_REQUIRE(std::isfinite(alpha) && alpha >= 0.f, HNM_EINVAL,
              "als_cg_rows: alpha must be finite and >= 0");
  HNM_REQUIRE(steps >= 1 && steps <= 32, HNM_EINVAL, "als_cg_rows: steps = %d outside [1, 32]",
              steps);
  HNM_REQUIRE(B >= 0 && n_rows >= 0 && tab_rows >= 0, HNM_EINVAL, "als_cg_rows: bad size");
  HNM_REQUIRE(B <= INT32_MAX && tab_rows < INT_BIG, HNM_EUNSUPPORTED,
              "als_cg_rows: B or tab_rows exceeds 2^31 - 1");
  if (B == 0 || n_rows == 0) return HNM_OK;
  HNM_REQUIRE(ld >= d && ldx >= d, HNM_EINVAL, "als_cg_rows: ld or ldx < d");
  HNM_REQUIRE(ptr && idx && gram && x && (tab || tab_rows == 0), HNM_EINVAL,
              "als_cg_rows: NULL argument");
  HNM_REQUIRE(w || !weighted, HNM_EINVAL, "als_cg_rows_weighted: w is NULL");
  HNM_REQUIRE(row_ids || B <= n_rows, HNM_EINVAL, "als_cg_rows: B > n_rows without row_ids");
  const int nt = (int)hnm_cdiv(d, 32);
  const dim3 grid((unsigned)B), block(256);
  const float one_alpha = 1.0f + alpha;
#define ALS_CG(NT, W)                                                                            \
  hipLaunchKernelGGL((als_solve_kernel<NT, W, AlsCg>), grid, block, 0, ctx->stream, ptr, idx, w, \
                     n_rows, tab, tab_rows, ld, (int)d, gram, alpha, one_alpha, reg, row_ids, x,  \
                     ldx, ctx->err_dev, steps)
  hnm_timer_begin(ctx, HNM_TIME_SCORE);
  if (weighted) {
    switch (nt) {
      case 1: ALS_CG(1, true); break;
      case 2: ALS_CG(2, true); break;
      case 3: ALS_CG(3, true); break;
      default: ALS_CG(4, true); break;
    }
  } else {
    switch (nt) {
      case 1: ALS_CG(1, false); break;
      case 2: ALS_CG(2, false); break;
      case 3: ALS_CG(3, false); break;
      default: ALS_CG(4, false); break;
    }
  }
  hnm_timer_end(ctx, HNM_TIME_SCORE);
#undef ALS_CG
  HNM_LAUNCH_CHECK();
  return HNM_OK;
}

}  // namespace

extern "C" hnm_status hnm_als_cg_rows_f32(hnm_ctx* ctx, const int64_t* ptr, const int32_t* idx,
                                          int64_t n_rows, const float* tab, int64_t tab_rows,
                                          int64_t ld, int64_t d, const float* gram, float alpha,
                                          float reg, const int64_t* row_ids, int64_t B, float* x,
                                          int64_t ldx, int steps) {
  return als_cg_rows(ctx, ptr, idx, nullptr, false, n_rows, tab, tab_rows, ld, d, gram, alpha, reg,
                     row_ids, B, x, ldx, steps);
}

extern "C" hnm_status hnm_als_cg_rows_weighted_f32(hnm_ctx* ctx, const int64_t* ptr,
                                                   const int32_t* idx, const float* w,
                                                   int64_t n_rows, const float* tab,
                                                   int64_t tab_rows, int64_t ld, int64_t d,
                                                   const float* gram, float alpha, float reg,
                                                   const int64_t* row_ids, int64_t B, float* x,
                                                   int64_t ldx, int steps) {
  return als_cg_rows(ctx, ptr, idx, w, true, n_rows, tab, tab_rows, ld, d, gram, alpha, reg,
                     row_ids, B, x, ldx, steps);
}
