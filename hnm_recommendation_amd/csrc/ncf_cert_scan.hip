// Certified NeuralCF path, the f16 scan: ncf16_scan_kernel in its three modes (ScanArgs and the
// modes: ncf_cert_internal.h) x {deep, 32x32x16, 16x16x32} and their launcher.  What the scan
// computes and why pruning by it is safe: the header of ncf_cert.hip.
#include <algorithm>

#include "ncf_cert_internal.h"

namespace {

__device__ __forceinline__ f32x16 mfma16(h8 a, h8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}

// SPARSE: the B operand of item half n, the converted and clamped accumulators m = 0, 1 of users a
// and b interleaved a dword at a time (element 4 q + i = user a's converted value e = 2 q + i,
// 4 q + 2 + i = user b's; e as in the dense epilogue's h8: unit 16 (e >> 2) + 4 (lane >> 4) + (e & 3))
typedef _Float16 h16 __attribute__((ext_vector_type(16)));
__device__ __forceinline__ h16 sparse_b(const f32x4 (&ca)[2][2], const f32x4 (&cb)[2][2], const int n) {
  // as two h8 whose clamp folds into the packed converts (on an h16 it does not), then a register
  // renaming
  h8 ya, yb;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    ya[e] = (_Float16)ca[e >> 2][n][e & 3];
    yb[e] = (_Float16)cb[e >> 2][n][e & 3];
  }
  ya = __builtin_elementwise_min(__builtin_elementwise_max(ya, (h8){}), (h8)(_Float16)1.f);
  yb = __builtin_elementwise_min(__builtin_elementwise_max(yb, (h8){}), (h8)(_Float16)1.f);
  return __builtin_shufflevector(ya, yb, 0, 1, 8, 9, 2, 3, 10, 11, 4, 5, 12, 13, 6, 7, 14, 15);
}

// A wave owns 32 users, a workgroup 128; 32-item tiles of Q16/G16 go through LDS.
// Per (user pair, tile): layer 2 as 4 + 4 v_mfma_f32_32x32x16_f16 (two independent chains;
// A = W2~, B = clamp(P~ + Q~) built with 16 packed adds per user; v_mfma_f32_32x32x16_f16 B
// operand: lane (j, h) holds B[k = 8h + e][col j], e = 0..7), GMF once per tile for all 32
// users (4 MFMAs).  THRESH / SAMPLE: the epilogue wm . relu(H~) of BOTH users runs on the matrix
// pipe as 4 v_mfma_f32_16x16x32_f16 -- relu(H~) by the [0, 1] clamp of the f32 -> f16
// converts, the 16x16x32 B operand taking each lane's 8 converted accumulator rows as they lie
// (k-group g = lanes 16g..16g+15 = half g >> 1, items 16 (g & 1) + c), A rows 0/1 = wm on user
// a's k-groups of items 0-15 / 16-31, rows 2/3 the same for user b -- so one MFMA sums both
// halves of a column (no cross-lane swap), and the accumulator is seeded with the tile's folded
// per-pair term (GMF + bound - threshold, pair-interleaved in LDS so lanes 0-15 read their 4
// seeds as one b128).  Lanes 0-15 end with the 64 test values; 4 ballots assemble the pair's
// 64-bit pass mask with bit u*32 + item (the lane layout of the append).  Measured against the
// earlier packed-dot epilogue (16 v_dot2c + a permlane32 swap per pair, 1.94 ms) and a
// software-pipelined two-waves-per-SIMD variant (2.1-2.2 ms): 1.87 ms (tools/scan_ablation.hip,
// profiles/r2_ncf_scan_variants.txt); splitting it (user a on the matrix pipe, user b by packed
// dots) measured 2.03 vs 1.88 ms (round 3, profiles/r3c_ncf_epilogue_ab.txt): the VALU side is
// the binding one.  DEBUG keeps a VALU epilogue (packed dots + swap).
// DEEP (round 6, towers [2 h0, h1 <= 64, h2 <= 32, h3 <= 16]): layer 2 as above, then layer 3 on
// the matrix pipe in place of the wm epilogue -- per user and item half g (items c / c + 16) two
// v_mfma_f32_16x16x32_f16 whose A rows are W3's 16 units with the k-groups of the other item half
// zeroed (the 16x16x32 B operand mixes items c and c + 16 across k-groups), accumulator seeded
// with b3 -- relu by the clamp of the f32 -> f16 converts, and the prediction wp3 . relu(h3) as a
// v_mfma_f32_16x16x16_f16 whose B operand is that accumulator as it lies (rows 4 (lane >> 4) + r =
// units, columns = items) and whose A row idx = 2 user + g holds wp3: four of them chained on the
// folded seeds leave the test values where the two-layer epilogue leaves them.  DEBUG uses the
// same matrix epilogue (seeds = GMF only).  Two waves per SIMD (28 more live registers).
// SHAPE 1 (HNM_OPT_SCAN_SHAPE, two-layer towers): layer 2 and the GMF on v_mfma_f32_16x16x32_f16,
// everything outside the pair body as it is.  Per user 2 unit halves m x 2 item halves n x 2
// k-steps s (8 x 16 cycles, the 4 x 32 of the other shape); the B operand clamp(P~ + Q~) of (n, s)
// serves both m, and the lane's P~ fragment depends on (s, k-group) only, so a user takes 2
// ds_read_b128 of P~ a tile instead of 4.  The four f32x4 accumulators of a user are seeded with
// b2 (8 registers).  Epilogue: the converted accumulators m = 0, 1 of (user, n) are one B operand
// of a 16x16x32 whose A row 2 user + n holds wm in that k order -- the same 4 chained MFMAs on
// the folded seeds, the same output lanes, ballots and appends.  The GMF is 2 x 2 x 2 of the same
// instruction (users as rows) stored into the same g7 table.  Its DEBUG pass takes this matrix
// epilogue with GMF-only seeds and the deep DEBUG pass's dense store.  The tiles' rows are 128 B
// with XOR-swizzled 16-B chunks (conflict-free for this shape's b128 reads: see so0 / so1).
// THRESH pass test (every layout): a pair's four compares are OR-ed first and the iteration ends
// there when no lane of 0-15 passes (~96 % of them); the bit layout, the history lookup and the
// ranks are built only behind that.  The test runs one pair late, among the next pair's layer-2
// MFMAs (pass_test / dprev below).  Kernel only at the bench shape (tools/scan_ablation.hip,
// profiles/ncf_scan_issue_ab.txt): 1.710 -> 1.632 ms for the early exit, -> 1.611 ms run late.
// 168 VGPRs, no scratch (SHAPE 0: 168 and four spilled registers); three waves per SIMD.
// PIPE (HNM_OPT_SCAN_PIPE, default 1: the THRESH pass of SHAPE 1): the pair loop pipelined by hand
// -- a pair's s = 1 operands formed in the gaps of its s = 0 MFMAs, the next pair's s = 0 operands
// in the gaps of its s = 1 MFMAs, the placement pinned with sched_group_barrier (VALU per gap in
// the emitted loop: 3 2 3 2 3 2 3 2 | 2 x 8; epilogue 10 ahead, then 3 2 3), the layer-2 block at
// wave priority 1.  The registers of the look-ahead are ag's (re-loaded per tile behind the pair
// loop, drained before the prefetch is issued) and those the plain kernel holds across the tile
// loop for lane-derived addresses and masks (recomputed per tile / in the append path here).
// Every MFMA keeps its operands and its place in its chain: results bitwise those of PIPE = false,
// whose code is as it was.  162 VGPRs, no scratch, 50,944 B of LDS (ps has two pad rows), three
// waves per SIMD.  Kernel only 1.595 -> 1.543 ms, the step 1.811 -> 1.763 ms
// (profiles/ncf_scan_pipe_ab.txt: the priority alone on the plain loop 1.558, the pipelined loop
// alone 1.577).
// SPARSE (HNM_OPT_SCAN_SPARSE, every pass of SHAPE 1 that runs the matrix epilogue): wm . relu(H~)
// as 2 v_smfmac_f32_16x16x64_f16, one per item half n, in place of the 4 dense instructions whose
// A operands carry one non-zero row of 16.  The sparse instruction takes a dense B of K = 64 (16
// halves a lane) and an A with two stored values for every four of k, their positions in 2-bit
// fields of an index register (tools/mfma_semantics_probe.hip (d): lane (row, ga)'s stored pair t
// meets elements 4 q .. 4 q + 3 of the B lanes of k-group 2 (ga & 1) + (t >> 1), q = 2 (ga >> 1) +
// (t & 1); the field of a pair is p0 | p1 << 2; D as the dense 16x16 one).  B of half n interleaves
// the converted accumulators of users a and b a dword at a time -- a a b b a a b b along every
// lane's 16 halves, each dword the packed convert + clamp it was -- so row n (user a) stores wm at
// positions {0, 1} of every group and row 2 + n (user b) at {2, 3}: exact 2:4, and a row never
// meets the other user's values.  The two instructions chain on the folded seeds and leave the 64
// test values where the four left them.  The products and their fp32 accumulation are those of
// the dense epilogue in another order, which (*) allows (the header of ncf_cert.hip: the third
// summation order of the scan, after the two layouts').  The instruction takes the dense 16x16x32's
// 16 cycles, so an iteration's matrix-pipe time falls from 20 to 18 of them.  152 VGPRs, no scratch,
// 50,944 B of LDS, three waves per SIMD; converts in the emitted loop 10 ahead, 6 under the first
// instruction.  Kernel only 1.667 -> 1.626 ms, the step 1.833 -> 1.786 ms; matrix-pipe busy cycles
// -9.7 %, the launch's cycles -3.0 % at an unchanged clock (profiles/ncf_scan_sparse_ab.txt).
// ROW0 (HNM_OPT_SCAN_ROW0, every pass of SHAPE 1 with the sparse epilogue): the same two sparse
// instructions with wm in A rows 4 (2 user + n) = 0, 4, 8, 12 instead of 0-3 (user b's rows, 8 and
// 12, at positions {2, 3}).  In the 16x16 D layout lane (c16, g4) holds rows 4 g4 + r, so the
// pair's 64 test values are register r = 0 of all 64 lanes, lane 32 user + item: the append's bit
// layout.  The THRESH test is one compare whose ballot IS the pass mask (four compares, three
// s_or_b64 and a mask to lanes 0-15 before), each lane appends its own value (slot: its user's
// count + its rank in that user's half of the mask, so slots, ids and values are the ones of the
// four-register layout; the user's row offset, now per lane, goes into the vector offset), SAMPLE
// and DEBUG store one value a lane (whole rows of 32 items, one store instruction a pair for
// four).  The folded table g7 is [pair][64] in that lane order, one ds_read_b32 a lane.  Rows
// 4 g4 + 1 .. 3 meet zero A rows; nothing reads them.  Same products, same accumulation order:
// test values, candidate segments and debug outputs are bitwise those of ROW0 = false
// (tests/test_gpu_ncf_scan_row0.py), whose kernels keep their instruction stream.  Pair loop of the
// pipelined THRESH pass: VALU 54 -> 51, scalar ALU 8 -> 3; 152 VGPRs, no scratch, 50,944 B of LDS.
// Kernel only 1.502 -> 1.467 ms, the step 1.744 -> 1.699 ms (profiles/ncf_scan_row0_ab.txt; unrolled
// by four for immediate LDS offsets, another -0.3 %, inside the spread: not kept).
template <int MODE, bool DEEP = false, int SHAPE = 0, bool PIPE = false, bool SPARSE = false,
          bool ROW0 = false>
__global__ __launch_bounds__(256, DEEP ? 2 : HNM_SCAN_OCC) void ncf16_scan_kernel(ScanArgs A) {
  constexpr bool S16 = SHAPE == 1;  // layer 2 and the GMF on v_mfma_f32_16x16x32_f16
  static_assert(!(S16 && DEEP), "the deep scan has the 32x32x16 layout only");
  static_assert(!PIPE || (S16 && MODE == SCAN_THRESH), "the pipelined pair loop: THRESH, layout 1");
  static_assert(!SPARSE || S16, "the sparse epilogue: layout 1");
  static_assert(!ROW0 || SPARSE, "test values in one register of 64 lanes: the sparse epilogue");
  // LDS row stride in halfs: 144 B (conflict-free b128 reads of the 32x32x16 operands: lane
  // (j, h) reads row j) / S16: 128 B with the row's 16-B chunks XOR-swizzled (s16_chunk)
  constexpr int RS = S16 ? 64 : 72;
  constexpr int NU = 128;  // users per workgroup
  // the matrix-pipe epilogue and its folded seed table (FOLD: GMF + bound - threshold; the deep
  // and the S16 DEBUG pass: GMF alone)
  constexpr bool FOLD = MODE == SCAN_THRESH || MODE == SCAN_SAMPLE ||
                        ((DEEP || S16) && MODE == SCAN_DEBUG);
  if (MODE == SCAN_SAMPLE && A.gate && *A.gate == 0) return;  // whole grid: gated off
  __shared__ __attribute__((aligned(16))) _Float16 qs[2][TILE * RS];  // double-buffered tiles
  __shared__ __attribute__((aligned(16))) _Float16 gs[2][TILE * RS];
  // PIPE: two more rows, which the look-ahead reads of a block's last pair may touch
  constexpr int PSR = NU + (PIPE ? 2 : 0);
  __shared__ __attribute__((aligned(16))) _Float16 ps[PSR * 64];
  // per wave: the GMF table of its 32 users x the tile's 32 items (FOLD: folded test terms,
  // pair-interleaved: g7 index below; DEBUG: gsm[row][item])
  __shared__ __attribute__((aligned(16))) float gsm[4][32][33];
  __shared__ float2 ut[4][32];  // FOLD: (tau or 0, cu) per user

  const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, j = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // uniform: scalar loop state
  // grid: x = item partition (NP a multiple of 8), y = user block -> the round-robin
  // workgroup -> XCD placement keeps partition p on XCD p % 8 (its tiles stay in that L2)
  const int upw = A.upw;  // <= 32 (NU / 4)
  const int64_t ublk = (int64_t)blockIdx.y * 4 * upw;
  const int64_t u0 = ublk + wave * upw;
  const int nu = (int)std::max<int64_t>(0, std::min<int64_t>(upw, A.B - u0));
  const int p = blockIdx.x;
  // Item and tile indices are 32-bit: A.I * 64 < 2^31 (ncf_cert_eligible; a sample pass scans
  // no more than the catalogue), ipp is I / NP rounded up to a tile and p * ipp < I (NP =
  // cdiv(I, ipp)), so every index below, one tile past a partition's end included, is < 2^27.
  const int part_start = p * (int)A.ipp;
  const int part_end = std::min<int>((int)A.I, part_start + (int)A.ipp);

  for (int e = tid; e < PSR * 8; e += 256) {
    const int r = e >> 3, c = e & 7;
    h8 v = {};
    if (ublk + r < A.B) v = *reinterpret_cast<const h8*>(A.P16 + (ublk + r) * 64 + 8 * c);
    *reinterpret_cast<h8*>(&ps[r * 64 + 8 * c]) = v;
  }
  // S16 (16x16x32: lane holds A[row lane & 15][k = 8 (lane >> 4) + e], B[k][col lane & 15] and
  // D[row 4 (lane >> 4) + r][col lane & 15]): aw[2 m + s] = W2~ rows 16 m + c16, k-step s;
  // ag[2 m + s] = the users 16 m + c16 of the wave; b2q[m] = the seeds of units 16 m + 4 g4 + r
  const int c16 = lane & 15, g4 = lane >> 4;
  h8 aw[4];
  h8 ag[4];  // GMF A operand: this wave's users' wp*g_u rows
  f32x16 b2c = {};
  f32x4 b2q[2];
  if constexpr (S16) {
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int ur = 16 * m + c16;
        h8 z = {};
        aw[2 * m + s] = *reinterpret_cast<const h8*>(A.W2h + ur * 64 + 32 * s + 8 * g4);
        ag[2 * m + s] =
            ur < nu ? *reinterpret_cast<const h8*>(A.WG16 + (u0 + ur) * 64 + 32 * s + 8 * g4) : z;
      }
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int r = 0; r < 4; ++r) b2q[m][r] = A.b2s[16 * m + 4 * g4 + r];
  } else {
#pragma unroll
    for (int s = 0; s < 4; ++s) aw[s] = *reinterpret_cast<const h8*>(A.W2h + j * 64 + 16 * s + 8 * h);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      h8 z = {};
      ag[s] = j < nu ? *reinterpret_cast<const h8*>(A.WG16 + (u0 + j) * 64 + 16 * s + 8 * h) : z;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) b2c[r] = A.b2s[mfma32_row(r, h)];
  }
  // epilogue A operands (16x16x32: lane holds A[row lane & 15][k = 8 (lane >> 4) + e])
  h8 ewa[2], ewb[2];
  h8 ews[2];     // SPARSE: stored A values [item half n], wm in rows n (user a) and 2 + n (user b)
  int ewi = 0;   // SPARSE: their positions, {0, 1} in user a's rows and {2, 3} in user b's
  h2 wm2[8];  // DEBUG: wm of this lane's accumulator rows, in pairs
  h8 e3[2][2];  // DEEP: layer-3 A operands [item half g][accumulator half f]
  h4 ep[4];     // DEEP: prediction A operands, wp3 in row idx = 2 user + g
  f32x4 b3c;    // DEEP: layer-3 accumulator seeds (rows 4 (lane >> 4) + r)
  if constexpr (DEEP) {
    const int m = lane & 15, kg = lane >> 4;
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
      for (int f = 0; f < 2; ++f)
#pragma unroll
        for (int e = 0; e < 8; ++e)
          e3[g][f][e] = (kg & 1) == g ? A.W3h[m * 32 + mfma32_row(8 * f + e, kg >> 1)] : (_Float16)0.f;
#pragma unroll
    for (int idx = 0; idx < 4; ++idx)
#pragma unroll
      for (int e = 0; e < 4; ++e) ep[idx][e] = m == idx ? A.wph[4 * kg + e] : (_Float16)0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) b3c[r] = A.b3s[4 * kg + r];
  } else if constexpr (SPARSE) {
    // stored value f of lane (c16, g4): pair t = f >> 1 meets dword q = 2 (g4 >> 1) + (t & 1) of
    // its user in the B lanes of k-group gb = 2 (g4 & 1) + (t >> 1), i.e. that lane's converted
    // accumulator e = 2 q + (f & 1): unit 16 (e >> 2) + 4 gb + (e & 3)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int f = 0; f < 8; ++f) {
        const int t = f >> 1, gb = 2 * (g4 & 1) + (t >> 1), e = 2 * (2 * (g4 >> 1) + (t & 1)) + (f & 1);
        const _Float16 wv = A.wmh[16 * (e >> 2) + 4 * gb + (e & 3)];
        // ROW0: rows 4 n (user a) and 8 + 4 n (user b), i.e. 4 (2 user + n)
        ews[n][f] = (ROW0 ? (c16 == 4 * n || c16 == 8 + 4 * n) : (c16 == n || c16 == 2 + n))
                        ? wv : (_Float16)0.f;
      }
    ewi = (c16 & (ROW0 ? 8 : 2)) ? 0xEEEE : 0x4444;
  } else if constexpr (S16) {
    // the B operand of (user, item half n) is the lane's converted accumulators m = 0, 1 as one
    // h8: k = 8 g4 + e is unit 16 (e >> 2) + 4 g4 + (e & 3); A row 2 user + n holds wm in that
    // order (ewa[n]: user a, ewb[n]: user b), every k-group of the item half's own
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const _Float16 wv = A.wmh[16 * (e >> 2) + 4 * g4 + (e & 3)];
        ewa[n][e] = c16 == n ? wv : (_Float16)0.f;
        ewb[n][e] = c16 == 2 + n ? wv : (_Float16)0.f;
      }
  } else {
    const int erow = lane & 15, eg = lane >> 4;
#pragma unroll
    for (int f = 0; f < 2; ++f)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const _Float16 wv = A.wmh[mfma32_row(8 * f + e, eg >> 1)];
        ewa[f][e] = erow == (eg & 1) ? wv : (_Float16)0.f;
        ewb[f][e] = erow == 2 + (eg & 1) ? wv : (_Float16)0.f;
      }
#pragma unroll
    for (int r = 0; r < 16; r += 2)
      wm2[r >> 1] = (h2){A.wmh[mfma32_row(r, h)], A.wmh[mfma32_row(r + 1, h)]};
  }
  float* const g7 = &gsm[wave][0][0];
  // uniform scalars in SGPRs (the compiler cannot prove prm read-only, so it would keep them
  // in VGPRs -- which are the scarce resource at three waves per SIMD)
  const float cg = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(A.prm->cg)));
  // per-user registers: lane u < nu follows user u0 + u
  const float cu = lane < nu ? A.Cu[u0 + lane] : 0.f;
  float tv = __builtin_inff(), eu = 0.f;
  if (MODE == SCAN_THRESH && lane < nu) tv = A.tau[u0 + lane];
  if (MODE == SCAN_DEBUG && lane < nu) eu = A.Eu[u0 + lane];
  if (FOLD && lane < 32)
    ut[wave][lane] = make_float2(MODE == SCAN_THRESH ? tv : 0.f, cu);  // lanes >= nu: (inf | 0, 0)
  int ccount = 0;  // THRESH: appended items of user u0 + lane in this partition
  int nm = INT_BIG, mpos = 0, mend = 0;
  const bool masked = MODE == SCAN_THRESH && A.mptr != nullptr;
  if (masked && lane < nu) {
    const int64_t lo = A.mptr[u0 + lane], hi = A.mptr[u0 + lane + 1];
    mpos = (int)mask_lower_bound(A.midx, lo, hi, (int)part_start);
    mend = (int)hi;
    nm = mpos < mend ? A.midx[mpos] : INT_BIG;
  }
  int32_t* seg = MODE == SCAN_THRESH ? A.buf + ((u0 * A.NP) + p) * (int64_t)A.capp : nullptr;
  // the wave's 32 rows of candidate ids / test values (THRESH): buffer resources over the rows'
  // segments, partition p's slots at row * segstride + slot (NP * capp * 128 < 2^31: cert_shape)
  const __amdgpu_buffer_rsrc_t segrs = __builtin_amdgcn_make_buffer_rsrc(
      MODE == SCAN_THRESH ? (void*)seg : (void*)A.buf, 0,
      MODE == SCAN_THRESH ? (int)(32 * (int64_t)A.NP * A.capp * 4) : 0, 0x00020000);
  const __amdgpu_buffer_rsrc_t segdrs = __builtin_amdgcn_make_buffer_rsrc(
      MODE == SCAN_THRESH ? (void*)(A.segd + ((u0 * A.NP) + p) * (int64_t)A.capp) : (void*)A.buf,
      0, MODE == SCAN_THRESH ? (int)(32 * (int64_t)A.NP * A.capp * 4) : 0, 0x00020000);
  const int64_t segstride = (int64_t)A.NP * A.capp;  // next user's segment

  const int ntiles = part_end > part_start ? (part_end - part_start + TILE - 1) / TILE : 0;
  // tile staging: thread (row, c) moves 16 B of Q~ and of G~; tile t + 1 is fetched into
  // registers while tile t is scored, then stored to the other LDS buffer (one barrier
  // per tile)
  // (row, 16-B chunk) of the thread's staging slot, recomputed where used: held across the
  // tile loop they were spilled, and a spill reload's vmcnt wait also waits for the prefetch
  auto srow_of = [&]() {
    int v;
    asm volatile("v_lshrrev_b32 %0, 3, %1" : "=v"(v) : "v"(tid));
    return v;
  };
  auto sc_of = [&]() {
    int v;
    asm volatile("v_and_b32 %0, 7, %1" : "=v"(v) : "v"(tid));
    return v;
  };
  h8 nq = {}, ng = {};
  float nb = 0.f, nd = 0.f;  // per-item bound terms of lane j's next item
  // the champion gather map is a SAMPLE-pass input only (compile-time null elsewhere: no
  // dependent index loads, hence no mid-tile vmcnt waits, in the THRESH scan)
  const int32_t* const sidx = MODE == SCAN_SAMPLE ? A.sidx : nullptr;
  // 32-bit element offsets from the (uniform) table bases: the loads take an SGPR base and a
  // VGPR offset, so no 64-bit per-lane addresses stay live across the tile loop (I * 64 <
  // 2^31: ncf_cert_eligible)
  auto fetch = [&](int base) {
    const int srow = srow_of(), sc = sc_of();
    const int n = (int)(base + srow);
    nq = (h8){};
    ng = (h8){};
    if (n < part_end) {
      const int it = sidx ? sidx[n] : n;
      nq = *reinterpret_cast<const h8*>(A.Q16 + (uint32_t)(it * 64 + 8 * sc));
      ng = *reinterpret_cast<const h8*>(A.G16 + (uint32_t)(it * 64 + 8 * sc));
    }
    const int cj = (int)std::min<int>(base + j, part_end - 1);
    const int nj = sidx ? sidx[cj] : cj;
    nb = A.Bi[(uint32_t)nj];
    nd = A.Di[(uint32_t)nj];
  };
  auto stash = [&](int buf) {
    const int srow = srow_of(), sc = sc_of();
    // S16: chunk sc of row r lies at chunk position sc ^ (r >> 1 & 7) (the read side: s16 below)
    const int pc = S16 ? sc ^ ((srow >> 1) & 7) : sc;
    *reinterpret_cast<h8*>(&qs[buf][srow * RS + 8 * pc]) = nq;
    *reinterpret_cast<h8*>(&gs[buf][srow * RS + 8 * pc]) = ng;
  };
  int t = 0;
  if (t < ntiles) {
    fetch(part_start + t * TILE);
    stash(0);
  }
  __syncthreads();
  // drain every prologue load on every path into the loop (incl. ntiles == 0): otherwise the
  // waitcnt pass merges a pending prologue load into the loop and waits vmcnt(0) -- i.e. for
  // the tile prefetch too -- at the first use of a prologue register in every iteration
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0) (gfx9 encoding: expcnt 7, lgkmcnt 15)
  for (int cur = 0; t < ntiles; cur ^= 1) {
    const int base = part_start + t * TILE;
    const int tn = t + 1;
    const float bj = nb, dj = nd;  // bound terms of this tile's item j (test units)
    // the prefetch is the only global load in the tile body (vmcnt waits are in order: any
    // later load's wait would also wait for it)
    // PIPE: ag, re-loaded behind the previous tile's pair loop, is drained first for that reason
    if constexpr (PIPE) __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
    if (tn < ntiles) fetch(part_start + tn * TILE);
    int lrow = 0;  // lane (j, h)'s operand row offset in the tile buffers (recomputed: see srow_of)
    if constexpr (!PIPE)  // (layout 1 reads by so0 / so1; PIPE has no registers for its inputs)
    asm volatile("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(lrow) : "v"(j), "v"(RS), "v"(8 * h));

    // S16: lane (c16, g4)'s operand offsets in the tile buffers at k-steps 0 and 1, item half 0
    // (half n: + 16 n RS).  Row r keeps chunk x at position x ^ (r >> 1 & 7): a b128 read's
    // 16-lane groups pair eight lanes of one k-group with eight of the next, whose chunks differ
    // in bit 0, and the rows' swizzles (0, 1, 6, 7 against 2, 3, 4, 5 on either row parity) keep
    // the sixteen 16-B slots of the 256-B bank row distinct.  Recomputed per tile as lrow is.
    int so0 = 0, so1 = 0;
    // PIPE: the GMF table's store addresses come from this per-tile copy of the lane index too
    // (one base and immediate offsets; from `lane` they are eight registers held across the tile
    // loop, which the pipelined pair loop has not got)
    int c16t = c16, g4t = g4;
    if constexpr (S16) {
      int ln;
      asm volatile("v_mov_b32 %0, %1" : "=v"(ln) : "v"(lane));
      if constexpr (PIPE) {
        c16t = ln & 15;
        g4t = ln >> 4;
      }
      const int x0 = (ln >> 4) ^ ((ln >> 1) & 7);
      so0 = (ln & 15) * RS + 8 * x0;
      so1 = (ln & 15) * RS + 8 * (x0 ^ 4);
    }

    if (nu > 0) {
    if constexpr (S16) {  // GMF as 2 x 2 x 2 16x16x32: users 16 m + c16 x items c16 + 16 n
      f32x4 ga[2][2] = {};
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int n = 0; n < 2; ++n) {
          const h8 gb = *reinterpret_cast<const h8*>(&gs[cur][(s ? so1 : so0) + 16 * n * RS]);
#pragma unroll
          for (int m = 0; m < 2; ++m)
            ga[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ag[2 * m + s], gb, ga[m][n], 0, 0, 0);
        }
      // the same folded table as below: lane (c16, g4) holds users 16 m + 4 g4 + r of items
      // c16 + 16 n, whose bound terms lanes c16 + 16 n carry
      constexpr float sgn = MODE == SCAN_THRESH ? 1.f : -1.f;
      float bjn[2] = {0.f, 0.f}, djn[2] = {0.f, 0.f};
      if (MODE != SCAN_DEBUG) {
#pragma unroll
        for (int n = 0; n < 2; ++n) {
          if constexpr (PIPE) {  // __shfl without its own copy of the lane index
            bjn[n] = __int_as_float(__builtin_amdgcn_ds_bpermute(4 * (c16t + 16 * n), __float_as_int(bj)));
            djn[n] = __int_as_float(__builtin_amdgcn_ds_bpermute(4 * (c16t + 16 * n), __float_as_int(dj)));
          } else {
          bjn[n] = __shfl(bj, c16 + 16 * n);
          djn[n] = __shfl(dj, c16 + 16 * n);
          }
        }
      }
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 16 * m + 4 * g4t + r;
          const float2 tc = ut[wave][row];
#pragma unroll
          for (int n = 0; n < 2; ++n)
            // ROW0: [pair][64], a pair's 64 seeds in the order of the lanes that read them
            g7[ROW0 ? (row >> 1) * 64 + (row & 1) * 32 + 16 * n + c16t
                    : (((row >> 1) * 16 + c16t) << 2) + ((row & 1) << 1) + n] =
                MODE == SCAN_DEBUG ? ga[m][n][r] * cg
                                   : (ga[m][n][r] * cg + sgn * fmaf(tc.y, djn[n], bjn[n])) - tc.x;
        }
    } else {  // GMF of the wave's 32 users x 32 items, in score units
      f32x16 gacc = {};
#pragma unroll
      for (int s = 0; s < 4; ++s)
        gacc = mfma16(ag[s], *reinterpret_cast<const h8*>(&gs[cur][lrow + 16 * s]), gacc);
      if constexpr (FOLD) {
        // folded test term gmf + sgn * e_i - tau (sgn = +1 for the threshold test, -1 for the
        // sample's lower bound; the deep DEBUG pass: gmf alone)
        constexpr float sgn = MODE == SCAN_THRESH ? 1.f : -1.f;
        // (measured, round 5: the same stores from one lane base + immediate offsets -- 6 fewer
        // VGPRs -- scheduled the pair loop's LDS reads differently, +1-2 % scan time)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = mfma32_row(r, h);
          const float2 tc = ut[wave][row];
          g7[(((row >> 1) * 16 + (j & 15)) << 2) + ((row & 1) << 1) + (j >> 4)] =
              MODE == SCAN_DEBUG ? gacc[r] * cg : (gacc[r] * cg + sgn * fmaf(tc.y, dj, bj)) - tc.x;
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) gsm[wave][mfma32_row(r, h)][j] = gacc[r] * cg;
      }
    }
    h8 q[4];  // S16: q[2 n + s] = Q~[item c16 + 16 n][k = 32 s + 8 g4 + e]
#pragma unroll
    for (int s = 0; s < 4; ++s)
      q[s] = *reinterpret_cast<const h8*>(
          S16 ? &qs[cur][((s & 1) ? so1 : so0) + 16 * (s >> 1) * RS] : &qs[cur][lrow + 16 * s]);
    const int n = base + j;
    const int tile_end = std::min<int>(base + TILE, part_end);
    const int nv = (int)(tile_end - base);  // valid items of the tile
    const uint64_t vm32 = nv >= 32 ? 0xffffffffull : ((1ull << nv) - 1ull);
    unsigned mbits = 0;
    if (masked) {  // scanned items are real items here (identity map in the THRESH pass)
      uint64_t pend = __ballot(lane < 32 && nm < tile_end) & 0xffffffffull;
      while (pend) {
        const int u = __builtin_ctzll(pend);
        pend &= pend - 1;
        while (true) {
          const int tgt = hnm_readlane_i(nm, u);
          if (tgt >= tile_end) break;
          if (lane == u) {
            mbits |= 1u << (tgt - (int)base);
            ++mpos;
            nm = mpos < mend ? A.midx[mpos] : INT_BIG;
          }
        }
      }
    }

    // user r, k-step s: pw[r * 64 + 16 s] (S16: pw[r * 64 + 32 s], the lane's k-group g4 -- one
    // fragment serves both item halves)
    const _Float16* pw = &ps[(wave * upw) * 64 + 8 * (S16 ? g4 : h)];
    // THRESH: the pass test and the appends of pair (u, u + 1), whose test values d lanes 0-15
    // hold
    auto pass_test = [&](const f32x4 d, const int u) {
      const int ua = u, ub = u + 1;
      const bool hasb = ub < nu;
      if constexpr (ROW0) {
        // lane 32 user + item holds the pair's test value d[0]: the one compare's ballot is the
        // pass mask in the append's bit layout.  Like the OR of four below it may count a padded
        // item of a partial last tile (and lanes of an absent user b: seed -inf), which vmask drops.
        uint64_t m = __ballot(!(d[0] < 0.f));  // ordered compare: a NaN or -0 test value passes
        if (m == 0) return;  // uniform
        m &= vm32 | (hasb ? vm32 << 32 : 0ull);
        if (masked && m) {  // uniform
          const unsigned mba = (unsigned)hnm_readlane_i((int)mbits, ua);
          const unsigned mbb = (unsigned)hnm_readlane_i((int)mbits, ub);
          m &= ~((uint64_t)mba | ((uint64_t)mbb << 32));
        }
        if (m) {
          // every lane appends its own value at the slot its rank in its user's half of the mask
          // gives: the slots, ids and values of the four-register layout.  The user's row offset
          // differs by lane here, so it goes into the vector offset.
          const int ca = hnm_readlane_i(ccount, ua), cb = hnm_readlane_i(ccount, ub);
          int pl = lane;
          if constexpr (PIPE) asm volatile("v_mov_b32 %0, %1" : "=v"(pl) : "v"(lane));  // as below
          const int uu = pl >> 5, it = pl & 31;
          const unsigned mu = uu ? (unsigned)(m >> 32) : (unsigned)m;
          const int ps = (uu ? cb : ca) + __builtin_popcount(mu & ((1u << it) - 1u));
          if (((mu >> it) & 1u) && ps < A.capp) {
            const int so = (uu ? ub : ua) * (int)segstride * 4;
            __builtin_amdgcn_raw_buffer_store_b32((int)(base + it), segrs, so + ps * 4, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_int(d[0]), segdrs, so + ps * 4, 0, 0);
          }
          if (pl == ua) ccount += __builtin_popcount((unsigned)m);
          if (pl == ub && hasb) ccount += __builtin_popcount((unsigned)(m >> 32));
        }
        return;
      }
      // !(score + e_i < tau), ordered compares: a NaN or -0 test value passes
      const uint64_t b0 = __ballot(!(d[0] < 0.f)), b1 = __ballot(!(d[1] < 0.f));
      const uint64_t b2 = __ballot(!(d[2] < 0.f)), b3 = __ballot(!(d[3] < 0.f));
      // ~96 % of pair iterations append nothing: those end at the OR of the four compares
      // over lanes 0-15.  It may count a pair vmask excludes (a padded item of a partial last
      // tile), which the exact mask below then drops.
      if (((b0 | b1 | b2 | b3) & 0xffffull) == 0) return;  // uniform
      const uint64_t m0 = b0 & 0xffffull, m1 = b1 & 0xffffull;
      const uint64_t m2 = b2 & 0xffffull, m3 = b3 & 0xffffull;
      const uint64_t vmask = vm32 | (hasb ? vm32 << 32 : 0ull);
      uint64_t m = (m0 | (m1 << 16) | (m2 << 32) | (m3 << 48)) & vmask;
      // filtered items of the two users, looked up only for a pair with a pass (a few % of
      // pairs): two readlanes per pair in the issue-bound loop cost ~7 % of the scan
      if (masked && m) {  // uniform
        const unsigned mba = (unsigned)hnm_readlane_i((int)mbits, ua);
        const unsigned mbb = (unsigned)hnm_readlane_i((int)mbits, ub);
        m &= ~((uint64_t)mba | ((uint64_t)mbb << 32));
      }
      if (m) {
        // lane c < 16 holds d[0..3] = the test values of (a, c), (a, c + 16), (b, c),
        // (b, c + 16): it appends its passing pairs itself -- the id and, for the
        // re-scoring's best-first order, the test value -- at the slot the pair's rank in the
        // pass mask gives (no cross-lane moves; the store addresses are uniform bases)
        const int ca = hnm_readlane_i(ccount, ua), cb = hnm_readlane_i(ccount, ub);
        if constexpr (PIPE) {
        // the appends below word for word, on a copy of the lane index made here: what they
        // derive from it (masks, item ids, the lanes of users a and b) is then computed in this
        // rare path, not held in registers across the pair loop
        int pl;
        asm volatile("v_mov_b32 %0, %1" : "=v"(pl) : "v"(lane));
        if (pl < 16) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int uu = r >> 1, it = pl + 16 * (r & 1);
            const unsigned mu = (unsigned)(m >> (32 * uu));
            const int ps = (uu ? cb : ca) + __builtin_popcount(mu & ((1u << it) - 1u));
            if (((mu >> it) & 1u) && ps < A.capp) {
              const int so = (uu ? ub : ua) * (int)segstride * 4;
              __builtin_amdgcn_raw_buffer_store_b32((int)(base + it), segrs, ps * 4, so, 0);
              __builtin_amdgcn_raw_buffer_store_b32(__float_as_int(d[r]), segdrs, ps * 4, so, 0);
            }
          }
        }
        if (pl == ua) ccount += __builtin_popcount((unsigned)m);
        if (pl == ub && hasb) ccount += __builtin_popcount((unsigned)(m >> 32));
        } else {
        if (lane < 16) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int uu = r >> 1, it = lane + 16 * (r & 1);
            const unsigned mu = (unsigned)(m >> (32 * uu));
            const int ps = (uu ? cb : ca) + __builtin_popcount(mu & ((1u << it) - 1u));
            if (((mu >> it) & 1u) && ps < A.capp) {
              // buffer stores: uniform row offset in an SGPR, the slot in one VGPR (the
              // tile loop runs at the 168-VGPR limit; 64-bit addresses here spilled)
              const int so = (uu ? ub : ua) * (int)segstride * 4;
              __builtin_amdgcn_raw_buffer_store_b32((int)(base + it), segrs, ps * 4, so, 0);
              __builtin_amdgcn_raw_buffer_store_b32(__float_as_int(d[r]), segdrs, ps * 4, so, 0);
            }
          }
        }
        if (lane == ua) ccount += __builtin_popcount((unsigned)m);
        if (lane == ub && hasb) ccount += __builtin_popcount((unsigned)(m >> 32));
        }  // !PIPE
      }
    };
    // The test of a pair runs one iteration late, among the next pair's layer-2 MFMAs (and after
    // the loop for the last pair): placed behind the pair's own epilogue it waited for the last
    // MFMA of the chain and then held the wave's next LDS reads back by its compares and scalar
    // tail.  The seed of the first iteration passes nothing.
    if constexpr (PIPE) {
      // The pair loop pipelined by hand (HNM_OPT_SCAN_PIPE): the same 20 MFMAs on the same
      // operands in the same chains, the B operands formed one k-step ahead so that the packed
      // adds sit two (three with a compare) to an MFMA gap instead of in front of the MFMAs.
      //   head          ds_read: pair k + 1's s = 0 fragments
      //   s = 0 MFMAs   form pair k's s = 1 operands; the compares of pair k - 1
      //   s = 1 MFMAs   form pair k + 1's s = 0 operands (the tile's last pair: from rows past
      //                 nu -- zeros, another wave's users or the two pad rows of ps -- and unused)
      //   epilogue      ds_read: pair k's seeds and pair k + 1's s = 1 fragments (into the
      //                 registers of pair k's: read at the head they cost eight register copies a
      //                 pair, and with the seeds there the tile prefetch spilled); ten converts,
      //                 then two under each of the first three MFMAs
      // ag's registers carry the look-ahead: it is re-loaded behind the loop for the next tile.
      auto ldp = [&](const int r, const int s) {
        return *reinterpret_cast<const h8*>(&pw[r * 64 + 32 * s]);
      };
      auto form = [](const h8 pf, const h8 qf) {
        const h8 x = pf + qf;
        return __builtin_elementwise_min(__builtin_elementwise_max(x, (h8){}), (h8)(_Float16)1.f);
      };
#define HNM_SGB(M, N) __builtin_amdgcn_sched_group_barrier(M, N, 0);
#define HNM_SGB_MFMA_VALU(NV) HNM_SGB(0x008, 1) HNM_SGB(0x002, NV)
      h8 xa[2], xb[2];  // the pair's s = 0 B operands [item half n], users a and b
      h8 pa1, pb1;      // its s = 1 fragments
      {
        const h8 pa0 = ldp(0, 0), pb0 = ldp(1, 0);
        pa1 = ldp(0, 1);
        pb1 = ldp(1, 1);
#pragma unroll
        for (int n = 0; n < 2; ++n) {
          xa[n] = form(pa0, q[2 * n]);
          xb[n] = form(pb0, q[2 * n]);
        }
      }
      f32x4 dprev = {-1.f, -1.f, -1.f, -1.f};
      float dprev0 = -1.f;  // ROW0: the one register that carries test values
      // ROW0: both sparse instructions accumulate in place, and rows 4 g4 + 1 .. 3 meet zero A
      // rows: registers 1-3 are zeroed here, once a tile, and carried from pair to pair with
      // register 0 re-seeded (nothing reads them)
      f32x4 dz = {};
      for (int u = 0; u < nu; u += 2) {
        // the wave issues its layer-2 block ahead of waves in their epilogue or append path
        // (kernel only 1.577 -> 1.556 ms: profiles/ncf_scan_pipe_ab.txt); 0 again at the epilogue
        __builtin_amdgcn_s_setprio(1);
        const h8 na0 = ldp(u + 2, 0), nb0 = ldp(u + 3, 0);
        f32x4 ca[2][2], cb[2][2];  // [unit half m][item half n], users a and b
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
          for (int m = 0; m < 2; ++m) {
            ca[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(aw[2 * m], xa[n], b2q[m], 0, 0, 0);
            cb[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(aw[2 * m], xb[n], b2q[m], 0, 0, 0);
          }
        h8 x1a[2], x1b[2];
#pragma unroll
        for (int n = 0; n < 2; ++n) {
          x1a[n] = form(pa1, q[2 * n + 1]);
          x1b[n] = form(pb1, q[2 * n + 1]);
        }
        // pass_test's four compares, named here too: in program order they then stand among the
        // formation above, and the group barriers below take them into the first eight gaps
        // (pass_test's own fold into these)
        // (ROW0: the one compare)
        const uint64_t early = ROW0 ? __ballot(!(dprev0 < 0.f))
                                    : __ballot(!(dprev[0] < 0.f)) | __ballot(!(dprev[1] < 0.f)) |
                                          __ballot(!(dprev[2] < 0.f)) | __ballot(!(dprev[3] < 0.f));
        asm volatile("" ::"s"(early));
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
          for (int m = 0; m < 2; ++m) {
            ca[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(aw[2 * m + 1], x1a[n], ca[m][n], 0, 0, 0);
            cb[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(aw[2 * m + 1], x1b[n], cb[m][n], 0, 0, 0);
          }
#pragma unroll
        for (int n = 0; n < 2; ++n) {
          xa[n] = form(na0, q[2 * n]);
          xb[n] = form(nb0, q[2 * n]);
          // formed here, under these MFMAs: unpinned they sink behind the early-exit branch
          asm volatile("" : "+v"(xa[n]), "+v"(xb[n]));
        }
        HNM_SGB(0x100, 2)
        if constexpr (ROW0) {  // 16 packed adds and the one compare
        HNM_SGB_MFMA_VALU(3) HNM_SGB_MFMA_VALU(2) HNM_SGB_MFMA_VALU(2) HNM_SGB_MFMA_VALU(2)
        HNM_SGB_MFMA_VALU(2) HNM_SGB_MFMA_VALU(2) HNM_SGB_MFMA_VALU(2) HNM_SGB_MFMA_VALU(2)
        } else {
        HNM_SGB_MFMA_VALU(3) HNM_SGB_MFMA_VALU(2) HNM_SGB_MFMA_VALU(3) HNM_SGB_MFMA_VALU(2)
        HNM_SGB_MFMA_VALU(3) HNM_SGB_MFMA_VALU(2) HNM_SGB_MFMA_VALU(3) HNM_SGB_MFMA_VALU(2)
        }
        HNM_SGB_MFMA_VALU(2) HNM_SGB_MFMA_VALU(2) HNM_SGB_MFMA_VALU(2) HNM_SGB_MFMA_VALU(2)
        HNM_SGB_MFMA_VALU(2) HNM_SGB_MFMA_VALU(2) HNM_SGB_MFMA_VALU(2) HNM_SGB_MFMA_VALU(2)
        if constexpr (ROW0) dprev = (f32x4){dprev0, 0.f, 0.f, 0.f};
        pass_test(dprev, u - 2);  // the pair before this one
        __builtin_amdgcn_s_setprio(0);
        // lanes 0-15: (a, c), (a, c + 16), (b, c), (b, c + 16); other lanes' rows are unused
        // ROW0: lane 32 user + item reads its one seed; rows 4 g4 + 1 .. 3 are unused (dz)
        f32x4 d;
        if constexpr (ROW0) {
          d = dz;
          d[0] = g7[(u >> 1) * 64 + lane];
        } else {
          d = *reinterpret_cast<const f32x4*>(&g7[((u >> 1) * 16 + (lane & 15)) << 2]);
        }
        pa1 = ldp(u + 2, 1);
        pb1 = ldp(u + 3, 1);
        if constexpr (SPARSE) {
          // the 16 converts as they were, into the interleaved operands; half 0's eight and two of
          // half 1's ahead of the first instruction, the rest under it
          d = __builtin_amdgcn_smfmac_f32_16x16x64_f16(ews[0], sparse_b(ca, cb, 0), d, ewi, 0, 0);
          d = __builtin_amdgcn_smfmac_f32_16x16x64_f16(ews[1], sparse_b(ca, cb, 1), d, ewi, 0, 0);
          HNM_SGB(0x100, 3)
          HNM_SGB(0x002, 10)
          HNM_SGB_MFMA_VALU(6)
          HNM_SGB(0x008, 1)
        } else {
        h8 ya[2], yb[2];  // [item half n], the accumulators m = 0, 1 of the half as one h8
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          ya[0][e] = (_Float16)ca[e >> 2][0][e & 3];
          ya[1][e] = (_Float16)ca[e >> 2][1][e & 3];
          yb[0][e] = (_Float16)cb[e >> 2][0][e & 3];
          yb[1][e] = (_Float16)cb[e >> 2][1][e & 3];
        }
#pragma unroll
        for (int f = 0; f < 2; ++f) {
          ya[f] = __builtin_elementwise_min(__builtin_elementwise_max(ya[f], (h8){}), (h8)(_Float16)1.f);
          yb[f] = __builtin_elementwise_min(__builtin_elementwise_max(yb[f], (h8){}), (h8)(_Float16)1.f);
        }
        d = __builtin_amdgcn_mfma_f32_16x16x32_f16(ewa[0], ya[0], d, 0, 0, 0);
        d = __builtin_amdgcn_mfma_f32_16x16x32_f16(ewa[1], ya[1], d, 0, 0, 0);
        d = __builtin_amdgcn_mfma_f32_16x16x32_f16(ewb[0], yb[0], d, 0, 0, 0);
        d = __builtin_amdgcn_mfma_f32_16x16x32_f16(ewb[1], yb[1], d, 0, 0, 0);
        HNM_SGB(0x100, 3)
        HNM_SGB(0x002, 10)
        HNM_SGB_MFMA_VALU(2) HNM_SGB_MFMA_VALU(2) HNM_SGB_MFMA_VALU(2)
        HNM_SGB(0x008, 1)
        }  // !SPARSE
        dprev = d;  // tested in the next iteration
        dprev0 = d[0];
        dz = d;
      }
#undef HNM_SGB_MFMA_VALU
#undef HNM_SGB
      // the next tile's GMF A operand: issued here, drained at the top of the tile before its
      // prefetch is issued (the lane index goes through an asm so that the loads stay here)
      {
        int ln;
        asm volatile("v_mov_b32 %0, %1" : "=v"(ln) : "v"(lane));
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
          for (int s = 0; s < 2; ++s) {
            const int ur = 16 * m + (ln & 15);
            h8 z = {};
            ag[2 * m + s] =
                ur < nu ? *reinterpret_cast<const h8*>(A.WG16 + (u0 + ur) * 64 + 32 * s + 8 * (ln >> 4))
                        : z;
          }
      }
      if constexpr (ROW0) dprev = (f32x4){dprev0, 0.f, 0.f, 0.f};
      pass_test(dprev, (nu - 1) & ~1);  // the tile's last pair
    } else {
    f32x4 dprev = {-1.f, -1.f, -1.f, -1.f};
    for (int u = 0; u < nu; u += 2) {
      // user b = u + 1 even past nu (zero P~ rows; FOLD: folded term -inf / not stored)
      const int ua = u, ub = u + 1;
      const bool hasb = ub < nu;
      const int uh = h ? ub : ua;
      f32x16 acc0 = b2c, acc1 = b2c;
      f32x4 ca[2][2], cb[2][2];  // S16: [unit half m][item half n], users a and b
      if constexpr (S16) {
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
          for (int n = 0; n < 2; ++n) ca[m][n] = cb[m][n] = b2q[m];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const h8 pa = *reinterpret_cast<const h8*>(&pw[ua * 64 + 32 * s]);
          const h8 pb = *reinterpret_cast<const h8*>(&pw[ub * 64 + 32 * s]);
#pragma unroll
          for (int n = 0; n < 2; ++n) {
            h8 x = pa + q[2 * n + s];
            x = __builtin_elementwise_min(__builtin_elementwise_max(x, (h8){}), (h8)(_Float16)1.f);
            h8 y = pb + q[2 * n + s];
            y = __builtin_elementwise_min(__builtin_elementwise_max(y, (h8){}), (h8)(_Float16)1.f);
#pragma unroll
            for (int m = 0; m < 2; ++m) {
              ca[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(aw[2 * m + s], x, ca[m][n], 0, 0, 0);
              cb[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(aw[2 * m + s], y, cb[m][n], 0, 0, 0);
            }
          }
        }
      } else {
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        // each fragment is read right before its MFMA (fewer live registers than a prefetch)
        const h8 pa = *reinterpret_cast<const h8*>(&pw[ua * 64 + 16 * s]);
        const h8 pb = *reinterpret_cast<const h8*>(&pw[ub * 64 + 16 * s]);
        h8 x = pa + q[s];
        x = __builtin_elementwise_min(__builtin_elementwise_max(x, (h8){}), (h8)(_Float16)1.f);
        h8 y = pb + q[s];
        y = __builtin_elementwise_min(__builtin_elementwise_max(y, (h8){}), (h8)(_Float16)1.f);
        acc0 = mfma16(aw[s], x, acc0);
        acc1 = mfma16(aw[s], y, acc1);
      }
      }  // !S16
      if constexpr (MODE == SCAN_THRESH) pass_test(dprev, u - 2);  // the pair before this one
      if constexpr (FOLD) {
        h8 ya[2], yb[2];  // S16: [item half n], the accumulators m = 0, 1 of the half as one h8
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          if constexpr (S16) {
            ya[0][e] = (_Float16)ca[e >> 2][0][e & 3];
            ya[1][e] = (_Float16)ca[e >> 2][1][e & 3];
            yb[0][e] = (_Float16)cb[e >> 2][0][e & 3];
            yb[1][e] = (_Float16)cb[e >> 2][1][e & 3];
          } else {
            ya[0][e] = (_Float16)acc0[e];
            ya[1][e] = (_Float16)acc0[8 + e];
            yb[0][e] = (_Float16)acc1[e];
            yb[1][e] = (_Float16)acc1[8 + e];
          }
        }
#pragma unroll
        for (int f = 0; f < 2; ++f) {
          ya[f] = __builtin_elementwise_min(__builtin_elementwise_max(ya[f], (h8){}), (h8)(_Float16)1.f);
          yb[f] = __builtin_elementwise_min(__builtin_elementwise_max(yb[f], (h8){}), (h8)(_Float16)1.f);
        }
        // lanes 0-15: (a, c), (a, c + 16), (b, c), (b, c + 16); other lanes' rows are unused
        // (ROW0: lane 32 user + item reads its one seed into d[0]; d[1..3] meet zero A rows)
        f32x4 d = {};
        if constexpr (ROW0) d[0] = g7[(u >> 1) * 64 + lane];
        else d = *reinterpret_cast<const f32x4*>(&g7[((u >> 1) * 16 + (lane & 15)) << 2]);
        if constexpr (DEEP) {
#pragma unroll
          for (int uu = 0; uu < 2; ++uu)
#pragma unroll
            for (int g = 0; g < 2; ++g) {
              f32x4 t3 = b3c;
              t3 = __builtin_amdgcn_mfma_f32_16x16x32_f16(e3[g][0], uu ? yb[0] : ya[0], t3, 0, 0, 0);
              t3 = __builtin_amdgcn_mfma_f32_16x16x32_f16(e3[g][1], uu ? yb[1] : ya[1], t3, 0, 0, 0);
              h4 z = {(_Float16)t3[0], (_Float16)t3[1], (_Float16)t3[2], (_Float16)t3[3]};
              z = __builtin_elementwise_min(__builtin_elementwise_max(z, (h4){}), (h4)(_Float16)1.f);
              d = __builtin_amdgcn_mfma_f32_16x16x16f16(ep[2 * uu + g], z, d, 0, 0, 0);
            }
        } else if constexpr (SPARSE) {
          d = __builtin_amdgcn_smfmac_f32_16x16x64_f16(ews[0], sparse_b(ca, cb, 0), d, ewi, 0, 0);
          d = __builtin_amdgcn_smfmac_f32_16x16x64_f16(ews[1], sparse_b(ca, cb, 1), d, ewi, 0, 0);
        } else {
          d = __builtin_amdgcn_mfma_f32_16x16x32_f16(ewa[0], ya[0], d, 0, 0, 0);
          d = __builtin_amdgcn_mfma_f32_16x16x32_f16(ewa[1], ya[1], d, 0, 0, 0);
          d = __builtin_amdgcn_mfma_f32_16x16x32_f16(ewb[0], yb[0], d, 0, 0, 0);
          d = __builtin_amdgcn_mfma_f32_16x16x32_f16(ewb[1], yb[1], d, 0, 0, 0);
        }
        if (MODE == SCAN_DEBUG) {  // DEEP: approx and the whole bound, per pair, scaled units
          float bjr[2], djr[2];  // the bound terms of items c and c + 16 (lanes c, c + 16)
#pragma unroll
          for (int q2 = 0; q2 < 2; ++q2) {
            bjr[q2] = __shfl(bj, (lane & 15) + 16 * q2);
            djr[q2] = __shfl(dj, (lane & 15) + 16 * q2);
          }
          const float cua = hnm_readlane_f(cu, ua), cub = hnm_readlane_f(cu, ub);
          const float eua = hnm_readlane_f(eu, ua), eub = hnm_readlane_f(eu, ub);
          const uint64_t vmask = vm32 | (hasb ? vm32 << 32 : 0ull);
          if constexpr (ROW0) {
            // every lane stores its one pair: user lane >> 5, item j, whose bound terms it holds
            if ((vmask >> lane) & 1) {
              const int64_t o = (u0 + ua + h) * A.ldo + base + j;
              A.dense[o] = d[0];
              A.dense2[o] = (h ? eub : eua) + fmaf(h ? cub : cua, dj, bj);
            }
          } else
          if (lane < 16) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int it = lane + 16 * (r & 1);
              if ((vmask >> (32 * (r >> 1) + it)) & 1) {
                const int64_t o = (u0 + ua + (r >> 1)) * A.ldo + base + it;
                A.dense[o] = d[r];
                A.dense2[o] = (r >> 1 ? eub : eua) + fmaf(r >> 1 ? cub : cua, djr[r & 1], bjr[r & 1]);
              }
            }
          }
        } else if (MODE == SCAN_SAMPLE) {
          const uint64_t vmask = vm32 | (hasb ? vm32 << 32 : 0ull);
          if constexpr (ROW0) {
            if ((vmask >> lane) & 1) A.dense[(u0 + ua + h) * A.ldo + base + j] = d[0];  // score - e_i
          } else
          if (lane < 16) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int it = lane + 16 * (r & 1);
              if ((vmask >> (32 * (r >> 1) + it)) & 1)
                A.dense[(u0 + ua + (r >> 1)) * A.ldo + base + it] = d[r];  // score - e_i
            }
          }
        } else {
          dprev = d;  // THRESH: tested in the next iteration
        }
      } else {  // DEBUG: approx score and the whole bound, per pair, in scaled units
        float ma = 0.f, mb = 0.f;
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
          h2 ya = {(_Float16)acc0[r], (_Float16)acc0[r + 1]};
          ya = __builtin_elementwise_min(__builtin_elementwise_max(ya, (h2){}), (h2)(_Float16)1.f);
          h2 yb = {(_Float16)acc1[r], (_Float16)acc1[r + 1]};
          yb = __builtin_elementwise_min(__builtin_elementwise_max(yb, (h2){}), (h2)(_Float16)1.f);
          ma = __builtin_amdgcn_fdot2(ya, wm2[r >> 1], ma, false);
          mb = __builtin_amdgcn_fdot2(yb, wm2[r >> 1], mb, false);
        }
        // after the swap lanes 0-31 hold user a's total, lanes 32-63 user b's
        const auto sw2 = __builtin_amdgcn_permlane32_swap(__float_as_uint(ma), __float_as_uint(mb),
                                                          false, false);
        const float score = (__uint_as_float(sw2[0]) + __uint_as_float(sw2[1])) + gsm[wave][uh][j];
        const float cuh = h ? hnm_readlane_f(cu, ub) : hnm_readlane_f(cu, ua);
        const float euh = h ? hnm_readlane_f(eu, ub) : hnm_readlane_f(eu, ua);
        if (n < part_end && (h == 0 || hasb)) {
          A.dense[(u0 + uh) * A.ldo + n] = score;
          A.dense2[(u0 + uh) * A.ldo + n] = euh + fmaf(cuh, dj, bj);
        }
      }
    }
    if constexpr (MODE == SCAN_THRESH) pass_test(dprev, (nu - 1) & ~1);  // the tile's last pair
    }  // !PIPE
    }  // nu > 0
    if (tn < ntiles) stash(cur ^ 1);
    __syncthreads();
    t = tn;
  }
  if (MODE == SCAN_THRESH && lane < nu) A.cnt[(u0 + lane) * A.NP + p] = ccount;
}

template <int MODE>
void launch_scan(hnm_ctx* ctx, dim3 grid, const ScanArgs& a) {
  // HNM_OPT_SCAN_SHAPE picks the two-layer scan's layout, every pass of a call alike (the deep
  // scan has the 32x32x16 layout only)
  if (a.W3h)
    hipLaunchKernelGGL((ncf16_scan_kernel<MODE, true>), grid, dim3(256), 0, ctx->stream, a);
  else if (ctx->scan_shape && ctx->scan_pipe && MODE == SCAN_THRESH) {
    // HNM_OPT_SCAN_PIPE: the threshold pass of layout 1 with its pair loop pipelined by hand
    // (HNM_OPT_SCAN_SPARSE: every pass of layout 1 with the epilogue on the sparse instruction)
    // (HNM_OPT_SCAN_ROW0: every pass with the sparse epilogue, the test values in one register)
    if (ctx->scan_sparse && ctx->scan_row0)
      hipLaunchKernelGGL((ncf16_scan_kernel<SCAN_THRESH, false, 1, true, true, true>), grid,
                         dim3(256), 0, ctx->stream, a);
    else if (ctx->scan_sparse)
      hipLaunchKernelGGL((ncf16_scan_kernel<SCAN_THRESH, false, 1, true, true>), grid, dim3(256), 0,
                         ctx->stream, a);
    else
      hipLaunchKernelGGL((ncf16_scan_kernel<SCAN_THRESH, false, 1, true>), grid, dim3(256), 0,
                         ctx->stream, a);
  } else if (ctx->scan_shape && ctx->scan_sparse && ctx->scan_row0)
    hipLaunchKernelGGL((ncf16_scan_kernel<MODE, false, 1, false, true, true>), grid, dim3(256), 0,
                       ctx->stream, a);
  else if (ctx->scan_shape && ctx->scan_sparse)
    hipLaunchKernelGGL((ncf16_scan_kernel<MODE, false, 1, false, true>), grid, dim3(256), 0,
                       ctx->stream, a);
  else if (ctx->scan_shape)
    hipLaunchKernelGGL((ncf16_scan_kernel<MODE, false, 1>), grid, dim3(256), 0, ctx->stream, a);
  else
    hipLaunchKernelGGL((ncf16_scan_kernel<MODE, false, 0>), grid, dim3(256), 0, ctx->stream, a);
}

}  // namespace

void cert_launch_scan(hnm_ctx* ctx, int mode, dim3 grid, const ScanArgs& a) {
  if (mode == SCAN_SAMPLE) launch_scan<SCAN_SAMPLE>(ctx, grid, a);
  else if (mode == SCAN_THRESH) launch_scan<SCAN_THRESH>(ctx, grid, a);
  else launch_scan<SCAN_DEBUG>(ctx, grid, a);
}
