// What the disparity head's units share (disparity.hip: the plain head, disparity_stats.hip:
// the head with per-pixel confidence, disparity_right.hip: the right view's head): the block
// shapes and the two exponentials, the row-staged forms' staging, plane accessor and
// per-pixel softmin phases, and the entries' host checks.  The up-sampling axis is common.h's
// axis_index (align_corners=False).  The plain and the stats kernels stage through the same
// functions and read their planes through the same accessor, so the disparity they write is
// the same number.
#pragma once
#include "common.h"

namespace lea {

constexpr int kDispThreads = 256;
constexpr int kDispChunk = 16;  // cost planes fetched per batch of loads

// LDS: the depth axis table (identical for every pixel) and, per thread, one
// batch of bilinearly interpolated cost planes (own column: conflict-free).
// FAST: hardware exp (v_exp_f32 on x*log2e, ~1e-6 relative) for the bf16 path
// (dtype LEA_BF16: its matching cost carries ~1e-2 relative error already); the
// f32 path keeps the accurate expf.
template <bool FAST>
__device__ __forceinline__ float dexp(float x) {
  if constexpr (FAST)
    return __expf(x);
  else
    return expf(x);
}

// expf(x) for x that cannot overflow (the register form's m - U <= rounding above 0):
// the device library's sequence -- x log2(e) split hi / lo, exp2 of the reduced
// argument, ldexp, the underflow select -- without its overflow select (bit-identical)
__device__ __forceinline__ float exp_noovf(float x) {
#pragma clang fp contract(off)
  const float ph = x * 0x1.715476p+0f;
  float pl = fmaf(x, 0x1.715476p+0f, -ph);
  pl = fmaf(x, 0x1.4ae0bep-26f, pl);
  const float rn = __builtin_rintf(ph);
  const float r = __builtin_ldexpf(__builtin_amdgcn_exp2f((ph - rn) + pl), (int)rn);
  return x < -0x1.9fe368p+6f ? 0.f : r;
}

// the row-staged forms: 256 consecutive outputs of a row read at most this many source columns
constexpr int kDispCols = 96;  // >= the source columns of 256 outputs at x3 (88), + slack

// the three-row form: 3 x 256 threads own 256 columns of output rows 3k .. 3k + 2
constexpr int kDisp3Threads = 3 * kDispThreads;

// ---- staging of the row-staged forms (every thread of the workgroup calls it; the caller
// places the barrier).  c_lo: the first staged source column; over: the tile needs more than
// was staged (the host checks that it does not: the outputs are NaN rather than wrong).
struct DispStage {
  int c_lo;
  bool over;
};

// Two-row form: the workgroup (blockDim.x threads) owns output columns ow0 .. ow0 +
// blockDim.x - 1 of output row oh, whose pixels read two source rows (ah.i0, ah.i1) of every
// plane over <= kDispCols source columns.  Those are H-lerped once into LDS,
// hl[dd][c] = ah.l0 * row0 + ah.l1 * row1 (coalesced loads, two per value).
template <int D3>
__device__ __forceinline__ DispStage stage_rows2(float (&hl)[D3 * kDispCols], const float* __restrict__ cost,
                                                 const int b, const int oh, const int ow0, const int H3,
                                                 const int W3, const float rh, const float rw) {
#pragma clang fp contract(off)
  const int Ho = 3 * H3, Wo = 3 * W3;
  const Axis ah = axis_index(rh, oh, H3, Ho, 0);
  const int c_lo = axis_index(rw, ow0, W3, Wo, 0).i0;
  const int c_hi = axis_index(rw, min(ow0 + (int)blockDim.x - 1, Wo - 1), W3, Wo, 0).i1;
  // host: <= kDispCols (Wo = 3 W3); past it the staging is clamped and the outputs are NaN
  const bool over = c_hi - c_lo + 1 > kDispCols;
  const int ncol = min(c_hi - c_lo + 1, kDispCols);
  const long long HW = (long long)H3 * W3;
  const float* base = cost + (long long)b * D3 * HW + c_lo;
  const float* r0 = base + (long long)ah.i0 * W3;
  const float* r1 = base + (long long)ah.i1 * W3;
  for (int e = threadIdx.x; e < D3 * ncol; e += blockDim.x) {
    const int dd = e / ncol, c = e - dd * ncol;
    const long long o = (long long)dd * HW + c;
    hl[dd * kDispCols + c] = ah.l0 * r0[o] + ah.l1 * r1[o];
  }
  return DispStage{c_lo, over};
}

// Three-row form: output rows 3k, 3k + 1, 3k + 2 read source rows k - 1, k, k + 1 only (x3
// up-sampling, align_corners=False), so one workgroup of kDisp3Threads owns 256 columns of all
// three and loads every raw source value once.  Each output row's LDS row is
// ah.l0 * row(ah.i0) + ah.l1 * row(ah.i1) with that row's own weights -- stage_rows2's
// expression on the same values, so hl[r] holds what stage_rows2 stages for row 3k + r.
//
// rows3_span: what the workgroup stages -- the three output rows' axes, the raw rows lo, r1, r2
// and the columns c_lo .. c_lo + ncol - 1.  A function of its own, called ahead of stage_rows3:
// with `over` formed inside the staging function the compiler moves it behind the loop and the
// kernels take one or two VGPRs more than with the staging written out in them.
struct DispRows3 {
  Axis a0, a1, a2;  // output rows 3k, 3k + 1, 3k + 2
  int lo, r1, r2, c_lo, ncol;
  bool over;
};

__device__ __forceinline__ DispRows3 rows3_span(const int k, const int ow0, const int H3, const int W3,
                                                const float rh, const float rw) {
  const int Ho = 3 * H3, Wo = 3 * W3;
  DispRows3 g;
  g.a0 = axis_index(rh, 3 * k, H3, Ho, 0), g.a1 = axis_index(rh, 3 * k + 1, H3, Ho, 0),
  g.a2 = axis_index(rh, 3 * k + 2, H3, Ho, 0);
  // the staged raw rows: lo = min of the three rows' i0 (k - 1, or 0 at the top), lo + 1, lo + 2
  // clamped to the map; every i0 / i1 of the three rows lies in [lo, lo + 2] (x3: k - 1 .. k + 1)
  g.lo = min(g.a0.i0, min(g.a1.i0, g.a2.i0));
  g.r1 = min(g.lo + 1, H3 - 1), g.r2 = min(g.lo + 2, H3 - 1);
  g.c_lo = axis_index(rw, ow0, W3, Wo, 0).i0;
  const int c_hi = axis_index(rw, min(ow0 + kDispThreads - 1, Wo - 1), W3, Wo, 0).i1;
  // host-checked; NaN rather than a wrong row
  g.over = c_hi - g.c_lo + 1 > kDispCols || max(g.a0.i1, max(g.a1.i1, g.a2.i1)) > g.lo + 2;
  g.ncol = min(c_hi - g.c_lo + 1, kDispCols);
  return g;
}

template <int D3>
__device__ __forceinline__ void stage_rows3(float (&hl)[3][D3 * kDispCols], const float* __restrict__ cost,
                                            const int b, const DispRows3& g, const int H3, const int W3) {
#pragma clang fp contract(off)
  const Axis a0 = g.a0, a1 = g.a1, a2 = g.a2;
  const int lo = g.lo, ncol = g.ncol;
  const long long HW = (long long)H3 * W3;
  const float* base = cost + (long long)b * D3 * HW + g.c_lo;
  const float* p0 = base + (long long)lo * W3;
  const float* p1 = base + (long long)g.r1 * W3;
  const float* p2 = base + (long long)g.r2 * W3;
  // row i of the map as one of the three staged values (workgroup-uniform selects)
  auto pick = [&](int i, float v0, float v1, float v2) { return i == lo ? v0 : (i == lo + 1 ? v1 : v2); };
  for (int e = threadIdx.x; e < D3 * ncol; e += kDisp3Threads) {
    const int dd = e / ncol, c = e - dd * ncol;
    const long long o = (long long)dd * HW + c;
    const float v0 = p0[o], v1 = p1[o], v2 = p2[o];
    const int s = dd * kDispCols + c;
    hl[0][s] = a0.l0 * pick(a0.i0, v0, v1, v2) + a0.l1 * pick(a0.i1, v0, v1, v2);
    hl[1][s] = a1.l0 * pick(a1.i0, v0, v1, v2) + a1.l1 * pick(a1.i1, v0, v1, v2);
    hl[2][s] = a2.l0 * pick(a2.i0, v0, v1, v2) + a2.l1 * pick(a2.i1, v0, v1, v2);
  }
}

// plane(dd): the bilinearly interpolated cost plane dd at output column ow, from the staged
// row h -- two LDS reads per plane, v = aw.l0 * h[dd][j0] + aw.l1 * h[dd][j1].  H before W:
// the bilinear weights are applied in the other order than disparity_reg_f32 (same values up
// to fp32 rounding).
struct DispPlane {
  const float* h;
  float l0, l1;
  int j0, j1;
  __device__ __forceinline__ float operator()(const int dd) const {
#pragma clang fp contract(off)
    return l0 * h[dd * kDispCols + j0] + l1 * h[dd * kDispCols + j1];
  }
};

__device__ __forceinline__ DispPlane disp_plane(const float* h, const float rw, const int ow, const int W3,
                                                const int c_lo) {
  const Axis aw = axis_index(rw, ow, W3, 3 * W3, 0);
  return DispPlane{h, aw.l0, aw.l1, min(aw.i0 - c_lo, kDispCols - 1), min(aw.i1 - c_lo, kDispCols - 1)};
}

// ---- the per-pixel phases of the row-staged forms: disp = sum_od od e^(m - U[od]) / sum_od
// e^(m - U[od]) over the MD depths U up-samples the D3 planes to.  Every U[od] is a convex
// combination of two planes, so m = min_dd plane(dd) <= min_od U[od] and the sum is >= e^(m -
// min U) > 0: the same ratio as the reference's softmax(-U) (max-subtracted), with no
// running-minimum rescale.

// One exponential per od.  Pass 1: the smallest plane value; pass 2 forms the planes again from
// LDS in depth order (the register form kept all D3 of them live: two waves per SIMD).
// D3 and MD are the kernel's template constants, passed as arguments on purpose: the loops then
// unroll after this function is inlined into the kernel.  As template parameters they unroll in
// the function first, the vectoriser sinks the second pass below the sched_barriers and the
// kernels take up to 128 VGPRs and scratch instead of 36-74.
template <bool FAST, class Plane>
__device__ __forceinline__ float softmin_twopass(const Plane& plane, const int D3, const int MD) {
#pragma clang fp contract(off)
  float m = plane(0);
#pragma unroll
  for (int dd = 1; dd < D3; ++dd) {
    m = fminf(m, plane(dd));
    if (dd % 8 == 7) __builtin_amdgcn_sched_barrier(0);
  }
  const float rd = (float)D3 / (float)MD;
  float s = 0.f, t = 0.f;
  float vlo = plane(0), vhi = plane(D3 > 1 ? 1 : 0);
  int k = 0;  // vlo = plane k, vhi = plane min(k + 1, D3 - 1): constants after unrolling
#pragma clang loop unroll(full)
  for (int od = 0; od < MD; ++od) {
    const Axis ad = axis_index(rd, od, D3, MD, 0);  // constants after unrolling
    while (k < ad.i0) {
      ++k;
      vlo = vhi;
      vhi = plane(k + 1 < D3 ? k + 1 : D3 - 1);
    }
    const float v1 = ad.i1 == k ? vlo : vhi;
    const float u = ad.l0 * vlo + ad.l1 * v1;
    const float e = FAST ? dexp<true>(m - u) : exp_noovf(m - u);
    s += e;
    t += (float)od * e;
    if (od % 12 == 11) __builtin_amdgcn_sched_barrier(0);
  }
  return t / s;
}

// FACT (r06, form 4): D3 exponentials instead of MD.  x3 up-sampling along D with
// align_corners=False puts od = 3k + 1 on plane k and od = 3k, 3k + 2 a third of the way
// towards planes k - 1, k + 1 (clamped at the ends), so with F_k = exp((m - v_k) / 3):
// exp(m - u) = F_{k-1} F_k^2,  F_k^3,  F_k^2 F_{k+1}, summed in the same od order.  The kernel
// is VALU-bound on the exponentials; rolled loops keep it at 32-49 VGPRs.  Not bit-identical
// to the per-od exponentials (a few ulp per term; the oracle bars).
template <int D3, int MD, bool FAST, class Plane>
__device__ __forceinline__ float softmin_fact(const Plane& plane) {
#pragma clang fp contract(off)
  static_assert(MD == 3 * D3, "x3 depth up-sampling");
  // a plain select (no NaN in the planes): fminf's NaN rule let the vectoriser split this loop
  // into per-pair NaN tests and divergent branches
  float m = plane(0);
#pragma unroll 8
  for (int dd = 1; dd < D3; ++dd) {
    const float v = plane(dd);
    m = v < m ? v : m;
  }
  auto fk = [&](int dd) {
    if constexpr (FAST)  // __expf's exp2(x log2 e) with the 1/3 folded into its multiplier
      return __builtin_amdgcn_exp2f((m - plane(dd)) * (0x1.715476p+0f / 3.f));
    else
      return exp_noovf((m - plane(dd)) * 0x1.555556p-2f);
  };
  float s = 0.f, t = 0.f;
  float fp = fk(0), fc = fp;  // F_{k-1}, F_k
  float od = 0.f;             // 3k (exact in float)
#pragma unroll 4
  for (int k = 0; k < D3; ++k) {
    const float fn = k + 1 < D3 ? fk(k + 1) : fc;
    const float f2 = fc * fc;
    const float e1 = f2 * fc;
    const float e0 = k == 0 ? e1 : fp * f2;
    const float e2 = k + 1 < D3 ? f2 * fn : e1;
    s += e0;
    t += od * e0;
    s += e1;
    t += (od + 1.f) * e1;
    s += e2;
    t += (od + 2.f) * e2;
    od += 3.f;
    fp = fc;
    fc = fn;
  }
  return t / s;
}

// ---- host: what the three entries check before they launch, and what they derive
struct DispHead {
  int Wo;
  float rh, rw;
  bool fast;     // dtype LEA_BF16: the hardware exponential
  bool cols_ok;  // the row-staged forms: 256 outputs of a row read <= kDispCols source columns
  dim3 grid;     // 256 output columns x one output row x one batch element per workgroup
};

// who: the entry's name.  outs[0 .. n_outs): the entry's outputs, [B, 3H3, 3W3] f32 each;
// outs[0] is required, a null one after it is not wanted.  need_x3: the entry takes
// maxdisp == 3 * D3 only.  overlap_fmt: the entry's text for two buffers that overlap -- the
// kernels read cost while they write -- given the two indices (0 = cost, 1 + i = outs[i]);
// null: the entry does not check.  LEA_OK, or the code with the text set.
inline int disp_head_check(const char* who, const bool need_x3, const char* overlap_fmt, const void* cost,
                           const float* const* outs, const int n_outs, const int B, const int D3, const int H3,
                           const int W3, const int maxdisp, const int dtype, DispHead* h) {
  LEA_CHECK_ARG(cost && outs[0], "%s: null pointer", who);
  LEA_CHECK_ARG(B > 0 && D3 > 0 && H3 > 0 && W3 > 0 && maxdisp > 0, "%s: bad shape B=%d D3=%d H3=%d W3=%d maxdisp=%d",
                who, B, D3, H3, W3, maxdisp);
  LEA_CHECK_ARG(3LL * H3 <= 65535 && B <= 65535 && 3LL * W3 <= 0x7fffffffLL - kDispThreads, "%s: grid too large",
                who);
  if (dtype != LEA_F32 && dtype != LEA_BF16) {
    set_error("%s: dtype %d unsupported", who, dtype);
    return LEA_E_UNSUPPORTED;
  }
  if (need_x3 && (maxdisp % 3 != 0 || maxdisp / 3 != D3)) {
    set_error("%s: maxdisp %d is not 3 * D3 (D3=%d)", who, maxdisp, D3);
    return LEA_E_UNSUPPORTED;
  }
  if (overlap_fmt) {
    const size_t n_out = (size_t)B * 9u * (size_t)H3 * (size_t)W3 * sizeof(float);
    const size_t n_cost = (size_t)B * (size_t)D3 * (size_t)H3 * (size_t)W3 * sizeof(float);
    for (int i = 0; i <= n_outs; ++i)
      for (int j = i + 1; j <= n_outs; ++j) {
        const void* a = i ? outs[i - 1] : cost;
        LEA_CHECK_ARG(!a || !outs[j - 1] || !spans_overlap(a, i ? n_out : n_cost, outs[j - 1], n_out), overlap_fmt,
                      i, j);
      }
  }
  h->Wo = 3 * W3;
  h->rh = (float)H3 / (float)(3 * H3);
  h->rw = (float)W3 / (float)(3 * W3);
  h->fast = dtype == LEA_BF16;
  h->cols_ok = (256LL * W3 + h->Wo - 1) / h->Wo + 2 <= kDispCols;
  h->grid = dim3((h->Wo + kDispThreads - 1) / kDispThreads, 3 * H3, B);
  return LEA_OK;
}

}  // namespace lea
