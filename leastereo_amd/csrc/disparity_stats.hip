// Disparity regression with per-pixel confidence: the fused head of disparity.hip
// (models/build_model_2d.py:52-57 + :33-42) that also writes what the softmin distribution
// p = softmax(-U) over maxdisp says about each pixel, from the registers that already hold
// it.  The reference started on this with DispEntropy (build_model_2d.py:11-24: softmax
// instead of softmin, then a softmin over the image height) and left it unused.
//
//   entropy    = -sum_od p ln p                       nats, [0, ln MD]
//   winner     k* = first index of min_k v[k], od* = 3 k* + 1   (on the planes, not on U:
//              U[0] == U[1] and U[MD-2] ~ U[MD-1], an argmin over od flips at the clamped ends)
//   peak       = sum_{|od - od*| <= r} p[od]          (0, 1]
//   disp_local = sum_{|od - od*| <= r} od p[od] / peak
//
// Built on the row-staged factored form the plain entry runs by default
// (disparity_rows3_f32 / disparity_rows_f32 with softmin_fact): the staging and the plane(k)
// accessor are that form's own functions (disparity_common.h) and the s and t accumulations
// run in softmin_fact's order, so disp is the plain entry's bit for bit.  With
// a_k = (m - v_k) / 3 the exponent of exp(m - U[od]) is a_{k-1} + 2 a_k, 3 a_k or
// 2 a_k + a_{k+1} -- sums of numbers the factored form has formed already -- so with
// q = sum e (m - U):
//   entropy = ln s - q / s      (no logarithm per term; the hardware-exp path carries a_k,
//                                and so q, in log2 units and scales by ln 2 once)
// and the window sums are e and od e under a per-term select.
#include "disparity_common.h"

namespace lea {

struct DispStats {
  float disp, entropy, peak, local;
};

// softmin_fact (disparity_common.h) with the stats accumulators.  `plane(k)`: the bilinearly
// interpolated cost plane k at this pixel, k in [0, D3); MD = 3 D3.  rf: the window radius.
template <bool FAST, class Plane>
__device__ __forceinline__ DispStats softmin_stats(const int D3, const float rf, const Plane& plane) {
#pragma clang fp contract(off)
  float m = plane(0);
  int ks = 0;  // first index of the minimum (strict <)
#pragma unroll 8
  for (int dd = 1; dd < D3; ++dd) {
    const float v = plane(dd);
    const bool lt = v < m;
    m = lt ? v : m;
    ks = lt ? dd : ks;
  }
  // a_k: the exponent of F_k, in nats (exp_noovf) or in log2 units (hardware exp2)
  auto ak = [&](int dd) {
    if constexpr (FAST)
      return (m - plane(dd)) * (0x1.715476p+0f / 3.f);
    else
      return (m - plane(dd)) * 0x1.555556p-2f;
  };
  auto fe = [&](float a) {
    if constexpr (FAST)
      return __builtin_amdgcn_exp2f(a);
    else
      return exp_noovf(a);
  };
  const float ods = (float)(3 * ks + 1);
  float s = 0.f, t = 0.f, q = 0.f, wm = 0.f, wt = 0.f;
  float ap = ak(0), ac = ap;          // a_{k-1}, a_k
  float fp = fe(ap), fc = fp;         // F_{k-1}, F_k
  float od = 0.f;                     // 3k (exact in float)
  auto term = [&](float o, float e, float g) {
    s += e;
    t += o * e;
    q += e * g;  // e = 0 (underflow) with g finite: 0
    const float w = fabsf(o - ods) <= rf ? e : 0.f;
    wm += w;
    wt += o * w;
  };
#pragma unroll 4
  for (int k = 0; k < D3; ++k) {
    const bool last = k + 1 >= D3;
    const float an = last ? ac : ak(k + 1);
    const float fn = last ? fc : fe(an);
    const float f2 = fc * fc, a2 = ac + ac;
    const float e1 = f2 * fc, g1 = a2 + ac;
    const float e0 = k == 0 ? e1 : fp * f2, g0 = k == 0 ? g1 : ap + a2;
    const float e2 = last ? e1 : f2 * fn, g2 = last ? g1 : a2 + an;
    term(od, e0, g0);
    term(od + 1.f, e1, g1);
    term(od + 2.f, e2, g2);
    od += 3.f;
    ap = ac;
    ac = an;
    fp = fc;
    fc = fn;
  }
  // s >= e1 at k* = 1 and wm >= 1 likewise: no division by zero.  The clamps take the last
  // rounding of ln s - q / s and wm / s back into the quantities' ranges.
  DispStats r;
  r.disp = t / s;
  const float h = logf(s) - (FAST ? q * 0x1.62e43p-1f : q) / s;
  r.entropy = fminf(fmaxf(h, 0.f), logf((float)(3 * D3)));
  r.peak = fminf(wm / s, 1.f);
  r.local = wt / wm;
  return r;
}

struct DispStatsOut {
  float *disp, *entropy, *peak, *local;  // entropy / peak / local: null = not wanted
};

__device__ __forceinline__ void store_stats(const DispStatsOut& o, long long i, const DispStats& r, bool over) {
  const float nan = __builtin_nanf("");
  o.disp[i] = over ? nan : r.disp;
  if (o.entropy) o.entropy[i] = over ? nan : r.entropy;
  if (o.peak) o.peak[i] = over ? nan : r.peak;
  if (o.local) o.local[i] = over ? nan : r.local;
}

// The staged kernels hand softmin_stats their plane accessor through a closure written at the
// call: given the DispPlane object itself, disparity_stats_rows3_f32<4, true> takes one VGPR
// more than before the accessor was shared (26 for 25).

// The two-row staged form (stage_rows2: two source rows of every plane, H-lerped into LDS);
// D3 = 88.
template <int D3, bool FAST>
__global__ __launch_bounds__(kDispThreads, 4) void disparity_stats_rows_f32(const float* __restrict__ cost,
                                                                           DispStatsOut out, int H3, int W3,
                                                                           float rh, float rw, float rf) {
  __shared__ float hl[D3 * kDispCols];
  const int Ho = 3 * H3, Wo = 3 * W3;
  const int ow0 = blockIdx.x * blockDim.x;
  const int oh = blockIdx.y;
  const int b = blockIdx.z;
  const DispStage st = stage_rows2<D3>(hl, cost, b, oh, ow0, H3, W3, rh, rw);
  __syncthreads();
  const int ow = ow0 + threadIdx.x;
  if (ow >= Wo) return;  // no barrier below
  const DispPlane plane = disp_plane(hl, rw, ow, W3, st.c_lo);
  const DispStats r = softmin_stats<FAST>(D3, rf, [&](int dd) { return plane(dd); });
  store_stats(out, ((long long)b * Ho + oh) * Wo + ow, r, st.over);
}

// The three-row staged form (stage_rows3: three source rows, the three output rows' H-lerps
// in LDS).
template <int D3, bool FAST>
__global__ __launch_bounds__(kDisp3Threads) void disparity_stats_rows3_f32(const float* __restrict__ cost,
                                                                          DispStatsOut out, int H3, int W3,
                                                                          float rh, float rw, float rf) {
  __shared__ float hl[3][D3 * kDispCols];
  const int Ho = 3 * H3, Wo = 3 * W3;
  const int ow0 = blockIdx.x * kDispThreads;
  const int k = blockIdx.y;  // source row k: output rows 3k .. 3k + 2
  const int b = blockIdx.z;
  const DispRows3 st = rows3_span(k, ow0, H3, W3, rh, rw);
  stage_rows3<D3>(hl, cost, b, st, H3, W3);
  __syncthreads();
  const int row = __builtin_amdgcn_readfirstlane(threadIdx.x / kDispThreads);  // wave-uniform
  const int ow = ow0 + (int)threadIdx.x % kDispThreads;
  const int oh = 3 * k + row;
  if (ow >= Wo) return;  // no barrier below
  const DispPlane plane = disp_plane(hl[row], rw, ow, W3, st.c_lo);
  const DispStats r = softmin_stats<FAST>(D3, rf, [&](int dd) { return plane(dd); });
  store_stats(out, ((long long)b * Ho + oh) * Wo + ow, r, st.over);
}

// Any other depth (MD = 3 D3): one thread per output pixel, the planes bilinearly
// interpolated from global memory (H before W, as the staged forms), minimum first, then the
// sums -- the same two passes, D3 a run-time value.  Every plane is formed twice; 3 x 3
// output pixels share its four source values (cache-resident).
template <bool FAST>
__global__ __launch_bounds__(kDispThreads) void disparity_stats_any_f32(const float* __restrict__ cost,
                                                                        DispStatsOut out, int D3, int H3, int W3,
                                                                        float rh, float rw, float rf) {
#pragma clang fp contract(off)
  const int Ho = 3 * H3, Wo = 3 * W3;
  const int ow = blockIdx.x * blockDim.x + threadIdx.x;
  if (ow >= Wo) return;
  const int oh = blockIdx.y;
  const int b = blockIdx.z;
  const Axis ah = axis_index(rh, oh, H3, Ho, 0);
  const Axis aw = axis_index(rw, ow, W3, Wo, 0);
  const long long HW = (long long)H3 * W3;
  const float* base = cost + (long long)b * D3 * HW;
  const float* r0 = base + (long long)ah.i0 * W3;
  const float* r1 = base + (long long)ah.i1 * W3;
  auto plane = [&](int dd) {
    const long long o = (long long)dd * HW;
    return aw.l0 * (ah.l0 * r0[o + aw.i0] + ah.l1 * r1[o + aw.i0]) +
           aw.l1 * (ah.l0 * r0[o + aw.i1] + ah.l1 * r1[o + aw.i1]);
  };
  store_stats(out, ((long long)b * Ho + oh) * Wo + ow, softmin_stats<FAST>(D3, rf, plane), false);
}

}  // namespace lea

extern "C" int lea_disparity_regression_stats(const void* cost, float* disp, float* entropy, float* peak,
                                              float* disp_local, int B, int D3, int H3, int W3, int maxdisp,
                                              int radius, int dtype, void* stream) {
  using namespace lea;
  clear_error();
  const char* who = "lea_disparity_regression_stats";
  const float* outs[4] = {disp, entropy, peak, disp_local};
  DispHead h;
  if (int rc = disp_head_check(who, true,
                               "lea_disparity_regression_stats: buffers %d and %d overlap "
                               "(0 = cost, 1 = disp, 2 = entropy, 3 = peak, 4 = disp_local)",
                               cost, outs, 4, B, D3, H3, W3, maxdisp, dtype, &h))
    return rc;
  LEA_CHECK_ARG(entropy || peak || disp_local, "%s: no output wanted (entropy, peak and disp_local all null)", who);
  LEA_CHECK_ARG(radius >= 1 && radius <= 16, "%s: radius %d outside 1..16", who, radius);
  const float rh = h.rh, rw = h.rw, rf = (float)radius;
  const bool fast = h.fast;
  const DispStatsOut out{disp, entropy, peak, disp_local};
  const dim3 grid = h.grid;
#define LEA_STATS_ROWS3(D3_)                                                                              \
  if (D3 == D3_) {                                                                                       \
    auto k_ = fast ? disparity_stats_rows3_f32<D3_, true> : disparity_stats_rows3_f32<D3_, false>;        \
    k_<<<dim3(grid.x, H3, B), kDisp3Threads, 0, as_stream(stream)>>>((const float*)cost, out, H3, W3, rh, \
                                                                      rw, rf);                            \
    return launch_status(who);                                                                           \
  }
  if (h.cols_ok) {
    LEA_STATS_ROWS3(4) LEA_STATS_ROWS3(8) LEA_STATS_ROWS3(16) LEA_STATS_ROWS3(32) LEA_STATS_ROWS3(64)
    // D3 = 88 -- config 5 -- keeps the two-row staging, as the plain entry does: three rows'
    // LDS (101 KB) leave one workgroup per CU there
    if (D3 == 88) {
      auto k_ = fast ? disparity_stats_rows_f32<88, true> : disparity_stats_rows_f32<88, false>;
      k_<<<grid, kDispThreads, 0, as_stream(stream)>>>((const float*)cost, out, H3, W3, rh, rw, rf);
      return launch_status(who);
    }
  }
#undef LEA_STATS_ROWS3
  auto k_ = fast ? disparity_stats_any_f32<true> : disparity_stats_any_f32<false>;
  k_<<<grid, kDispThreads, 0, as_stream(stream)>>>((const float*)cost, out, D3, H3, W3, rh, rw, rf);
  return launch_status(who);
}
