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
// (disparity_rows3_f32 / disparity_rows_f32 with softmin_fact): the same staging, the same
// plane(k) expression and the same order of the s and t accumulations, so disp is the plain
// entry's bit for bit.  With a_k = (m - v_k) / 3 the exponent of exp(m - U[od]) is
// a_{k-1} + 2 a_k, 3 a_k or 2 a_k + a_{k+1} -- sums of numbers the factored form has formed
// already -- so with q = sum e (m - U):
//   entropy = ln s - q / s      (no logarithm per term; the hardware-exp path carries a_k,
//                                and so q, in log2 units and scales by ln 2 once)
// and the window sums are e and od e under a per-term select.
#include "disparity_common.h"

namespace lea {

struct DispStats {
  float disp, entropy, peak, local;
};

// softmin_fact (disparity.hip) with the stats accumulators.  `plane(k)`: the bilinearly
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

// disparity_rows_f32's staging (two source rows of every plane, H-lerped into LDS); D3 = 88.
template <int D3, bool FAST>
__global__ __launch_bounds__(kDispThreads, 4) void disparity_stats_rows_f32(const float* __restrict__ cost,
                                                                           DispStatsOut out, int H3, int W3,
                                                                           float rh, float rw, float rf) {
#pragma clang fp contract(off)
  __shared__ float hl[D3 * kDispCols];
  const int Ho = 3 * H3, Wo = 3 * W3;
  const int ow0 = blockIdx.x * blockDim.x;
  const int oh = blockIdx.y;
  const int b = blockIdx.z;
  const AxisW ah = src_axis(rh, oh, H3, Ho);
  const int c_lo = src_axis(rw, ow0, W3, Wo).i0;
  const int c_hi = src_axis(rw, min(ow0 + (int)blockDim.x - 1, Wo - 1), W3, Wo).i1;
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
  __syncthreads();
  const int ow = ow0 + threadIdx.x;
  if (ow >= Wo) return;  // no barrier below
  const AxisW aw = src_axis(rw, ow, W3, Wo);
  const int j0 = min(aw.i0 - c_lo, kDispCols - 1), j1 = min(aw.i1 - c_lo, kDispCols - 1);
  auto plane = [&](int dd) { return aw.l0 * hl[dd * kDispCols + j0] + aw.l1 * hl[dd * kDispCols + j1]; };
  store_stats(out, ((long long)b * Ho + oh) * Wo + ow, softmin_stats<FAST>(D3, rf, plane), over);
}

// disparity_rows3_f32's staging (three source rows, the three output rows' H-lerps in LDS).
template <int D3, bool FAST>
__global__ __launch_bounds__(kDisp3Threads) void disparity_stats_rows3_f32(const float* __restrict__ cost,
                                                                          DispStatsOut out, int H3, int W3,
                                                                          float rh, float rw, float rf) {
#pragma clang fp contract(off)
  __shared__ float hl[3][D3 * kDispCols];
  const int Ho = 3 * H3, Wo = 3 * W3;
  const int ow0 = blockIdx.x * kDispThreads;
  const int k = blockIdx.y;  // source row k: output rows 3k .. 3k + 2
  const int b = blockIdx.z;
  const AxisW a0 = src_axis(rh, 3 * k, H3, Ho), a1 = src_axis(rh, 3 * k + 1, H3, Ho),
              a2 = src_axis(rh, 3 * k + 2, H3, Ho);
  // the staged raw rows: lo = min of the three rows' i0 (k - 1, or 0 at the top), lo + 1, lo + 2
  // clamped to the map; every i0 / i1 of the three rows lies in [lo, lo + 2] (x3: k - 1 .. k + 1)
  const int lo = min(a0.i0, min(a1.i0, a2.i0));
  const int r1 = min(lo + 1, H3 - 1), r2 = min(lo + 2, H3 - 1);
  const int c_lo = src_axis(rw, ow0, W3, Wo).i0;
  const int c_hi = src_axis(rw, min(ow0 + kDispThreads - 1, Wo - 1), W3, Wo).i1;
  const bool over = c_hi - c_lo + 1 > kDispCols ||
                    max(a0.i1, max(a1.i1, a2.i1)) > lo + 2;  // host-checked; NaN rather than a wrong row
  const int ncol = min(c_hi - c_lo + 1, kDispCols);
  const long long HW = (long long)H3 * W3;
  const float* base = cost + (long long)b * D3 * HW + c_lo;
  const float* p0 = base + (long long)lo * W3;
  const float* p1 = base + (long long)r1 * W3;
  const float* p2 = base + (long long)r2 * W3;
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
  __syncthreads();
  const int row = __builtin_amdgcn_readfirstlane(threadIdx.x / kDispThreads);  // wave-uniform
  const int ow = ow0 + (int)threadIdx.x % kDispThreads;
  const int oh = 3 * k + row;
  if (ow >= Wo) return;  // no barrier below
  const float* h = hl[row];
  const AxisW aw = src_axis(rw, ow, W3, Wo);
  const int j0 = min(aw.i0 - c_lo, kDispCols - 1), j1 = min(aw.i1 - c_lo, kDispCols - 1);
  auto plane = [&](int dd) { return aw.l0 * h[dd * kDispCols + j0] + aw.l1 * h[dd * kDispCols + j1]; };
  store_stats(out, ((long long)b * Ho + oh) * Wo + ow, softmin_stats<FAST>(D3, rf, plane), over);
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
  const AxisW ah = src_axis(rh, oh, H3, Ho);
  const AxisW aw = src_axis(rw, ow, W3, Wo);
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
  LEA_CHECK_ARG(cost && disp, "lea_disparity_regression_stats: null pointer");
  LEA_CHECK_ARG(entropy || peak || disp_local,
                "lea_disparity_regression_stats: no output wanted (entropy, peak and disp_local all null)");
  LEA_CHECK_ARG(B > 0 && D3 > 0 && H3 > 0 && W3 > 0 && maxdisp > 0,
                "lea_disparity_regression_stats: bad shape B=%d D3=%d H3=%d W3=%d maxdisp=%d", B, D3, H3,
                W3, maxdisp);
  LEA_CHECK_ARG(radius >= 1 && radius <= 16, "lea_disparity_regression_stats: radius %d outside 1..16", radius);
  LEA_CHECK_ARG(3LL * H3 <= 65535 && B <= 65535, "lea_disparity_regression_stats: grid too large");
  if (dtype != LEA_F32 && dtype != LEA_BF16) {
    set_error("lea_disparity_regression_stats: dtype %d unsupported", dtype);
    return LEA_E_UNSUPPORTED;
  }
  if (maxdisp % 3 != 0 || maxdisp / 3 != D3) {
    set_error("lea_disparity_regression_stats: maxdisp %d is not 3 * D3 (D3=%d)", maxdisp, D3);
    return LEA_E_UNSUPPORTED;
  }
  {  // no output may overlap another or the cost (the kernels read cost while they write)
    const size_t n_out = (size_t)B * 9u * (size_t)H3 * (size_t)W3 * sizeof(float);
    const size_t n_cost = (size_t)B * (size_t)D3 * (size_t)H3 * (size_t)W3 * sizeof(float);
    const uintptr_t lo[5] = {(uintptr_t)cost, (uintptr_t)disp, (uintptr_t)entropy, (uintptr_t)peak,
                             (uintptr_t)disp_local};
    for (int i = 0; i < 5; ++i)
      for (int j = i + 1; j < 5; ++j) {
        if (!lo[i] || !lo[j]) continue;
        const size_t ni = i == 0 ? n_cost : n_out;
        LEA_CHECK_ARG(lo[i] + ni <= lo[j] || lo[j] + n_out <= lo[i],
                      "lea_disparity_regression_stats: buffers %d and %d overlap "
                      "(0 = cost, 1 = disp, 2 = entropy, 3 = peak, 4 = disp_local)", i, j);
      }
  }
  const int Wo = 3 * W3;
  const float rh = (float)H3 / (float)(3 * H3), rw = (float)W3 / (float)(3 * W3);
  const float rf = (float)radius;
  const bool fast = dtype == LEA_BF16;
  const DispStatsOut out{disp, entropy, peak, disp_local};
  const dim3 grid((Wo + kDispThreads - 1) / kDispThreads, 3 * H3, B);
  // the row-staged forms: 256 outputs of a row read <= kDispCols source columns (Wo = 3 W3)
  const bool cols_ok = (256LL * W3 + Wo - 1) / Wo + 2 <= kDispCols;
#define LEA_STATS_ROWS3(D3_)                                                                              \
  if (D3 == D3_) {                                                                                       \
    auto k_ = fast ? disparity_stats_rows3_f32<D3_, true> : disparity_stats_rows3_f32<D3_, false>;        \
    k_<<<dim3(grid.x, H3, B), kDisp3Threads, 0, as_stream(stream)>>>((const float*)cost, out, H3, W3, rh, \
                                                                      rw, rf);                            \
    return launch_status("lea_disparity_regression_stats");                                              \
  }
  if (cols_ok) {
    LEA_STATS_ROWS3(4) LEA_STATS_ROWS3(8) LEA_STATS_ROWS3(16) LEA_STATS_ROWS3(32) LEA_STATS_ROWS3(64)
    // D3 = 88 -- config 5 -- keeps the two-row staging, as the plain entry does: three rows'
    // LDS (101 KB) leave one workgroup per CU there
    if (D3 == 88) {
      auto k_ = fast ? disparity_stats_rows_f32<88, true> : disparity_stats_rows_f32<88, false>;
      k_<<<grid, kDispThreads, 0, as_stream(stream)>>>((const float*)cost, out, H3, W3, rh, rw, rf);
      return launch_status("lea_disparity_regression_stats");
    }
  }
#undef LEA_STATS_ROWS3
  auto k_ = fast ? disparity_stats_any_f32<true> : disparity_stats_any_f32<false>;
  k_<<<grid, kDispThreads, 0, as_stream(stream)>>>((const float*)cost, out, D3, H3, W3, rh, rw, rf);
  return launch_status("lea_disparity_regression_stats");
}
