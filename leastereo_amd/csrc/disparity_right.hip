// Right-view disparity from the left-view matching cost: the disparity head read along the
// diagonals of the up-sampled cost (the classical SGM construction), fused like
// disparity.hip and disparity_stats.hip so that U is never materialised.
//
// U[od, y, x]: the trilinear align_corners=False up-sampling of cost[b, 0] to [MD, Ho, Wo],
// MD = maxdisp = 3 D3, Ho = 3 H3, Wo = 3 W3 (lea_disparity_regression's U).  For a
// right-image pixel (y, xr):
//   candidate od is in view iff xr + od <= Wo - 1 (od = 0 always is); n = min(MD, Wo - xr)
//   p_R[od]            = softmax over od < n of (-U[od, y, xr + od])
//   disp_right[b,y,xr] = sum_{od < n} od p_R[od]
// The last column is exactly 0; MD > Wo is legal.  The softmax shift m is the minimum of U
// over the in-view candidates only: a minimum over every plane can lie far below all of
// them, and every exponential underflows (s = 0).
//
// Staged form (the configured depths): one workgroup owns 256 right pixels of one output
// row.  Right column xr = 3c + r and candidate od = 3k + j read left column
// 3(c + k) + r + j, so plane k needs source columns c0 + k - 2 .. c0 + k + 88 (c0: the
// tile's first source column): a parallelogram.  It is stored skewed, plane k at
// [k][col - k - (c0 - 2)], every plane indexed by the same c + const: at one od a wave's
// lanes read consecutive addresses, three lanes per address (a broadcast), whatever the
// row stride -- no bank conflict.  Column col + 1 is the next address and plane k + 1 at
// the same column is kRCols - 1 further, so the four taps of a candidate are two
// two-address reads off one base.  Plane D3 repeats plane D3 - 1 (the depth clamp) and
// columns are clamped into [0, W3) when staged (the width clamp): k1 = k0 + 1 and
// i1 = i0 + 1 always.  The depth and width axes' aten weights come from axis_index once per
// workgroup, as two small LDS tables (per od; per left column of the tile).
//
// The round-6 factorisation does not carry over: along the diagonal the three samples of a
// plane sit at three different columns, so MD exponentials are formed per pixel.  The staged
// form walks the candidates once, twelve at a time (MD is a multiple of 12 at every
// configured depth): the twelve U in registers, the running minimum m lowered by theirs,
// the sums so far rescaled by exp(m_new - m_old) -- one more exponential per twelve -- then
// the twelve terms; m is only ever a minimum of in-view candidates.  The generic form makes
// two passes over the same U expression (minimum, then sums; m - U <= 0 exactly).
#include "disparity_common.h"

namespace lea {

constexpr int kRCols = 92;  // staged columns per plane: local index 0 .. 90 is read

template <bool FAST>
__device__ __forceinline__ float right_exp(float x) {  // x <= 0, -inf included (0)
  if constexpr (FAST)
    return __builtin_amdgcn_exp2f(x * 0x1.715476p+0f);
  else
    return exp_noovf(x);
}

// disp_right of one pixel from n in-view candidates; u(od) must give the same bits twice
template <bool FAST, class UF>
__device__ __forceinline__ float right_softmin(const int n, const UF& u) {
#pragma clang fp contract(off)
  float m = u(0);
#pragma unroll 4
  for (int od = 1; od < n; ++od) m = fminf(m, u(od));
  float s = 0.f, t = 0.f;
#pragma unroll 4
  for (int od = 0; od < n; ++od) {
    const float e = right_exp<FAST>(m - u(od));
    s += e;
    t += (float)od * e;
  }
  return t / s;  // s >= 1: the minimum's own term
}

constexpr int kRChunk = 12;

// the same sum in one walk: u(od) is called once per candidate, od < ceil(n / 12) * 12
template <bool FAST, class UF>
__device__ __forceinline__ float right_softmin_online(const int n, const UF& u) {
#pragma clang fp contract(off)
  const float inf = __builtin_inff();
  float m = inf, s = 0.f, t = 0.f;
  for (int o0 = 0; o0 < n; o0 += kRChunk) {
    float uu[kRChunk];
    float mn = m;
#pragma unroll
    for (int i = 0; i < kRChunk; ++i) {
      uu[i] = o0 + i < n ? u(o0 + i) : inf;  // out of view: a term of exp(-inf) = 0
      mn = fminf(mn, uu[i]);
    }
    // the first chunk: m = inf, s = t = 0, and exp(-200) is 0 in f32
    const float sc = right_exp<FAST>(fmaxf(mn - m, -200.f));
    s *= sc;
    t *= sc;
    m = mn;
#pragma unroll
    for (int i = 0; i < kRChunk; ++i) {
      const float e = right_exp<FAST>(m - uu[i]);
      s += e;
      t += (float)(o0 + i) * e;
    }
  }
  return t / s;  // s >= 1: the minimum's own term
}

struct RDepth {  // candidate od: the lower plane's skewed offset and the depth weights
  int off;
  float l0, l1;
};
struct RCol {  // left column x of the tile: its lower source column (+ 2 - c0) and the weight
  int wi;
  float lam;
};

template <int D3, bool FAST>
__global__ __launch_bounds__(kDispThreads) void disparity_right_rows_f32(const float* __restrict__ cost,
                                                                         float* __restrict__ disp_right, int H3,
                                                                         int W3, float rd, float rh, float rw) {
#pragma clang fp contract(off)
  constexpr int MD = 3 * D3;
  static_assert(MD % kRChunk == 0, "the walk reads whole chunks of the depth table");
  constexpr int kX = kDispThreads + MD;  // left columns xr0 .. xr0 + 255 + MD - 1 (one spare)
  __shared__ float hl[(D3 + 1) * kRCols];
  __shared__ RDepth dt[MD];
  __shared__ RCol ct[kX];
  const int Ho = 3 * H3, Wo = 3 * W3;
  const int xr0 = blockIdx.x * kDispThreads;
  const int oh = blockIdx.y;
  const int b = blockIdx.z;
  const int c0 = xr0 / 3;
  const Axis ah = axis_index(rh, oh, H3, Ho, 0);
  const long long HW = (long long)H3 * W3;
  const float* base = cost + (long long)b * D3 * HW;
  const float* r0 = base + (long long)ah.i0 * W3;
  const float* r1 = base + (long long)ah.i1 * W3;
  for (int e = threadIdx.x; e < (D3 + 1) * kRCols; e += kDispThreads) {
    const int k = e / kRCols, i = e - k * kRCols;
    const int col = min(max(c0 + k - 2 + i, 0), W3 - 1);  // nothing outside [0, W3) is read
    const long long o = (long long)min(k, D3 - 1) * HW + col;
    hl[e] = ah.l0 * r0[o] + ah.l1 * r1[o];
  }
  for (int od = threadIdx.x; od < MD; od += kDispThreads) {
    const Axis ad = axis_index(rd, od, D3, MD, 0);
    dt[od] = RDepth{ad.i0 * (kRCols - 1), ad.l0, ad.l1};
  }
  for (int e = threadIdx.x; e < kX; e += kDispThreads) {
    const Axis aw = axis_index(rw, min(xr0 + e, Wo - 1), W3, Wo, 0);
    ct[e] = RCol{aw.i0 - c0 + 2, aw.l1};
  }
  __syncthreads();
  const int xr = xr0 + threadIdx.x;
  if (xr >= Wo) return;  // no barrier below
  const int n = min(MD, Wo - xr);
  const RCol* cx = ct + threadIdx.x;
  auto u = [&](int od) {
    const RDepth d = dt[od];
    const RCol c = cx[od];
    const float* p = hl + (d.off + c.wi);
    const float w0 = 1.f - c.lam;
    const float v0 = w0 * p[0] + c.lam * p[1];
    const float v1 = w0 * p[kRCols - 1] + c.lam * p[kRCols];
    return d.l0 * v0 + d.l1 * v1;
  };
  disp_right[((long long)b * Ho + oh) * Wo + xr] = right_softmin_online<FAST>(n, u);
}

// Any other depth: one thread per right pixel, the taps read from global memory (H before
// W before D, as the staged form), D3 a run-time value.
template <bool FAST>
__global__ __launch_bounds__(kDispThreads) void disparity_right_any_f32(const float* __restrict__ cost,
                                                                        float* __restrict__ disp_right, int D3,
                                                                        int H3, int W3, float rd, float rh,
                                                                        float rw) {
#pragma clang fp contract(off)
  const int MD = 3 * D3, Ho = 3 * H3, Wo = 3 * W3;
  const int xr = blockIdx.x * blockDim.x + threadIdx.x;
  if (xr >= Wo) return;
  const int oh = blockIdx.y;
  const int b = blockIdx.z;
  const Axis ah = axis_index(rh, oh, H3, Ho, 0);
  const long long HW = (long long)H3 * W3;
  const float* base = cost + (long long)b * D3 * HW;
  const float* r0 = base + (long long)ah.i0 * W3;
  const float* r1 = base + (long long)ah.i1 * W3;
  const int n = min(MD, Wo - xr);
  auto u = [&](int od) {
    const Axis ad = axis_index(rd, od, D3, MD, 0);
    const Axis aw = axis_index(rw, xr + od, W3, Wo, 0);  // xr + od <= Wo - 1: i0, i1 in [0, W3)
    auto plane = [&](int k) {
      const long long o = (long long)k * HW;
      return aw.l0 * (ah.l0 * r0[o + aw.i0] + ah.l1 * r1[o + aw.i0]) +
             aw.l1 * (ah.l0 * r0[o + aw.i1] + ah.l1 * r1[o + aw.i1]);
    };
    return ad.l0 * plane(ad.i0) + ad.l1 * plane(ad.i1);
  };
  disp_right[((long long)b * Ho + oh) * Wo + xr] = right_softmin<FAST>(n, u);
}

}  // namespace lea

extern "C" int lea_disparity_regression_right(const void* cost, float* disp_right, int B, int D3, int H3, int W3,
                                              int maxdisp, int dtype, void* stream) {
  using namespace lea;
  clear_error();
  const char* who = "lea_disparity_regression_right";
  DispHead h;
  if (int rc = disp_head_check(who, true, "lea_disparity_regression_right: disp_right overlaps cost", cost,
                               &disp_right, 1, B, D3, H3, W3, maxdisp, dtype, &h))
    return rc;
  const float rd = (float)D3 / (float)maxdisp, rh = h.rh, rw = h.rw;
  const bool fast = h.fast;
  const dim3 grid = h.grid;
#define LEA_RIGHT_ROWS(D3_)                                                                                \
  if (D3 == D3_) {                                                                                        \
    auto k_ = fast ? disparity_right_rows_f32<D3_, true> : disparity_right_rows_f32<D3_, false>;            \
    k_<<<grid, kDispThreads, 0, as_stream(stream)>>>((const float*)cost, disp_right, H3, W3, rd, rh, rw);   \
    return launch_status(who);                                                                            \
  }
  LEA_RIGHT_ROWS(4) LEA_RIGHT_ROWS(8) LEA_RIGHT_ROWS(16) LEA_RIGHT_ROWS(32) LEA_RIGHT_ROWS(64) LEA_RIGHT_ROWS(88)
#undef LEA_RIGHT_ROWS
  auto k_ = fast ? disparity_right_any_f32<true> : disparity_right_any_f32<false>;
  k_<<<grid, kDispThreads, 0, as_stream(stream)>>>((const float*)cost, disp_right, D3, H3, W3, rd, rh, rw);
  return launch_status(who);
}
