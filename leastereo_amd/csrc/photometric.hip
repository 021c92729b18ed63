// Photometric consistency on the device: warp the right image to the left view with the
// predicted disparity, compare it with the left image by an SSIM + L1 error, and give the
// gradient of that error with respect to the disparity.  The contract is the comment on
// lea_photometric_f32 / lea_photometric_grad_f32 in include/leastereo_hip.h; in short
//
//   xs = float(x) - disp          one f32 subtraction
//   in_view = isfinite(disp) && 0 <= xs <= W-1,  x0 = min(floor(xs), W-2),  t = xs - x0 (exact)
//   w_c = R_c[y,x0] + t (R_c[y,x0+1] - R_c[y,x0]),  dw_c/ddisp = -(R_c[y,x0+1] - R_c[y,x0])
//   v  = in_view && !exclude;  vs(p) = p interior and v on all nine pixels of its 3x3 window
//   l1 = mean_c |L_c - w_c|;  dssim = mean_c clamp((1 - SSIM_c) / 2, 0, 1)
//   sums = { #v, sum_v l1, #vs, sum_vs dssim }
//
// The interpolation is evaluated in float64 and rounded once: the f32 expression loses all
// its digits where R0 and t (R1 - R0) cancel, and both kernels must see the same w.  The
// SSIM moments are centred (sum (x - mu)^2 / 9), which is the same function as E[x^2] - mu^2
// and does not cancel.  Terms are f32; they are summed in float64 per thread, per wave by
// shuffles, per workgroup into the workspace and by one workgroup in a fixed order: no
// atomics, the same inputs give the same bits.
//
// Forward (photometric_kernel): a 64 x 16 tile (kPhW, kPhH) with a halo of 1; the warped and
// the left tile of all C <= 4 channels and the mask v are staged in LDS, the right image is
// read by a row gather from global memory.  9 maps of 66 x 18 dwords = 42.8 KB: 3 workgroups
// per CU.  Lanes of a wave run along x, so every LDS access is a dword at consecutive
// addresses (no bank conflict at any row stride).
//
// Gradient (photometric_grad_kernel), gather form, one launch, no atomics.  With
// S = n1 n2 / (d1 d2) the four SSIM factors of window p (x = left, y = warped),
//   dS_p/dw_q = (a_p + b_p w_q + c_p L_q) / 9
//   a = 2 mu_x (n2 - n1) / (d1 d2) - 2 S mu_y (1/d1 - 1/d2),  b = -2 S / d2,  c = 2 n1 / (d1 d2)
// so the gradient at q is three 3x3 box sums of coefficient maps masked by vs.  A workgroup
// stages x0 and t of its tile plus a halo of 2 once, then per channel the warped, left and
// slope maps, writes a, b, c of the tile plus 1 into LDS and gathers from them.  46.2 KB of
// LDS: 3 workgroups per CU.  The coefficients are worked out in float64 from the f32 maps and
// rounded once (1/d1 and 1/d2 reach the hundreds where a window's means or variances are
// small, and a, b, c are then differences of large terms); the box sums and the rest are f32.
#include "reduce4.h"

namespace lea {

constexpr int kPhW = 64, kPhH = 16, kPhThreads = 256, kPhMaxC = 4;
constexpr int kPhRows = kPhH / (kPhThreads / kPhW);  // rows per thread

struct PhotoMaps {
  const float* left;
  const float* right;
  const float* disp;
  const unsigned char* exclude;  // may be null
  long long lbs, rbs, dbs, ebs;
  int C, H, W;
  float c1, c2;
};

struct WarpAt {
  int x0;
  float t;
  bool in_view;
};

__device__ __forceinline__ WarpAt warp_at(const float d, const int x, const int W) {
#pragma clang fp contract(off)
  WarpAt s{0, 0.f, false};
  const float xs = (float)x - d;
  if (__builtin_isfinite(d) && xs >= 0.f && xs <= (float)(W - 1)) {
    const int f = (int)floorf(xs);
    s.in_view = true;
    s.x0 = f < W - 2 ? f : W - 2;
    s.t = xs - (float)s.x0;  // exact: xs in [x0, x0 + 1]
  }
  return s;
}

// one correctly rounded interpolation; the slope is the f32 difference
__device__ __forceinline__ float lerp_row(const float* __restrict__ row, const int x0, const float t,
                                          float* __restrict__ slope) {
  const float r0 = row[x0], r1 = row[x0 + 1];
  *slope = r1 - r0;
  return (float)fma((double)t, (double)r1 - (double)r0, (double)r0);
}

template <typename T>
struct SsimFactors {
  T mx, my, n1, n2, d1, d2;
};

// x, y: top-left corners of the 3x3 windows of the left and the warped map, row stride s;
// T = float for the forward terms, double for the gradient's coefficients
template <typename T>
__device__ __forceinline__ SsimFactors<T> ssim_factors(const float* __restrict__ x, const float* __restrict__ y,
                                                       const int s, const float c1, const float c2) {
  T sx = 0, sy = 0;
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      sx += (T)x[j * s + i];
      sy += (T)y[j * s + i];
    }
  SsimFactors<T> f;
  f.mx = sx / (T)9;
  f.my = sy / (T)9;
  T vx = 0, vy = 0, vxy = 0;
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const T dx = (T)x[j * s + i] - f.mx, dy = (T)y[j * s + i] - f.my;
      vx += dx * dx;
      vy += dy * dy;
      vxy += dx * dy;
    }
  f.n1 = (T)2 * f.mx * f.my + (T)c1;
  f.n2 = (T)2 * (vxy / (T)9) + (T)c2;
  f.d1 = f.mx * f.mx + f.my * f.my + (T)c1;
  f.d2 = vx / (T)9 + vy / (T)9 + (T)c2;
  return f;
}

// v on all nine pixels of the window whose top-left corner is m (row stride s)
__device__ __forceinline__ bool window_valid(const int* __restrict__ m, const int s) {
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int i = 0; i < 3; ++i) ok = ok && m[j * s + i] >= 0;
  return ok;
}

__global__ __launch_bounds__(kPhThreads) void photometric_kernel(const PhotoMaps a, const float alpha,
                                                                 double* __restrict__ partial,
                                                                 float* __restrict__ warped, float* __restrict__ err) {
  constexpr int SW = kPhW + 2, SH = kPhH + 2, SN = SH * SW;  // staged pixels, origin tile - 1
  __shared__ float Wp[kPhMaxC * SN];
  __shared__ float Lf[kPhMaxC * SN];
  __shared__ int V[SN];  // 0 where v holds, -1 elsewhere
  __shared__ double red[kPhThreads / kWave][4];
  const int tx0 = blockIdx.x * kPhW, ty0 = blockIdx.y * kPhH, b = blockIdx.z;
  const long long hw = (long long)a.H * a.W;
  const float* lf = a.left + b * a.lbs;
  const float* rt = a.right + b * a.rbs;
  const float* dp = a.disp + b * a.dbs;
  const unsigned char* ex = a.exclude ? a.exclude + b * a.ebs : nullptr;
  for (int idx = threadIdx.x; idx < SN; idx += kPhThreads) {
    const int sy = idx / SW, sx = idx - sy * SW;
    const int gy = ty0 - 1 + sy, gx = tx0 - 1 + sx;
    const bool inside = gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
    WarpAt s{0, 0.f, false};
    bool excluded = false;
    const long long o = (long long)gy * a.W + gx;
    if (inside) {
      s = warp_at(dp[o], gx, a.W);
      excluded = ex && ex[o] != 0;
    }
    V[idx] = (s.in_view && !excluded) ? 0 : -1;
    const bool own = inside && sy >= 1 && sy <= kPhH && sx >= 1 && sx <= kPhW;  // the tile itself
    for (int c = 0; c < a.C; ++c) {
      float w = 0.f, l = 0.f, slope;
      if (s.in_view) w = lerp_row(rt + c * hw + (long long)gy * a.W, s.x0, s.t, &slope);
      if (inside) l = lf[c * hw + o];
      Wp[c * SN + idx] = w;
      Lf[c * SN + idx] = l;
      if (own && warped) warped[((long long)b * a.C + c) * hw + o] = w;
    }
  }
  __syncthreads();
  const int ox = threadIdx.x % kPhW, rg = threadIdx.x / kPhW;
  const float inv_c = 1.f / (float)a.C;  // C in {1, 2, 4}: exact; C = 3 is divided below
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int r = 0; r < kPhRows; ++r) {
    const int oy = rg * kPhRows + r;
    const int gy = ty0 + oy, gx = tx0 + ox;
    if (gy >= a.H || gx >= a.W) continue;
    const int ci = (oy + 1) * SW + ox + 1;
    float e = -1.f;
    if (V[ci] >= 0) {
      float l1 = 0.f;
      for (int c = 0; c < a.C; ++c) l1 += fabsf(Lf[c * SN + ci] - Wp[c * SN + ci]);
      l1 = a.C == 3 ? l1 / 3.f : l1 * inv_c;
      acc[0] += 1.0;
      acc[1] += (double)l1;
      e = l1;
      const int wi = oy * SW + ox;  // the window's top-left corner
      if (gy >= 1 && gy <= a.H - 2 && gx >= 1 && gx <= a.W - 2 && window_valid(V + wi, SW)) {
        float ds = 0.f;
        for (int c = 0; c < a.C; ++c) {
          const SsimFactors<float> f = ssim_factors<float>(Lf + c * SN + wi, Wp + c * SN + wi, SW, a.c1, a.c2);
          const float ssim = (f.n1 * f.n2) / (f.d1 * f.d2);
          ds += fminf(fmaxf(0.5f * (1.f - ssim), 0.f), 1.f);
        }
        ds = a.C == 3 ? ds / 3.f : ds * inv_c;
        acc[2] += 1.0;
        acc[3] += (double)ds;
        e = (1.f - alpha) * l1 + alpha * ds;
      }
    }
    if (err) err[(long long)b * hw + (long long)gy * a.W + gx] = e;
  }
  reduce4_block<kPhThreads>(acc, red, partial);
}

__global__ __launch_bounds__(kPhThreads) void photometric_grad_kernel(const PhotoMaps a,
                                                                      const double* __restrict__ sums,
                                                                      const float* __restrict__ scales,
                                                                      float* __restrict__ ddisp, const long long gbs) {
  constexpr int SW = kPhW + 4, SH = kPhH + 4, SN = SH * SW;  // staged pixels, origin tile - 2
  constexpr int FW = kPhW + 2, FH = kPhH + 2, FN = FH * FW;  // windows by their centre, origin tile - 1
  __shared__ int X0[SN];  // x0 where v holds, -1 elsewhere
  __shared__ float T[SN];
  __shared__ float Wm[SN];
  __shared__ float Lm[SN];
  __shared__ float Sl[SN];
  __shared__ int VS[FN];
  __shared__ float CA[FN];
  __shared__ float CB[FN];
  __shared__ float CC[FN];
  const int tx0 = blockIdx.x * kPhW, ty0 = blockIdx.y * kPhH, b = blockIdx.z;
  const long long hw = (long long)a.H * a.W;
  const float* lf = a.left + b * a.lbs;
  const float* rt = a.right + b * a.rbs;
  const float* dp = a.disp + b * a.dbs;
  const unsigned char* ex = a.exclude ? a.exclude + b * a.ebs : nullptr;
  for (int idx = threadIdx.x; idx < SN; idx += kPhThreads) {
    const int sy = idx / SW, sx = idx - sy * SW;
    const int gy = ty0 - 2 + sy, gx = tx0 - 2 + sx;
    int x0 = -1;
    float t = 0.f;
    if (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) {
      const long long o = (long long)gy * a.W + gx;
      const WarpAt s = warp_at(dp[o], gx, a.W);
      if (s.in_view && !(ex && ex[o] != 0)) {
        x0 = s.x0;
        t = s.t;
      }
    }
    X0[idx] = x0;
    T[idx] = t;
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < FN; idx += kPhThreads) {
    const int fy = idx / FW, fx = idx - fy * FW;
    const int py = ty0 - 1 + fy, px = tx0 - 1 + fx;
    VS[idx] = (py >= 1 && py <= a.H - 2 && px >= 1 && px <= a.W - 2 && window_valid(X0 + fy * SW + fx, SW)) ? 1 : 0;
  }
  // the two means' scales, with the sign of dw/ddisp = -slope folded in
  const double nv = sums[0], nvs = sums[2];
  const float kl = nv > 0.0 ? (float)(-(double)scales[0] / (nv * (double)a.C)) : 0.f;
  const float ks = nvs > 0.0 ? (float)((double)scales[1] / (18.0 * nvs * (double)a.C)) : 0.f;
  const int ox = threadIdx.x % kPhW, rg = threadIdx.x / kPhW;
  float acc[kPhRows];
#pragma unroll
  for (int r = 0; r < kPhRows; ++r) acc[r] = 0.f;
  for (int c = 0; c < a.C; ++c) {
    for (int idx = threadIdx.x; idx < SN; idx += kPhThreads) {
      const int x0 = X0[idx];
      float w = 0.f, l = 0.f, slope = 0.f;
      if (x0 >= 0) {
        const int sy = idx / SW, sx = idx - sy * SW;
        const long long row = c * hw + (long long)(ty0 - 2 + sy) * a.W;
        w = lerp_row(rt + row, x0, T[idx], &slope);
        l = lf[row + tx0 - 2 + sx];
      }
      Wm[idx] = w;
      Lm[idx] = l;
      Sl[idx] = slope;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < FN; idx += kPhThreads) {
      float ca = 0.f, cb = 0.f, cc = 0.f;
      if (VS[idx]) {
        const int fy = idx / FW, fx = idx - fy * FW;
        const SsimFactors<double> f = ssim_factors<double>(Lm + fy * SW + fx, Wm + fy * SW + fx, SW, a.c1, a.c2);
        const double dd = f.d1 * f.d2;
        const double ssim = (f.n1 * f.n2) / dd;
        ca = (float)(2.0 * f.mx * (f.n2 - f.n1) / dd - 2.0 * ssim * f.my * (1.0 / f.d1 - 1.0 / f.d2));
        cb = (float)(-2.0 * ssim / f.d2);
        cc = (float)(2.0 * f.n1 / dd);
      }
      CA[idx] = ca;
      CB[idx] = cb;
      CC[idx] = cc;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kPhRows; ++r) {
      const int oy = rg * kPhRows + r;
      const int qi = (oy + 2) * SW + ox + 2;
      if (X0[qi] < 0) continue;  // also every pixel outside the image
      float sa = 0.f, sb = 0.f, sc = 0.f;
#pragma unroll
      for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          const int fi = (oy + j) * FW + ox + i;
          sa += CA[fi];
          sb += CB[fi];
          sc += CC[fi];
        }
      const float w = Wm[qi], l = Lm[qi];
      const float g = sa + sb * w + sc * l;
      acc[r] += Sl[qi] * (kl * (float)((w > l) - (w < l)) + ks * g);
    }
    __syncthreads();
  }
  float* out = ddisp + b * gbs;
#pragma unroll
  for (int r = 0; r < kPhRows; ++r) {
    const int oy = rg * kPhRows + r;
    const int gy = ty0 + oy, gx = tx0 + ox;
    if (gy < a.H && gx < a.W) out[(long long)gy * a.W + gx] = acc[r];
  }
}

static long long photo_blocks(int B, int H, int W) {
  return (long long)B * ((H + kPhH - 1) / kPhH) * ((W + kPhW - 1) / kPhW);
}

struct PhotoSpans {  // bytes each input spans
  size_t left, right, disp, exclude;
};

// shared argument checks; 0 = fine
static int photo_check(const char* who, const float* left, int64_t lbs, const float* right, int64_t rbs,
                       const float* disp, int64_t dbs, const uint8_t* exclude, int64_t ebs, int B, int C, int H, int W,
                       float c1, float c2, PhotoSpans* sp) {
  LEA_CHECK_ARG(left, "%s: left is null", who);
  LEA_CHECK_ARG(right, "%s: right is null", who);
  LEA_CHECK_ARG(disp, "%s: disp is null", who);
  LEA_CHECK_ARG(B > 0, "%s: bad B=%d", who, B);
  LEA_CHECK_ARG(C >= 1 && C <= kPhMaxC, "%s: C=%d outside 1..%d", who, C, kPhMaxC);
  LEA_CHECK_ARG(H >= 3 && W >= 3, "%s: bad shape H=%d W=%d (H, W >= 3)", who, H, W);
  const long long hw = (long long)H * W, chw = (long long)C * hw;
  LEA_CHECK_ARG(lbs >= chw, "%s: left batch stride below C*H*W", who);
  LEA_CHECK_ARG(rbs >= chw, "%s: right batch stride below C*H*W", who);
  LEA_CHECK_ARG(dbs >= hw, "%s: disp batch stride below H*W", who);
  LEA_CHECK_ARG(!exclude || ebs >= hw, "%s: exclude batch stride below H*W", who);
  LEA_CHECK_ARG(c1 > 0.f && __builtin_isfinite(c1), "%s: c1 must be positive and finite", who);
  LEA_CHECK_ARG(c2 > 0.f && __builtin_isfinite(c2), "%s: c2 must be positive and finite", who);
  LEA_CHECK_ARG(B <= 65535 && (H + kPhH - 1) / kPhH <= 65535, "%s: grid too large", who);
  sp->left = 4 * ((size_t)(B - 1) * (size_t)lbs + (size_t)chw);
  sp->right = 4 * ((size_t)(B - 1) * (size_t)rbs + (size_t)chw);
  sp->disp = 4 * ((size_t)(B - 1) * (size_t)dbs + (size_t)hw);
  sp->exclude = exclude ? (size_t)(B - 1) * (size_t)ebs + (size_t)hw : 0;
  return LEA_OK;
}

// 0 = the output (named what) overlaps none of the inputs
static int photo_no_overlap(const char* who, const char* what, const void* out, size_t n, const float* left,
                            const float* right, const float* disp, const uint8_t* exclude, const PhotoSpans& sp) {
  LEA_CHECK_ARG(!spans_overlap(out, n, left, sp.left), "%s: %s overlaps left", who, what);
  LEA_CHECK_ARG(!spans_overlap(out, n, right, sp.right), "%s: %s overlaps right", who, what);
  LEA_CHECK_ARG(!spans_overlap(out, n, disp, sp.disp), "%s: %s overlaps disp", who, what);
  LEA_CHECK_ARG(!exclude || !spans_overlap(out, n, exclude, sp.exclude), "%s: %s overlaps exclude", who, what);
  return LEA_OK;
}

}  // namespace lea

extern "C" size_t lea_photometric_workspace_bytes(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  return (size_t)lea::photo_blocks(B, H, W) * 4 * sizeof(double);
}

extern "C" int lea_photometric_f32(const float* left, int64_t left_bstride, const float* right, int64_t right_bstride,
                                   const float* disp, int64_t disp_bstride, const uint8_t* exclude,
                                   int64_t exclude_bstride, int B, int C, int H, int W, float alpha, float c1, float c2,
                                   double* sums, void* workspace, float* warped, float* err, void* stream) {
  using namespace lea;
  clear_error();
  const char* who = "lea_photometric_f32";
  PhotoSpans sp;
  if (int rc = photo_check(who, left, left_bstride, right, right_bstride, disp, disp_bstride, exclude, exclude_bstride,
                           B, C, H, W, c1, c2, &sp))
    return rc;
  LEA_CHECK_ARG(alpha >= 0.f && alpha <= 1.f, "%s: alpha outside [0, 1]", who);
  LEA_CHECK_ARG(sums, "%s: sums is null", who);
  LEA_CHECK_ARG(workspace, "%s: workspace is null", who);
  LEA_CHECK_ARG(((uintptr_t)sums & 7) == 0, "%s: sums must be 8-byte aligned", who);
  LEA_CHECK_ARG(((uintptr_t)workspace & 7) == 0, "%s: workspace must be 8-byte aligned", who);
  const long long nblk = photo_blocks(B, H, W);
  const size_t wsn = (size_t)nblk * 4 * sizeof(double), hwn = 4 * (size_t)B * (size_t)H * (size_t)W;
  // every output against every input and against the outputs before it
  const void* outs[4] = {sums, workspace, warped, err};
  const size_t outn[4] = {4 * sizeof(double), wsn, hwn * (size_t)C, hwn};
  const char* names[4] = {"sums", "the workspace", "warped", "err"};
  for (int i = 0; i < 4; ++i) {
    if (!outs[i]) continue;
    if (int rc = photo_no_overlap(who, names[i], outs[i], outn[i], left, right, disp, exclude, sp)) return rc;
    for (int j = 0; j < i; ++j)
      LEA_CHECK_ARG(!outs[j] || !spans_overlap(outs[i], outn[i], outs[j], outn[j]), "%s: %s overlaps %s", who, names[i],
                    names[j]);
  }
  const PhotoMaps a{left, right, disp, exclude, left_bstride, right_bstride, disp_bstride, exclude_bstride,
                    C, H, W, c1, c2};
  const dim3 grid((unsigned)((W + kPhW - 1) / kPhW), (unsigned)((H + kPhH - 1) / kPhH), (unsigned)B);
  double* partial = static_cast<double*>(workspace);
  photometric_kernel<<<grid, kPhThreads, 0, as_stream(stream)>>>(a, alpha, partial, warped, err);
  if (int rc = launch_status(who)) return rc;
  reduce4_final_kernel<kPhThreads><<<1, kPhThreads, 0, as_stream(stream)>>>(partial, nblk, sums);
  return launch_status("lea_photometric_f32 (final)");
}

extern "C" int lea_photometric_grad_f32(const float* left, int64_t left_bstride, const float* right,
                                        int64_t right_bstride, const float* disp, int64_t disp_bstride,
                                        const uint8_t* exclude, int64_t exclude_bstride, int B, int C, int H, int W,
                                        float c1, float c2, const double* sums, const float* scales, float* ddisp,
                                        int64_t ddisp_bstride, void* stream) {
  using namespace lea;
  clear_error();
  const char* who = "lea_photometric_grad_f32";
  PhotoSpans sp;
  if (int rc = photo_check(who, left, left_bstride, right, right_bstride, disp, disp_bstride, exclude, exclude_bstride,
                           B, C, H, W, c1, c2, &sp))
    return rc;
  LEA_CHECK_ARG(sums, "%s: sums is null", who);
  LEA_CHECK_ARG(scales, "%s: scales is null", who);
  LEA_CHECK_ARG(ddisp, "%s: ddisp is null", who);
  LEA_CHECK_ARG(((uintptr_t)sums & 7) == 0, "%s: sums must be 8-byte aligned", who);
  const long long hw = (long long)H * W;
  LEA_CHECK_ARG(ddisp_bstride >= hw, "%s: ddisp batch stride below H*W", who);
  const size_t dn = 4 * ((size_t)(B - 1) * (size_t)ddisp_bstride + (size_t)hw);
  if (int rc = photo_no_overlap(who, "ddisp", ddisp, dn, left, right, disp, exclude, sp)) return rc;
  LEA_CHECK_ARG(!spans_overlap(ddisp, dn, sums, 4 * sizeof(double)), "%s: ddisp overlaps sums", who);
  LEA_CHECK_ARG(!spans_overlap(ddisp, dn, scales, 2 * sizeof(float)), "%s: ddisp overlaps scales", who);
  const PhotoMaps a{left, right, disp, exclude, left_bstride, right_bstride, disp_bstride, exclude_bstride,
                    C, H, W, c1, c2};
  const dim3 grid((unsigned)((W + kPhW - 1) / kPhW), (unsigned)((H + kPhH - 1) / kPhH), (unsigned)B);
  photometric_grad_kernel<<<grid, kPhThreads, 0, as_stream(stream)>>>(a, sums, scales, ddisp, ddisp_bstride);
  return launch_status(who);
}
