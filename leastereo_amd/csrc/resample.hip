// Trilinear resample of an NCDHW volume with PyTorch's source-index rule, with an
// optional per-channel affine + ReLU epilogue.
// Replaces F.interpolate(..., mode='trilinear', align_corners=True) at
// retrain/skip_model_3d.py:48,50 and nn.Upsample at :162-164 (the level changes
// between the 1x, 1/2x and 1/4x matching-net resolutions).
//
// The epilogue serves the up-sampling cell preprocess: ConvBR1x1(interp(x)) =
// relu(scale * interp(W x) + shift) because the 1x1 conv W and the trilinear
// interpolation are both linear maps on different axes and commute.  The 1x1
// conv then runs at the *input* resolution (8x fewer voxels for x2 up-sampling)
// and only its narrow output is resampled -- straight into the cell's cat slot.
//
// Mapping: grid.y = output plane (b, c, od) -- its depth weights are uniform;
// threads walk the plane's (oh, 4-wide ow quad) cells with a grid stride, so a
// workgroup writes several KB (the first version launched one 256-thread group
// per half row and was dispatch-bound at ~0.55 TB/s).  Output is stored as one
// 16-byte vector per quad when Wo % 4 == 0.  Bound by the output write.
#include "common.h"

namespace lea {

template <bool VEC>
__global__ __launch_bounds__(256) void resample3d_f32(const float* __restrict__ x, long long xbs,
                                                      float* __restrict__ y, long long ybs, int C,
                                                      int Di, int Hi, int Wi, int Do, int Ho, int Wo,
                                                      float rd, float rh, float rw, int ac,
                                                      const float* __restrict__ scale,
                                                      const float* __restrict__ shift,
                                                      unsigned flags) {
#pragma clang fp contract(off)
  const int plane = blockIdx.y;  // (b * C + c) * Do + od
  const int od = plane % Do;
  const int bc = plane / Do;
  const int b = bc / C, c = bc - b * C;
  const Axis ad = axis_index(rd, od, Di, Do, ac);
  const long long HWi = (long long)Hi * Wi;
  const float* xc = x + (long long)b * xbs + (long long)c * Di * HWi;
  const float* q0 = xc + ad.i0 * HWi;
  const float* q1 = xc + ad.i1 * HWi;
  float* yp = y + (long long)b * ybs + ((long long)c * Do + od) * Ho * Wo;
  const float sc = scale ? scale[c] : 1.f;
  const float sh = scale ? shift[c] : 0.f;
  const bool relu = flags & LEA_RELU;
  const int wq = VEC ? Wo / 4 : Wo;
  const int cells = Ho * wq;
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < cells; t += gridDim.x * blockDim.x) {
    const int oh = t / wq;
    const int q = t - oh * wq;
    const Axis ah = axis_index(rh, oh, Hi, Ho, ac);
    const float* p00 = q0 + (long long)ah.i0 * Wi;
    const float* p01 = q0 + (long long)ah.i1 * Wi;
    const float* p10 = q1 + (long long)ah.i0 * Wi;
    const float* p11 = q1 + (long long)ah.i1 * Wi;
    float v[VEC ? 4 : 1];
#pragma unroll
    for (int e = 0; e < (VEC ? 4 : 1); ++e) {
      const Axis aw = axis_index(rw, (VEC ? 4 * q : q) + e, Wi, Wo, ac);
      float r = trilerp(ad, ah, aw, p00, p01, p10, p11);
      if (scale) r = r * sc + sh;
      if (relu) r = fmaxf(r, 0.f);
      v[e] = r;
    }
    if constexpr (VEC)
      *reinterpret_cast<float4*>(yp + (long long)oh * Wo + 4 * q) = make_float4(v[0], v[1], v[2], v[3]);
    else
      yp[(long long)oh * Wo + q] = v[0];
  }
}

// Row-staged variant (the up-sampling level changes, 8-16 channels at x2):
// a workgroup owns R output rows of one output plane; the <= R*rh + 2 source
// rows of its two source planes are first copied into LDS with coalesced loads,
// then every output quad interpolates from LDS.  The gather version above issued
// 32 dependent global loads per quad and ran at ~1.2 TB/s; here each source
// element is read from HBM/L2 once per workgroup.  Same Axis/trilerp arithmetic,
// so both kernels produce identical bits.
template <bool VEC>
__global__ __launch_bounds__(256) void resample3d_rows_f32(
    const float* __restrict__ x, long long xbs, float* __restrict__ y, long long ybs, int C, int Di,
    int Hi, int Wi, int Do, int Ho, int Wo, float rd, float rh, float rw, int ac, int R, int nrmax,
    const float* __restrict__ scale, const float* __restrict__ shift, unsigned flags) {
#pragma clang fp contract(off)
  extern __shared__ float rows[];  // [2][nrmax][Wi]
  const int plane = blockIdx.y;
  const int od = plane % Do;
  const int bc = plane / Do;
  const int b = bc / C, c = bc - b * C;
  const int oh0 = blockIdx.x * R;
  const int oh1 = min(oh0 + R, Ho);
  const Axis ad = axis_index(rd, od, Di, Do, ac);
  const int r_lo = axis_index(rh, oh0, Hi, Ho, ac).i0;
  const int r_hi = axis_index(rh, oh1 - 1, Hi, Ho, ac).i1;
  // nrmax = the host's exact bound (staged_rows); past it: NaN outputs, never unstaged rows
  const bool over = r_hi - r_lo + 1 > nrmax;
  const int nr = over ? 0 : r_hi - r_lo + 1;
  const long long HWi = (long long)Hi * Wi;
  const float* xc = x + (long long)b * xbs + (long long)c * Di * HWi + (long long)r_lo * Wi;
  const float* src[2] = {xc + ad.i0 * HWi, xc + ad.i1 * HWi};
  const int n1 = nr * Wi;
  for (int e = threadIdx.x; e < 2 * n1; e += blockDim.x) {
    const int p = e >= n1;
    const int r = e - p * n1;
    rows[p * nrmax * Wi + r] = src[p][r];
  }
  __syncthreads();
  float* yp = y + (long long)b * ybs + ((long long)c * Do + od) * Ho * Wo;
  const float sc = scale ? scale[c] : 1.f;
  const float sh = scale ? shift[c] : 0.f;
  const bool relu = flags & LEA_RELU;
  const int wq = VEC ? Wo / 4 : Wo;
  const int cells = (oh1 - oh0) * wq;
  const float* l0 = rows;
  const float* l1 = rows + nrmax * Wi;
  for (int t = threadIdx.x; t < cells; t += blockDim.x) {
    const int oh = oh0 + t / wq;
    const int q = t % wq;
    const Axis ah = axis_index(rh, oh, Hi, Ho, ac);
    const int r0 = over ? 0 : (ah.i0 - r_lo) * Wi, r1 = over ? 0 : (ah.i1 - r_lo) * Wi;
    float v[VEC ? 4 : 1];
#pragma unroll
    for (int e = 0; e < (VEC ? 4 : 1); ++e) {
      const Axis aw = axis_index(rw, (VEC ? 4 * q : q) + e, Wi, Wo, ac);
      float r = trilerp(ad, ah, aw, l0 + r0, l0 + r1, l1 + r0, l1 + r1);
      if (scale) r = r * sc + sh;
      if (relu) r = fmaxf(r, 0.f);
      v[e] = over ? __builtin_nanf("") : r;
    }
    if constexpr (VEC)
      *reinterpret_cast<float4*>(yp + (long long)oh * Wo + 4 * q) = make_float4(v[0], v[1], v[2], v[3]);
    else
      yp[(long long)oh * Wo + q] = v[0];
  }
}

// Separable variant (r04; the default when Wo % 4 == 0): trilerp's innermost terms are the
// W-lerps of the four source rows, aw.l0 * row[aw.i0] + aw.l1 * row[aw.i1], so a workgroup
// first forms the W-lerped rows of its <= nrmax source rows of both source planes at every
// output column (each thread owns columns: one W axis per column, loads straight from
// global), then every output quad combines four float4s of them with the H and D weights
// in trilerp's own expression tree -- bit-identical to the row-staged and gather kernels.
// Per output value: ~1.25 W-lerps (the rows two output rows share are lerped once) and one
// 16-byte LDS read per source-row pair, instead of 4 W-lerps and 8 LDS reads.
__global__ __launch_bounds__(256) void resample3d_sep_f32(
    const float* __restrict__ x, long long xbs, float* __restrict__ y, long long ybs, int C, int Di,
    int Hi, int Wi, int Do, int Ho, int Wo, float rd, float rh, float rw, int ac, int R, int nrmax,
    const float* __restrict__ scale, const float* __restrict__ shift, unsigned flags) {
#pragma clang fp contract(off)
  extern __shared__ float wrows[];  // [2][nrmax][Wo]: W-lerped source rows
  const int plane = blockIdx.y;
  const int od = plane % Do;
  const int bc = plane / Do;
  const int b = bc / C, c = bc - b * C;
  const int oh0 = blockIdx.x * R;
  const int oh1 = min(oh0 + R, Ho);
  const Axis ad = axis_index(rd, od, Di, Do, ac);
  const int r_lo = axis_index(rh, oh0, Hi, Ho, ac).i0;
  const int r_hi = axis_index(rh, oh1 - 1, Hi, Ho, ac).i1;
  // nrmax = the host's exact bound (staged_rows); past it: NaN outputs, never unstaged rows
  const bool over = r_hi - r_lo + 1 > nrmax;
  const int nr = over ? 0 : r_hi - r_lo + 1;
  const long long HWi = (long long)Hi * Wi;
  const float* xc = x + (long long)b * xbs + (long long)c * Di * HWi + (long long)r_lo * Wi;
  const float* src0 = xc + ad.i0 * HWi;
  const float* src1 = xc + ad.i1 * HWi;
  for (int xo = threadIdx.x; xo < Wo; xo += blockDim.x) {
    const Axis aw = axis_index(rw, xo, Wi, Wo, ac);
    for (int r = 0; r < nr; ++r) {
      const float* q0 = src0 + (long long)r * Wi;
      const float* q1 = src1 + (long long)r * Wi;
      wrows[r * Wo + xo] = aw.l0 * q0[aw.i0] + aw.l1 * q0[aw.i1];
      wrows[(nrmax + r) * Wo + xo] = aw.l0 * q1[aw.i0] + aw.l1 * q1[aw.i1];
    }
  }
  __syncthreads();
  float* yp = y + (long long)b * ybs + ((long long)c * Do + od) * Ho * Wo;
  const float sc = scale ? scale[c] : 1.f;
  const float sh = scale ? shift[c] : 0.f;
  const bool relu = flags & LEA_RELU;
  const int wq = Wo / 4;
  const int cells = (oh1 - oh0) * wq;
  const float4* w4 = reinterpret_cast<const float4*>(wrows);
  for (int t = threadIdx.x; t < cells; t += blockDim.x) {
    const int oh = oh0 + t / wq;
    const int q = t % wq;
    const Axis ah = axis_index(rh, oh, Hi, Ho, ac);
    const int r0 = over ? 0 : ah.i0 - r_lo, r1 = over ? 0 : ah.i1 - r_lo;
    const float4 a00 = w4[r0 * wq + q], a01 = w4[r1 * wq + q];
    const float4 a10 = w4[(nrmax + r0) * wq + q], a11 = w4[(nrmax + r1) * wq + q];
    const float p00[4] = {a00.x, a00.y, a00.z, a00.w}, p01[4] = {a01.x, a01.y, a01.z, a01.w};
    const float p10[4] = {a10.x, a10.y, a10.z, a10.w}, p11[4] = {a11.x, a11.y, a11.z, a11.w};
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float r = ad.l0 * (ah.l0 * p00[e] + ah.l1 * p01[e]) + ad.l1 * (ah.l0 * p10[e] + ah.l1 * p11[e]);
      if (scale) r = r * sc + sh;
      if (relu) r = fmaxf(r, 0.f);
      v[e] = over ? __builtin_nanf("") : r;
    }
    *reinterpret_cast<float4*>(yp + (long long)oh * Wo + 4 * q) = make_float4(v[0], v[1], v[2], v[3]);
  }
}

// The separable kernel with a down-sampled side output (lea_resample3d_trilinear_down2): besides
// y it writes y2 = the trilinear (align_corners) resample of y to exactly half (an aligned
// 2 x 2 x 2 block of y per y2 voxel), bit-identical to resampling y again, without reading y back.
// A workgroup owns R (even) output rows of an output plane PAIR: the W-lerped source rows of the
// pair's <= 3 source planes (an up-sampling along D: the first source plane of output plane
// o + 1 is at most one past that of o); a thread owns a 2 x 2 x 4 block of y -- four float4 stores
// by resample3d_sep_f32's own expression, then trilerp's tree on the block (W pairs in-lane, H,
// D) and one float2 of y2.
__global__ __launch_bounds__(256) void resample3d_sep_down2_f32(
    const float* __restrict__ x, long long xbs, float* __restrict__ y, long long ybs, float* __restrict__ y2,
    long long y2bs, int C, int Di, int Hi, int Wi, int Do, int Ho, int Wo, float rd, float rh, float rw,
    float rd2, float rh2, float rw2, int R, int nrmax, const float* __restrict__ scale,
    const float* __restrict__ shift, unsigned flags) {
#pragma clang fp contract(off)
  extern __shared__ float wrows[];  // [3][nrmax][Wo]: W-lerped source rows
  const int D2 = Do / 2, H2 = Ho / 2, W2 = Wo / 2;
  const int pp = blockIdx.y % D2;  // output planes 2 pp, 2 pp + 1
  const int bc = blockIdx.y / D2;
  const int b = bc / C, c = bc - b * C;
  const int oh0 = blockIdx.x * R;
  const int oh1 = min(oh0 + R, Ho);
  const Axis ad[2] = {axis_index(rd, 2 * pp, Di, Do, 1), axis_index(rd, 2 * pp + 1, Di, Do, 1)};
  const int db = ad[0].i0;
  const int r_lo = axis_index(rh, oh0, Hi, Ho, 1).i0;
  const int r_hi = axis_index(rh, oh1 - 1, Hi, Ho, 1).i1;
  // nrmax = the host's exact bound (staged_rows); past it, or past the three-plane window: NaN
  // outputs, never unstaged rows
  const bool over = r_hi - r_lo + 1 > nrmax || ad[1].i1 - db > 2;
  const int nr = over ? 0 : r_hi - r_lo + 1;
  const long long HWi = (long long)Hi * Wi;
  const float* xc = x + (long long)b * xbs + (long long)c * Di * HWi + (long long)r_lo * Wi;
  for (int xo = threadIdx.x; xo < Wo; xo += blockDim.x) {
    const Axis aw = axis_index(rw, xo, Wi, Wo, 1);
#pragma unroll
    for (int p = 0; p < 3; ++p) {
      const float* src = xc + min(db + p, Di - 1) * HWi;
      for (int r = 0; r < nr; ++r) {
        const float* q = src + (long long)r * Wi;
        wrows[(p * nrmax + r) * Wo + xo] = aw.l0 * q[aw.i0] + aw.l1 * q[aw.i1];
      }
    }
  }
  __syncthreads();
  const float sc = scale ? scale[c] : 1.f;
  const float sh = scale ? shift[c] : 0.f;
  const bool relu = flags & LEA_RELU;
  const int wq = Wo / 4;
  const int cells = ((oh1 - oh0) / 2) * wq;
  const float4* w4 = reinterpret_cast<const float4*>(wrows);
  const Axis ad2 = axis_index(rd2, pp, Do, D2, 1);
  float* yc = y + (long long)b * ybs + (long long)c * Do * Ho * Wo;
  float* y2c = y2 + (long long)b * y2bs + ((long long)c * D2 + pp) * H2 * W2;
  for (int t = threadIdx.x; t < cells; t += blockDim.x) {
    const int j = t / wq, q = t % wq;
    const int oh = oh0 + 2 * j;
    float v[2][2][4];  // [plane][row][column]
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
      const Axis ah = axis_index(rh, oh + rr, Hi, Ho, 1);
      const int r0 = over ? 0 : ah.i0 - r_lo, r1 = over ? 0 : ah.i1 - r_lo;
#pragma unroll
      for (int pl = 0; pl < 2; ++pl) {
        const int k0 = over ? 0 : ad[pl].i0 - db, k1 = over ? 0 : ad[pl].i1 - db;
        const float4 a00 = w4[(k0 * nrmax + r0) * wq + q], a01 = w4[(k0 * nrmax + r1) * wq + q];
        const float4 a10 = w4[(k1 * nrmax + r0) * wq + q], a11 = w4[(k1 * nrmax + r1) * wq + q];
        const float p00[4] = {a00.x, a00.y, a00.z, a00.w}, p01[4] = {a01.x, a01.y, a01.z, a01.w};
        const float p10[4] = {a10.x, a10.y, a10.z, a10.w}, p11[4] = {a11.x, a11.y, a11.z, a11.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float r = ad[pl].l0 * (ah.l0 * p00[e] + ah.l1 * p01[e]) + ad[pl].l1 * (ah.l0 * p10[e] + ah.l1 * p11[e]);
          if (scale) r = r * sc + sh;
          if (relu) r = fmaxf(r, 0.f);
          v[pl][rr][e] = over ? __builtin_nanf("") : r;
        }
        *reinterpret_cast<float4*>(yc + ((long long)(2 * pp + pl) * Ho + oh + rr) * Wo + 4 * q) =
            make_float4(v[pl][rr][0], v[pl][rr][1], v[pl][rr][2], v[pl][rr][3]);
      }
    }
    // the block's resample to one y2 row pair of columns: trilerp's tree with the half-size axes
    const Axis ah2 = axis_index(rh2, oh / 2, Ho, H2, 1);
    float o2[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const Axis aw2 = axis_index(rw2, 2 * q + k, Wo, W2, 1);
      float hl[2];
#pragma unroll
      for (int pl = 0; pl < 2; ++pl) {
        float wl[2];
#pragma unroll
        for (int rr = 0; rr < 2; ++rr)
          wl[rr] = aw2.l0 * ((aw2.i0 & 1) ? v[pl][rr][2 * k + 1] : v[pl][rr][2 * k]) +
                   aw2.l1 * ((aw2.i1 & 1) ? v[pl][rr][2 * k + 1] : v[pl][rr][2 * k]);
        hl[pl] = ah2.l0 * ((ah2.i0 & 1) ? wl[1] : wl[0]) + ah2.l1 * ((ah2.i1 & 1) ? wl[1] : wl[0]);
      }
      o2[k] = ad2.l0 * ((ad2.i0 & 1) ? hl[1] : hl[0]) + ad2.l1 * ((ad2.i1 & 1) ? hl[1] : hl[0]);
    }
    *reinterpret_cast<float2*>(y2c + (long long)(oh / 2) * W2 + 2 * q) = make_float2(o2[0], o2[1]);
  }
}

// 0 auto, 1 row-staged, 2 gather
LEA_TUNING_INT(lea_resample_set_mode, g_resample_mode, 0, 0, 2, "mode=%d")

}  // namespace lea

extern "C" int lea_staged_rows(int Hi, int Ho, int ac, int R, int halo) {
  lea::clear_error();
  // a row count can be any positive int (~1008 rows at config 5), so an error is -1, never
  // LEA_E_INVALID
  if (!(Hi > 0 && Ho > 0 && R > 0 && halo >= 0 && (ac == 0 || ac == 1))) {
    lea::set_error("lea_staged_rows: Hi=%d Ho=%d ac=%d R=%d halo=%d", Hi, Ho, ac, R, halo);
    return -1;
  }
  return lea::staged_rows(Hi, Ho, ac, R, halo);
}

extern "C" int lea_resample3d_trilinear(const void* x, int64_t x_bstride, void* y, int64_t y_bstride,
                                        int B, int C, int Di, int Hi, int Wi, int Do, int Ho, int Wo,
                                        int align_corners, const float* scale, const float* shift,
                                        unsigned flags, int dtype, void* stream) {
  using namespace lea;
  clear_error();
  LEA_CHECK_FLAGS(flags, LEA_RELU, "lea_resample3d_trilinear");
  LEA_CHECK_ARG(x && y && x != y, "lea_resample3d_trilinear: null or aliased pointer");
  LEA_CHECK_ARG((scale == nullptr) == (shift == nullptr),
                "lea_resample3d_trilinear: scale/shift must both be set or both NULL");
  LEA_CHECK_ARG(B > 0 && C > 0 && Di > 0 && Hi > 0 && Wi > 0 && Do > 0 && Ho > 0 && Wo > 0,
                "lea_resample3d_trilinear: bad shape");
  LEA_CHECK_ARG((long long)B * C * Do <= 65535 && (long long)Ho * Wo < (1LL << 31),
                "lea_resample3d_trilinear: grid too large (B*C*Do=%lld)", (long long)B * C * Do);
  if (dtype != LEA_F32) {
    set_error("lea_resample3d_trilinear: dtype %d unsupported", dtype);
    return LEA_E_UNSUPPORTED;
  }
  // 16-byte stores need Wo % 4 == 0 and a 16-byte aligned output (y and its batch stride)
  const bool vec = (Wo % 4) == 0 && ((uintptr_t)y % 16) == 0 && (y_bstride % 4) == 0;
  const int ac = align_corners ? 1 : 0;
  const long long cells = (long long)Ho * (vec ? Wo / 4 : Wo);
  const int threads = 256;
  // ~8 cells per thread: a workgroup covers 2048 cells (8 KB written with quads)
  const int gx = (int)((cells + threads * 8 - 1) / (threads * 8));
  dim3 grid(gx, B * C * Do);
  const float rd = axis_ratio(Di, Do, ac), rh = axis_ratio(Hi, Ho, ac), rw = axis_ratio(Wi, Wo, ac);
  // Separable kernel (16-byte outputs) when R output rows' W-lerped source rows fit 64 KB
  if (vec && g_resample_mode == 0) {
    for (int R = 16; R >= 2; R /= 2) {
      const int nrmax = staged_rows(Hi, Ho, ac, R, 0);  // exact (common.h)
      const size_t lds = (size_t)2 * nrmax * Wo * sizeof(float);
      if (lds > 65536) continue;
      dim3 g((Ho + R - 1) / R, B * C * Do);
      resample3d_sep_f32<<<g, threads, lds, as_stream(stream)>>>(
          (const float*)x, x_bstride, (float*)y, y_bstride, C, Di, Hi, Wi, Do, Ho, Wo, rd, rh, rw, ac, R, nrmax,
          scale, shift, flags);
      return launch_status("lea_resample3d_trilinear");
    }
  }
  // Row-staged kernel when R output rows' sources fit 64 KB of LDS: R = 16 rows
  // (20 KB of output per workgroup at Wo = 320), fewer for wide rows.
  for (int R = 16; R >= 2 && g_resample_mode != 2; R /= 2) {
    const int nrmax = staged_rows(Hi, Ho, ac, R, 0);  // exact (common.h)
    const size_t lds = (size_t)2 * nrmax * Wi * sizeof(float);
    if (lds > 65536) continue;
    dim3 g((Ho + R - 1) / R, B * C * Do);
    if (vec)
      resample3d_rows_f32<true><<<g, threads, lds, as_stream(stream)>>>(
          (const float*)x, x_bstride, (float*)y, y_bstride, C, Di, Hi, Wi, Do, Ho, Wo, rd, rh, rw, ac,
          R, nrmax, scale, shift, flags);
    else
      resample3d_rows_f32<false><<<g, threads, lds, as_stream(stream)>>>(
          (const float*)x, x_bstride, (float*)y, y_bstride, C, Di, Hi, Wi, Do, Ho, Wo, rd, rh, rw, ac,
          R, nrmax, scale, shift, flags);
    return launch_status("lea_resample3d_trilinear");
  }
  if (vec)
    resample3d_f32<true><<<grid, threads, 0, as_stream(stream)>>>(
        (const float*)x, x_bstride, (float*)y, y_bstride, C, Di, Hi, Wi, Do, Ho, Wo, rd, rh, rw, ac,
        scale, shift, flags);
  else
    resample3d_f32<false><<<grid, threads, 0, as_stream(stream)>>>(
        (const float*)x, x_bstride, (float*)y, y_bstride, C, Di, Hi, Wi, Do, Ho, Wo, rd, rh, rw, ac,
        scale, shift, flags);
  return launch_status("lea_resample3d_trilinear");
}

// the largest even R whose W-lerped rows of three source planes fit 64 KB, or 0
static int sep_down2_rows(int Hi, int Ho, int Wo, int* nrmax) {
  for (int R = 8; R >= 2; R /= 2) {
    const int n = lea::staged_rows(Hi, Ho, 1, R, 0);  // exact (common.h)
    if ((size_t)3 * n * Wo * sizeof(float) > 65536) continue;
    if (nrmax) *nrmax = n;
    return R;
  }
  return 0;
}

// the shapes lea_resample3d_trilinear_down2 takes: an output volume with even D and H and
// W % 4 == 0, no down-sampling along D (the three-plane window), rows that fit the LDS
extern "C" int lea_resample3d_down2_supported(int Di, int Hi, int Wi, int Do, int Ho, int Wo, int dtype) {
  if (dtype != LEA_F32 || Di <= 0 || Hi <= 0 || Wi <= 0 || Do < 2 || Ho < 2 || Wo < 4) return 0;
  if (Do < Di || Do % 2 || Ho % 2 || Wo % 4 || Do > 2048) return 0;
  return sep_down2_rows(Hi, Ho, Wo, nullptr) ? 1 : 0;
}

extern "C" int lea_resample3d_trilinear_down2(const void* x, int64_t x_bstride, void* y, int64_t y_bstride,
                                              void* y2, int64_t y2_bstride, int B, int C, int Di, int Hi, int Wi,
                                              int Do, int Ho, int Wo, const float* scale, const float* shift,
                                              unsigned flags, int dtype, void* stream) {
  using namespace lea;
  const char* what = "lea_resample3d_trilinear_down2";
  clear_error();
  LEA_CHECK_FLAGS(flags, LEA_RELU, what);
  LEA_CHECK_ARG(x && y && y2 && x != y && x != y2 && y != y2, "%s: null or aliased pointer", what);
  LEA_CHECK_ARG((scale == nullptr) == (shift == nullptr), "%s: scale/shift must both be set or both NULL", what);
  LEA_CHECK_ARG(B > 0 && C > 0 && Di > 0 && Hi > 0 && Wi > 0 && Do > 0 && Ho > 0 && Wo > 0, "%s: bad shape", what);
  if (!lea_resample3d_down2_supported(Di, Hi, Wi, Do, Ho, Wo, dtype)) {
    set_error("%s: needs LEA_F32, an output volume with even D and H and W %% 4 == 0, no down-sampling along D "
              "and rows that fit the LDS (%d x %d x %d -> %d x %d x %d, dtype %d)", what, Di, Hi, Wi, Do, Ho, Wo,
              dtype);
    return LEA_E_UNSUPPORTED;
  }
  LEA_CHECK_ARG((long long)B * C * (Do / 2) <= 65535 && (long long)Ho * Wo < (1LL << 31),
                "%s: grid too large (B*C*Do/2=%lld)", what, (long long)B * C * (Do / 2));
  LEA_CHECK_ARG((uintptr_t)y % 16 == 0 && y_bstride % 4 == 0 && (uintptr_t)y2 % 8 == 0 && y2_bstride % 2 == 0,
                "%s: y needs 16-byte, y2 8-byte alignment", what);
  int nrmax = 0;
  const int R = sep_down2_rows(Hi, Ho, Wo, &nrmax);
  const size_t lds = (size_t)3 * nrmax * Wo * sizeof(float);
  dim3 g((Ho + R - 1) / R, B * C * (Do / 2));
  resample3d_sep_down2_f32<<<g, 256, lds, as_stream(stream)>>>(
      (const float*)x, x_bstride, (float*)y, y_bstride, (float*)y2, y2_bstride, C, Di, Hi, Wi, Do, Ho, Wo,
      axis_ratio(Di, Do, 1), axis_ratio(Hi, Ho, 1), axis_ratio(Wi, Wo, 1), axis_ratio(Do, Do / 2, 1),
      axis_ratio(Ho, Ho / 2, 1), axis_ratio(Wo, Wo / 2, 1), R, nrmax, scale, shift, flags);
  return launch_status(what);
}
