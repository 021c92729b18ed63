// Device helpers shared by the disparity head's units (disparity.hip: the plain head,
// disparity_stats.hip: the head with per-pixel confidence): the up-sampling axis, the
// block shapes and the two exponentials.  Both units form U and exp(m - U) from these, so
// the disparity they write is the same number.
#pragma once
#include "common.h"

namespace lea {

struct AxisW {
  int i0, i1;
  float l0, l1;
};

// aten area_pixel_compute_source_index, align_corners=False, clamped at 0.
__device__ __forceinline__ AxisW src_axis(float ratio, int o, int in, int out) {
#pragma clang fp contract(off)
  AxisW a;
  if (in == out) {
    a.i0 = a.i1 = o;
    a.l0 = 1.f;
    a.l1 = 0.f;
    return a;
  }
  float real = ratio * ((float)o + 0.5f) - 0.5f;
  if (real < 0.f) real = 0.f;
  int i = (int)floorf(real);
  if (i > in - 1) i = in - 1;
  float lam = fminf(fmaxf(real - (float)i, 0.f), 1.f);
  a.i0 = i;
  a.i1 = i + ((i < in - 1) ? 1 : 0);
  a.l1 = lam;
  a.l0 = 1.f - lam;
  return a;
}

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

}  // namespace lea
