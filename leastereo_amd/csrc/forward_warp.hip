// View synthesis: an image pushed forward through its disparity map into another view, as a 1-D
// mesh render per scanline, with occlusion by depth and the scanline fill of what nothing covers.
//
// Per item b and row y, s = scales[b], every operation one rounded f32 operation:
//   t_x = x - (s * d_x);  ok(x): d_x finite, not excluded, t_x finite
//   point x   (ok(x)):  covers u = rintf(t_x) if 0 <= u <= W - 1;  a = 0, z = d_x
//   segment x (ok(x), ok(x + 1), |d_{x+1} - d_x| <= max_diff, 0 < den = t_{x+1} - t_x <= max_stretch):
//             covers every integer t_x <= u <= t_{x+1} in the row;
//             a = (u - t_x) / den,  z = ((1 - a) * d_x) + (a * d_{x+1})
//   winner at u: the largest z (-0 = +0), then the larger column, then the segment over the point
// The full contract is in include/leastereo_hip.h.
//
// Layout.  A row lives in LDS as d (NaN where excluded) and one 64-bit winner key per target:
// 12 bytes a pixel, 48 KB at the width limit.  t is never stored: x - (s * d_x) is two exact
// operations and every phase forms it again.  Four phases, a barrier between them:
//   load     d and exclude, coalesced; keys cleared
//   scatter  a lane owns a source column and offers its point and its segment's targets with one
//            LDS integer max each on (orderable z bits << 32 | column << 1 | kind); a max does not
//            depend on the order of the offers, so the winner is the same bits call after call
//   resolve  a lane owns a target, decodes its winner, forms a and z again from d, gathers the two
//            source values per channel from global memory and stores, coalesced
//   fill     (fill = 1) a lane owns a run of consecutive targets, the nearest hit on either side
//            comes from a wave scan of the runs' last / first hits (lr_check.hip's carry scan),
//            and each hole forms the chosen hit's values again from that hit's key: no output is
//            read back
// Rows of at most 256 pixels take a wave each, four to a workgroup; wider rows a workgroup of
// four waves.  Every trip count depends on W alone, so all barriers are uniform; a wave whose row
// does not exist runs along with every access predicated off.  Plain vector loads and stores.
#include "common.h"

namespace lea {

constexpr int kWarpThreads = 256;
constexpr int kWarpWaves = kWarpThreads / kWave;
constexpr int kWarpWaveRowW = 256;  // up to here a wave takes a row

// one IEEE operation each (tile_blend.hip: the __f*_rn intrinsics are inlined from a header
// compiled with contraction allowed)
__device__ __forceinline__ float w_mul(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float w_add(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}
__device__ __forceinline__ float w_sub(float a, float b) {
#pragma clang fp contract(off)
  return a - b;
}
__device__ __forceinline__ float w_div(float a, float b) {
#pragma clang fp contract(off)
  return a / b;  // correctly rounded: the build does not relax float division
}
__device__ __forceinline__ float w_lerp(float a, float v0, float v1) {
  return w_add(w_mul(w_sub(1.f, a), v0), w_mul(a, v1));
}

__device__ __forceinline__ float warp_target(int x, float s, float d) { return w_sub((float)x, w_mul(s, d)); }

// z as an unsigned integer of the same order, -0 with +0; never 0 for a number
__device__ __forceinline__ unsigned warp_order(float z) {
  unsigned b = __float_as_uint(z);
  if (z == 0.f) b = 0u;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ unsigned long long warp_key(float z, int x, int kind) {
  return ((unsigned long long)warp_order(z) << 32) | (unsigned)((x << 1) | kind);
}

struct WarpHit {
  int x, kind;
  float a, z;
};

// the winner behind a key (key != 0): a and z by the same operations that offered it
__device__ __forceinline__ WarpHit warp_decode(unsigned long long key, int u, float s, const float* dl) {
  WarpHit h;
  const unsigned low = (unsigned)key;
  h.x = (int)(low >> 1);
  h.kind = (int)(low & 1u);
  const float d0 = dl[h.x];
  h.a = 0.f;
  h.z = d0;
  if (h.kind) {
    const float d1 = dl[h.x + 1];
    const float t0 = warp_target(h.x, s, d0), t1 = warp_target(h.x + 1, s, d1);
    h.a = w_div(w_sub((float)u, t0), w_sub(t1, t0));
    h.z = w_lerp(h.a, d0, d1);
  }
  return h;
}

__device__ __forceinline__ float warp_colour(const float* __restrict__ img_row, const WarpHit& h) {
  const float v0 = img_row[h.x];
  return h.kind ? w_lerp(h.a, v0, img_row[h.x + 1]) : v0;
}

template <bool WAVEROWS>
__global__ __launch_bounds__(kWarpThreads) void forward_warp_rows(
    const float* __restrict__ image, long long img_bs, const float* __restrict__ disp, long long disp_bs,
    const unsigned char* __restrict__ exclude, const float* __restrict__ scales, long long rows, int C, int H, int W,
    float max_diff, float max_stretch, int fill, float fill_value, float* __restrict__ warped,
    float* __restrict__ zview, unsigned char* __restrict__ state, float* __restrict__ source) {
  extern __shared__ unsigned long long warp_lds[];
  __shared__ int wave_first[kWarpWaves], wave_last[kWarpWaves];
  constexpr int NL = WAVEROWS ? kWave : kWarpThreads;  // lanes to a row
  constexpr int RB = WAVEROWS ? kWarpWaves : 1;        // rows to a workgroup
  const int tid = threadIdx.x;
  const int sub = WAVEROWS ? tid / kWave : 0;
  const int lt = WAVEROWS ? tid % kWave : tid;
  const int lane = tid % kWave, wave = tid / kWave;
  const long long row = (long long)blockIdx.x * RB + sub;
  const bool live = row < rows;
  const long long b = live ? row / H : 0;
  const int y = live ? (int)(row - b * H) : 0;

  unsigned long long* key = warp_lds + (size_t)sub * W;
  float* dl = reinterpret_cast<float*>(warp_lds + (size_t)RB * W) + (size_t)sub * W;

  const long long plane = (long long)H * W;
  const float* d_row = disp + b * disp_bs + (long long)y * W;
  const unsigned char* e_row = exclude ? exclude + b * plane + (long long)y * W : nullptr;
  const float* i_row = image + b * img_bs + (long long)y * W;  // channel c: + c * plane
  const long long o = b * plane + (long long)y * W;            // this row in a [B, H, W] output
  float* w_row = warped ? warped + b * C * plane + (long long)y * W : nullptr;
  const float s = live ? scales[b] : 0.f;
  const float nan = __builtin_nanf("");
  const float wmax = (float)(W - 1);

  // load
  for (int x = lt; x < W; x += NL) {
    float d = nan;
    if (live) {
      d = d_row[x];
      if (e_row && e_row[x]) d = nan;
    }
    dl[x] = d;
    key[x] = 0ull;
  }
  __syncthreads();

  // scatter
  for (int x = lt; x < W; x += NL) {
    const float d0 = dl[x];
    const float t0 = warp_target(x, s, d0);
    if (!(__builtin_isfinite(d0) && __builtin_isfinite(t0))) continue;
    const float up = rintf(t0);
    if (up >= 0.f && up <= wmax) atomicMax(&key[(int)up], warp_key(d0, x, 0));
    if (x + 1 >= W) continue;
    const float d1 = dl[x + 1];
    const float t1 = warp_target(x + 1, s, d1);
    if (!(__builtin_isfinite(d1) && __builtin_isfinite(t1))) continue;
    if (!(fabsf(w_sub(d1, d0)) <= max_diff)) continue;
    const float den = w_sub(t1, t0);
    if (!(den > 0.f && den <= max_stretch)) continue;
    const float lo = fmaxf(ceilf(t0), 0.f), hi = fminf(floorf(t1), wmax);
    if (!(lo <= hi)) continue;
    const int u0 = (int)lo, u1 = (int)hi;  // both in 0 .. W - 1
    for (int u = u0; u <= u1; ++u) {
      const float a = w_div(w_sub((float)u, t0), den);
      atomicMax(&key[u], warp_key(w_lerp(a, d0, d1), x, 1));
    }
  }
  __syncthreads();

  // resolve: hits always; holes here unless the fill phase takes them
  if (live)
    for (int u = lt; u < W; u += NL) {
      const unsigned long long k = key[u];
      if (k) {
        const WarpHit h = warp_decode(k, u, s, dl);
        if (w_row)
          for (int c = 0; c < C; ++c) w_row[c * plane + u] = warp_colour(i_row + c * plane, h);
        if (zview) zview[o + u] = h.z;
        if (state) state[o + u] = 0;
        if (source) source[o + u] = w_add((float)h.x, h.a);
      } else {
        if (state) state[o + u] = 1;
        if (source) source[o + u] = -1.f;
        if (!fill) {
          if (w_row)
            for (int c = 0; c < C; ++c) w_row[c * plane + u] = fill_value;
          if (zview) zview[o + u] = nan;
        }
      }
    }
  if (!fill || !(w_row || zview)) return;  // uniform

  // fill: lane lt owns targets lt * K .. lt * K + K - 1
  const int K = (W + NL - 1) / NL;
  const int r0 = min(lt * K, W), r1 = min(r0 + K, W);
  int first = W, last = -1;  // this run's first and last hit
  for (int u = r0; u < r1; ++u)
    if (key[u]) {
      if (last < 0) first = u;
      last = u;
    }
  // the nearest hit before this run and after it: exclusive max / min scans over the lanes
  int pl = last, pf = first;
  for (int dlt = 1; dlt < kWave; dlt <<= 1) {
    const int vl = __shfl_up(pl, dlt), vf = __shfl_down(pf, dlt);
    if (lane >= dlt) pl = max(pl, vl);
    if (lane + dlt < kWave) pf = min(pf, vf);
  }
  int before = __shfl_up(pl, 1), after = __shfl_down(pf, 1);
  if (lane == 0) before = -1;
  if (lane == kWave - 1) after = W;
  if (!WAVEROWS) {
    if (lane == kWave - 1) wave_last[wave] = pl;  // inclusive over the wave
    if (lane == 0) wave_first[wave] = pf;
    __syncthreads();
    for (int w2 = 0; w2 < wave; ++w2) before = max(before, wave_last[w2]);
    for (int w2 = wave + 1; w2 < kWarpWaves; ++w2) after = min(after, wave_first[w2]);
  }
  if (!live) return;
  int left = before;
  for (int u = r0; u < r1; ++u) {
    if (key[u]) {
      left = u;
      continue;
    }
    int right = after;
    for (int v = u + 1; v < r1; ++v)
      if (key[v]) {
        right = v;
        break;
      }
    const bool hl = left >= 0, hr = right < W;
    if (!hl && !hr) {  // a row with no hit
      if (w_row)
        for (int c = 0; c < C; ++c) w_row[c * plane + u] = fill_value;
      if (zview) zview[o + u] = nan;
      continue;
    }
    WarpHit h;
    if (hl) h = warp_decode(key[left], left, s, dl);
    if (hr) {
      const WarpHit g = warp_decode(key[right], right, s, dl);
      if (!hl || g.z < h.z) h = g;  // the background; the left one on a tie
    }
    if (w_row)
      for (int c = 0; c < C; ++c) w_row[c * plane + u] = warp_colour(i_row + c * plane, h);
    if (zview) zview[o + u] = h.z;
  }
}

}  // namespace lea

extern "C" int lea_forward_warp_f32(const float* image, int64_t image_bstride, const float* disp,
                                    int64_t disp_bstride, const uint8_t* exclude, const float* scales, int B, int C,
                                    int H, int W, float max_diff, float max_stretch, int fill, float fill_value,
                                    float* warped, float* zview, uint8_t* state, float* source, void* stream) {
  using namespace lea;
  const char* who = "lea_forward_warp_f32";
  clear_error();
  LEA_CHECK_ARG(image && disp && scales, "%s: null pointer (image, disp and scales are required)", who);
  LEA_CHECK_ARG(warped || zview || state || source, "%s: no output wanted (all four null)", who);
  LEA_CHECK_ARG(B > 0 && H > 0 && W > 0, "%s: bad shape B=%d H=%d W=%d", who, B, H, W);
  LEA_CHECK_ARG(W <= LEA_FORWARD_WARP_MAX_W, "%s: W=%d is above the limit %d", who, W, LEA_FORWARD_WARP_MAX_W);
  LEA_CHECK_ARG((long long)B * H <= 0x7fffffffLL, "%s: B*H=%lld is above 2^31 - 1", who, (long long)B * H);
  LEA_CHECK_ARG(C >= 1 && C <= 4, "%s: C=%d is outside 1 .. 4", who, C);
  const long long plane = (long long)H * W;
  LEA_CHECK_ARG(image_bstride >= C * plane, "%s: image batch stride %lld is below C*H*W = %lld", who,
                (long long)image_bstride, C * plane);
  LEA_CHECK_ARG(disp_bstride >= plane, "%s: disp batch stride %lld is below H*W = %lld", who,
                (long long)disp_bstride, plane);
  LEA_CHECK_ARG(max_diff >= 0.f && max_diff <= 3.402823466e+38f, "%s: max_diff %g is not a finite number >= 0", who,
                (double)max_diff);
  LEA_CHECK_ARG(max_stretch >= 1.f && max_stretch <= 64.f, "%s: max_stretch %g is outside 1 .. 64", who,
                (double)max_stretch);
  LEA_CHECK_ARG(fill == 0 || fill == 1, "%s: fill %d is neither 0 nor 1", who, fill);
  {  // no output may overlap an input, scales or another output
    const size_t n = (size_t)B * (size_t)plane;
    const void* p[8] = {image, disp, exclude, scales, warped, zview, state, source};
    const size_t len[8] = {4 * ((size_t)(B - 1) * (size_t)image_bstride + (size_t)C * (size_t)plane),
                           4 * ((size_t)(B - 1) * (size_t)disp_bstride + (size_t)plane),
                           n, 4 * (size_t)B, 4 * n * (size_t)C, 4 * n, n, 4 * n};
    for (int i = 0; i < 8; ++i)
      for (int j = (i < 4 ? 4 : i + 1); j < 8; ++j) {
        if (!p[i] || !p[j]) continue;
        LEA_CHECK_ARG(!spans_overlap(p[i], len[i], p[j], len[j]),
                      "%s: buffers %d and %d overlap (0 = image, 1 = disp, 2 = exclude, 3 = scales, 4 = warped, "
                      "5 = zview, 6 = state, 7 = source)", who, i, j);
      }
  }
  const long long rows = (long long)B * H;
  if (W <= kWarpWaveRowW) {
    const unsigned grid = (unsigned)((rows + kWarpWaves - 1) / kWarpWaves);
    forward_warp_rows<true><<<grid, kWarpThreads, (size_t)kWarpWaves * W * 12, as_stream(stream)>>>(
        image, image_bstride, disp, disp_bstride, exclude, scales, rows, C, H, W, max_diff, max_stretch, fill,
        fill_value, warped, zview, state, source);
  } else {
    forward_warp_rows<false><<<(unsigned)rows, kWarpThreads, (size_t)W * 12, as_stream(stream)>>>(
        image, image_bstride, disp, disp_bstride, exclude, scales, rows, C, H, W, max_diff, max_stretch, fill,
        fill_value, warped, zview, state, source);
  }
  return launch_status(who);
}
