// Left-right consistency check of a disparity pair, with the scanline fill of what fails it.
//
// Per left pixel (y, x), dL = disp_left[b, y, x], threshold thr > 0:
//   xi = floor(x - dL + 0.5)                               (f32, no contraction)
//   state = 2 (out of view)   if xi < 0 or xi > W - 1
//           1 (inconsistent)  else if dL is not finite or !(|dL - disp_right[b, y, xi]| <= thr)
//           0 (consistent)    otherwise
//   disp_filled = dL (bit for bit) where state == 0; elsewhere the dL of the nearest
//           state-0 pixel to the left on the row and of the nearest one to the right, the
//           smaller of the two (the background); the one that exists; dL if neither does.
//
// One wave owns a row and walks it in chunks of 256 pixels, twice.  A chunk is loaded
// coalesced (lane l: pixels l, l + 64, l + 128, l + 192 of the chunk), its states formed
// and put in LDS with dL; then lane l scans its segment of four consecutive pixels for the
// last consistent value, the 64 segment carries are scanned across the wave with
// __shfl_up, and the chunk's carry goes on to the next chunk.  The forward walk leaves the
// left candidate (NaN: none) in disp_filled itself; the backward walk (chunks and segments
// in reverse, __shfl_down) forms the right candidate, reads the left one back -- each
// element by the lane that wrote it -- and writes the result.  Plain vector loads and
// stores only.
#include "common.h"

namespace lea {

constexpr int kLrSeg = 4;                  // consecutive pixels per lane in the scan
constexpr int kLrChunk = kWave * kLrSeg;   // pixels per pass of the wave

__device__ __forceinline__ int lr_state(const float dl, const int x, const int W, const float* __restrict__ dr_row,
                                        const float thr) {
#pragma clang fp contract(off)
  float v = (float)x - dl;
  v = v + 0.5f;
  const float xi = floorf(v);
  if (xi < 0.f || xi > (float)(W - 1)) return 2;  // NaN: neither
  if (!__builtin_isfinite(dl)) return 1;
  const int i = min(max((int)xi, 0), W - 1);  // in range already; the clamp is for the load's sake
  return fabsf(dl - dr_row[i]) <= thr ? 0 : 1;
}

struct LrCarry {  // the nearest consistent value seen so far
  int has;
  float val;
};

// c = later ? later : earlier, across the wave: after it lane l holds the carry of the lanes
// before it (BACK: after it) -- exclusive
template <bool BACK>
__device__ __forceinline__ LrCarry lr_wave_scan(LrCarry c, const int lane) {
  for (int d = 1; d < kWave; d <<= 1) {
    const int h = BACK ? __shfl_down(c.has, d) : __shfl_up(c.has, d);
    const float v = BACK ? __shfl_down(c.val, d) : __shfl_up(c.val, d);
    const bool in = BACK ? lane + d < kWave : lane >= d;
    if (in && !c.has) {
      c.has = h;
      c.val = v;
    }
  }
  LrCarry p;
  p.has = BACK ? __shfl_down(c.has, 1) : __shfl_up(c.has, 1);
  p.val = BACK ? __shfl_down(c.val, 1) : __shfl_up(c.val, 1);
  if (BACK ? lane == kWave - 1 : lane == 0) p.has = 0;
  return p;
}

__global__ __launch_bounds__(kWave) void lr_check_rows(const float* __restrict__ disp_left,
                                                       const float* __restrict__ disp_right,
                                                       unsigned char* __restrict__ state,
                                                       float* __restrict__ filled, long long rows, int W,
                                                       float thr) {
  __shared__ float val[kLrChunk];
  __shared__ int st[kLrChunk];
  __shared__ float res[kLrChunk];
  const int lane = threadIdx.x;
  const long long row = (long long)blockIdx.y * gridDim.x + blockIdx.x;
  if (row >= rows) return;  // the grid's last line may be partial (workgroup-uniform)
  const float* dl_row = disp_left + row * W;
  const float* dr_row = disp_right + row * W;
  unsigned char* st_row = state ? state + row * W : nullptr;
  float* out_row = filled ? filled + row * W : nullptr;
  const float nan = __builtin_nanf("");
  const int nchunk = (W + kLrChunk - 1) / kLrChunk;

  // forward: states out, the left candidate into disp_filled
  LrCarry carry{0, 0.f};
  for (int ch = 0; ch < nchunk; ++ch) {
    const int x0 = ch * kLrChunk;
#pragma unroll
    for (int i = 0; i < kLrSeg; ++i) {
      const int e = lane + i * kWave, x = x0 + e;
      float d = 0.f;
      int s = 3;  // past the row: never consistent
      if (x < W) {
        d = dl_row[x];
        s = lr_state(d, x, W, dr_row, thr);
        if (st_row) st_row[x] = (unsigned char)s;
      }
      val[e] = d;
      st[e] = s;
    }
    if (!out_row) continue;  // states alone: no scan (uniform)
    __syncthreads();
    LrCarry loc[kLrSeg], c{0, 0.f};
#pragma unroll
    for (int i = 0; i < kLrSeg; ++i) {
      const int e = lane * kLrSeg + i;
      if (st[e] == 0) c = LrCarry{1, val[e]};
      loc[i] = c;
    }
    LrCarry pre = lr_wave_scan<false>(c, lane);
    if (!pre.has) pre = carry;
#pragma unroll
    for (int i = 0; i < kLrSeg; ++i) {
      const LrCarry r = loc[i].has ? loc[i] : pre;
      res[lane * kLrSeg + i] = r.has ? r.val : nan;
    }
    // the chunk's carry: the last lane's inclusive value
    const LrCarry tot = c.has ? c : pre;
    carry.has = __shfl(tot.has, kWave - 1);
    carry.val = __shfl(tot.val, kWave - 1);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kLrSeg; ++i) {
      const int e = lane + i * kWave, x = x0 + e;
      if (x < W) out_row[x] = res[e];
    }
    __syncthreads();
  }
  if (!out_row) return;

  // backward: the right candidate, joined with the left one
  carry = LrCarry{0, 0.f};
  for (int ch = nchunk - 1; ch >= 0; --ch) {
    const int x0 = ch * kLrChunk;
    float d[kLrSeg], left[kLrSeg];
    int s[kLrSeg];
#pragma unroll
    for (int i = 0; i < kLrSeg; ++i) {
      const int e = lane + i * kWave, x = x0 + e;
      d[i] = 0.f;
      left[i] = nan;
      s[i] = 3;
      if (x < W) {
        d[i] = dl_row[x];
        s[i] = lr_state(d[i], x, W, dr_row, thr);
        left[i] = out_row[x];  // this lane's own store of the forward walk
      }
      val[e] = d[i];
      st[e] = s[i];
    }
    __syncthreads();
    LrCarry loc[kLrSeg], c{0, 0.f};
#pragma unroll
    for (int i = kLrSeg - 1; i >= 0; --i) {
      const int e = lane * kLrSeg + i;
      if (st[e] == 0) c = LrCarry{1, val[e]};
      loc[i] = c;
    }
    LrCarry pre = lr_wave_scan<true>(c, lane);
    if (!pre.has) pre = carry;
#pragma unroll
    for (int i = 0; i < kLrSeg; ++i) {
      const LrCarry r = loc[i].has ? loc[i] : pre;
      res[lane * kLrSeg + i] = r.has ? r.val : nan;
    }
    const LrCarry tot = c.has ? c : pre;
    carry.has = __shfl(tot.has, 0);
    carry.val = __shfl(tot.val, 0);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kLrSeg; ++i) {
      const int e = lane + i * kWave, x = x0 + e;
      if (x >= W) continue;
      const float l = left[i], r = res[e];
      float o = d[i];
      if (s[i] != 0) {
        const bool hl = l == l, hr = r == r;  // candidates are finite; NaN: none
        if (hl && hr)
          o = r < l ? r : l;
        else if (hl)
          o = l;
        else if (hr)
          o = r;
      }
      out_row[x] = o;
    }
    __syncthreads();
  }
}

}  // namespace lea

extern "C" int lea_disparity_lr_check(const float* disp_left, const float* disp_right, uint8_t* state,
                                      float* disp_filled, int B, int H, int W, float threshold, void* stream) {
  using namespace lea;
  clear_error();
  LEA_CHECK_ARG(disp_left && disp_right, "lea_disparity_lr_check: null pointer");
  LEA_CHECK_ARG(state || disp_filled, "lea_disparity_lr_check: no output wanted (state and disp_filled both null)");
  LEA_CHECK_ARG(B > 0 && H > 0 && W > 0, "lea_disparity_lr_check: bad shape B=%d H=%d W=%d", B, H, W);
  LEA_CHECK_ARG(threshold > 0.f && threshold <= 3.402823466e+38f,
                "lea_disparity_lr_check: threshold %g is not a finite number > 0", (double)threshold);
  const long long rows = (long long)B * H;
  LEA_CHECK_ARG(rows <= 65535LL * 65535LL && W <= 0x7fffffff - kLrChunk, "lea_disparity_lr_check: grid too large");
  {  // no output may overlap an input or the other output
    const size_t n = (size_t)B * (size_t)H * (size_t)W;
    const uintptr_t lo[4] = {(uintptr_t)disp_left, (uintptr_t)disp_right, (uintptr_t)state, (uintptr_t)disp_filled};
    const size_t len[4] = {4 * n, 4 * n, n, 4 * n};
    for (int i = 0; i < 4; ++i)
      for (int j = (i < 2 ? 2 : i + 1); j < 4; ++j) {
        if (!lo[i] || !lo[j]) continue;
        LEA_CHECK_ARG(lo[i] + len[i] <= lo[j] || lo[j] + len[j] <= lo[i],
                      "lea_disparity_lr_check: buffers %d and %d overlap "
                      "(0 = disp_left, 1 = disp_right, 2 = state, 3 = disp_filled)", i, j);
      }
  }
  // rows over a 2-D grid: x as wide as it goes, y the rest
  const unsigned gx = (unsigned)(rows < 65535 ? rows : 65535);
  const unsigned gy = (unsigned)((rows + gx - 1) / gx);
  lr_check_rows<<<dim3(gx, gy), kWave, 0, as_stream(stream)>>>(disp_left, disp_right, state, disp_filled, rows, W,
                                                                threshold);
  return launch_status("lea_disparity_lr_check");
}
