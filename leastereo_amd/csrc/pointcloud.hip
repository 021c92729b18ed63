// Point cloud of a disparity map: reprojection through a 4 x 4 matrix Q (OpenCV's
// reprojectImageTo3D), the validity test, and the valid points compacted in row-major pixel
// order with their colours, pixel indices and normals.  The definition is at
// lea_disparity_pointcloud_f32 in include/leastereo_hip.h.
//
// Up to three launches on one stream, ordered by the launch boundaries and by nothing else:
//   1. pc_count    a workgroup takes kPcBlk consecutive pixels of one image, a wave 64
//                  consecutive pixels at a time: the organised outputs (points, valid) and the
//                  number of valid pixels of the block, from the waves' ballots.
//   2. pc_scan     one workgroup per image turns its block counts into exclusive offsets, in
//                  place, kPcScan counts a pass with the running total carried from pass to
//                  pass in a register; the total is count[b].
//   3. pc_scatter  the same blocks again: a valid lane's row is the block's offset + the valid
//                  pixels of the block's earlier 64-pixel segments (LDS) + the valid lanes
//                  below it in its wave (ballot, mbcnt).  Rows at or above capacity are dropped.
// The row of a pixel is a function of the validity map alone: no atomic decides a position, no
// workgroup waits for another, nothing is read back.  pc_count and pc_scatter both get a
// pixel's validity and point from pc_point(), the one copy of that arithmetic (contraction
// off), which is why xyz equals the points rows at index bit for bit and why the scatter's
// ballots repeat the counts the offsets were made from.
#include <cmath>

#include "common.h"

namespace lea {

constexpr int kPcThreads = 256;                   // 4 waves
constexpr int kPcPer = 4;                         // pixels of a lane
constexpr int kPcBlk = kPcThreads * kPcPer;       // pixels of a workgroup (BLK)
constexpr int kPcWaves = kPcThreads / kWave;
constexpr int kPcSegs = kPcPer * kPcWaves;        // 64-pixel segments of a block, in pixel order
constexpr int kPcScanPer = 4;                     // block counts of a lane in a scan pass
constexpr int kPcScan = kPcThreads * kPcScanPer;  // block counts of a scan pass (SCAN)

struct PcQ {
  float q[16];
};

__device__ __forceinline__ PcQ pc_load_q(const float* __restrict__ Q) {
  PcQ m;
#pragma unroll
  for (int k = 0; k < 16; ++k) m.q[k] = Q[k];
  return m;
}

// the validity of pixel (x, y) with disparity d and exclude byte e, and its point: the products
// and sums in the order written, each rounded on its own, then three IEEE divisions
__device__ __forceinline__ bool pc_point(const PcQ& m, int x, int y, float d, unsigned char e, float lo, float hi,
                                         float P[3]) {
#pragma clang fp contract(off)
  if (e || !__builtin_isfinite(d) || !(d > lo && d <= hi)) return false;
  const float fx = (float)x, fy = (float)y;
  float h[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) h[r] = ((m.q[4 * r] * fx + m.q[4 * r + 1] * fy) + m.q[4 * r + 2] * d) + m.q[4 * r + 3];
  P[0] = h[0] / h[3];
  P[1] = h[1] / h[3];
  P[2] = h[2] / h[3];
  return __builtin_isfinite(P[0]) && __builtin_isfinite(P[1]) && __builtin_isfinite(P[2]);
}

// the neighbour (x, y) of a valid pixel with disparity dp, inside the image: usable when it is
// valid and within nmd of dp
__device__ __forceinline__ bool pc_neighbour(const PcQ& m, const float* __restrict__ disp,
                                             const unsigned char* __restrict__ exclude, int W, int x, int y, float dp,
                                             float lo, float hi, float nmd, float P[3]) {
  const int i = y * W + x;
  const float d = disp[i];
  const unsigned char e = exclude ? exclude[i] : (unsigned char)0;
  return pc_point(m, x, y, d, e, lo, hi, P) && fabsf(d - dp) <= nmd;
}

// P(plus) - P(minus), one-sided against the pixel's own point when one neighbour is usable
__device__ __forceinline__ bool pc_diff(bool um, const float* Pm, bool up, const float* Pp, const float* P0,
                                        float dlt[3]) {
  if (!um && !up) return false;
  const float* a = up ? Pp : P0;
  const float* b = um ? Pm : P0;
#pragma unroll
  for (int k = 0; k < 3; ++k) dlt[k] = a[k] - b[k];
  return true;
}

__device__ __forceinline__ void pc_normal(const PcQ& m, const float* __restrict__ disp,
                                          const unsigned char* __restrict__ exclude, int H, int W, int x, int y, float d,
                                          const float* P0, float lo, float hi, float nmd, float n[3]) {
#pragma clang fp contract(off)
  n[0] = n[1] = n[2] = 0.f;
  float Pm[3], Pp[3], dx[3], dy[3];
  bool um = x > 0 && pc_neighbour(m, disp, exclude, W, x - 1, y, d, lo, hi, nmd, Pm);
  bool up = x < W - 1 && pc_neighbour(m, disp, exclude, W, x + 1, y, d, lo, hi, nmd, Pp);
  if (!pc_diff(um, Pm, up, Pp, P0, dx)) return;
  um = y > 0 && pc_neighbour(m, disp, exclude, W, x, y - 1, d, lo, hi, nmd, Pm);
  up = y < H - 1 && pc_neighbour(m, disp, exclude, W, x, y + 1, d, lo, hi, nmd, Pp);
  if (!pc_diff(um, Pm, up, Pp, P0, dy)) return;
  const float c0 = dx[1] * dy[2] - dx[2] * dy[1];
  const float c1 = dx[2] * dy[0] - dx[0] * dy[2];
  const float c2 = dx[0] * dy[1] - dx[1] * dy[0];
  const float len = sqrtf((c0 * c0 + c1 * c1) + c2 * c2);
  if (!(len > 0.f) || !__builtin_isfinite(len)) return;  // no length, or one that overflowed
  float v[3] = {c0 / len, c1 / len, c2 / len};
  const float dot = (v[0] * P0[0] + v[1] * P0[1]) + v[2] * P0[2];
  const bool flip = dot > 0.f;  // towards the camera at the origin
#pragma unroll
  for (int k = 0; k < 3; ++k) n[k] = flip ? -v[k] : v[k];
}

// lanes of this wave below this one whose bit is set in mask
__device__ __forceinline__ int pc_rank(unsigned long long mask) {
  return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

// Stage 1.  Pass j of the block covers pixels blk * kPcBlk + j * kPcThreads + tid: a wave reads
// 64 consecutive floats and writes 64 consecutive 12-byte points.
__global__ __launch_bounds__(kPcThreads) void pc_count(const float* __restrict__ disp,
                                                       const unsigned char* __restrict__ exclude,
                                                       const float* __restrict__ Q, long long q_bstride, int hw, int W,
                                                       float lo, float hi, float* __restrict__ points,
                                                       unsigned char* __restrict__ valid, int* __restrict__ blocks) {
  __shared__ int seg[kPcWaves];
  const int b = blockIdx.y;
  const size_t base = (size_t)b * (size_t)hw;
  const PcQ m = pc_load_q(Q + (long long)b * q_bstride);
  const float nan = __builtin_nanf("");
  int mine = 0;  // valid pixels of this wave, the same in every lane
#pragma unroll
  for (int j = 0; j < kPcPer; ++j) {
    const long long i = (long long)blockIdx.x * kPcBlk + j * kPcThreads + threadIdx.x;
    bool ok = false;
    float P[3] = {nan, nan, nan};
    if (i < hw) {
      const size_t o = base + (size_t)i;
      const int y = (int)i / W, x = (int)i - y * W;
      ok = pc_point(m, x, y, disp[o], exclude ? exclude[o] : (unsigned char)0, lo, hi, P);
      if (points) {
        float* p = points + 3 * o;
        p[0] = ok ? P[0] : nan;
        p[1] = ok ? P[1] : nan;
        p[2] = ok ? P[2] : nan;
      }
      if (valid) valid[o] = ok ? 1 : 0;
    }
    mine += __builtin_popcountll(__ballot(ok));
  }
  if ((threadIdx.x & (kWave - 1)) == 0) seg[threadIdx.x / kWave] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    int n = 0;
#pragma unroll
    for (int w = 0; w < kPcWaves; ++w) n += seg[w];
    blocks[(size_t)b * gridDim.x + blockIdx.x] = n;
  }
}

// Stage 2.  One workgroup per image; lane t of a pass owns kPcScanPer consecutive counts.  The
// carry is the same in every lane: each adds the same four wave totals to it.
__global__ __launch_bounds__(kPcThreads) void pc_scan(int* __restrict__ blocks, int nblk, int* __restrict__ count) {
  __shared__ int tot[2][kPcWaves];
  int* c = blocks + (size_t)blockIdx.x * (size_t)nblk;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  int carry = 0, buf = 0;
  for (int p0 = 0; p0 < nblk; p0 += kPcScan, buf ^= 1) {
    const int k0 = p0 + threadIdx.x * kPcScanPer;
    int v[kPcScanPer], s = 0;
#pragma unroll
    for (int k = 0; k < kPcScanPer; ++k) {
      v[k] = k0 + k < nblk ? c[k0 + k] : 0;
      s += v[k];
    }
    int incl = s;  // inclusive scan of s over the wave
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
      const int t = __shfl_up(incl, d);
      if (lane >= d) incl += t;
    }
    if (lane == kWave - 1) tot[buf][wave] = incl;
    __syncthreads();  // one barrier a pass: the next pass writes the other half of tot
    int before = carry, all = 0;
#pragma unroll
    for (int w = 0; w < kPcWaves; ++w) {
      const int t = tot[buf][w];
      if (w < wave) before += t;
      all += t;
    }
    int run = before + incl - s;
#pragma unroll
    for (int k = 0; k < kPcScanPer; ++k) {
      if (k0 + k < nblk) c[k0 + k] = run;
      run += v[k];
    }
    carry += all;
  }
  if (count && threadIdx.x == 0) count[blockIdx.x] = carry;
}

// Stage 3.  The blocks and passes of stage 1; blocks[] now holds the exclusive offsets.
__global__ __launch_bounds__(kPcThreads) void pc_scatter(
    const float* __restrict__ disp, const unsigned char* __restrict__ exclude, const unsigned char* __restrict__ image,
    int pix_stride, const float* __restrict__ Q, long long q_bstride, int hw, int H, int W, float lo, float hi,
    float nmd, int capacity, const int* __restrict__ blocks, float* __restrict__ xyz, unsigned char* __restrict__ rgb,
    int* __restrict__ index, float* __restrict__ normals) {
  __shared__ int seg[kPcSegs];
  const int b = blockIdx.y;
  const size_t base = (size_t)b * (size_t)hw;
  const float* dimg = disp + base;
  const unsigned char* eimg = exclude ? exclude + base : nullptr;
  const PcQ m = pc_load_q(Q + (long long)b * q_bstride);
  const int wave = threadIdx.x / kWave;
  bool ok[kPcPer];
  float P[kPcPer][3];
  int below[kPcPer];
#pragma unroll
  for (int j = 0; j < kPcPer; ++j) {
    const long long i = (long long)blockIdx.x * kPcBlk + j * kPcThreads + threadIdx.x;
    ok[j] = false;
    if (i < hw) {
      const int y = (int)i / W, x = (int)i - y * W;
      ok[j] = pc_point(m, x, y, dimg[i], eimg ? eimg[i] : (unsigned char)0, lo, hi, P[j]);
    }
    const unsigned long long mask = __ballot(ok[j]);
    below[j] = pc_rank(mask);
    if ((threadIdx.x & (kWave - 1)) == 0) seg[j * kPcWaves + wave] = __builtin_popcountll(mask);
  }
  __syncthreads();
  const int first = blocks[(size_t)b * gridDim.x + blockIdx.x];
#pragma unroll
  for (int j = 0; j < kPcPer; ++j) {
    if (!ok[j]) continue;
    int row = first + below[j];
    for (int s = 0; s < j * kPcWaves + wave; ++s) row += seg[s];
    if (row >= capacity) continue;
    const int i = blockIdx.x * kPcBlk + j * kPcThreads + (int)threadIdx.x;
    const size_t o = (size_t)b * (size_t)capacity + (size_t)row;
    if (xyz) {
      float* p = xyz + 3 * o;
      p[0] = P[j][0];
      p[1] = P[j][1];
      p[2] = P[j][2];
    }
    if (rgb) {
      const unsigned char* px = image + (base + (size_t)i) * (size_t)pix_stride;
      unsigned char* p = rgb + 3 * o;
      p[0] = px[0];
      p[1] = px[1];
      p[2] = px[2];
    }
    if (index) index[o] = i;
    if (normals) {
      const int y = i / W, x = i - y * W;
      float n[3];
      pc_normal(m, dimg, eimg, H, W, x, y, dimg[i], P[j], lo, hi, nmd, n);
      float* p = normals + 3 * o;
      p[0] = n[0];
      p[1] = n[1];
      p[2] = n[2];
    }
  }
}

}  // namespace lea

extern "C" size_t lea_disparity_pointcloud_workspace_bytes(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  const size_t hw = (size_t)H * (size_t)W;
  return (size_t)B * ((hw + lea::kPcBlk - 1) / lea::kPcBlk) * sizeof(int);
}

extern "C" int lea_disparity_pointcloud_f32(const float* disp, const uint8_t* exclude, const void* image,
                                            int pix_stride, const float* Q, int64_t q_bstride, int B, int H, int W,
                                            float min_disp, float max_disp, float normal_max_diff, int capacity,
                                            void* workspace, float* points, uint8_t* valid, int32_t* count,
                                            float* xyz, uint8_t* rgb, int32_t* index, float* normals, void* stream) {
  using namespace lea;
  clear_error();
  const char* who = "lea_disparity_pointcloud_f32";
  LEA_CHECK_ARG(disp, "%s: disp is null", who);
  LEA_CHECK_ARG(Q, "%s: Q is null", who);
  LEA_CHECK_ARG(workspace, "%s: workspace is null", who);
  const bool compact = xyz || rgb || index || normals;
  LEA_CHECK_ARG(points || valid || count || compact, "%s: every output is null", who);
  LEA_CHECK_ARG(!rgb || image, "%s: rgb needs the image", who);
  LEA_CHECK_ARG(!image || pix_stride == 3 || pix_stride == 4, "%s: pix_stride %d is not 3 or 4", who, pix_stride);
  LEA_CHECK_ARG(B > 0 && H > 0 && W > 0, "%s: bad shape B=%d H=%d W=%d", who, B, H, W);
  LEA_CHECK_ARG(B <= 65535, "%s: B=%d above 65535", who, B);
  LEA_CHECK_ARG((long long)H * W <= 0x7fffffffLL && (long long)B * H * W <= 0x7fffffffLL,
                "%s: B*H*W = %lld*%lld is above 2^31 - 1", who, (long long)B, (long long)H * W);
  LEA_CHECK_ARG(q_bstride == 0 || q_bstride >= 16, "%s: Q batch stride %lld is neither 0 nor >= 16", who,
                (long long)q_bstride);
  LEA_CHECK_ARG(capacity >= 0, "%s: capacity %d is negative", who, capacity);
  LEA_CHECK_ARG(!compact || capacity > 0, "%s: capacity 0 with a compact output", who);
  LEA_CHECK_ARG(min_disp == min_disp && max_disp == max_disp, "%s: min_disp %g or max_disp %g is NaN", who,
                (double)min_disp, (double)max_disp);
  LEA_CHECK_ARG(normal_max_diff >= 0.f, "%s: normal_max_diff %g is not a number >= 0", who, (double)normal_max_diff);
  LEA_CHECK_ARG(((uintptr_t)workspace & 3) == 0, "%s: workspace must be 4-byte aligned", who);
  const int hw = H * W;
  const size_t n = (size_t)B * (size_t)hw, rows = (size_t)B * (size_t)capacity;
  const size_t wsn = lea_disparity_pointcloud_workspace_bytes(B, H, W);
  {  // no output may overlap an input, the workspace or another output
    const void* ins[5] = {disp, exclude, image, Q, workspace};
    const size_t inn[5] = {4 * n, n, n * (size_t)(image ? pix_stride : 0),
                           4 * ((size_t)(B - 1) * (size_t)q_bstride + 16), wsn};
    const char* inname[5] = {"disp", "exclude", "image", "Q", "the workspace"};
    const void* outs[7] = {points, valid, count, xyz, rgb, index, normals};
    const size_t outn[7] = {12 * n, n, 4 * (size_t)B, 12 * rows, 3 * rows, 4 * rows, 12 * rows};
    const char* outname[7] = {"points", "valid", "count", "xyz", "rgb", "index", "normals"};
    for (int o = 0; o < 7; ++o) {
      if (!outs[o]) continue;
      for (int i = 0; i < 5; ++i)
        LEA_CHECK_ARG(!ins[i] || !spans_overlap(outs[o], outn[o], ins[i], inn[i]), "%s: %s overlaps %s", who,
                      outname[o], inname[i]);
      for (int q = 0; q < o; ++q)
        LEA_CHECK_ARG(!outs[q] || !spans_overlap(outs[o], outn[o], outs[q], outn[q]), "%s: %s overlaps %s", who,
                      outname[o], outname[q]);
    }
    for (int i = 0; i < 4; ++i)
      LEA_CHECK_ARG(!ins[i] || !spans_overlap(workspace, wsn, ins[i], inn[i]), "%s: the workspace overlaps %s", who,
                    inname[i]);
  }
  int* blocks = static_cast<int*>(workspace);
  const int nblk = (int)(((long long)hw + kPcBlk - 1) / kPcBlk);
  const dim3 grid((unsigned)nblk, (unsigned)B);
  hipStream_t s = as_stream(stream);
  const unsigned char* img = static_cast<const unsigned char*>(image);
  pc_count<<<grid, kPcThreads, 0, s>>>(disp, exclude, Q, (long long)q_bstride, hw, W, min_disp, max_disp, points, valid,
                                       blocks);
  if (int rc = launch_status("lea_disparity_pointcloud_f32 (count)")) return rc;
  if (!count && !compact) return LEA_OK;
  pc_scan<<<(unsigned)B, kPcThreads, 0, s>>>(blocks, nblk, count);
  if (int rc = launch_status("lea_disparity_pointcloud_f32 (scan)")) return rc;
  if (!compact) return LEA_OK;
  pc_scatter<<<grid, kPcThreads, 0, s>>>(disp, exclude, img, pix_stride, Q, (long long)q_bstride, hw, H, W, min_disp,
                                         max_disp, normal_max_diff, capacity, blocks, xyz, rgb, index, normals);
  return launch_status("lea_disparity_pointcloud_f32 (scatter)");
}
