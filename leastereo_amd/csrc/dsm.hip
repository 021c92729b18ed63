// Surface model of point clouds: a z-buffered ground grid (DSM) with the colour or the row of
// the surface seen in each cell (orthophoto), accumulated over any number of calls.  The
// definition is at lea_dsm_splat_f32 in include/leastereo_hip.h.
//
// A cell is one uint64 key, (ord(z) << 32) | payload, 0 = empty; the highest surface is the
// unsigned maximum, so the only operation on the grid is a 64-bit integer max: order-independent,
// hence the same bits whatever the scheduling, the call order or the form of the scatter.
//   dsm_splat<false>  the global form: one 64-bit atomic max on the grid per covered cell.
//   dsm_splat<true>   the LDS-staged form: a workgroup reduces the bounding box of the cells its
//                     kDsmBlk rows cover; a box of at most kDsmTile cells is zeroed in LDS, takes
//                     the block's hits with LDS atomics and is flushed, non-empty cells only, as
//                     contiguous runs of global atomics; a larger box takes the global form.
//                     kDsmTile = 4096 cells = 32 KB of keys + 16 KB of counts: three workgroups
//                     a CU by LDS (160 KB), and a 32 x 32 patch at one point per cell on a grid
//                     rotated by 45 degrees (a box of 48 x 48) still fits.
// Both forms get a row's span, key and nearest cell from dsm_row(), the one copy of that
// arithmetic (contraction off).  Nothing waits: no lock, no spin, no float atomic.
//   dsm_fill    one fill pass of lea_dsm_resolve_f32, from one buffer to another.
//   dsm_decode  keys to height / rgb / source / state.
//   dsm_zero    lea_dsm_clear.
#include <cmath>

#include "common.h"

namespace lea {

constexpr int kDsmThreads = 256;                    // 4 waves
constexpr int kDsmPer = 4;                          // rows of a lane
constexpr int kDsmBlk = kDsmThreads * kDsmPer;      // rows of a workgroup
constexpr int kDsmPatch = 32;                       // a block of an image of rows: 32 x 32 pixels
constexpr int kDsmWaves = kDsmThreads / kWave;
constexpr int kDsmTile = 4096;                      // cells of the LDS tile
constexpr float kDsmMaxCoord = 1073741824.f;        // 2^30
constexpr int kDsmMaxFill = 1024;                   // fill passes of a resolve

static_assert(kDsmPatch * kDsmPatch == kDsmBlk, "a patch is a block of rows");

typedef unsigned long long u64;

struct DsmG {
  float g[12];
};

// the order-preserving map of float32 bits to uint32 and back
__device__ __forceinline__ unsigned dsm_ord(float z) {
  const unsigned b = __float_as_uint(z);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float dsm_unord(unsigned o) {
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

// what a row does to the grid: the clipped span of cells [c0, c1] x [r0, r1] (empty when
// c0 > c1 or r0 > r1), its nearest cell (nc, nr; in the grid when near) and ord(z)
struct DsmRow {
  int c0, c1, r0, r1, nc, nr;
  unsigned hi;
  bool near;
};

__device__ __forceinline__ bool dsm_row(const DsmG& m, float X, float Y, float Z, float radius, int GH, int GW,
                                        DsmRow& h) {
#pragma clang fp contract(off)
  if (!(__builtin_isfinite(X) && __builtin_isfinite(Y) && __builtin_isfinite(Z))) return false;
  const float u = ((m.g[0] * X + m.g[1] * Y) + m.g[2] * Z) + m.g[3];
  const float v = ((m.g[4] * X + m.g[5] * Y) + m.g[6] * Z) + m.g[7];
  const float z = ((m.g[8] * X + m.g[9] * Y) + m.g[10] * Z) + m.g[11];
  if (!(__builtin_isfinite(u) && __builtin_isfinite(v) && __builtin_isfinite(z))) return false;
  if (fabsf(u) > kDsmMaxCoord || fabsf(v) > kDsmMaxCoord) return false;
  // bounded by 2^30 + 3 in size: the conversions are exact
  const int c0 = (int)floorf((u - radius) + 0.5f), c1 = (int)floorf((u + radius) + 0.5f);
  const int r0 = (int)floorf((v - radius) + 0.5f), r1 = (int)floorf((v + radius) + 0.5f);
  h.nc = (int)floorf(u + 0.5f);
  h.nr = (int)floorf(v + 0.5f);
  h.near = h.nc >= 0 && h.nc < GW && h.nr >= 0 && h.nr < GH;
  h.c0 = c0 > 0 ? c0 : 0;
  h.c1 = c1 < GW - 1 ? c1 : GW - 1;
  h.r0 = r0 > 0 ? r0 : 0;
  h.r1 = r1 < GH - 1 ? r1 : GH - 1;
  h.hi = dsm_ord(z);
  return h.c0 <= h.c1 && h.r0 <= h.r1;
}

// local row l (0 .. kDsmBlk - 1) of this workgroup as a row of the item, or -1: consecutive rows,
// or with row_width > 0 pixel (l % 32, l / 32) of patch blockIdx.x of an image of that width
__device__ __forceinline__ long long dsm_row_index(int l, int row_width, int patches_x) {
  if (row_width <= 0) return (long long)blockIdx.x * kDsmBlk + l;
  const int py = (int)blockIdx.x / patches_x, px = (int)blockIdx.x - py * patches_x;
  const int x = px * kDsmPatch + (l & (kDsmPatch - 1)), y = py * kDsmPatch + l / kDsmPatch;
  return x < row_width ? (long long)y * row_width + x : -1;
}

__device__ __forceinline__ void dsm_apply_global(const DsmRow& h, u64 key, int GW, u64* __restrict__ keys,
                                                 int* __restrict__ hits) {
  for (int r = h.r0; r <= h.r1; ++r)
    for (int c = h.c0; c <= h.c1; ++c)
      __hip_atomic_fetch_max(keys + (size_t)r * GW + c, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (hits && h.near)
    __hip_atomic_fetch_add(hits + (size_t)h.nr * GW + h.nc, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <bool kStaged>
__global__ __launch_bounds__(kDsmThreads) void dsm_splat(const float* __restrict__ points,
                                                         const int* __restrict__ count,
                                                         const unsigned char* __restrict__ colours,
                                                         const float* __restrict__ G, long long g_bstride, int rows,
                                                         int row_width, int patches_x, float radius, int GH, int GW,
                                                         u64* __restrict__ keys, int* __restrict__ hits) {
  __shared__ u64 tile[kStaged ? kDsmTile : 1];
  __shared__ int htile[kStaged ? kDsmTile : 1];
  __shared__ int box[kDsmWaves][4];
  const int b = blockIdx.y;
  int n = rows;
  if (count) {
    const int c = count[b];
    n = c < rows ? (c > 0 ? c : 0) : rows;
  }
  DsmG m;
#pragma unroll
  for (int k = 0; k < 12; ++k) m.g[k] = G[(long long)b * g_bstride + k];
  const size_t cells = (size_t)GH * (size_t)GW;
  keys += (size_t)b * cells;
  if (hits) hits += (size_t)b * cells;
  const float* pts = points + (size_t)b * (size_t)rows * 3;
  const unsigned char* col = colours ? colours + (size_t)b * (size_t)rows * 3 : nullptr;

  DsmRow h[kDsmPer];
  u64 key[kDsmPer];
  bool ok[kDsmPer];
#pragma unroll
  for (int j = 0; j < kDsmPer; ++j) {
    const long long row = dsm_row_index(j * kDsmThreads + (int)threadIdx.x, row_width, patches_x);
    ok[j] = false;
    key[j] = 0;
    if (row >= 0 && row < n) {
      const float* p = pts + 3 * (size_t)row;
      ok[j] = dsm_row(m, p[0], p[1], p[2], radius, GH, GW, h[j]);
    }
    if (ok[j]) {
      unsigned payload = 0xFFFFFFFFu - (unsigned)row;
      if (col) {
        const unsigned char* q = col + 3 * (size_t)row;
        payload = ((unsigned)q[0] << 16) | ((unsigned)q[1] << 8) | (unsigned)q[2];
      }
      key[j] = ((u64)h[j].hi << 32) | payload;
    }
  }

  if (!kStaged) {
#pragma unroll
    for (int j = 0; j < kDsmPer; ++j)
      if (ok[j]) dsm_apply_global(h[j], key[j], GW, keys, hits);
    return;
  }

  // the bounding box of the block's covered cells
  int x0 = 0x7fffffff, y0 = 0x7fffffff, x1 = -1, y1 = -1;
#pragma unroll
  for (int j = 0; j < kDsmPer; ++j) {
    if (!ok[j]) continue;
    x0 = h[j].c0 < x0 ? h[j].c0 : x0;
    y0 = h[j].r0 < y0 ? h[j].r0 : y0;
    x1 = h[j].c1 > x1 ? h[j].c1 : x1;
    y1 = h[j].r1 > y1 ? h[j].r1 : y1;
  }
#pragma unroll
  for (int d = kWave / 2; d > 0; d >>= 1) {
    const int a0 = __shfl_xor(x0, d), b0 = __shfl_xor(y0, d), a1 = __shfl_xor(x1, d), b1 = __shfl_xor(y1, d);
    x0 = a0 < x0 ? a0 : x0;
    y0 = b0 < y0 ? b0 : y0;
    x1 = a1 > x1 ? a1 : x1;
    y1 = b1 > y1 ? b1 : y1;
  }
  if ((threadIdx.x & (kWave - 1)) == 0) {
    int* bx = box[threadIdx.x / kWave];
    bx[0] = x0, bx[1] = y0, bx[2] = x1, bx[3] = y1;
  }
  __syncthreads();
#pragma unroll
  for (int w = 0; w < kDsmWaves; ++w) {
    x0 = box[w][0] < x0 ? box[w][0] : x0;
    y0 = box[w][1] < y0 ? box[w][1] : y0;
    x1 = box[w][2] > x1 ? box[w][2] : x1;
    y1 = box[w][3] > y1 ? box[w][3] : y1;
  }
  if (x1 < 0) return;  // no row of the block covers a cell (the same in every lane)
  const long long bw = (long long)x1 - x0 + 1, bh = (long long)y1 - y0 + 1;
  if (bw * bh > kDsmTile) {  // the same in every lane
#pragma unroll
    for (int j = 0; j < kDsmPer; ++j)
      if (ok[j]) dsm_apply_global(h[j], key[j], GW, keys, hits);
    return;
  }
  const int tw = (int)bw, area = (int)(bw * bh);
  for (int i = threadIdx.x; i < area; i += kDsmThreads) {
    tile[i] = 0;
    htile[i] = 0;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kDsmPer; ++j) {
    if (!ok[j]) continue;
    for (int r = h[j].r0; r <= h[j].r1; ++r)
      for (int c = h[j].c0; c <= h[j].c1; ++c)
        __hip_atomic_fetch_max(&tile[(r - y0) * tw + (c - x0)], key[j], __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_WORKGROUP);
    if (hits && h[j].near)
      __hip_atomic_fetch_add(&htile[(h[j].nr - y0) * tw + (h[j].nc - x0)], 1, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < area; i += kDsmThreads) {
    const u64 k = tile[i];
    if (k == 0) continue;  // a counted cell is a covered cell
    const int r = i / tw, c = i - r * tw;
    const size_t o = (size_t)(y0 + r) * GW + (size_t)(x0 + c);
    __hip_atomic_fetch_max(keys + o, k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (hits && htile[i] != 0)
      __hip_atomic_fetch_add(hits + o, htile[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// one fill pass: a cell empty in `in` with at least minn non-empty 8-neighbours takes the smallest
// of their keys; every other cell is copied
__global__ __launch_bounds__(kDsmThreads) void dsm_fill(const u64* __restrict__ in, u64* __restrict__ out, int GH,
                                                        int GW, int minn) {
  const long long cells = (long long)GH * GW;
  const long long i = (long long)blockIdx.x * kDsmThreads + threadIdx.x;
  if (i >= cells) return;
  const u64* src = in + (size_t)blockIdx.y * (size_t)cells;
  u64 k = src[i];
  if (k == 0) {
    const int y = (int)(i / GW), x = (int)(i - (long long)y * GW);
    int cnt = 0;
    u64 lo = ~(u64)0;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx) {
        if (dx == 0 && dy == 0) continue;
        const int yy = y + dy, xx = x + dx;
        if (yy < 0 || yy >= GH || xx < 0 || xx >= GW) continue;
        const u64 q = src[(size_t)yy * GW + xx];
        if (q == 0) continue;
        ++cnt;
        lo = q < lo ? q : lo;
      }
    }
    if (cnt >= minn) k = lo;
  }
  out[(size_t)blockIdx.y * (size_t)cells + i] = k;
}

// `fin` after the fill passes (keys itself without one) to the outputs
__global__ __launch_bounds__(kDsmThreads) void dsm_decode(const u64* __restrict__ keys, const u64* __restrict__ fin,
                                                          long long cells, float nodata, float* __restrict__ height,
                                                          unsigned char* __restrict__ rgb, int* __restrict__ source,
                                                          unsigned char* __restrict__ state) {
  const long long i = (long long)blockIdx.x * kDsmThreads + threadIdx.x;
  if (i >= cells) return;
  const size_t o = (size_t)blockIdx.y * (size_t)cells + (size_t)i;
  const u64 k = fin[o];
  const unsigned payload = (unsigned)k;
  if (height) height[o] = k ? dsm_unord((unsigned)(k >> 32)) : nodata;
  if (rgb) {
    unsigned char* p = rgb + 3 * o;
    p[0] = k ? (unsigned char)(payload >> 16) : 0;
    p[1] = k ? (unsigned char)(payload >> 8) : 0;
    p[2] = k ? (unsigned char)payload : 0;
  }
  if (source) source[o] = k ? (int)(0xFFFFFFFFu - payload) : -1;
  if (state) state[o] = keys[o] ? 0 : (k ? 1 : 2);
}

__global__ __launch_bounds__(kDsmThreads) void dsm_zero(u64* __restrict__ keys, int* __restrict__ hits, long long n) {
  const long long i = (long long)blockIdx.x * kDsmThreads + threadIdx.x;
  if (i >= n) return;
  keys[i] = 0;
  if (hits) hits[i] = 0;
}

// the size checks the three entries share: B, GH, GW >= 1, B <= 65535, B * GH * GW <= 2^31 - 1
static int dsm_check_grid(const char* who, int B, int GH, int GW) {
  LEA_CHECK_ARG(B > 0 && GH > 0 && GW > 0, "%s: bad shape B=%d GH=%d GW=%d", who, B, GH, GW);
  LEA_CHECK_ARG(B <= 65535, "%s: B=%d above 65535", who, B);
  LEA_CHECK_ARG((long long)GH * GW <= 0x7fffffffLL && (long long)B * GH * GW <= 0x7fffffffLL,
                "%s: B*GH*GW = %lld*%lld is above 2^31 - 1", who, (long long)B, (long long)GH * GW);
  return LEA_OK;
}

}  // namespace lea

extern "C" size_t lea_dsm_resolve_workspace_bytes(int B, int GH, int GW) {
  if (B <= 0 || GH <= 0 || GW <= 0) return 0;
  return 2 * sizeof(lea::u64) * (size_t)B * (size_t)GH * (size_t)GW;
}

extern "C" int lea_dsm_splat_f32(const float* points, const int32_t* count, const uint8_t* colours, const float* G,
                                 int64_t g_bstride, int B, int rows, int row_width, float radius, int staging,
                                 int GH, int GW, uint64_t* keys, int32_t* hits, void* stream) {
  using namespace lea;
  clear_error();
  const char* who = "lea_dsm_splat_f32";
  LEA_CHECK_ARG(points, "%s: points is null", who);
  LEA_CHECK_ARG(G, "%s: G is null", who);
  LEA_CHECK_ARG(keys, "%s: keys is null", who);
  if (int rc = dsm_check_grid(who, B, GH, GW)) return rc;
  LEA_CHECK_ARG(rows > 0, "%s: rows %d is not positive", who, rows);
  LEA_CHECK_ARG((long long)B * rows <= 0x7fffffffLL, "%s: B*rows = %lld*%lld is above 2^31 - 1", who, (long long)B,
                (long long)rows);
  LEA_CHECK_ARG(row_width >= 0 && row_width <= rows, "%s: row_width %d is outside 0 .. rows = %d", who, row_width,
                rows);
  LEA_CHECK_ARG(g_bstride == 0 || g_bstride >= 12, "%s: G batch stride %lld is neither 0 nor >= 12", who,
                (long long)g_bstride);
  LEA_CHECK_ARG(radius >= 0.f && radius <= (float)LEA_DSM_MAX_RADIUS, "%s: radius %g is outside 0 .. %d", who,
                (double)radius, LEA_DSM_MAX_RADIUS);
  LEA_CHECK_ARG(staging >= LEA_DSM_STAGING_AUTO && staging <= LEA_DSM_STAGING_LDS,
                "%s: staging %d is not 0 (auto), 1 (global) or 2 (LDS)", who, staging);
  LEA_CHECK_ARG(((uintptr_t)keys & 7) == 0, "%s: keys must be 8-byte aligned", who);
  LEA_CHECK_ARG(((uintptr_t)points & 3) == 0 && ((uintptr_t)G & 3) == 0 && ((uintptr_t)count & 3) == 0 &&
                    ((uintptr_t)hits & 3) == 0,
                "%s: points, G, count and hits must be 4-byte aligned", who);
  const size_t cells = (size_t)B * (size_t)GH * (size_t)GW, n = (size_t)B * (size_t)rows;
  {  // no output may overlap an input or the other output
    const void* ins[4] = {points, count, colours, G};
    const size_t inn[4] = {12 * n, 4 * (size_t)B, 3 * n, 4 * ((size_t)(B - 1) * (size_t)g_bstride + 12)};
    const char* inname[4] = {"points", "count", "colours", "G"};
    for (int i = 0; i < 4; ++i) {
      if (!ins[i]) continue;
      LEA_CHECK_ARG(!spans_overlap(keys, 8 * cells, ins[i], inn[i]), "%s: keys overlaps %s", who, inname[i]);
      LEA_CHECK_ARG(!hits || !spans_overlap(hits, 4 * cells, ins[i], inn[i]), "%s: hits overlaps %s", who,
                    inname[i]);
    }
    LEA_CHECK_ARG(!hits || !spans_overlap(hits, 4 * cells, keys, 8 * cells), "%s: hits overlaps keys", who);
  }
  long long nblk = ((long long)rows + kDsmBlk - 1) / kDsmBlk;
  int patches_x = 0;
  if (row_width > 0) {
    const long long height = ((long long)rows + row_width - 1) / row_width;
    patches_x = (row_width + kDsmPatch - 1) / kDsmPatch;
    nblk = (long long)patches_x * ((height + kDsmPatch - 1) / kDsmPatch);
  }
  const dim3 grid((unsigned)nblk, (unsigned)B);
  hipStream_t s = as_stream(stream);
  u64* k = reinterpret_cast<u64*>(keys);
  // auto: the staged form where it was measured not slower than the global one on model-like fields
  // (DESIGN.md "Surface model", profiles/dsm_probe.txt): patches of an image, not runs of rows
  const bool staged = staging == LEA_DSM_STAGING_LDS || (staging == LEA_DSM_STAGING_AUTO && row_width > 0);
  if (staged)
    dsm_splat<true><<<grid, kDsmThreads, 0, s>>>(points, count, colours, G, (long long)g_bstride, rows, row_width,
                                                 patches_x, radius, GH, GW, k, hits);
  else
    dsm_splat<false><<<grid, kDsmThreads, 0, s>>>(points, count, colours, G, (long long)g_bstride, rows, row_width,
                                                  patches_x, radius, GH, GW, k, hits);
  return launch_status(who);
}

extern "C" int lea_dsm_resolve_f32(const uint64_t* keys, const int32_t* hits, int B, int GH, int GW, int iterations,
                                   int min_neighbours, float nodata, void* workspace, float* height, uint8_t* rgb,
                                   int32_t* source, uint8_t* state, void* stream) {
  using namespace lea;
  clear_error();
  const char* who = "lea_dsm_resolve_f32";
  LEA_CHECK_ARG(keys, "%s: keys is null", who);
  LEA_CHECK_ARG(height || rgb || source || state, "%s: every output is null", who);
  LEA_CHECK_ARG(!(rgb && source), "%s: rgb and source are the two readings of one payload: at most one", who);
  if (int rc = dsm_check_grid(who, B, GH, GW)) return rc;
  LEA_CHECK_ARG(iterations >= 0 && iterations <= kDsmMaxFill, "%s: iterations %d is outside 0 .. %d", who, iterations,
                kDsmMaxFill);
  LEA_CHECK_ARG(min_neighbours >= 1 && min_neighbours <= 8, "%s: min_neighbours %d is outside 1 .. 8", who,
                min_neighbours);
  LEA_CHECK_ARG(iterations == 0 || workspace, "%s: workspace is null with fill passes", who);
  LEA_CHECK_ARG(((uintptr_t)keys & 7) == 0 && ((uintptr_t)workspace & 7) == 0,
                "%s: keys and the workspace must be 8-byte aligned", who);
  LEA_CHECK_ARG(((uintptr_t)height & 3) == 0 && ((uintptr_t)source & 3) == 0 && ((uintptr_t)hits & 3) == 0,
                "%s: height, source and hits must be 4-byte aligned", who);
  const size_t cells = (size_t)B * (size_t)GH * (size_t)GW;
  const size_t wsn = workspace ? lea_dsm_resolve_workspace_bytes(B, GH, GW) : 0;
  {  // no output may overlap an input, the workspace or another output
    const void* ins[3] = {keys, hits, workspace};
    const size_t inn[3] = {8 * cells, 4 * cells, wsn};
    const char* inname[3] = {"keys", "hits", "the workspace"};
    const void* outs[4] = {height, rgb, source, state};
    const size_t outn[4] = {4 * cells, 3 * cells, 4 * cells, cells};
    const char* outname[4] = {"height", "rgb", "source", "state"};
    for (int o = 0; o < 4; ++o) {
      if (!outs[o]) continue;
      for (int i = 0; i < 3; ++i)
        LEA_CHECK_ARG(!ins[i] || !spans_overlap(outs[o], outn[o], ins[i], inn[i]), "%s: %s overlaps %s", who,
                      outname[o], inname[i]);
      for (int q = 0; q < o; ++q)
        LEA_CHECK_ARG(!outs[q] || !spans_overlap(outs[o], outn[o], outs[q], outn[q]), "%s: %s overlaps %s", who,
                      outname[o], outname[q]);
    }
    for (int i = 0; i < 2; ++i)
      LEA_CHECK_ARG(!workspace || !ins[i] || !spans_overlap(workspace, wsn, ins[i], inn[i]),
                    "%s: the workspace overlaps %s", who, inname[i]);
  }
  const long long per = (long long)GH * GW;
  const dim3 grid((unsigned)((per + kDsmThreads - 1) / kDsmThreads), (unsigned)B);
  hipStream_t s = as_stream(stream);
  const u64* cur = reinterpret_cast<const u64*>(keys);
  u64* buf[2] = {static_cast<u64*>(workspace), static_cast<u64*>(workspace) + (workspace ? cells : 0)};
  for (int t = 0; t < iterations; ++t) {
    dsm_fill<<<grid, kDsmThreads, 0, s>>>(cur, buf[t & 1], GH, GW, min_neighbours);
    if (int rc = launch_status("lea_dsm_resolve_f32 (fill)")) return rc;
    cur = buf[t & 1];
  }
  dsm_decode<<<grid, kDsmThreads, 0, s>>>(reinterpret_cast<const u64*>(keys), cur, per, nodata, height, rgb, source,
                                          state);
  return launch_status("lea_dsm_resolve_f32 (decode)");
}

extern "C" int lea_dsm_clear(uint64_t* keys, int32_t* hits, int B, int GH, int GW, void* stream) {
  using namespace lea;
  clear_error();
  const char* who = "lea_dsm_clear";
  LEA_CHECK_ARG(keys, "%s: keys is null", who);
  if (int rc = dsm_check_grid(who, B, GH, GW)) return rc;
  LEA_CHECK_ARG(((uintptr_t)keys & 7) == 0 && ((uintptr_t)hits & 3) == 0,
                "%s: keys must be 8-byte and hits 4-byte aligned", who);
  const size_t cells = (size_t)B * (size_t)GH * (size_t)GW;
  LEA_CHECK_ARG(!hits || !spans_overlap(hits, 4 * cells, keys, 8 * cells), "%s: hits overlaps keys", who);
  const unsigned nblk = (unsigned)((cells + kDsmThreads - 1) / kDsmThreads);
  dsm_zero<<<nblk, kDsmThreads, 0, as_stream(stream)>>>(reinterpret_cast<lea::u64*>(keys), hits, (long long)cells);
  return launch_status(who);
}
