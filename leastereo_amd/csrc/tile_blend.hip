// Whole-scene inference's blend ("Whole-scene inference"): the per-tile maps of
// a separable tile plan (tile k = ky * nx + kx at origin (ys[ky], xs[kx])) gathered into one
// scene-sized map.  One thread owns 4 consecutive output pixels of a row; nothing is
// scattered, so there are no float atomics and the result does not depend on the launch.
//
// Per axis (scene length S, tile length L, origin o, guards g0 / g1, ramp r) tile coordinate i
// has the integer weight
//   lo = o > 0, hi = o + L < S, a = lo ? g0 : 0, b = hi ? g1 : 0
//   w  = 0                                               for i < a or i >= L - b
//   w  = min(lo ? i - a + 1 : r, hi ? (L - b) - i : r, r) otherwise
// and a pixel's weight in a tile is the product wy * wx (<= 65536: exact in float32, as are
// sums of up to 256 of them).  Per output pixel, over the tiles of positive weight in
// ascending k:
//   exactly one -> its value is copied (most of a scene: bit-identical to the tile's forward)
//   several     -> (sum w * v) / (sum w), every product, add and the divide rounded once
//   none        -> 0, and the pixel is counted
// A tile is never read where its weight is 0, so whatever a guard band holds (a NaN
// included) cannot reach the result.  HBM-streaming: every read is a run of a tile row.
#include "common.h"

namespace lea {

constexpr int kBlendThreads = 256;
constexpr int kBlendMaxAxis = 64;

struct BlendArgs {
  const float* tiles;
  long long bstride;
  const int* ys;
  const int* xs;
  int ny, nx, th, tw;
  int gy0, gy1, gx0, gx1, ramp;
  float* out;
  int H, W;
  int* uncovered;
};

__device__ __forceinline__ int axis_weight(long long i, long long o, int L, int S, int g0, int g1, int ramp) {
  if (i < 0 || i >= L) return 0;
  const bool lo = o > 0, hi = o + L < S;
  const int a = lo ? g0 : 0, e = L - (hi ? g1 : 0);
  if (i < a || i >= e) return 0;
  int w = ramp;
  if (lo) w = min(w, (int)i - a + 1);
  if (hi) w = min(w, e - (int)i);
  return w;
}

// One IEEE operation each, rounded once.  Written out under `fp contract(off)` instead of
// __fmul_rn / __fadd_rn: those are plain operators inlined from a header compiled with
// contraction allowed, and the product and the add that follows were fused into one v_fma.
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}
__device__ __forceinline__ float div_rn(float a, float b) {
#pragma clang fp contract(off)
  return a / b;  // correctly rounded: the build does not relax float division
}

__global__ __launch_bounds__(256) void blend_clear_kernel(int* __restrict__ uncovered) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *uncovered = 0;
}

__global__ __launch_bounds__(kBlendThreads) void tile_blend_kernel(const BlendArgs a) {
  __shared__ int sy[kBlendMaxAxis], sx[kBlendMaxAxis];
  for (int e = threadIdx.x; e < a.ny; e += blockDim.x) sy[e] = a.ys[e];
  for (int e = threadIdx.x; e < a.nx; e += blockDim.x) sx[e] = a.xs[e];
  __syncthreads();
  const int qw = (a.W + 3) / 4;  // float4 columns per output row
  const long long quads = (long long)a.H * qw;
  int holes = 0;
  for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < quads;
       t += (long long)gridDim.x * blockDim.x) {
    const int Y = (int)(t / qw), X0 = (int)(t - (long long)Y * qw) * 4;
    // the rows and columns of tiles that reach this row and these 4 columns
    int ky0 = a.ny, ky1 = -1, kx0 = a.nx, kx1 = -1;
    for (int ky = 0; ky < a.ny; ++ky) {
      const long long d = (long long)Y - sy[ky];
      if (d >= 0 && d < a.th) {
        ky0 = min(ky0, ky);
        ky1 = ky;
      }
    }
    for (int kx = 0; kx < a.nx; ++kx) {
      const long long d = (long long)X0 - sx[kx];
      if (d > -4 && d < a.tw) {
        kx0 = min(kx0, kx);
        kx1 = kx;
      }
    }
    float num[4], den[4], one[4];
    int n[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 4; ++j) num[j] = den[j] = one[j] = 0.f;
    for (int ky = ky0; ky <= ky1; ++ky) {
      const long long iy = (long long)Y - sy[ky];
      const int wy = axis_weight(iy, sy[ky], a.th, a.H, a.gy0, a.gy1, a.ramp);
      if (wy == 0) continue;
      for (int kx = kx0; kx <= kx1; ++kx) {
        const float* row = a.tiles + ((long long)ky * a.nx + kx) * a.bstride + iy * a.tw;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const long long ix = (long long)X0 + j - sx[kx];
          const int wx = X0 + j < a.W ? axis_weight(ix, sx[kx], a.tw, a.W, a.gx0, a.gx1, a.ramp) : 0;
          if (wx == 0) continue;  // 0 <= ix < tw from here on
          const float v = row[ix];
          const float w = (float)(wy * wx);
          const float p = mul_rn(w, v);
          if (n[j] == 0) {
            one[j] = v;
            num[j] = p;
            den[j] = w;
          } else {
            num[j] = add_rn(num[j], p);
            den[j] = add_rn(den[j], w);
          }
          ++n[j];
        }
      }
    }
    float r[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      r[j] = n[j] == 0 ? 0.f : (n[j] == 1 ? one[j] : div_rn(num[j], den[j]));
      holes += (X0 + j < a.W) && n[j] == 0;
    }
    float* dst = a.out + (long long)Y * a.W + X0;
    if ((a.W & 3) == 0) {
      *reinterpret_cast<float4*>(dst) = make_float4(r[0], r[1], r[2], r[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (X0 + j < a.W) dst[j] = r[j];
    }
  }
  if (!a.uncovered) return;  // uniform over the grid
  // an integer count: order-free
  for (int o = kWave / 2; o > 0; o >>= 1) holes += __shfl_xor(holes, o);
  if ((threadIdx.x & (kWave - 1)) == 0 && holes) atomicAdd(a.uncovered, holes);
}

}  // namespace lea

extern "C" int lea_tile_blend_f32(const float* tiles, int64_t tile_bstride, const int* ys, int ny,
                                  const int* xs, int nx, int tile_h, int tile_w, int guard_y0, int guard_y1,
                                  int guard_x0, int guard_x1, int ramp, float* out, int H, int W,
                                  int* n_uncovered, void* stream) {
  using namespace lea;
  clear_error();
  LEA_CHECK_ARG(tiles && ys && xs && out, "lea_tile_blend_f32: null pointer");
  LEA_CHECK_ARG(ny > 0 && nx > 0 && ny <= kBlendMaxAxis && nx <= kBlendMaxAxis,
                "lea_tile_blend_f32: %d x %d tiles (1..%d per axis)", ny, nx, kBlendMaxAxis);
  LEA_CHECK_ARG(H > 0 && W > 0 && tile_h > 0 && tile_w > 0 && (long long)H * W < (1LL << 31) &&
                    (long long)tile_h * tile_w < (1LL << 31),
                "lea_tile_blend_f32: bad shape H=%d W=%d tile %dx%d", H, W, tile_h, tile_w);
  LEA_CHECK_ARG(tile_bstride >= (int64_t)tile_h * tile_w,
                "lea_tile_blend_f32: tile batch stride %lld below the tile's %lld elements",
                (long long)tile_bstride, (long long)tile_h * tile_w);
  LEA_CHECK_ARG(ramp >= 1 && ramp <= 256, "lea_tile_blend_f32: ramp %d (1..256)", ramp);
  LEA_CHECK_ARG(guard_y0 >= 0 && guard_y1 >= 0 && guard_x0 >= 0 && guard_x1 >= 0,
                "lea_tile_blend_f32: negative guard (%d, %d, %d, %d)", guard_y0, guard_y1, guard_x0, guard_x1);
  LEA_CHECK_ARG((const void*)tiles != (const void*)out, "lea_tile_blend_f32: out aliases tiles");
  // the kernel stores float4 when W % 4 == 0
  LEA_CHECK_ARG((((uintptr_t)tiles) & 3) == 0 && (((uintptr_t)out) & ((W & 3) == 0 ? 15 : 3)) == 0,
                "lea_tile_blend_f32: misaligned tiles or out (out 16-byte aligned when W %% 4 == 0)");
  LEA_CHECK_ARG(((((uintptr_t)ys) | ((uintptr_t)xs) | ((uintptr_t)n_uncovered)) & 3) == 0,
                "lea_tile_blend_f32: misaligned ys, xs or n_uncovered");
  hipStream_t st = as_stream(stream);
  if (n_uncovered) {
    // a launch and not a memset node, so that a captured call is kernels only
    blend_clear_kernel<<<1, 256, 0, st>>>(n_uncovered);
    int rc = launch_status("lea_tile_blend_f32 (clear)");
    if (rc) return rc;
  }
  BlendArgs a;
  a.tiles = tiles;
  a.bstride = tile_bstride;
  a.ys = ys;
  a.xs = xs;
  a.ny = ny;
  a.nx = nx;
  a.th = tile_h;
  a.tw = tile_w;
  a.gy0 = guard_y0;
  a.gy1 = guard_y1;
  a.gx0 = guard_x0;
  a.gx1 = guard_x1;
  a.ramp = ramp;
  a.out = out;
  a.H = H;
  a.W = W;
  a.uncovered = n_uncovered;
  const long long quads = (long long)H * ((W + 3) / 4);
  const int grid = (int)((quads + kBlendThreads - 1) / kBlendThreads);
  tile_blend_kernel<<<grid, kBlendThreads, 0, st>>>(a);
  return launch_status("lea_tile_blend_f32");
}
