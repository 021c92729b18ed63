// Exact 5x5 median filter of a [B, H, W] f32 map, once or twice over, in one launch.
//
// y = median5x5(x) (iterations = 1) or median5x5(median5x5(x)) (iterations = 2): the 13th of
// the 25 window values, the border replicated -- OpenCV's medianBlur, whose documentation
// states BORDER_REPLICATE (cv2 is not available to this project's tests; scipy's
// median_filter(size=5, mode="nearest") and a sort on an edge-padded array are the judges).
// The second pass replicates the FIRST PASS'S OUTPUTS at the border; that is not the median
// of the input replicated four wide.  Inputs are NaN-free by contract (min/max would drop a
// NaN rather than order it); +-inf is an ordinary value.
//
// A workgroup of 256 owns a 32 x 16 tile.  It stages the tile plus a halo of 2 per pass in
// LDS with the coordinates clamped to the image (40 x 24 floats for two passes).  For two
// passes it then writes the first medians of the tile plus 2 (36 x 20) into LDS -- a
// position outside the image takes the first median AT THE CLAMPED COORDINATE, whose window
// the staged region always holds -- and takes the second median from there.  Every median is
// median25 (median_net.h) on 25 registers read from LDS: lanes read consecutive dwords of a
// row, so the layout is row-contiguous and free of bank conflicts beyond a row's wrap.
#include "common.h"
#include "median_net.h"

namespace lea {

constexpr int kMedTW = 32, kMedTH = 16, kMedThreads = 256;

__device__ __forceinline__ float med_window(const float* __restrict__ s, const int stride) {
  float w[25];
#pragma unroll
  for (int dy = 0; dy < 5; ++dy)
#pragma unroll
    for (int dx = 0; dx < 5; ++dx) w[dy * 5 + dx] = s[dy * stride + dx];
  return median25(w);
}

template <int ITER>
__global__ __launch_bounds__(kMedThreads) void median5x5_kernel(const float* __restrict__ x, long long x_bstride,
                                                                float* __restrict__ y, long long y_bstride, int H,
                                                                int W) {
  constexpr int HALO = 2 * ITER;
  constexpr int SW = kMedTW + 2 * HALO, SH = kMedTH + 2 * HALO;
  constexpr int IW = kMedTW + 4, IH = kMedTH + 4;
  __shared__ float S[SH * SW];
  __shared__ float I[ITER == 2 ? IH * IW : 1];
  const int tid = threadIdx.x;
  const int tx0 = blockIdx.x * kMedTW, ty0 = blockIdx.y * kMedTH;
  const float* xb = x + (long long)blockIdx.z * x_bstride;
  float* yb = y + (long long)blockIdx.z * y_bstride;

  for (int idx = tid; idx < SH * SW; idx += kMedThreads) {
    const int sy = idx / SW, sx = idx - sy * SW;
    const int gy = min(max(ty0 - HALO + sy, 0), H - 1), gx = min(max(tx0 - HALO + sx, 0), W - 1);
    S[idx] = xb[(long long)gy * W + gx];
  }
  __syncthreads();

  if constexpr (ITER == 2) {
#pragma unroll 1
    for (int idx = tid; idx < IH * IW; idx += kMedThreads) {
      const int iy = idx / IW, ix = idx - iy * IW;
      // the position's clamped image coordinate, in the coordinates of I (origin: tile - 2);
      // S's origin is tile - 4, so the window of I-coordinate c starts at S-coordinate c
      const int cy = min(max(ty0 - 2 + iy, 0), H - 1) - (ty0 - 2);
      const int cx = min(max(tx0 - 2 + ix, 0), W - 1) - (tx0 - 2);
      I[idx] = med_window(S + cy * SW + cx, SW);
    }
    __syncthreads();
  }
#pragma unroll 1
  for (int idx = tid; idx < kMedTH * kMedTW; idx += kMedThreads) {
    const int oy = idx / kMedTW, ox = idx - oy * kMedTW;
    const int gy = ty0 + oy, gx = tx0 + ox;
    if (gy < H && gx < W)
      yb[(long long)gy * W + gx] = ITER == 2 ? med_window(I + oy * IW + ox, IW) : med_window(S + oy * SW + ox, SW);
  }
}

}  // namespace lea

extern "C" int lea_median5x5_f32(const float* x, int64_t x_bstride, float* y, int64_t y_bstride, int B, int H, int W,
                                 int iterations, void* stream) {
  using namespace lea;
  clear_error();
  LEA_CHECK_ARG(x && y, "lea_median5x5_f32: null pointer");
  LEA_CHECK_ARG(B > 0 && H > 0 && W > 0, "lea_median5x5_f32: bad shape B=%d H=%d W=%d", B, H, W);
  LEA_CHECK_ARG(iterations == 1 || iterations == 2, "lea_median5x5_f32: iterations %d is not 1 or 2", iterations);
  const long long hw = (long long)H * W;
  LEA_CHECK_ARG(x_bstride >= hw && y_bstride >= hw,
                "lea_median5x5_f32: batch stride below H*W (x %lld, y %lld, H*W %lld)", (long long)x_bstride,
                (long long)y_bstride, hw);
  const unsigned gx = (unsigned)((W + kMedTW - 1) / kMedTW), gy = (unsigned)((H + kMedTH - 1) / kMedTH);
  LEA_CHECK_ARG(B <= 65535 && gy <= 65535, "lea_median5x5_f32: grid too large");
  {  // y may not overlap x
    const uintptr_t xa = (uintptr_t)x, ya = (uintptr_t)y;
    const uintptr_t xn = 4 * ((uintptr_t)(B - 1) * (uintptr_t)x_bstride + (uintptr_t)hw);
    const uintptr_t yn = 4 * ((uintptr_t)(B - 1) * (uintptr_t)y_bstride + (uintptr_t)hw);
    LEA_CHECK_ARG(xa + xn <= ya || ya + yn <= xa, "lea_median5x5_f32: y overlaps x");
  }
  const dim3 grid(gx, gy, (unsigned)B);
  if (iterations == 2)
    median5x5_kernel<2><<<grid, kMedThreads, 0, as_stream(stream)>>>(x, x_bstride, y, y_bstride, H, W);
  else
    median5x5_kernel<1><<<grid, kMedThreads, 0, as_stream(stream)>>>(x, x_bstride, y, y_bstride, H, W);
  return launch_status("lea_median5x5_f32");
}
