// The edge-aware training loss on the device (reference: train.py:107-118 combined_loss and
// the validity mask, edge_detection.py:32-57,68-74 gradient_aware_loss2), forward sums and
// the gradient with respect to the prediction.
//
// pred, target, tsmooth (the twice-median target, lea_median5x5_f32): [B, H, W] f32.
//   m      = (target < maxdisp) & (target > 0.001)
//   d      = pred - target
//   Sx q   = (q02 - q00) + 2 (q12 - q10) + (q22 - q20)       3x3 cross-correlations at the
//   Sy q   = (q00 - q20) + 2 (q01 - q21) + (q02 - q22)       (H-2) x (W-2) valid positions
// Each response is a sum of pair differences, so a constant window gives exactly 0.
//
// Forward (edge_loss_partial_kernel, then reduce4.h's final kernel in the same call):
//   sums[0] = #m   sums[1] = sum_m smooth_l1(d), beta 1   sums[2] = sum_m |d|
//   sums[3] = sum over positions and batch of |Sx p| exp(-|Sx t~|) + |Sy p| exp(-|Sy t~|)
// per-pixel terms in f32 (expf), summed in float64: per thread, per wave by shuffles, per
// workgroup into the workspace, and the workgroups' partials by one workgroup in a fixed
// order.  No float atomics; the same inputs give the same bits.
//
// Backward (edge_loss_grad_kernel), gather form, one launch, no atomics:
//   dpred = g_d m clamp(d, -1, 1) / n
//         + g_e / (B (H-2)(W-2)) sum over the <= 9 positions covering the pixel of
//             sign(Sx p) exp(-|Sx t~|) Sx[ky][kx] + sign(Sy p) exp(-|Sy t~|) Sy[ky][kx]
// sign(0) = 0 (torch's abs backward).  n = sums[0] and (g_d, g_e) are read on the device.
// n == 0: the direct part is 0 (torch's mean over an empty selection would give NaN; the
// reference's train loop skips such a batch, train.py:152).
// A workgroup stages pred and tsmooth for its 64 x 16 tile plus a halo of 2, writes the two
// weighted sign fields of the tile plus 1 into LDS and gathers from them; again the sums
// are pair differences, so the edge part is exactly 0 where pred is constant all around.
#include "reduce4.h"

namespace lea {

constexpr int kElW = 64, kElH = 16, kElThreads = 256;
constexpr int kElRows = kElH / (kElThreads / kElW);  // rows per thread

__device__ __forceinline__ float sobel_x(const float* __restrict__ q, const int s) {
  return ((q[2] - q[0]) + 2.f * (q[s + 2] - q[s])) + (q[2 * s + 2] - q[2 * s]);
}
__device__ __forceinline__ float sobel_y(const float* __restrict__ q, const int s) {
  return ((q[0] - q[2 * s]) + 2.f * (q[1] - q[2 * s + 1])) + (q[2] - q[2 * s + 2]);
}

struct EdgeMaps {
  const float* pred;
  const float* target;
  const float* tsmooth;
  long long pbs, tbs, sbs;
  int H, W;
  float maxdisp;
};

// stage rows y0 .. y0 + SH - 1, columns x0 .. x0 + SW - 1 of a map; 0 outside the image
template <int SH, int SW>
__device__ __forceinline__ void stage_map(float* __restrict__ dst, const float* __restrict__ src, const int y0,
                                          const int x0, const int H, const int W) {
  for (int idx = threadIdx.x; idx < SH * SW; idx += kElThreads) {
    const int sy = idx / SW, sx = idx - sy * SW;
    const int gy = y0 + sy, gx = x0 + sx;
    dst[idx] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? src[(long long)gy * W + gx] : 0.f;
  }
}

__global__ __launch_bounds__(kElThreads) void edge_loss_partial_kernel(const EdgeMaps a,
                                                                       double* __restrict__ partial) {
  constexpr int SW = kElW + 2, SH = kElH + 2;
  __shared__ float P[SH * SW];
  __shared__ float T[SH * SW];
  __shared__ double red[kElThreads / kWave][4];
  const int tx0 = blockIdx.x * kElW, ty0 = blockIdx.y * kElH, b = blockIdx.z;
  stage_map<SH, SW>(P, a.pred + b * a.pbs, ty0, tx0, a.H, a.W);
  stage_map<SH, SW>(T, a.tsmooth + b * a.sbs, ty0, tx0, a.H, a.W);
  __syncthreads();
  const float* tg = a.target + b * a.tbs;
  const int ox = threadIdx.x % kElW, rg = threadIdx.x / kElW;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int r = 0; r < kElRows; ++r) {
    const int oy = rg * kElRows + r;
    const int gy = ty0 + oy, gx = tx0 + ox;
    if (gy < a.H && gx < a.W) {
      const float t = tg[(long long)gy * a.W + gx];
      const float d = P[oy * SW + ox] - t;
      const float ad = fabsf(d);
      const float sl = ad < 1.f ? 0.5f * d * d : ad - 0.5f;
      if (t < a.maxdisp && t > 0.001f) {
        acc[0] += 1.0;
        acc[1] += (double)sl;
        acc[2] += (double)ad;
      }
    }
    if (gy < a.H - 2 && gx < a.W - 2) {
      const float* p = P + oy * SW + ox;
      const float* t = T + oy * SW + ox;
      const float e = fabsf(sobel_x(p, SW)) * expf(-fabsf(sobel_x(t, SW))) +
                      fabsf(sobel_y(p, SW)) * expf(-fabsf(sobel_y(t, SW)));
      acc[3] += (double)e;
    }
  }
  reduce4_block<kElThreads>(acc, red, partial);
}

__global__ __launch_bounds__(kElThreads) void edge_loss_grad_kernel(const EdgeMaps a, const double* __restrict__ sums,
                                                                    const float* __restrict__ scales,
                                                                    float* __restrict__ dpred, long long dbs,
                                                                    double inv_positions) {
  constexpr int SW = kElW + 4, SH = kElH + 4;  // staged pixels, origin tile - 2
  constexpr int FW = kElW + 2, FH = kElH + 2;  // fields, origin tile - 2 (top-left anchored positions)
  __shared__ float P[SH * SW];
  __shared__ float T[SH * SW];
  __shared__ float FX[FH * FW];
  __shared__ float FY[FH * FW];
  const int tx0 = blockIdx.x * kElW, ty0 = blockIdx.y * kElH, b = blockIdx.z;
  stage_map<SH, SW>(P, a.pred + b * a.pbs, ty0 - 2, tx0 - 2, a.H, a.W);
  stage_map<SH, SW>(T, a.tsmooth + b * a.sbs, ty0 - 2, tx0 - 2, a.H, a.W);
  __syncthreads();
  for (int idx = threadIdx.x; idx < FH * FW; idx += kElThreads) {
    const int fy = idx / FW, fx = idx - fy * FW;
    const int py = ty0 - 2 + fy, px = tx0 - 2 + fx;
    float vx = 0.f, vy = 0.f;
    if (py >= 0 && py < a.H - 2 && px >= 0 && px < a.W - 2) {
      const float* p = P + fy * SW + fx;
      const float* t = T + fy * SW + fx;
      const float sxp = sobel_x(p, SW), syp = sobel_y(p, SW);
      vx = (float)((sxp > 0.f) - (sxp < 0.f)) * expf(-fabsf(sobel_x(t, SW)));
      vy = (float)((syp > 0.f) - (syp < 0.f)) * expf(-fabsf(sobel_y(t, SW)));
    }
    FX[idx] = vx;
    FY[idx] = vy;
  }
  __syncthreads();
  const double n = sums[0];
  const float scale_d = n > 0.0 ? (float)((double)scales[0] / n) : 0.f;
  const float scale_e = (float)((double)scales[1] * inv_positions);
  const float* tg = a.target + b * a.tbs;
  float* out = dpred + b * dbs;
  const int ox = threadIdx.x % kElW, rg = threadIdx.x / kElW;
#pragma unroll
  for (int r = 0; r < kElRows; ++r) {
    const int oy = rg * kElRows + r;
    const int gy = ty0 + oy, gx = tx0 + ox;
    if (gy >= a.H || gx >= a.W) continue;
    const float t = tg[(long long)gy * a.W + gx];
    const float d = P[(oy + 2) * SW + ox + 2] - t;
    const bool m = t < a.maxdisp && t > 0.001f;
    const float direct = m ? fminf(fmaxf(d, -1.f), 1.f) * scale_d : 0.f;
    // pixel (y, x) is tap (ky, kx) of position (y - ky, x - kx): field row oy + 2 - ky, column ox + 2 - kx
    const float* fx = FX + oy * FW + ox;
    const float* fy = FY + oy * FW + ox;
    const float ex = ((fx[2 * FW] - fx[2 * FW + 2]) + 2.f * (fx[FW] - fx[FW + 2])) + (fx[0] - fx[2]);
    const float ey = ((fy[2 * FW + 2] - fy[2]) + 2.f * (fy[2 * FW + 1] - fy[1])) + (fy[2 * FW] - fy[0]);
    out[(long long)gy * a.W + gx] = direct + (ex + ey) * scale_e;
  }
}

static long long edge_blocks(int B, int H, int W) {
  return (long long)B * ((H + kElH - 1) / kElH) * ((W + kElW - 1) / kElW);
}

// shared argument checks; 0 = fine
static int edge_check(const char* who, const float* pred, int64_t pbs, const float* target, int64_t tbs,
                      const float* tsmooth, int64_t sbs, int B, int H, int W, float maxdisp) {
  LEA_CHECK_ARG(pred && target && tsmooth, "%s: null pointer", who);
  LEA_CHECK_ARG(B > 0 && H >= 3 && W >= 3, "%s: bad shape B=%d H=%d W=%d (H, W >= 3)", who, B, H, W);
  const long long hw = (long long)H * W;
  LEA_CHECK_ARG(pbs >= hw && tbs >= hw && sbs >= hw, "%s: batch stride below H*W", who);
  LEA_CHECK_ARG(maxdisp == maxdisp, "%s: maxdisp is NaN", who);
  LEA_CHECK_ARG(B <= 65535 && (H + kElH - 1) / kElH <= 65535, "%s: grid too large", who);
  return LEA_OK;
}

}  // namespace lea

extern "C" size_t lea_edge_loss_workspace_bytes(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  return (size_t)lea::edge_blocks(B, H, W) * 4 * sizeof(double);
}

extern "C" int lea_edge_loss_f32(const float* pred, int64_t pred_bstride, const float* target, int64_t target_bstride,
                                 const float* tsmooth, int64_t tsmooth_bstride, int B, int H, int W, float maxdisp,
                                 double* sums, void* workspace, void* stream) {
  using namespace lea;
  clear_error();
  const char* who = "lea_edge_loss_f32";
  if (int rc = edge_check(who, pred, pred_bstride, target, target_bstride, tsmooth, tsmooth_bstride, B, H, W, maxdisp))
    return rc;
  LEA_CHECK_ARG(sums && workspace, "%s: null sums or workspace", who);
  LEA_CHECK_ARG(((uintptr_t)sums & 7) == 0 && ((uintptr_t)workspace & 7) == 0,
                "%s: sums and workspace must be 8-byte aligned", who);
  const long long nblk = edge_blocks(B, H, W);
  LEA_CHECK_ARG(!spans_overlap(sums, 4 * sizeof(double), workspace, (size_t)nblk * 4 * sizeof(double)),
                "%s: sums overlaps the workspace", who);
  const EdgeMaps a{pred, target, tsmooth, pred_bstride, target_bstride, tsmooth_bstride, H, W, maxdisp};
  const dim3 grid((unsigned)((W + kElW - 1) / kElW), (unsigned)((H + kElH - 1) / kElH), (unsigned)B);
  double* partial = static_cast<double*>(workspace);
  edge_loss_partial_kernel<<<grid, kElThreads, 0, as_stream(stream)>>>(a, partial);
  if (int rc = launch_status(who)) return rc;
  reduce4_final_kernel<kElThreads><<<1, kElThreads, 0, as_stream(stream)>>>(partial, nblk, sums);
  return launch_status("lea_edge_loss_f32 (final)");
}

extern "C" int lea_edge_loss_grad_f32(const float* pred, int64_t pred_bstride, const float* target,
                                      int64_t target_bstride, const float* tsmooth, int64_t tsmooth_bstride,
                                      const double* sums, const float* scales, float* dpred, int64_t dpred_bstride,
                                      int B, int H, int W, float maxdisp, void* stream) {
  using namespace lea;
  clear_error();
  const char* who = "lea_edge_loss_grad_f32";
  if (int rc = edge_check(who, pred, pred_bstride, target, target_bstride, tsmooth, tsmooth_bstride, B, H, W, maxdisp))
    return rc;
  LEA_CHECK_ARG(sums && scales && dpred, "%s: null sums, scales or dpred", who);
  LEA_CHECK_ARG(((uintptr_t)sums & 7) == 0, "%s: sums must be 8-byte aligned", who);
  const long long hw = (long long)H * W;
  LEA_CHECK_ARG(dpred_bstride >= hw, "%s: batch stride below H*W", who);
  {
    const size_t dn = 4 * ((size_t)(B - 1) * (size_t)dpred_bstride + (size_t)hw);
    const void* in[3] = {pred, target, tsmooth};
    const int64_t bs[3] = {pred_bstride, target_bstride, tsmooth_bstride};
    for (int i = 0; i < 3; ++i)
      LEA_CHECK_ARG(!spans_overlap(dpred, dn, in[i], 4 * ((size_t)(B - 1) * (size_t)bs[i] + (size_t)hw)),
                    "%s: dpred overlaps input %d (0 = pred, 1 = target, 2 = tsmooth)", who, i);
    LEA_CHECK_ARG(!spans_overlap(dpred, dn, sums, 4 * sizeof(double)) &&
                      !spans_overlap(dpred, dn, scales, 2 * sizeof(float)),
                  "%s: dpred overlaps sums or scales", who);
  }
  const EdgeMaps a{pred, target, tsmooth, pred_bstride, target_bstride, tsmooth_bstride, H, W, maxdisp};
  const dim3 grid((unsigned)((W + kElW - 1) / kElW), (unsigned)((H + kElH - 1) / kElH), (unsigned)B);
  const double inv_positions = 1.0 / ((double)B * (double)(H - 2) * (double)(W - 2));
  edge_loss_grad_kernel<<<grid, kElThreads, 0, as_stream(stream)>>>(a, sums, scales, dpred, dpred_bstride,
                                                                    inv_positions);
  return launch_status(who);
}
