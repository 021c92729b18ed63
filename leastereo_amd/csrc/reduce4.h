// The deterministic sum of four float64 accumulators over a grid (edge_loss.hip's and
// photometric.hip's forward sums): per wave by shuffles, per workgroup by a serial sum over
// its waves into partial[blk * 4 + k], and the workgroups' partials by one workgroup in a
// fixed order.  No atomics: the same inputs give the same bits.
#pragma once
#include "common.h"

namespace lea {

// The block epilogue of a THREADS-wide workgroup: every thread calls it (a barrier inside).
// red: the workgroup's __shared__ scratch; blk = (z * gridDim.y + y) * gridDim.x + x.
template <int THREADS>
__device__ __forceinline__ void reduce4_block(double (&acc)[4], double (&red)[THREADS / kWave][4],
                                              double* __restrict__ partial) {
#pragma unroll
  for (int k = 0; k < 4; ++k)
    for (int o = kWave / 2; o > 0; o >>= 1) acc[k] += __shfl_down(acc[k], o);
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  if (lane == 0)
    for (int k = 0; k < 4; ++k) red[wave][k] = acc[k];
  __syncthreads();
  if (threadIdx.x < 4) {
    double s = 0.0;
    for (int w = 0; w < THREADS / kWave; ++w) s += red[w][threadIdx.x];
    const long long blk = ((long long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    partial[blk * 4 + threadIdx.x] = s;
  }
}

// one workgroup: thread t sums partials t, t + THREADS, ... in order, then a fixed tree
template <int THREADS>
__global__ __launch_bounds__(THREADS) void reduce4_final_kernel(const double* __restrict__ partial,
                                                                const long long nblk, double* __restrict__ sums) {
  __shared__ double red[THREADS][4];
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (long long i = threadIdx.x; i < nblk; i += THREADS)
    for (int k = 0; k < 4; ++k) acc[k] += partial[i * 4 + k];
  for (int k = 0; k < 4; ++k) red[threadIdx.x][k] = acc[k];
  __syncthreads();
  for (int o = THREADS / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o)
      for (int k = 0; k < 4; ++k) red[threadIdx.x][k] += red[threadIdx.x + o][k];
    __syncthreads();
  }
  if (threadIdx.x < 4) sums[threadIdx.x] = red[0][threadIdx.x];
}

}  // namespace lea
