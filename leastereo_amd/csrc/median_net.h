// Median of 25 floats by a fixed network of min/max pairs on registers (no data-dependent
// branch, no indexing by a run-time value).
//
// Forgetful selection: of any 14 of the 25 values neither the smallest nor the largest can
// be the median (13 others lie on one side of it), so both are dropped and the next value
// joins; of 13 out of the remaining 23 the same holds, and so on down to 3 of 3, whose
// middle is the answer.  drop_minmax<K> moves the minimum of v[0..K-1] to v[0] and the
// maximum to v[K-1]: K/2 exchanges split the values into a low and a high half, the minimum
// is then pulled through the low half and the maximum through the high half (an odd K's
// middle value takes part in both).  132 exchanges in all, 264 v_min/v_max.
// Ties and +-inf are ordinary values to min/max; NaN is excluded by the entry's contract.
#pragma once
#include <hip/hip_runtime.h>

namespace lea {

__host__ __device__ __forceinline__ void med_cx(float& a, float& b) {  // a <= b afterwards
  const float lo = __builtin_fminf(a, b), hi = __builtin_fmaxf(a, b);
  a = lo;
  b = hi;
}

template <int K>
__host__ __device__ __forceinline__ void drop_minmax(float (&v)[14]) {
  constexpr int h = K / 2;
#pragma unroll
  for (int i = 0; i < h; ++i) med_cx(v[i], v[K - 1 - i]);
  constexpr int low_end = (K & 1) ? h : h - 1;  // last index of the low half
#pragma unroll
  for (int i = 1; i <= low_end; ++i) med_cx(v[0], v[i]);
#pragma unroll
  for (int i = h; i < K - 1; ++i) med_cx(v[i], v[K - 1]);
}

template <int K>
struct Med25Step {
  static __host__ __device__ __forceinline__ float run(float (&v)[14], const float (&w)[25]) {
    drop_minmax<K>(v);
    v[0] = w[14 + (14 - K)];  // the next value takes the dropped minimum's place;
    return Med25Step<K - 1>::run(v, w);  // the maximum, at v[K - 1], falls out of the range
  }
};
template <>
struct Med25Step<3> {
  static __host__ __device__ __forceinline__ float run(float (&v)[14], const float (&)[25]) {
    drop_minmax<3>(v);
    return v[1];
  }
};

// the 13th smallest of w[0..24]
__host__ __device__ __forceinline__ float median25(const float (&w)[25]) {
  float v[14];
#pragma unroll
  for (int i = 0; i < 14; ++i) v[i] = w[i];
  return Med25Step<14>::run(v, w);
}

}  // namespace lea
