// Wave reductions of the frame-side kernels (render.hip, evaluation.hip): ONE xor butterfly over the 64 lanes, offsets 32, 16, ..., 1,
// the result valid in every lane.  The order is part of the bits of the fp64 sums, so it is written once, here.
#pragma once
#include "ts_common.hpp"

namespace ts {

template <class T, class Op>
__device__ __forceinline__ T wave_reduce(T v, Op op) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, kWave));
  return v;
}

__device__ __forceinline__ float nan_max(float a, float b) {          // np.max: a NaN anywhere makes the maximum NaN
  return (a != a || b != b) ? __builtin_nanf("") : fmaxf(a, b);
}

template <class T>
__device__ __forceinline__ T wave_sum(T v) {
  return wave_reduce(v, [](T a, T b) { return a + b; });
}
__device__ __forceinline__ float wave_min(float v) {
  return wave_reduce(v, [](float a, float b) { return fminf(a, b); });
}
__device__ __forceinline__ float wave_max(float v) {
  return wave_reduce(v, [](float a, float b) { return fmaxf(a, b); });
}
__device__ __forceinline__ float wave_nan_max(float v) {
  return wave_reduce(v, [](float a, float b) { return nan_max(a, b); });
}

}  // namespace ts
