// The fast sigmoid of every epilogue and element kernel, and what is built on it: sigmoid_fast, silu_fast, tanh_fast.
//
// 1 / (1 + e^-v) on v_exp_f32 and v_rcp_f32 (1 ulp each) with one Newton step on the reciprocal, instead of the library's expf and an
// IEEE division: 8 instructions per value instead of ~30-40.  A convolution lane finishes 16-32 values with nothing left to hide them
// -- 4.5 k of a 7 k-cycle epilogue in the x6 kernels (tools/exp/x6p_trace.py), 1-2 us of every launch-bound layer of the pyramid, 6.7 us
// of the 13.9 us bn_finish_apply_act_kernel took on a 32 x 272 x 480 layer (and of every backward kernel's, which evaluates it again
// for the derivative).  |error| ~1.5 ulp of the result, the class of the exact form (the unrefined reciprocal's extra ulp was enough to
// move one more near-tie of a temporal sequence in tests/test_fullsize_gpu.py's audit); the e^-v argument's rounding (|v| 2^-24
// relative: |v| 6e-8 of e^-v) only meets results that are themselves ~e^-|v|.
// The ends of the range: below v = -88.7 e^-v is inf, the reciprocal 0 and the Newton step would be inf * 0 -- the unrefined 0 is kept
// there (silu: v * 0 = -0, as the exact form's v / inf).  d >= 1 and the refined quotient is one rounding of r (2 - d r) <= 1 / d, so
// the sigmoid lies in [0, 1].  NaN stays NaN.  (tests/test_conv_x6_gpu.py::test_silu_epilogue_at_the_ends_of_the_range)
// TS_EXACT_SILU (compile-time, a lab flag) restores the library forms of sigmoid_fast and silu_fast in every kernel that uses them,
// the ConvGRU's gates included; tanh_fast has one form.
#pragma once
#include <hip/hip_runtime.h>

namespace {

__device__ __forceinline__ float rcp_newton(float d) {
  const float r = __builtin_amdgcn_rcpf(d);
  return fmaf(fmaf(-d, r, 1.f), r, r);          // one Newton step: the quotient to ~0.5 ulp, as the IEEE division's
}

__device__ __forceinline__ float sigmoid_fast(float v) {
#ifdef TS_EXACT_SILU
  return 1.f / (1.f + expf(-v));
#else
  const float d = 1.f + __builtin_amdgcn_exp2f(v * -1.4426950408889634f);
  const float r = __builtin_amdgcn_rcpf(d);
  const float rn = fmaf(fmaf(-d, r, 1.f), r, r);
  return d < 3.0e38f ? rn : r;
#endif
}

__device__ __forceinline__ float silu_fast(float v) {
#ifdef TS_EXACT_SILU
  return v / (1.f + expf(-v));
#else
  return v * sigmoid_fast(v);
#endif
}

// tanh(v) = sign(v) (1 - e) / (1 + e), e = e^(-2|v|) in [0, 1]: the denominator stays in [1, 2] (no overflow anywhere; 2|v| = inf gives
// e = 0), both factors are <= 1, so |result| <= 1.
__device__ __forceinline__ float tanh_fast(float v) {
  const float e = __builtin_amdgcn_exp2f(fabsf(v) * -2.8853900817779268f);
  return copysignf((1.f - e) * rcp_newton(1.f + e), v);
}

}  // namespace
