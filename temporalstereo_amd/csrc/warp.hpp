// The warp coordinate of the reference, in ONE place: the cost volume (block_cost.hip: forward taps, the backward kernels, the dense
// siblings) and the warp-free first layer (conv3d.hip: warp_gather_kernel) must put every tap at the same position, bit for bit.
#pragma once
#include <hip/hip_runtime.h>

namespace ts {

// Source POSITION of output pixel x for candidate value dispv, sampled at x - dispv: the reference's float sequence -- normalise to
// [-1, 1] (inverse_warp_3d.py:41-47) and back (grid_sample, align_corners=True) -- so that a tap rounds as it does there.  xs / Wm1
// is a true division: it decides how a tap near an integer rounds.  Wm1 = float(W - 1).  The clamp to [-2, W + 1] keeps the
// conversion to int defined; every position it moves is outside the row on both taps either way.  Column and fraction are a floor away.
__device__ __forceinline__ float source_position(int x, float dispv, int W, float Wm1) {
  const float xs = static_cast<float>(x) + (-dispv);
  const float gx = (xs / Wm1 * 2.f) - 1.f;
  const float ix = ((gx + 1.f) / 2.f) * Wm1;
  return fminf(fmaxf(ix, -2.f), static_cast<float>(W) + 1.f);
}

// The 2-D form of the same round trip, for the 2-D inverse_warp (layers/inverse_warp.py:67-72; inverse_warp.hip): a source
// coordinate X in pixels of the MOTION map (n = its W or H) to the position grid_sample (align_corners=True) samples in an image of
// ni columns or rows:  g = (2 * X) / (n - 1) - 1, then ((g + 1) / 2) * (ni - 1).  Every step is rounded on its own (no fused
// multiply-add can form), in the order the framework takes them.  No clamp here: the padding mode comes first (warp_pad below).
__device__ __forceinline__ float source_position_2d(float X, float nm1, float nim1) {
  const float g = __fsub_rn(__fdiv_rn(__fmul_rn(2.f, X), nm1), 1.f);
  return __fmul_rn(__fdiv_rn(__fadd_rn(g, 1.f), 2.f), nim1);
}

enum WarpPad { kPadZeros = 0, kPadBorder = 1, kPadReflection = 2 };

// grid_sample's padding of a position over [0, nim1] (align_corners=True): border clips; reflection reflects as often as needed,
// then clips.  `mult` is d(result) / d(position): 0 where the clip moved it, -1 after an odd number of reflections, else 1.
// The last line keeps every later conversion to int defined (a non-finite position lands on -2, outside on both taps): under
// zeros it moves only positions whose taps are all outside either way, under the other two modes it moves nothing finite.
template <int PAD>
__device__ __forceinline__ float warp_pad(float p, float nim1, float& mult) {
  mult = 1.f;
  if (PAD == kPadReflection) {
    const float a = fabsf(p);
    const float extra = fmodf(a, nim1);
    const bool odd = fmodf(floorf(a / nim1), 2.f) == 1.f;
    mult = (p < 0.f) ? -1.f : 1.f;
    if (odd) { p = nim1 - extra; mult = -mult; }
    else p = extra;
  }
  if (PAD != kPadZeros) {
    if (!(p > 0.f)) { p = 0.f; mult = 0.f; }
    else if (p >= nim1) { p = nim1; mult = 0.f; }
  }
  return fminf(fmaxf(p, -2.f), nim1 + 2.f);
}

}  // namespace ts
