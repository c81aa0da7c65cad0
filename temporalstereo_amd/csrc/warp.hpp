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

}  // namespace ts
