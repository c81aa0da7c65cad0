// torch's align_corners=True bilinear rescale of a disparity map, evaluated at one output pixel in registers: the arithmetic of
// ts_resize_bilinear_fwd (pyramid_ops.hip), shared by the kernels that read a low-resolution disparity at full resolution without
// writing the rescaled map (losses.hip: smooth-L1 on the wrapper's rescale; evaluation.hip: the validation metrics; render.hip;
// flow_frame.hip: each flow component through its strides).
// Same expressions as resize_bilinear_kernel, so the same contraction into fused multiply-adds and the same bits.
#pragma once
#include <hip/hip_runtime.h>

namespace ts {

// align_corners source of one output index: i0 / i1 and the weight of i1
__device__ __forceinline__ void lin_src(float scale, int dst, int in_size, int& i0, int& i1, float& l1) {
  const float s = scale * static_cast<float>(dst);
  i0 = static_cast<int>(s);
  i1 = i0 + ((i0 < in_size - 1) ? 1 : 0);
  l1 = s - static_cast<float>(i0);
}

// F.interpolate(e, bilinear, align_corners=True) at (oy, ox) of the full-size map, times vs; e is one [h, w] plane whose pixel
// (y, x) is e[y sy + x sx] (element strides: a dense plane has sy = w, sx = 1)
template <class Idx>
__device__ __forceinline__ float rescaled_at(const float* __restrict__ e, Idx sy, Idx sx, int h, int w, float sh, float sw, float vs,
                                             int oy, int ox) {
  int y0, y1, x0, x1;
  float ly, lx;
  lin_src(sh, oy, h, y0, y1, ly);
  lin_src(sw, ox, w, x0, x1, lx);
  const float top = (1.f - lx) * e[y0 * sy + x0 * sx] + lx * e[y0 * sy + x1 * sx];
  const float bot = (1.f - lx) * e[y1 * sy + x0 * sx] + lx * e[y1 * sy + x1 * sx];
  return ((1.f - ly) * top + ly * bot) * vs;
}

// the same of a dense plane
__device__ __forceinline__ float rescaled(const float* __restrict__ e, int h, int w, float sh, float sw, float vs, int oy, int ox) {
  return rescaled_at<int>(e, w, 1, h, w, sh, sw, vs, oy, ox);
}

// source step of an align_corners resize from in_size to out_size samples
inline float ac_scale(int in_size, int out_size) {
  return out_size > 1 ? static_cast<float>(in_size - 1) / static_cast<float>(out_size - 1) : 0.f;
}

}  // namespace ts
