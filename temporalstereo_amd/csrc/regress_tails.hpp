// Per-pixel arithmetic of the regression tails (K4a top-k soft-argmax, K5 9-tap upsamplers), shared by the stand-alone kernels
// (regress.hip, pyramid_ops.hip) and the fused ones (regress.hip: regression + convex upsampling; conv_x6s.hip: 4x4 deconvolution +
// UNet upsampling).  A fused kernel must reproduce the two launches it replaces BIT FOR BIT, so each expression exists once, here:
// -ffp-contract=on contracts within a statement, so the same statement gives the same instructions at every call site.
#pragma once
#include <hip/hip_runtime.h>

namespace ts_tail {

// source index / weight of torch's align_corners=True linear interpolation
__device__ __forceinline__ void lin_src(float scale, int dst, int in_size, int& i0, int& i1, float& l1) {
  const float s = scale * static_cast<float>(dst);
  i0 = static_cast<int>(s);
  i1 = i0 + ((i0 < in_size - 1) ? 1 : 0);
  l1 = s - static_cast<float>(i0);
}

// ---------------------------------------------------------------------------------------- K4a
// Top-k soft-argmax of one pixel: cost / samp / off point at the pixel's first candidate, planes are HW apart.
// Out: bc / bi the k best costs (descending; ties: lowest index first) and their indices, td = (sample + offset) of each.
template <int K>
__device__ __forceinline__ float topk_softargmax_pixel(const float* __restrict__ cost, const float* __restrict__ samp,
                                                       const float* __restrict__ off, int D, int HW, float (&bc)[K], int (&bi)[K],
                                                       float (&td)[K]) {
#pragma unroll
  for (int j = 0; j < K; ++j) { bc[j] = -INFINITY; bi[j] = -1; }
  // eight candidates requested at a time (clamped index: unconditional loads), then inserted in order -- a
  // load-per-iteration loop serialises D global round trips on the small levels
  for (int d0 = 0; d0 < D; d0 += 8) {
    float cc[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) cc[u] = cost[static_cast<size_t>(min(d0 + u, D - 1)) * HW];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      float c = cc[u];
      int ci = d0 + u;
      const bool real = ci < D;
      // insertion into the descending list; strict '>' keeps the lowest index first among ties
#pragma unroll
      for (int j = 0; j < K; ++j) {
        const bool take = real && ((c > bc[j]) || (bi[j] < 0));
        const float tc = bc[j];
        const int ti = bi[j];
        if (take) { bc[j] = c; bi[j] = ci; c = tc; ci = ti; }
      }
    }
  }
  // softmax over the k kept costs (bc[0] is the maximum)
  float w[K], den = 0.f;
#pragma unroll
  for (int j = 0; j < K; ++j) { w[j] = expf(bc[j] - bc[0]); den += w[j]; }
  float acc = 0.f;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const size_t o = static_cast<size_t>(bi[j]) * HW;
    td[j] = samp[o] + off[o];
    acc += (w[j] / den) * td[j];
  }
  return acc;
}

// ---------------------------------------------------------------------------------------- ConvexUpsample
// The nine logits of one output pixel (planes `kstride` apart) and their maximum.
__device__ __forceinline__ float convex_logits(const float* __restrict__ mp, size_t kstride, float (&m)[9]) {
  float mx = -INFINITY;
#pragma unroll
  for (int k = 0; k < 9; ++k) { m[k] = mp[static_cast<size_t>(k) * kstride]; mx = fmaxf(mx, m[k]); }
  return mx;
}

// softmax(m) . taps; tap(k) = the scaled disparity under tap k (row k / 3 - 1, column k % 3 - 1), zero outside the map
template <class Tap>
__device__ __forceinline__ float convex_combine(const float (&m)[9], float mx, Tap tap) {
  float den = 0.f, acc = 0.f;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const float e = expf(m[k] - mx);
    den += e;
    const float v = tap(k);
    acc += e * v;
  }
  return acc / den;
}

// zero padding by select: dv is whatever an unconditional (clamped) read returned
__device__ __forceinline__ float convex_tap_value(float dv, bool inside, float disp_scale) { return inside ? dv * disp_scale : 0.f; }

// the next level's search range and candidates from the upsampled value (range_candidates_kernel); c: the pixel in the first plane
__device__ __forceinline__ void convex_store_range(float dup, float range, float* __restrict__ low, float* __restrict__ high,
                                                   float* __restrict__ c, size_t HWo) {
  const float lo = dup - range, hi = dup + range;
  *low = lo; *high = hi;
  const float span = fabsf(hi - lo), base = fminf(lo, hi);
  c[0] = span * 0.f + base;
  c[HWo] = span * 0.375f + base;
  c[2 * HWo] = span * 0.5f + base;
  c[3 * HWo] = span * 0.625f + base;
  c[4 * HWo] = span * 1.f + base;
}

// ---------------------------------------------------------------------------------------- UNet.upsample
// One element of the 4x4 disparity patch around (y0, x0): disp * w_out / w_in in the reference's evaluation order
// (module.py:478); zero padding of unfold.  The read is unconditional (clamped).
__device__ __forceinline__ float unet_patch_value(const float* __restrict__ dp, int yy, int xx, int h, int w, int Wo) {
  const float dv = dp[min(max(yy, 0), h - 1) * w + min(max(xx, 0), w - 1)];
  return (yy >= 0 && yy < h && xx >= 0 && xx < w) ? dv * static_cast<float>(Wo) / static_cast<float>(w) : 0.f;
}

// softmax over the nine logits of one output pixel times the bilinear samples of the nine shifted maps: pd[r][c] is the patch
// element (y0 - 1 + r, x0 - 1 + c); ix / iy: the pixel has a second source column / row.
__device__ __forceinline__ float unet_combine(const float (&m)[9], const float (&pd)[4][4], float lx, float ly, bool ix, bool iy) {
  float mx = -INFINITY;
#pragma unroll
  for (int k = 0; k < 9; ++k) mx = fmaxf(mx, m[k]);
  float den = 0.f, acc = 0.f;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const float e = expf(m[k] - mx);
    den += e;
    const int ry = k / 3, rx = k % 3;            // patch row / column of (y0 + dy, x0 + dx)
    const float a00 = pd[ry][rx];
    const float a01 = ix ? pd[ry][rx + 1] : a00;
    const float a10 = iy ? pd[ry + 1][rx] : a00;
    const float a11 = iy ? (ix ? pd[ry + 1][rx + 1] : pd[ry + 1][rx]) : a01;
    const float top = (1.f - lx) * a00 + lx * a01;
    const float bot = (1.f - lx) * a10 + lx * a11;
    acc += e * ((1.f - ly) * top + ly * bot);
  }
  return acc / den;
}

// ---------------------------------------------------------------------------------------- bilinear resize
// align_corners bilinear sample from the four corner values (row y0 | y1, column xa | xb), times vscale
__device__ __forceinline__ float bilinear_value(float v00, float v01, float v10, float v11, float ly, float lx, float vscale) {
  const float top = (1.f - lx) * v00 + lx * v01;
  const float bot = (1.f - lx) * v10 + lx * v11;
  return ((1.f - ly) * top + ly * bot) * vscale;
}

}  // namespace ts_tail
