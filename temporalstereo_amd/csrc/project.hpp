// The rigid re-projection of the reference's project_to_3d (architecture/modeling/layers/inverse_warp.py:119-170), per pixel, in
// ONE place: ts_project_to_3d_fwd (softsplat.hip) and the depth mode of ts_inverse_warp_fwd / _bwd (inverse_warp.hip) call it, so
// the two can never disagree on a bit.  Every expression below is written exactly as it was in project_kernel: with
// -ffp-contract=on the compiler fuses multiply-adds per expression, so the text of an expression is part of its bits.
#pragma once
#include <hip/hip_runtime.h>

namespace ts {

struct Projection {
  float P[3][4];      // (new_K * T)[:3]: K identity-padded to 4x4 when it is 3x3  (:138-146)
  float iK[3][3];     // inv_K[:3, :3]
};

// Fills `pr` (in LDS) for batch element b; called by every lane of a workgroup of >= 25 lanes, ends in the barrier.
__device__ __forceinline__ void load_projection(Projection& pr, const float* __restrict__ K, const float* __restrict__ invK,
                                                const float* __restrict__ T, int b, int kdim, int ikdim) {
  if (threadIdx.x < 12) {
    const int r = threadIdx.x / 4, c = threadIdx.x % 4;
    float acc = 0.f;
    for (int k = 0; k < 4; ++k) {
      float kv;
      if (k < kdim && r < kdim) kv = K[(static_cast<size_t>(b) * kdim + r) * kdim + k];
      else kv = (r == k) ? 1.f : 0.f;
      acc += kv * T[(static_cast<size_t>(b) * 4 + k) * 4 + c];
    }
    pr.P[r][c] = acc;
  } else if (threadIdx.x >= 16 && threadIdx.x < 25) {
    const int j = threadIdx.x - 16;
    pr.iK[j / 3][j % 3] = invK[(static_cast<size_t>(b) * ikdim + j / 3) * ikdim + j % 3];
  }
  __syncthreads();
}

struct Projected {
  float X, Y, Z;      // the 3-D point inv_K * [u v 1]^T * depth          (homo_points_3d, :138)
  float cx, cy, cz;   // P * [X Y Z 1]^T; cz is triangular_depth           (:154-157)
  float sx, sy;       // src_pixel_coord = (cx, cy) / (cz + eps)           (:160)
};

__device__ __forceinline__ Projected project_pixel(const Projection& pr, float u, float v, float z, float eps) {
  Projected o;
  o.X = (pr.iK[0][0] * u + pr.iK[0][1] * v + pr.iK[0][2]) * z;
  o.Y = (pr.iK[1][0] * u + pr.iK[1][1] * v + pr.iK[1][2]) * z;
  o.Z = (pr.iK[2][0] * u + pr.iK[2][1] * v + pr.iK[2][2]) * z;
  o.cx = pr.P[0][0] * o.X + pr.P[0][1] * o.Y + pr.P[0][2] * o.Z + pr.P[0][3];
  o.cy = pr.P[1][0] * o.X + pr.P[1][1] * o.Y + pr.P[1][2] * o.Z + pr.P[1][3];
  o.cz = pr.P[2][0] * o.X + pr.P[2][1] * o.Y + pr.P[2][2] * o.Z + pr.P[2][3];
  o.sx = o.cx / (o.cz + eps);
  o.sy = o.cy / (o.cz + eps);
  return o;
}

// flow_mask of :165-166
__device__ __forceinline__ bool projected_inside(float sx, float sy, int H, int W) {
  return (sx >= 0.f) & (sx <= static_cast<float>(W - 1)) & (sy >= 0.f) & (sy <= static_cast<float>(H - 1));
}

// d(sx, sy) / d depth: with s = depth * a + t, a = P[:, :3] * inv_K * [u v 1]^T, t = P[:, 3]:
//   d sx / d depth = (a_x * (s_z + eps) - s_x * a_z) / (s_z + eps)^2, likewise for y.  K, inv_K and T are constants.
__device__ __forceinline__ void project_pixel_ddepth(const Projection& pr, float u, float v, const Projected& o, float eps,
                                                     float& dsx, float& dsy) {
  const float rx = pr.iK[0][0] * u + pr.iK[0][1] * v + pr.iK[0][2];
  const float ry = pr.iK[1][0] * u + pr.iK[1][1] * v + pr.iK[1][2];
  const float rz = pr.iK[2][0] * u + pr.iK[2][1] * v + pr.iK[2][2];
  const float ax = pr.P[0][0] * rx + pr.P[0][1] * ry + pr.P[0][2] * rz;
  const float ay = pr.P[1][0] * rx + pr.P[1][1] * ry + pr.P[1][2] * rz;
  const float az = pr.P[2][0] * rx + pr.P[2][1] * ry + pr.P[2][2] * rz;
  const float den = o.cz + eps;
  dsx = (ax * den - o.cx * az) / (den * den);
  dsy = (ay * den - o.cy * az) / (den * den);
}

}  // namespace ts
