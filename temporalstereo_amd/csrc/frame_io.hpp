// Byte, quad and row helpers shared by the frame-side kernels (preprocess.hip, augment.hip, render.hip, evaluation.hip), gfx950.
// These kernels are bit-exact against reference-made fixtures, so whatever decides a bit is written once, here:
//   ByteTables         byte / 255 and ((byte / 255) - mean[c]) / std[c], correctly rounded divisions, 1,024 floats in LDS
//   load_quad, store4  four horizontally adjacent pixels: 12 source bytes in, one 16-byte store per channel out
//   u16 quads          four 16-bit disparities in, raw / scale where raw > 0 and the mask raw > 0 out
//   load_row           V floats of a row
//   grid_blocks        the one ceil / cap / at-least-one rule of the grid sizes
//   frames_check_*     the argument checks ts_frames_prepare_fwd and ts_frames_augment_fwd have in common
// The device helpers hold no multiply-add pair, only explicitly rounded intrinsics and integer work, so a
// `#pragma clang fp contract(off)` before or after this include changes nothing.  Keep it that way: bilinear.hpp, whose
// contraction into fused multiply-adds is part of its bits, stays out of here.
#pragma once
#include "ts_common.hpp"

#include <initializer_list>

namespace ts {

struct ByteTables {
  float v[256];                 // byte / 255
  float n[3][256];              // (v - mean[c]) / std[c]
};

// called by all 256 lanes of the workgroup (one byte value per lane); ends in the barrier
__device__ __forceinline__ void build_byte_tables(const float (&mean)[3], const float (&sd)[3], ByteTables& t) {
  const int i = threadIdx.x;
  const float v = __fdiv_rn(static_cast<float>(i), 255.f);
  t.v[i] = v;
#pragma unroll
  for (int c = 0; c < 3; ++c) t.n[c][i] = __fdiv_rn(__fsub_rn(v, mean[c]), sd[c]);
  __syncthreads();
}

// up to four values of row `p` (nv of them inside the row): one 16-byte store where the address allows
__device__ __forceinline__ void store4(float* p, int nv, const float (&q)[4]) {
  if (nv == 4 && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
    *reinterpret_cast<float4*>(p) = make_float4(q[0], q[1], q[2], q[3]);
  } else {
#pragma unroll
    for (int v = 0; v < 4; ++v)
      if (v < nv) p[v] = q[v];
  }
}

// the bytes of nv <= 4 adjacent pixels of row ys from column xs of image b: px[v][c]
template <bool CHW>
__device__ __forceinline__ void load_quad(const unsigned char* __restrict__ src, int b, int Hs, int Ws, int ys, int xs, int nv,
                                          unsigned (&px)[4][3]) {
#pragma unroll
  for (int v = 0; v < 4; ++v) px[v][0] = px[v][1] = px[v][2] = 0u;
  if constexpr (!CHW) {
    const unsigned char* p = src + ((static_cast<size_t>(b) * Hs + ys) * Ws + xs) * 3;
    if (nv == 4 && (reinterpret_cast<uintptr_t>(p) & 3u) == 0) {
      const unsigned* d = reinterpret_cast<const unsigned*>(p);
      const unsigned w[3] = {d[0], d[1], d[2]};
#pragma unroll
      for (int k = 0; k < 12; ++k) px[k / 3][k % 3] = (w[k / 4] >> (8 * (k % 4))) & 255u;
    } else {
#pragma unroll
      for (int k = 0; k < 12; ++k)
        if (k / 3 < nv) px[k / 3][k % 3] = p[k];
    }
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const unsigned char* p = src + ((static_cast<size_t>(b) * 3 + c) * Hs + ys) * Ws + xs;
      if (nv == 4 && (reinterpret_cast<uintptr_t>(p) & 3u) == 0) {
        const unsigned w = *reinterpret_cast<const unsigned*>(p);
#pragma unroll
        for (int v = 0; v < 4; ++v) px[v][c] = (w >> (8 * v)) & 255u;
      } else {
#pragma unroll
        for (int v = 0; v < 4; ++v)
          if (v < nv) px[v][c] = p[v];
      }
    }
  }
}

// nv <= 4 adjacent 16-bit values from p (8 bytes at once where the address allows); the others stay 0
__device__ __forceinline__ void load_u16_quad(const unsigned short* __restrict__ p, int nv, unsigned (&r)[4]) {
  r[0] = r[1] = r[2] = r[3] = 0u;
  if (nv == 4 && (reinterpret_cast<uintptr_t>(p) & 7u) == 0) {
    const uint2 w = *reinterpret_cast<const uint2*>(p);
    r[0] = w.x & 65535u; r[1] = w.x >> 16; r[2] = w.y & 65535u; r[3] = w.y >> 16;
  } else {
#pragma unroll
    for (int v = 0; v < 4; ++v)
      if (v < nv) r[v] = p[v];
  }
}

// read_disparity: raw / scale where raw > 0, else 0
__device__ __forceinline__ void decode_u16_quad(const unsigned (&r)[4], float scale, float (&q)[4]) {
#pragma unroll
  for (int v = 0; v < 4; ++v) q[v] = r[v] > 0u ? __fdiv_rn(static_cast<float>(r[v]), scale) : 0.f;
}

// the mask raw > 0 of nv <= 4 values as bytes: one packed dword where the address allows
__device__ __forceinline__ void store_valid4(unsigned char* p, int nv, const unsigned (&r)[4]) {
  if (nv == 4 && (reinterpret_cast<uintptr_t>(p) & 3u) == 0) {
    *reinterpret_cast<unsigned*>(p) = (r[0] > 0u ? 1u : 0u) | (r[1] > 0u ? 1u << 8 : 0u) | (r[2] > 0u ? 1u << 16 : 0u) |
                                      (r[3] > 0u ? 1u << 24 : 0u);
  } else {
#pragma unroll
    for (int v = 0; v < 4; ++v)
      if (v < nv) p[v] = r[v] > 0u ? 1 : 0;
  }
}

// V = 4: one 16-byte load (the caller has checked the alignment); V = 1: one float
template <int V>
__device__ __forceinline__ void load_row(const float* __restrict__ p, float (&out)[V]) {
  if constexpr (V == 4) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    out[0] = q.x; out[1] = q.y; out[2] = q.z; out[3] = q.w;
  } else {
    out[0] = p[0];
  }
}

// workgroups for `items` work items at `threads` items each: at most `cap`, at least one (a grid-stride loop takes the rest)
inline int grid_blocks(long long items, int threads, long long cap) {
  long long nb = (items + threads - 1) / threads;
  if (nb > cap) nb = cap;
  return static_cast<int>(nb < 1 ? 1 : nb);
}

// ------------------------------------------------------------------ the checks of ts_frames_prepare_fwd / ts_frames_augment_fwd
struct NamedPtr {
  const char* name;
  const void* p;
};

// sizes, flags, the required pointers, "no output selected", right-eye outputs without a right image, zero std.
// `op` prefixes every message; `target` is the op's word for its [H, W] ("target" / "window").
inline int frames_check_args(const char* op, const char* target, int B, int Hs, int Ws, int H, int W, int flags,
                             std::initializer_list<NamedPtr> required, const void* right, const float* color_l, const float* color_r,
                             const float* color_aug_l, const float* color_aug_r, float std0, float std1, float std2) {
  TS_REQUIRE(B > 0 && Hs > 0 && Ws > 0 && H > 0 && W > 0, TS_ERR_SHAPE, "%s: bad size (B %d, source %dx%d, %s %dx%d)", op, B, Hs, Ws,
             target, H, W);
  TS_REQUIRE((flags & ~TS_PREPARE_CHW) == 0, TS_ERR_SHAPE, "%s: unknown flags %d", op, flags);
  for (const NamedPtr& r : required) TS_REQUIRE(r.p != nullptr, TS_ERR_NULL, "%s is NULL", r.name);
  TS_REQUIRE(color_l || color_r || color_aug_l || color_aug_r, TS_ERR_NULL, "%s: no output selected", op);
  TS_REQUIRE(right != nullptr || (color_r == nullptr && color_aug_r == nullptr), TS_ERR_NULL,
             "%s: an output of the right eye without a right image", op);
  TS_REQUIRE(std0 != 0.f && std1 != 0.f && std2 != 0.f, TS_ERR_SHAPE, "%s: a zero std", op);
  return TS_OK;
}

// the lower bounds of the two image strides ([Hc, Wc] images of color, [H, W] of color_aug) and the 4-byte alignment of the
// outputs and of `ints` (the crop origins / the parameter table)
inline int frames_check_outputs(const char* op, int Hc, int Wc, int H, int W, const float* color_l, const float* color_r,
                                long long color_stride, const float* color_aug_l, const float* color_aug_r,
                                long long color_aug_stride, const int* ints) {
  if (color_l || color_r)
    TS_REQUIRE(color_stride >= 3LL * Hc * Wc, TS_ERR_SHAPE, "%s: color_stride %lld below 3 x %d x %d", op, color_stride, Hc, Wc);
  if (color_aug_l || color_aug_r)
    TS_REQUIRE(color_aug_stride >= 3LL * H * W, TS_ERR_SHAPE, "%s: color_aug_stride %lld below 3 x %d x %d", op, color_aug_stride, H, W);
  for (const void* p : {static_cast<const void*>(color_l), static_cast<const void*>(color_r), static_cast<const void*>(color_aug_l),
                        static_cast<const void*>(color_aug_r), static_cast<const void*>(ints)})
    TS_REQUIRE((reinterpret_cast<uintptr_t>(p) & 3u) == 0, TS_ERR_ALIGN, "%s: a 4-byte pointer is not 4-byte aligned", op);
  return TS_OK;
}

}  // namespace ts
