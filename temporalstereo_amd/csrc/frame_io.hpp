// Byte, quad and row helpers shared by the frame-side kernels (preprocess.hip, augment.hip, render.hip, evaluation.hip,
// flow_frame.hip), gfx950.
// These kernels are bit-exact against reference-made fixtures, so whatever decides a bit is written once, here:
//   ByteTables         byte / 255 and ((byte / 255) - mean[c]) / std[c], correctly rounded divisions, 1,024 floats in LDS
//   load_quad, store4  four horizontally adjacent pixels: 12 source bytes in, one 16-byte store per channel out
//   u16 quads          four 16-bit disparities in, raw / scale where raw > 0 and the mask raw > 0 out
//   load_row           V floats of a row
//   FlowMap, load_uv   a two-channel flow map read in place through element strides, [B,2,H,W] or [B,H,W,2]
//   q8, store_rgb      the uint8 code of a colour and V pixels of a colour output, fp32 or uint8, HWC or CHW
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

// ------------------------------------------------------------------------------------------------------------- two-channel flow maps
// A flow map read in place: channel c of pixel (y, x) of image b is p[b sb + c sc + y sy + x sx] (element strides), so
// [B,2,H,W] (sx = 1) and [B,H,W,2] (sx = 2, sc = 1) need no copy.
struct FlowMap {
  const float* p;
  long long sb, sc, sy, sx;
  int h, w;
};

inline FlowMap flow_map(const float* p, int h, int w, bool hwc) {
  const long long hw = static_cast<long long>(h) * w;
  return hwc ? FlowMap{p, 2 * hw, 1, 2LL * w, 2, h, w} : FlowMap{p, 2 * hw, hw, w, 1, h, w};
}

// whether load_uv<4> may be used on every row quad of the map: whole rows of quads, every quad's first float 16-byte aligned
inline bool flow_quads_ok(const FlowMap& m) {
  if (m.p == nullptr) return true;
  const bool dense = (m.sx == 1) || (m.sx == 2 && m.sc == 1);
  return dense && m.w % 4 == 0 && aligned16(m.p) && m.sb % 4 == 0 && m.sy % 4 == 0 && (m.sx == 2 || m.sc % 4 == 0);
}

// (u, v) of V horizontally adjacent pixels of row y from column x0 of image b.  V = 4 (the caller has checked flow_quads_ok):
// two 16-byte loads, one per plane (sx = 1) or the eight interleaved floats (sx = 2); V = 1: two floats through the strides.
template <int V>
__device__ __forceinline__ void load_uv(const FlowMap& m, int b, int y, int x0, float (&u)[V], float (&v)[V]) {
  const float* p = m.p + b * m.sb + y * m.sy + x0 * m.sx;
  if constexpr (V == 4) {
    if (m.sx == 1) {
      load_row<4>(p, u);
      load_row<4>(p + m.sc, v);
    } else {
      float lo[4], hi[4];
      load_row<4>(p, lo);
      load_row<4>(p + 4, hi);
      u[0] = lo[0]; v[0] = lo[1]; u[1] = lo[2]; v[1] = lo[3];
      u[2] = hi[0]; v[2] = hi[1]; u[3] = hi[2]; v[3] = hi[3];
    }
  } else {
    u[0] = p[0];
    v[0] = p[m.sc];
  }
}

// workgroups for `items` work items at `threads` items each: at most `cap`, at least one (a grid-stride loop takes the rest)
inline int grid_blocks(long long items, int threads, long long cap) {
  long long nb = (items + threads - 1) / threads;
  if (nb > cap) nb = cap;
  return static_cast<int>(nb < 1 ? 1 : nb);
}

// floor(255 v + 0.5) after a clamp to [0,1], NaN -> 0; the product and the sum are rounded separately (an elementwise restatement
// in a tensor library does the same)
__device__ __forceinline__ unsigned q8(float v) {
  if (v != v) return 0u;
  v = v < 0.f ? 0.f : (v > 1.f ? 1.f : v);
  return static_cast<unsigned>(floorf(__fadd_rn(__fmul_rn(255.f, v), 0.5f)));
}

// V pixels of row `row`, from column x0, of image b of a colour output with `rows` rows: HWC [B,rows,W,3] or CHW [B,3,rows,W]
template <int V, bool U8>
__device__ __forceinline__ void store_rgb(void* base, bool chw, int rows, int W, int b, int row, int x0, const float (&c)[V][3]) {
  if (!chw) {
    const size_t o = ((static_cast<size_t>(b) * rows + row) * W + x0) * 3;
    if constexpr (U8) {
      unsigned char* p = static_cast<unsigned char*>(base) + o;
      if constexpr (V == 4) {
        unsigned q[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) q[i] = q8(c[i / 3][i % 3]);
        unsigned* d = reinterpret_cast<unsigned*>(p);
#pragma unroll
        for (int i = 0; i < 3; ++i) d[i] = q[4 * i] | (q[4 * i + 1] << 8) | (q[4 * i + 2] << 16) | (q[4 * i + 3] << 24);
      } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) p[k] = static_cast<unsigned char>(q8(c[0][k]));
      }
    } else {
      float* p = static_cast<float*>(base) + o;
      if constexpr (V == 4) {
        float4* d = reinterpret_cast<float4*>(p);
        d[0] = make_float4(c[0][0], c[0][1], c[0][2], c[1][0]);
        d[1] = make_float4(c[1][1], c[1][2], c[2][0], c[2][1]);
        d[2] = make_float4(c[2][2], c[3][0], c[3][1], c[3][2]);
      } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) p[k] = c[0][k];
      }
    }
  } else {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const size_t o = ((static_cast<size_t>(b) * 3 + k) * rows + row) * W + x0;
      if constexpr (U8) {
        unsigned char* p = static_cast<unsigned char*>(base) + o;
        if constexpr (V == 4)
          *reinterpret_cast<unsigned*>(p) = q8(c[0][k]) | (q8(c[1][k]) << 8) | (q8(c[2][k]) << 16) | (q8(c[3][k]) << 24);
        else
          p[0] = static_cast<unsigned char>(q8(c[0][k]));
      } else {
        float* p = static_cast<float*>(base) + o;
        if constexpr (V == 4) *reinterpret_cast<float4*>(p) = make_float4(c[0][k], c[1][k], c[2][k], c[3][k]);
        else p[0] = c[0][k];
      }
    }
  }
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
