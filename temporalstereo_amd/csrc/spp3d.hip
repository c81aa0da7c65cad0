// SPP3D (architecture/modeling/aggregation/utils/SPP3D.py:8-49): the memory-bound pieces of the 3-D pyramid pooling module.
//
//   for stride s:  k = (min(D,s), min(H,s), min(W,s));  level = avg_pool3d(x, k, k)          -> spp_pool_{fwd,bwd}_kernel
//                  level = ReLU(BN(conv1x1x1(level)))                                        (the "d" family, _ConvBNAct)
//                  level = interpolate(level, (D,H,W), trilinear, align_corners=True)  \
//   cat([x, level_0 .. level_{L-1}], 1)                                                /     -> spp_expand_{fwd,bwd}_kernel
//   fuse[0]: 3x3x3 convolution = three (1,3,3) convolutions on depth-shifted planes          -> depth_sum3_kernel
//
// Pool: every level leaves ONE launch.  Levels are grouped into chains: level i joins the chain of level i-1 when its box is a whole
// multiple of that level's box on every axis (2 -> 4 -> 8 -> 16 where nothing is clamped); a chain's first level is summed from x and
// the others from the previous level's partial sums, kept in LDS, so x is read once per chain.  A clamped box such as (5,6,7) is no
// multiple of (4,4,4) and starts a chain of its own (x is read again by that chain's workgroups, in the same launch).  A workgroup owns
// a tile of one (batch, channel) volume: one box of the chain's last level, widened along W to a run of such boxes.
// No atomics anywhere in this file: the two backward kernels are gathers, so their results do not depend on the schedule.
#include <cmath>

#include "conv_common.hpp"

namespace {

constexpr int kMaxLevels = 4;
constexpr int kMaxDim = 1 << 20;          // every axis below 2^20: cell_of()'s fp32 quotient is exact there
constexpr int kTileCells = 4096;          // cells of a chain's first level per workgroup tile (16 KiB of LDS)

struct Lv {
  int k[3];            // box (z, y, x)
  int n[3];            // cells
  long long off;       // float offset of the level in the one-buffer layout: [B][C][n0][n1][n2] per level, level after level
  float inv[3];        // 1 / k
  float inv_vol;       // 1 / (k0 k1 k2)
};

struct Spp {
  Lv lv[kMaxLevels];
  int L, B, C, D, H, W;
};

// floor(v / k) for 0 <= v < 2^20 as one multiply: (v + 0.5) / k lies at least 0.5 / k away from every integer, and the two roundings
// (of 1 / k and of the product) move it by less than 2^-23 * 2^20 / k = 0.125 / k.
__device__ __forceinline__ int cell_of(int v, float inv_k) { return static_cast<int>((static_cast<float>(v) + 0.5f) * inv_k); }

bool fill_levels(Spp& p, int B, int C, int D, int H, int W, int L, const int* s) {
  p.L = L; p.B = B; p.C = C; p.D = D; p.H = H; p.W = W;
  long long off = 0;
  const int dim[3] = {D, H, W};
  for (int i = 0; i < L; ++i) {
    if (s[i] < 1) return false;
    long long cells = 1, vol = 1;
    for (int a = 0; a < 3; ++a) {
      p.lv[i].k[a] = dim[a] < s[i] ? dim[a] : s[i];
      p.lv[i].n[a] = dim[a] / p.lv[i].k[a];
      p.lv[i].inv[a] = 1.f / static_cast<float>(p.lv[i].k[a]);
      cells *= p.lv[i].n[a];
      vol *= p.lv[i].k[a];
    }
    p.lv[i].inv_vol = 1.f / static_cast<float>(vol);
    p.lv[i].off = off;
    off += static_cast<long long>(B) * C * cells;
  }
  return true;
}

int check_geometry(const char* what, int B, int C, int D, int H, int W, int L, const int* s) {
  TS_REQUIRE(B > 0 && C > 0 && D > 0 && H > 0 && W > 0, TS_ERR_SHAPE, "%s: non-positive size", what);
  TS_REQUIRE(L >= 1, TS_ERR_SHAPE, "%s: num_levels = %d", what, L);
  TS_REQUIRE(L <= kMaxLevels, TS_ERR_UNSUPPORTED, "%s: num_levels = %d > %d", what, L, kMaxLevels);
  for (int i = 0; i < L; ++i) TS_REQUIRE(s[i] >= 1, TS_ERR_SHAPE, "%s: stride %d of level %d", what, s[i], i);
  TS_REQUIRE(D < kMaxDim && H < kMaxDim && W < kMaxDim, TS_ERR_UNSUPPORTED, "%s: an axis of 2^20 or more", what);
  TS_REQUIRE(static_cast<long long>(B) * C <= 65535, TS_ERR_UNSUPPORTED, "%s: B * C = %lld > 65535", what, static_cast<long long>(B) * C);
  TS_REQUIRE(static_cast<long long>(D) * H * W < (1ll << 31), TS_ERR_UNSUPPORTED, "%s: a channel of 2^31 elements or more", what);
  return TS_OK;
}

// ------------------------------------------------------------------------------------------------------------------ pool forward
struct Chain {
  int first, count;        // levels [first, first + count)
  int tile[3];             // voxels per workgroup tile: the last level's box, times `wide` along x
  int nt[3];               // tiles per axis (over the region the first level covers)
  unsigned block0;         // first workgroup of the chain
  int lds[kMaxLevels];     // float offset of each chain level's tile sums in LDS
};

struct PoolPlan {
  Chain ch[kMaxLevels];
  int nch;
};

template <bool V2>
__global__ void __launch_bounds__(256)
spp_pool_fwd_kernel(const float* __restrict__ x, float* __restrict__ out, Spp p, PoolPlan plan, long long x_bs, long long x_cs) {
  extern __shared__ float sums[];
  int ci = 0;
  for (int i = 1; i < plan.nch; ++i)
    if (blockIdx.x >= plan.ch[i].block0) ci = i;
  const Chain& ch = plan.ch[ci];
  unsigned r = blockIdx.x - ch.block0;
  const int tx = r % ch.nt[2]; r /= ch.nt[2];
  const int ty = r % ch.nt[1]; r /= ch.nt[1];
  const int tz = r % ch.nt[0]; r /= ch.nt[0];
  const int bc = static_cast<int>(r), b = bc / p.C, c = bc - b * p.C;
  const float* xs = x + b * x_bs + c * x_cs;

  // the chain's first level, from x: a lane per cell, neighbouring lanes on neighbouring cells of a row
  {
    const Lv& l = p.lv[ch.first];
    const int t0 = ch.tile[0] / l.k[0], t1 = ch.tile[1] / l.k[1], t2 = ch.tile[2] / l.k[2];
    const long long cells = static_cast<long long>(l.n[0]) * l.n[1] * l.n[2];
    for (int i = threadIdx.x; i < t0 * t1 * t2; i += 256) {
      const int cx = i % t2, q = i / t2, cy = q % t1, cz = q / t1;
      const int gz = tz * t0 + cz, gy = ty * t1 + cy, gx = tx * t2 + cx;
      float s = 0.f;
      if (gz < l.n[0] && gy < l.n[1] && gx < l.n[2]) {
        for (int dz = 0; dz < l.k[0]; ++dz)
          for (int dy = 0; dy < l.k[1]; ++dy) {
            const float* row = xs + (static_cast<long long>(gz * l.k[0] + dz) * p.H + (gy * l.k[1] + dy)) * p.W + gx * l.k[2];
            if (V2) {           // even boxes on even rows: 8 bytes per load
              for (int dx = 0; dx < l.k[2]; dx += 2) {
                const float2 v = *reinterpret_cast<const float2*>(row + dx);
                s += v.x; s += v.y;
              }
            } else {
              for (int dx = 0; dx < l.k[2]; ++dx) s += row[dx];
            }
          }
        out[l.off + bc * cells + (static_cast<long long>(gz) * l.n[1] + gy) * l.n[2] + gx] = s * l.inv_vol;
      }
      sums[ch.lds[0] + i] = s;
    }
  }
  // the others, each from the one before it
  for (int j = 1; j < ch.count; ++j) {
    __syncthreads();
    const Lv& l = p.lv[ch.first + j];
    const Lv& lp = p.lv[ch.first + j - 1];
    const int m0 = l.k[0] / lp.k[0], m1 = l.k[1] / lp.k[1], m2 = l.k[2] / lp.k[2];
    const int t0 = ch.tile[0] / l.k[0], t1 = ch.tile[1] / l.k[1], t2 = ch.tile[2] / l.k[2];
    const int u1 = t1 * m1, u2 = t2 * m2;          // the previous level's tile
    const long long cells = static_cast<long long>(l.n[0]) * l.n[1] * l.n[2];
    const float* prev = sums + ch.lds[j - 1];
    for (int i = threadIdx.x; i < t0 * t1 * t2; i += 256) {
      const int cx = i % t2, q = i / t2, cy = q % t1, cz = q / t1;
      const int gz = tz * t0 + cz, gy = ty * t1 + cy, gx = tx * t2 + cx;
      float s = 0.f;
      if (gz < l.n[0] && gy < l.n[1] && gx < l.n[2]) {          // then every child cell exists too
        for (int a = 0; a < m0; ++a)
          for (int e = 0; e < m1; ++e)
            for (int f = 0; f < m2; ++f) s += prev[((cz * m0 + a) * u1 + cy * m1 + e) * u2 + cx * m2 + f];
        out[l.off + bc * cells + (static_cast<long long>(gz) * l.n[1] + gy) * l.n[2] + gx] = s * l.inv_vol;
      }
      sums[ch.lds[j] + i] = s;
    }
  }
}

// ----------------------------------------------------------------------------------------------------------------- pool backward
// grad_x[v] = addend[v] + sum over the levels whose covered region holds v of g_i[cell_i(v)] / |k_i|: four lanes' worth of a row per
// lane (one 16-byte store where rows allow), blockIdx.y = the (batch, channel) volume.
struct PoolGrads {
  const float* g[kMaxLevels];      // [B][C][n_i] each
};

template <bool V4>
__global__ void __launch_bounds__(256)
spp_pool_bwd_kernel(PoolGrads g, const float* __restrict__ addend, float* __restrict__ gx, Spp p, long long add_bs,
                    long long add_cs, long long gx_bs, long long gx_cs) {
  const int bc = blockIdx.y, b = bc / p.C, c = bc - b * p.C;
  const int wq = (p.W + 3) >> 2;
  const long long quads = static_cast<long long>(p.D) * p.H * wq;
  const float* as = addend ? addend + b * add_bs + c * add_cs : nullptr;
  float* os = gx + b * gx_bs + c * gx_cs;
  for (long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x; i < quads; i += static_cast<long long>(gridDim.x) * 256) {
    const int xq = static_cast<int>(i % wq);
    const long long zy = i / wq;
    const int y = static_cast<int>(zy % p.H), z = static_cast<int>(zy / p.H), x0 = xq * 4;
    const long long at = zy * p.W + x0;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (as) {
      if (V4) {
        const float4 a = *reinterpret_cast<const float4*>(as + at);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (x0 + e < p.W) v[e] = as[at + e];
      }
    }
#pragma unroll
    for (int li = 0; li < kMaxLevels; ++li) {
      if (li >= p.L) break;
      const Lv& l = p.lv[li];
      if (z >= l.n[0] * l.k[0] || y >= l.n[1] * l.k[1]) continue;
      const int cz = cell_of(z, l.inv[0]), cy = cell_of(y, l.inv[1]);
      const float* gl = g.g[li] + (static_cast<long long>(bc) * l.n[0] * l.n[1] + static_cast<long long>(cz) * l.n[1] + cy) * l.n[2];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int xx = x0 + e;
        if (xx < l.n[2] * l.k[2]) v[e] += gl[cell_of(xx, l.inv[2])] * l.inv_vol;
      }
    }
    if (V4) {
      *reinterpret_cast<float4*>(os + at) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (x0 + e < p.W) os[at + e] = v[e];
    }
  }
}

// --------------------------------------------------------------------------------------------------------------- expand forward
// One axis of the framework's trilinear resize with align_corners=True, in its fp32 order (UpSampleTrilinear3d): scale =
// (n_in - 1) / (n_out - 1) (0 for n_out == 1), pos = scale * o, lower index = (int)pos, upper = lower + 1 clamped, weights (1 - f, f).
struct Tap {
  int i0, i1;
  float w0, w1;
};

__device__ __forceinline__ Tap tap_of(int o, float scale, int n_in) {
  const float pos = scale * static_cast<float>(o);
  Tap t;
  t.i0 = static_cast<int>(pos);
  if (t.i0 > n_in - 1) t.i0 = n_in - 1;          // (never taken: scale * (n_out - 1) rounds to at most n_in - 1; keeps every index in bounds)
  t.i1 = t.i0 + (t.i0 < n_in - 1 ? 1 : 0);
  t.w1 = pos - static_cast<float>(t.i0);
  t.w0 = 1.f - t.w1;
  return t;
}

inline float axis_scale(int n_in, int n_out) { return n_out > 1 ? static_cast<float>(n_in - 1) / static_cast<float>(n_out - 1) : 0.f; }

struct Expand {
  const float* lv[kMaxLevels];     // [B][Cl][n0][n1][n2] each
  int n[kMaxLevels][3];
  float scale[kMaxLevels][3];
  int L, B, C, Cl, D, H, W;
};

// cat[b][cc]: cc < C copies x (its own strides), the rest is level (cc - C) / Cl, channel (cc - C) % Cl resized.  blockIdx.y = b * Ccat +
// cc, so which of the two a workgroup does, and from which level, is uniform; four outputs of a row per lane.
template <bool V4>
__global__ void __launch_bounds__(256)
spp_expand_fwd_kernel(const float* __restrict__ x, float* __restrict__ cat, Expand p, long long x_bs, long long x_cs) {
  const int ccat = p.C + p.Cl * p.L;
  const int b = blockIdx.y / ccat, cc = blockIdx.y - b * ccat;
  const int wq = (p.W + 3) >> 2;
  const long long quads = static_cast<long long>(p.D) * p.H * wq, vol = static_cast<long long>(p.D) * p.H * p.W;
  float* os = cat + (static_cast<long long>(b) * ccat + cc) * vol;
  if (cc < p.C) {
    const float* xs = x + b * x_bs + cc * x_cs;
    if (V4) {
      const float4* s4 = reinterpret_cast<const float4*>(xs);
      float4* d4 = reinterpret_cast<float4*>(os);
      for (long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x; i < quads; i += static_cast<long long>(gridDim.x) * 256) d4[i] = s4[i];
    } else {
      for (long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x; i < vol; i += static_cast<long long>(gridDim.x) * 256) os[i] = xs[i];
    }
    return;
  }
  const int li = (cc - p.C) / p.Cl, j = (cc - p.C) - li * p.Cl;
  const int n0 = p.n[li][0], n1 = p.n[li][1], n2 = p.n[li][2];
  const float s0 = p.scale[li][0], s1 = p.scale[li][1], s2 = p.scale[li][2];
  const float* src = p.lv[li] + (static_cast<long long>(b) * p.Cl + j) * n0 * n1 * n2;
  for (long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x; i < quads; i += static_cast<long long>(gridDim.x) * 256) {
    const int xq = static_cast<int>(i % wq);
    const long long zy = i / wq;
    const int y = static_cast<int>(zy % p.H), z = static_cast<int>(zy / p.H), x0 = xq * 4;
    const Tap tz = tap_of(z, s0, n0), ty = tap_of(y, s1, n1);
    const float* r00 = src + (static_cast<long long>(tz.i0) * n1 + ty.i0) * n2;
    const float* r01 = src + (static_cast<long long>(tz.i0) * n1 + ty.i1) * n2;
    const float* r10 = src + (static_cast<long long>(tz.i1) * n1 + ty.i0) * n2;
    const float* r11 = src + (static_cast<long long>(tz.i1) * n1 + ty.i1) * n2;
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int xx = x0 + e < p.W ? x0 + e : p.W - 1;
      const Tap tx = tap_of(xx, s2, n2);
      v[e] = tz.w0 * (ty.w0 * (tx.w0 * r00[tx.i0] + tx.w1 * r00[tx.i1]) + ty.w1 * (tx.w0 * r01[tx.i0] + tx.w1 * r01[tx.i1])) +
             tz.w1 * (ty.w0 * (tx.w0 * r10[tx.i0] + tx.w1 * r10[tx.i1]) + ty.w1 * (tx.w0 * r11[tx.i0] + tx.w1 * r11[tx.i1]));
    }
    const long long at = zy * p.W + x0;
    if (V4) {
      *reinterpret_cast<float4*>(os + at) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (x0 + e < p.W) os[at + e] = v[e];
    }
  }
}

// -------------------------------------------------------------------------------------------------------------- expand backward
struct ExpandBwd {
  float* glv[kMaxLevels];          // gradients of the levels, [B][Cl][n0][n1][n2] each, OVERWRITTEN
  long long first[kMaxLevels + 1]; // cumulative cell counts: level i owns work items [first[i], first[i + 1])
  int n[kMaxLevels][3];
  float scale[kMaxLevels][3];
  int L, B, C, Cl, D, H, W;
};

// the fine indices along one axis whose taps can touch coarse cell c: a superset, since weight_of() decides per index
__device__ __forceinline__ void support_of(int c, float scale, int n_out, int& lo, int& hi) {
  if (scale <= 0.f) { lo = 0; hi = n_out - 1; return; }
  const float a = (static_cast<float>(c) - 1.f) / scale, e = (static_cast<float>(c) + 1.f) / scale;
  lo = static_cast<int>(floorf(a)) - 1;
  hi = static_cast<int>(ceilf(e)) + 1;
  if (lo < 0) lo = 0;
  if (hi > n_out - 1) hi = n_out - 1;
}

__device__ __forceinline__ float weight_of(int o, int c, float scale, int n_in) {
  const Tap t = tap_of(o, scale, n_in);
  return (t.i0 == c ? t.w0 : 0.f) + (t.i1 == c ? t.w1 : 0.f);
}

// One wave per coarse cell: its lanes walk the cell's support in the fine volume (x fastest), evaluate the forward's own taps there
// and sum in a fixed order (lane-strided, then a butterfly), so two runs agree to the bit.
__global__ void __launch_bounds__(256)
spp_expand_bwd_kernel(const float* __restrict__ gcat, ExpandBwd p, long long g_bs, long long g_cs) {
  const int lane = threadIdx.x & 63;
  const long long item = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6)) + static_cast<long long>(blockIdx.x) * 4;
  if (item >= p.first[p.L]) return;
  int li = 0;
  for (int i = 1; i < p.L; ++i)
    if (item >= p.first[i]) li = i;
  const int n0 = p.n[li][0], n1 = p.n[li][1], n2 = p.n[li][2];
  const float s0 = p.scale[li][0], s1 = p.scale[li][1], s2 = p.scale[li][2];
  long long r = item - p.first[li];
  const int cx = static_cast<int>(r % n2); r /= n2;
  const int cy = static_cast<int>(r % n1); r /= n1;
  const int cz = static_cast<int>(r % n0); r /= n0;
  const int j = static_cast<int>(r % p.Cl), b = static_cast<int>(r / p.Cl);
  const float* gs = gcat + b * g_bs + (p.C + li * p.Cl + j) * g_cs;
  int z_lo, z_hi, y_lo, y_hi, x_lo, x_hi;
  support_of(cz, s0, p.D, z_lo, z_hi);
  support_of(cy, s1, p.H, y_lo, y_hi);
  support_of(cx, s2, p.W, x_lo, x_hi);
  const int rz = z_hi - z_lo + 1, ry = y_hi - y_lo + 1, rx = x_hi - x_lo + 1;
  const long long total = (rz > 0 && ry > 0 && rx > 0) ? static_cast<long long>(rz) * ry * rx : 0;
  float acc = 0.f;
  for (long long e = lane; e < total; e += 64) {
    const int dx = static_cast<int>(e % rx);
    const long long q = e / rx;
    const int dy = static_cast<int>(q % ry), dz = static_cast<int>(q / ry);
    const int z = z_lo + dz, y = y_lo + dy, xx = x_lo + dx;
    const float w = weight_of(z, cz, s0, n0) * weight_of(y, cy, s1, n1) * weight_of(xx, cx, s2, n2);
    if (w != 0.f) acc += w * gs[(static_cast<long long>(z) * p.H + y) * p.W + xx];
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if (lane == 0) p.glv[li][item - p.first[li]] = acc;
}

// ------------------------------------------------------------------------------------------------------------------- depth sum
// y[b][c][d] = act(scale[c] * (z0[b][c][d-1] + z1[b][c][d] + z2[b][c][d+1]) + shift[c]), planes outside [0, D) are zero.  y may BE z1
// (every element is read before it is written, by the lane that writes it).  Grid: (plane chunks, B * C, D).
template <bool V4>
__global__ void __launch_bounds__(256)
depth_sum3_kernel(const float* z0, const float* z1, const float* z2, const float* __restrict__ scale, const float* __restrict__ shift,
                  float* y, int C, int D, long long plane, int act, long long s0b, long long s0c, long long s1b, long long s1c,
                  long long s2b, long long s2c, long long yb, long long yc) {
  const int bc = blockIdx.y, b = bc / C, c = bc - b * C, d = blockIdx.z;
  const bool lo = d > 0, hi = d < D - 1;
  const float* p0 = z0 + b * s0b + c * s0c + (d - 1) * plane;
  const float* p1 = z1 + b * s1b + c * s1c + d * plane;
  const float* p2 = z2 + b * s2b + c * s2c + (d + 1) * plane;
  float* py = y + b * yb + c * yc + d * plane;
  const float sc = scale ? scale[c] : 1.f, sh = shift ? shift[c] : 0.f;
  if (V4) {
    const long long quads = plane >> 2;
    for (long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x; i < quads; i += static_cast<long long>(gridDim.x) * 256) {
      float4 v = reinterpret_cast<const float4*>(p1)[i];
      if (lo) {
        const float4 a = reinterpret_cast<const float4*>(p0)[i];
        v.x = a.x + v.x; v.y = a.y + v.y; v.z = a.z + v.z; v.w = a.w + v.w;
      }
      if (hi) {
        const float4 a = reinterpret_cast<const float4*>(p2)[i];
        v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w;
      }
      v.x = apply_act(v.x * sc + sh, act, 0.f); v.y = apply_act(v.y * sc + sh, act, 0.f);
      v.z = apply_act(v.z * sc + sh, act, 0.f); v.w = apply_act(v.w * sc + sh, act, 0.f);
      reinterpret_cast<float4*>(py)[i] = v;
    }
  } else {
    for (long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x; i < plane; i += static_cast<long long>(gridDim.x) * 256) {
      float v = p1[i];
      if (lo) v = p0[i] + v;
      if (hi) v += p2[i];
      py[i] = apply_act(v * sc + sh, act, 0.f);
    }
  }
}

inline bool quad_ok(const void* p, long long a, long long b) {
  return (reinterpret_cast<uintptr_t>(p) & 15u) == 0 && a % 4 == 0 && b % 4 == 0;
}

constexpr int kGridCap = 2048;          // blocks of the grid-stride element kernels
using ts::strides_ok;

}  // namespace

extern "C" int ts_spp3d_pool_fwd(const float* x, float* pooled, int B, int C, int D, int H, int W, int num_levels, int s0, int s1,
                                 int s2, int s3, long long x_bstride, long long x_cstride, void* stream) {
  const int s[kMaxLevels] = {s0, s1, s2, s3};
  if (int rc = check_geometry("spp3d_pool_fwd", B, C, D, H, W, num_levels, s)) return rc;
  const long long vol = static_cast<long long>(D) * H * W;
  TS_REQUIRE(strides_ok(B, C, vol, x_bstride, x_cstride), TS_ERR_SHAPE, "spp3d_pool_fwd: x strides %lld / %lld overlap", x_bstride, x_cstride);
  TS_REQUIRE_PTR(x); TS_REQUIRE_PTR(pooled);
  Spp p;
  fill_levels(p, B, C, D, H, W, num_levels, s);
  PoolPlan plan;
  plan.nch = 0;
  unsigned long long blocks = 0;
  size_t lds = 0;
  bool v2 = (reinterpret_cast<uintptr_t>(x) & 7u) == 0 && W % 2 == 0 && x_bstride % 2 == 0 && x_cstride % 2 == 0;
  for (int i = 0; i < num_levels;) {
    Chain& ch = plan.ch[plan.nch++];
    ch.first = i;
    ch.count = 1;
    // extend while the next box is a whole multiple and a tile's first-level cells still fit
    while (i + ch.count < num_levels) {
      const Lv& a = p.lv[i + ch.count - 1];
      const Lv& n = p.lv[i + ch.count];
      long long unit = 1;
      bool mult = true;
      for (int ax = 0; ax < 3; ++ax) {
        mult = mult && n.k[ax] % a.k[ax] == 0;
        unit *= n.k[ax] / p.lv[i].k[ax];
      }
      if (!mult || unit > kTileCells) break;
      ++ch.count;
    }
    const Lv& base = p.lv[i];
    const Lv& top = p.lv[i + ch.count - 1];
    long long unit = 1;
    for (int ax = 0; ax < 3; ++ax) unit *= top.k[ax] / base.k[ax];
    const int covered = base.n[2] * base.k[2];
    int wide = static_cast<int>(kTileCells / unit);
    const int most = (covered + top.k[2] - 1) / top.k[2];
    if (wide > most) wide = most;
    if (wide < 1) wide = 1;
    size_t at = 0;
    for (int ax = 0; ax < 3; ++ax) {
      ch.tile[ax] = top.k[ax] * (ax == 2 ? wide : 1);
      ch.nt[ax] = (base.n[ax] * base.k[ax] + ch.tile[ax] - 1) / ch.tile[ax];
    }
    for (int j = 0; j < ch.count; ++j) {
      const Lv& l = p.lv[i + j];
      ch.lds[j] = static_cast<int>(at);
      at += static_cast<size_t>(ch.tile[0] / l.k[0]) * (ch.tile[1] / l.k[1]) * (ch.tile[2] / l.k[2]);
    }
    if (at * sizeof(float) > lds) lds = at * sizeof(float);
    ch.block0 = static_cast<unsigned>(blocks);
    blocks += static_cast<unsigned long long>(B) * C * ch.nt[0] * ch.nt[1] * ch.nt[2];
    TS_REQUIRE(blocks < 0x7fffffffull, TS_ERR_UNSUPPORTED, "spp3d_pool_fwd: grid too large");
    v2 = v2 && base.k[2] % 2 == 0;
    i += ch.count;
  }
  TS_REQUIRE(lds <= 64 * 1024, TS_ERR_UNSUPPORTED, "spp3d_pool_fwd: %zu bytes of LDS", lds);
  ts::dispatch_bool(v2, [&](auto V) {
    hipLaunchKernelGGL(spp_pool_fwd_kernel<V()>, dim3(static_cast<unsigned>(blocks)), dim3(256), lds, ts::as_stream(stream), x, pooled, p,
                       plan, x_bstride, x_cstride);
  });
  return ts::launched("spp_pool_fwd_kernel");
}

extern "C" int ts_spp3d_pool_bwd(const float* g0, const float* g1, const float* g2, const float* g3, const float* addend, float* grad_x,
                                 int B, int C, int D, int H, int W, int num_levels, int s0, int s1, int s2, int s3,
                                 long long addend_bstride, long long addend_cstride, long long gx_bstride, long long gx_cstride,
                                 void* stream) {
  const int s[kMaxLevels] = {s0, s1, s2, s3};
  if (int rc = check_geometry("spp3d_pool_bwd", B, C, D, H, W, num_levels, s)) return rc;
  const long long vol = static_cast<long long>(D) * H * W;
  TS_REQUIRE(strides_ok(B, C, vol, gx_bstride, gx_cstride), TS_ERR_SHAPE, "spp3d_pool_bwd: grad_x strides %lld / %lld overlap", gx_bstride, gx_cstride);
  TS_REQUIRE(addend == nullptr || strides_ok(B, C, vol, addend_bstride, addend_cstride), TS_ERR_SHAPE,
             "spp3d_pool_bwd: addend strides %lld / %lld overlap", addend_bstride, addend_cstride);
  TS_REQUIRE_PTR(grad_x);
  PoolGrads grad_pooled{{g0, g1, g2, g3}};
  for (int i = 0; i < num_levels; ++i) TS_REQUIRE(grad_pooled.g[i] != nullptr, TS_ERR_NULL, "spp3d_pool_bwd: gradient of level %d is NULL", i);
  Spp p;
  fill_levels(p, B, C, D, H, W, num_levels, s);
  const bool v4 = W % 4 == 0 && quad_ok(grad_x, gx_bstride, gx_cstride) && (addend == nullptr || quad_ok(addend, addend_bstride, addend_cstride));
  const dim3 grid(ts::blocks_for(static_cast<long long>(D) * H * ((W + 3) / 4), kGridCap), static_cast<unsigned>(B * C));
  ts::dispatch_bool(v4, [&](auto V) {
    hipLaunchKernelGGL(spp_pool_bwd_kernel<V()>, grid, dim3(256), 0, ts::as_stream(stream), grad_pooled, addend, grad_x, p, addend_bstride,
                       addend_cstride, gx_bstride, gx_cstride);
  });
  return ts::launched("spp_pool_bwd_kernel");
}

namespace {
int check_expand(const char* what, int B, int C, int Cl, int D, int H, int W, int L, const int* s) {
  if (int rc = check_geometry(what, B, C, D, H, W, L, s)) return rc;
  TS_REQUIRE(Cl > 0, TS_ERR_SHAPE, "%s: level channels = %d", what, Cl);
  TS_REQUIRE(static_cast<long long>(B) * (C + static_cast<long long>(Cl) * L) <= 65535, TS_ERR_UNSUPPORTED, "%s: B * (C + Cl * L) > 65535", what);
  return TS_OK;
}
}  // namespace

extern "C" int ts_spp3d_expand_fwd(const float* x, const float* lv0, const float* lv1, const float* lv2, const float* lv3, float* cat,
                                   int B, int C, int Cl, int D, int H, int W, int num_levels, int s0, int s1, int s2, int s3,
                                   long long x_bstride, long long x_cstride, void* stream) {
  const int s[kMaxLevels] = {s0, s1, s2, s3};
  if (int rc = check_expand("spp3d_expand_fwd", B, C, Cl, D, H, W, num_levels, s)) return rc;
  const long long vol = static_cast<long long>(D) * H * W;
  TS_REQUIRE(strides_ok(B, C, vol, x_bstride, x_cstride), TS_ERR_SHAPE, "spp3d_expand_fwd: x strides %lld / %lld overlap", x_bstride, x_cstride);
  const float* lv[kMaxLevels] = {lv0, lv1, lv2, lv3};
  TS_REQUIRE_PTR(x); TS_REQUIRE_PTR(cat);
  for (int i = 0; i < num_levels; ++i) TS_REQUIRE(lv[i] != nullptr, TS_ERR_NULL, "spp3d_expand_fwd: level %d is NULL", i);
  Spp g;
  fill_levels(g, B, Cl, D, H, W, num_levels, s);
  Expand p;
  p.L = num_levels; p.B = B; p.C = C; p.Cl = Cl; p.D = D; p.H = H; p.W = W;
  const int dim[3] = {D, H, W};
  for (int i = 0; i < kMaxLevels; ++i) {
    p.lv[i] = i < num_levels ? lv[i] : nullptr;
    for (int a = 0; a < 3; ++a) {
      p.n[i][a] = i < num_levels ? g.lv[i].n[a] : 1;
      p.scale[i][a] = i < num_levels ? axis_scale(g.lv[i].n[a], dim[a]) : 0.f;
    }
  }
  const bool v4 = W % 4 == 0 && quad_ok(x, x_bstride, x_cstride) && (reinterpret_cast<uintptr_t>(cat) & 15u) == 0;
  const dim3 grid(ts::blocks_for(static_cast<long long>(D) * H * ((W + 3) / 4), kGridCap), static_cast<unsigned>(B * (C + Cl * num_levels)));
  ts::dispatch_bool(v4, [&](auto V) {
    hipLaunchKernelGGL(spp_expand_fwd_kernel<V()>, grid, dim3(256), 0, ts::as_stream(stream), x, cat, p, x_bstride, x_cstride);
  });
  return ts::launched("spp_expand_fwd_kernel");
}

extern "C" int ts_spp3d_expand_bwd(const float* grad_cat, float* g0, float* g1, float* g2, float* g3, int B, int C, int Cl, int D, int H,
                                   int W, int num_levels, int s0, int s1, int s2, int s3, long long g_bstride, long long g_cstride,
                                   void* stream) {
  const int s[kMaxLevels] = {s0, s1, s2, s3};
  if (int rc = check_expand("spp3d_expand_bwd", B, C, Cl, D, H, W, num_levels, s)) return rc;
  const long long vol = static_cast<long long>(D) * H * W;
  TS_REQUIRE(strides_ok(B, C + Cl * num_levels, vol, g_bstride, g_cstride), TS_ERR_SHAPE, "spp3d_expand_bwd: grad_cat strides %lld / %lld overlap",
             g_bstride, g_cstride);
  float* gl[kMaxLevels] = {g0, g1, g2, g3};
  TS_REQUIRE_PTR(grad_cat);
  for (int i = 0; i < num_levels; ++i) TS_REQUIRE(gl[i] != nullptr, TS_ERR_NULL, "spp3d_expand_bwd: gradient of level %d is NULL", i);
  Spp g;
  fill_levels(g, B, Cl, D, H, W, num_levels, s);
  ExpandBwd p;
  p.L = num_levels; p.B = B; p.C = C; p.Cl = Cl; p.D = D; p.H = H; p.W = W;
  const int dim[3] = {D, H, W};
  p.first[0] = 0;
  for (int i = 0; i < kMaxLevels; ++i) {
    p.glv[i] = i < num_levels ? gl[i] : nullptr;
    long long cells = 0;
    if (i < num_levels) cells = static_cast<long long>(B) * Cl * g.lv[i].n[0] * g.lv[i].n[1] * g.lv[i].n[2];
    p.first[i + 1] = p.first[i] + cells;
    for (int a = 0; a < 3; ++a) {
      p.n[i][a] = i < num_levels ? g.lv[i].n[a] : 1;
      p.scale[i][a] = i < num_levels ? axis_scale(g.lv[i].n[a], dim[a]) : 0.f;
    }
  }
  const long long blocks = (p.first[num_levels] + 3) / 4;
  TS_REQUIRE(blocks < 0x7fffffffll, TS_ERR_UNSUPPORTED, "spp3d_expand_bwd: grid too large");
  hipLaunchKernelGGL(spp_expand_bwd_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, ts::as_stream(stream), grad_cat, p, g_bstride,
                     g_cstride);
  return ts::launched("spp_expand_bwd_kernel");
}

extern "C" int ts_depth_sum3_fwd(const float* z0, const float* z1, const float* z2, const float* scale, const float* shift, float* y,
                                 int B, int C, int D, int H, int W, int act, long long z0_bstride, long long z0_cstride,
                                 long long z1_bstride, long long z1_cstride, long long z2_bstride, long long z2_cstride,
                                 long long y_bstride, long long y_cstride, void* stream) {
  TS_REQUIRE(B > 0 && C > 0 && D > 0 && H > 0 && W > 0, TS_ERR_SHAPE, "depth_sum3: non-positive size");
  TS_REQUIRE(act >= ACT_NONE && act <= ACT_RELU, TS_ERR_SHAPE, "depth_sum3: unknown activation %d", act);
  TS_REQUIRE(static_cast<long long>(B) * C <= 65535 && D <= 65535, TS_ERR_UNSUPPORTED, "depth_sum3: B * C or D above 65535");
  const long long plane = static_cast<long long>(H) * W, vol = plane * D;
  TS_REQUIRE(vol < (1ll << 31), TS_ERR_UNSUPPORTED, "depth_sum3: a channel of 2^31 elements or more");
  TS_REQUIRE(strides_ok(B, C, vol, z0_bstride, z0_cstride) && strides_ok(B, C, vol, z1_bstride, z1_cstride) &&
             strides_ok(B, C, vol, z2_bstride, z2_cstride) && strides_ok(B, C, vol, y_bstride, y_cstride), TS_ERR_SHAPE,
             "depth_sum3: strides overlap");
  TS_REQUIRE_PTR(z0); TS_REQUIRE_PTR(z1); TS_REQUIRE_PTR(z2); TS_REQUIRE_PTR(y);
  const bool v4 = plane % 4 == 0 && quad_ok(z0, z0_bstride, z0_cstride) && quad_ok(z1, z1_bstride, z1_cstride) &&
                  quad_ok(z2, z2_bstride, z2_cstride) && quad_ok(y, y_bstride, y_cstride);
  long long bx = (plane / (v4 ? 4 : 1) + 255) / 256;
  if (bx > 64) bx = 64;
  if (bx < 1) bx = 1;
  const dim3 grid(static_cast<unsigned>(bx), static_cast<unsigned>(B * C), static_cast<unsigned>(D));
  ts::dispatch_bool(v4, [&](auto V) {
    hipLaunchKernelGGL(depth_sum3_kernel<V()>, grid, dim3(256), 0, ts::as_stream(stream), z0, z1, z2, scale, shift, y, C, D, plane, act,
                       z0_bstride, z0_cstride, z1_bstride, z1_cstride, z2_bstride, z2_cstride, y_bstride, y_cstride);
  });
  return ts::launched("depth_sum3_kernel");
}

// ------------------------------------------------------------------------------------------- BatchNorm backward, few values per channel
// A coarse level has a handful of cells, down to ONE per batch item: its train-mode BatchNorm then normalises two values per channel
// to +-1 / sqrt(1 + eps / var), and the gradient it passes on, g_i - mean(g) - xhat_i mean(g xhat), is what a cancellation leaves:
// O(eps / var) of its terms.  One fp32 rounding of xhat or of 1 / sqrt(var + eps) is an error of 2^-24 var / eps relative to that
// result (3e-4 at var = 0.03).  For such populations (B * N <= 4096) the statistics are formed again from y and everything up to the
// final rounding of dy is carried in fp64: a workgroup per channel, fixed-order tree sums, no atomics.  The activation's derivative is
// taken at the pre-activation formed HERE, in fp64: for a pre-activation within an fp32 rounding of 0 a ReLU's mask can differ from
// the one the fp32 forward applied (the fp32 backward kernels recompute theirs in fp32 and share the forward's).
namespace {

constexpr int kSmallBnMax = 4096;

__device__ __forceinline__ double block_sum(double v, double* red) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = 128; s >= 1; s >>= 1) {
    if (static_cast<int>(threadIdx.x) < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  return red[0];
}

__global__ void __launch_bounds__(256)
bn_small_train_bwd_kernel(const float* __restrict__ y, const float* __restrict__ g, const float* __restrict__ gamma,
                          const float* __restrict__ beta, float* __restrict__ sum_g, float* __restrict__ sum_gx, float* __restrict__ dy,
                          int B, int N, long long y_bs, long long y_cs, long long g_bs, long long g_cs, long long dy_bs, long long dy_cs,
                          double eps, int act) {
  __shared__ double red[256];
  const int c = blockIdx.x, n = B * N;
  const float* ys = y + c * y_cs;
  const float* gs = g + c * g_cs;
  float* ds = dy + c * dy_cs;
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) acc += static_cast<double>(ys[(i / N) * y_bs + i % N]);
  const double mean = block_sum(acc, red) / n;
  acc = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) {
    const double d = static_cast<double>(ys[(i / N) * y_bs + i % N]) - mean;
    acc += d * d;
  }
  const double invstd = 1.0 / sqrt(block_sum(acc, red) / n + eps);
  const double ga = gamma ? static_cast<double>(gamma[c]) : 1.0, be = beta ? static_cast<double>(beta[c]) : 0.0;
  // the cotangent behind the activation, from the pre-activation formed here
  auto behind = [&](int i, double& xhat) {
    xhat = (static_cast<double>(ys[(i / N) * y_bs + i % N]) - mean) * invstd;
    const double z = ga * xhat + be, gi = static_cast<double>(gs[(i / N) * g_bs + i % N]);
    if (act == ACT_RELU) return z > 0.0 ? gi : 0.0;
    if (act == ACT_SILU) {
      const double sg = 1.0 / (1.0 + exp(-z));
      return gi * sg * (1.0 + z * (1.0 - sg));
    }
    return gi;
  };
  double a1 = 0.0, a2 = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) {
    double xhat;
    const double gz = behind(i, xhat);
    a1 += gz;
    a2 += gz * xhat;
  }
  const double s1 = block_sum(a1, red);
  const double s2 = block_sum(a2, red);
  if (threadIdx.x == 0) {
    sum_g[c] = static_cast<float>(s1);
    sum_gx[c] = static_cast<float>(s2);
  }
  for (int i = threadIdx.x; i < n; i += 256) {
    double xhat;
    const double gz = behind(i, xhat);
    ds[(i / N) * dy_bs + i % N] = static_cast<float>(ga * invstd * (gz - s1 / n - xhat * s2 / n));
  }
}

}  // namespace

extern "C" int ts_bn_small_train_bwd(const float* y, const float* g, const float* gamma, const float* beta, float* sum_g, float* sum_gx,
                                     float* dy, int B, int C, int N, long long y_bstride, long long y_cstride, long long g_bstride,
                                     long long g_cstride, long long dy_bstride, long long dy_cstride, float eps, int act, void* stream) {
  TS_REQUIRE(B > 0 && C > 0 && N > 0, TS_ERR_SHAPE, "bn_small_train_bwd: non-positive size");
  TS_REQUIRE(act >= ACT_NONE && act <= ACT_RELU, TS_ERR_SHAPE, "bn_small_train_bwd: unknown activation %d", act);
  TS_REQUIRE(static_cast<long long>(B) * N <= kSmallBnMax, TS_ERR_UNSUPPORTED, "bn_small_train_bwd: %lld values per channel > %d",
             static_cast<long long>(B) * N, kSmallBnMax);
  TS_REQUIRE(static_cast<long long>(B) * N >= 2, TS_ERR_SHAPE, "bn_small_train_bwd: one value per channel");
  TS_REQUIRE(strides_ok(B, C, N, y_bstride, y_cstride) && strides_ok(B, C, N, g_bstride, g_cstride) &&
             strides_ok(B, C, N, dy_bstride, dy_cstride), TS_ERR_SHAPE, "bn_small_train_bwd: strides overlap");
  TS_REQUIRE_PTR(y); TS_REQUIRE_PTR(g); TS_REQUIRE_PTR(sum_g); TS_REQUIRE_PTR(sum_gx); TS_REQUIRE_PTR(dy);
  hipLaunchKernelGGL(bn_small_train_bwd_kernel, dim3(static_cast<unsigned>(C)), dim3(256), 0, ts::as_stream(stream), y, g, gamma, beta, sum_g,
                     sum_gx, dy, B, N, y_bstride, y_cstride, g_bstride, g_cstride, dy_bstride, dy_cstride, static_cast<double>(eps), act);
  return ts::launched("bn_small_train_bwd_kernel");
}
