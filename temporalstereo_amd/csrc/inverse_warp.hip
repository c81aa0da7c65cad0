// The 2-D inverse warp of the reference on the device, gfx950: inverse_warp()  architecture/modeling/layers/inverse_warp.py:6-77
// (disparity, flow and depth mode; the depth mode's project_to_3d :92-178 in the same launch), forward and backward.
//
//   source coordinate   disparity: X = x + m, Y = y;  flow: X = x + m0, Y = y + m1;  depth: (X, Y) = src_pixel_coord of
//                       project_to_3d -- project.hpp, the very expressions of ts_project_to_3d_fwd
//   position            warp.hpp source_position_2d: normalise with the MOTION map's size (:67-68), un-normalise with the IMAGE's
//                       (grid_sample, align_corners=True), each step rounded on its own; then the padding mode (warp_pad), whose
//                       last step clamps to a finite range, so no motion -- huge, infinite, NaN -- can index outside the image
//   sample              bilinear: the four taps, those outside the image contribute 0; nearest: round half to even
//
// ts_inverse_warp_fwd, one launch.  A lane owns four horizontally adjacent output pixels of one row (a ragged last quad is masked, not
// a second kernel): it reads their motion once (16 bytes where aligned), computes the four positions, tap offsets and weights once,
// then walks its range of channels -- 16 gathers and one 16-byte store per channel.  The channel range is split over grid.y so that
// a 3-channel full-size image and a 64-channel 1/4-size feature map both put >= 4 workgroups on every CU; grid.y == 0 also writes
// the depth mode's side outputs.  Nothing is staged: no LDS besides the 21 floats of the projection, no scratch.
//
// ts_inverse_warp_bwd, one launch.  A workgroup is four waves on the same 64 output pixels (lanes along x: grad_out and motion reads
// are coalesced); wave w takes channels w, w + 4, ... of the range, so a 64-channel map keeps four times as many loads and atomics
// in flight as one lane per pixel would.
//   grad_img     ACCUMULATED with fp32 hardware atomics (the caller zero-fills): the summation order is not deterministic, the
//                same contract as softsplat.hip's default mode.
//   grad_motion  OVERWRITTEN; a gather: each wave reduces its channels in order, wave 0 adds the four partial sums from LDS in a fixed
//                order: deterministic.  That is why the channel range is split over grid.y only when grad_motion is not asked for.
#include "frame_io.hpp"
#include "project.hpp"
#include "warp.hpp"

namespace {

constexpr int kFwdThreads = 256;
constexpr int kBwdPixels = ts::kWave;          // backward: a wave per channel slice, all on the same 64 pixels
constexpr int kBwdSlices = 4;
constexpr int kBwdThreads = kBwdPixels * kBwdSlices;

struct WarpArgs {
  const float* img;
  const float* motion;
  const float* K;
  const float* inv_K;
  const float* T;
  const float* gout;             // backward only
  float* out;                    // forward: the warped image; backward: grad_img
  float* gmotion;                // backward only
  float* tri;
  float* coord;
  float* flow;
  unsigned char* mask;
  float* homo;
  int B, C, Hi, Wi, H, W, kdim, ikdim, cpc;      // cpc: channels per grid.y slice
  float eps;
};

// taps of one output pixel: clamped (always addressable) columns and row offsets, the one-dimensional weights, which taps are
// inside the image (bit 0 nw, 1 ne, 2 sw, 3 se; nearest: bit 0 only), d(position) / d(unpadded position)
struct Taps {
  int xa, xb, ra, rb;
  float ww, we, wn, ws;
  unsigned in;
  float mx, my;
};

template <int PAD, bool NEAREST>
__device__ __forceinline__ Taps taps_at(float X, float Y, int Hi, int Wi, float Hm1, float Wm1, float Him1, float Wim1) {
  Taps t;
  const float ix = ts::warp_pad<PAD>(ts::source_position_2d(X, Wm1, Wim1), Wim1, t.mx);
  const float iy = ts::warp_pad<PAD>(ts::source_position_2d(Y, Hm1, Him1), Him1, t.my);
  if (NEAREST) {
    const int xn = static_cast<int>(rintf(ix)), yn = static_cast<int>(rintf(iy));      // round half to even, as nearbyint
    t.in = (xn >= 0 && xn < Wi && yn >= 0 && yn < Hi) ? 1u : 0u;
    t.xa = t.xb = min(max(xn, 0), Wi - 1);
    t.ra = t.rb = min(max(yn, 0), Hi - 1) * Wi;
    t.ww = t.wn = 1.f;
    t.we = t.ws = 0.f;
  } else {
    const float fx = floorf(ix), fy = floorf(iy);
    const int x0 = static_cast<int>(fx), y0 = static_cast<int>(fy);
    t.we = __fsub_rn(ix, fx);
    t.ww = __fsub_rn(__fadd_rn(fx, 1.f), ix);
    t.ws = __fsub_rn(iy, fy);
    t.wn = __fsub_rn(__fadd_rn(fy, 1.f), iy);
    const bool xw = x0 >= 0 && x0 < Wi, xe = x0 + 1 >= 0 && x0 + 1 < Wi;
    const bool yn = y0 >= 0 && y0 < Hi, ys = y0 + 1 >= 0 && y0 + 1 < Hi;
    t.in = ((xw && yn) ? 1u : 0u) | ((xe && yn) ? 2u : 0u) | ((xw && ys) ? 4u : 0u) | ((xe && ys) ? 8u : 0u);
    t.xa = min(max(x0, 0), Wi - 1);
    t.xb = min(max(x0 + 1, 0), Wi - 1);
    t.ra = min(max(y0, 0), Hi - 1) * Wi;
    t.rb = min(max(y0 + 1, 0), Hi - 1) * Wi;
  }
  return t;
}

// up to four mask bytes of a row: one packed dword where the address allows
__device__ __forceinline__ void store_mask4(unsigned char* p, int nv, const bool (&m)[4]) {
  if (nv == 4 && (reinterpret_cast<uintptr_t>(p) & 3u) == 0) {
    *reinterpret_cast<unsigned*>(p) = (m[0] ? 1u : 0u) | (m[1] ? 1u << 8 : 0u) | (m[2] ? 1u << 16 : 0u) | (m[3] ? 1u << 24 : 0u);
  } else {
#pragma unroll
    for (int v = 0; v < 4; ++v)
      if (v < nv) p[v] = m[v] ? 1 : 0;
  }
}

__device__ __forceinline__ void load4(const float* __restrict__ p, int nv, float (&q)[4]) {
  if (nv == 4 && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
    ts::load_row<4>(p, q);
  } else {
#pragma unroll
    for (int v = 0; v < 4; ++v) q[v] = v < nv ? p[v] : 0.f;
  }
}

// MODE 0 disparity, 1 flow, 2 depth
template <int MODE, int PAD, bool NEAREST>
__global__ void __launch_bounds__(kFwdThreads)
inverse_warp_fwd_kernel(const WarpArgs a) {
  __shared__ ts::Projection pr;
  const int b = blockIdx.z;
  if (MODE == 2) ts::load_projection(pr, a.K, a.inv_K, a.T, b, a.kdim, a.ikdim);
  const int H = a.H, W = a.W, Hi = a.Hi, Wi = a.Wi;
  const int Wq = (W + 3) >> 2;
  const int q = blockIdx.x * kFwdThreads + threadIdx.x;          // host: H * Wq < 2^31
  const int y = q / Wq;
  if (y >= H) return;
  const int x0 = (q - y * Wq) << 2;
  const int nv = min(4, W - x0);
  const size_t HW = static_cast<size_t>(H) * W;
  const size_t p = static_cast<size_t>(y) * W + x0;
  const float Hm1 = static_cast<float>(H - 1), Wm1 = static_cast<float>(W - 1);
  const float Him1 = static_cast<float>(Hi - 1), Wim1 = static_cast<float>(Wi - 1);
  const float v = static_cast<float>(y);

  float m0[4], m1[4] = {0.f, 0.f, 0.f, 0.f};
  const float* mp = a.motion + static_cast<size_t>(b) * (MODE == 1 ? 2 : 1) * HW + p;
  load4(mp, nv, m0);
  if (MODE == 1) load4(mp + HW, nv, m1);

  float X[4], Y[4];
  if (MODE == 2) {
    float cz[4], fx[4], fy[4], hx[4], hy[4], hz[4];
    bool in[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float u = static_cast<float>(x0 + k);
      const ts::Projected o = ts::project_pixel(pr, u, v, m0[k], a.eps);
      X[k] = o.sx; Y[k] = o.sy;
      cz[k] = o.cz; fx[k] = o.sx - u; fy[k] = o.sy - v;
      hx[k] = o.X; hy[k] = o.Y; hz[k] = o.Z;
      in[k] = ts::projected_inside(o.sx, o.sy, H, W);
    }
    if (blockIdx.y == 0) {
      if (a.tri) ts::store4(a.tri + static_cast<size_t>(b) * HW + p, nv, cz);
      if (a.coord) {
        ts::store4(a.coord + static_cast<size_t>(b) * 2 * HW + p, nv, X);
        ts::store4(a.coord + static_cast<size_t>(b) * 2 * HW + HW + p, nv, Y);
      }
      if (a.flow) {
        ts::store4(a.flow + static_cast<size_t>(b) * 2 * HW + p, nv, fx);
        ts::store4(a.flow + static_cast<size_t>(b) * 2 * HW + HW + p, nv, fy);
      }
      if (a.mask) store_mask4(a.mask + static_cast<size_t>(b) * HW + p, nv, in);
      if (a.homo) {
        const float one[4] = {1.f, 1.f, 1.f, 1.f};
        float* h = a.homo + static_cast<size_t>(b) * 4 * HW + p;
        ts::store4(h, nv, hx);
        ts::store4(h + HW, nv, hy);
        ts::store4(h + 2 * HW, nv, hz);
        ts::store4(h + 3 * HW, nv, one);
      }
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      X[k] = __fadd_rn(static_cast<float>(x0 + k), m0[k]);
      Y[k] = MODE == 1 ? __fadd_rn(v, m1[k]) : v;
    }
  }

  int xa[4], xb[4], ra[4], rb[4];
  unsigned in[4];
  float nw[4], ne[4], sw[4], se[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const Taps t = taps_at<PAD, NEAREST>(X[k], Y[k], Hi, Wi, Hm1, Wm1, Him1, Wim1);
    xa[k] = t.xa; xb[k] = t.xb; ra[k] = t.ra; rb[k] = t.rb;
    in[k] = k < nv ? t.in : 0u;
    nw[k] = __fmul_rn(t.ww, t.wn); ne[k] = __fmul_rn(t.we, t.wn);
    sw[k] = __fmul_rn(t.ww, t.ws); se[k] = __fmul_rn(t.we, t.ws);
  }

  const int c0 = blockIdx.y * a.cpc, c1 = min(a.C, c0 + a.cpc);
  const size_t HWi = static_cast<size_t>(Hi) * Wi;
  for (int c = c0; c < c1; ++c) {
    const float* __restrict__ ic = a.img + (static_cast<size_t>(b) * a.C + c) * HWi;
    float r[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (NEAREST) {
        const float t0 = ic[ra[k] + xa[k]];
        r[k] = (in[k] & 1u) ? t0 : 0.f;
      } else {
        // every address is inside the image (clamped); a tap outside it is replaced by 0 after the load, so that nothing of
        // the clamped pixel (a NaN, say) reaches the sum
        const float t0 = ic[ra[k] + xa[k]], t1 = ic[ra[k] + xb[k]], t2 = ic[rb[k] + xa[k]], t3 = ic[rb[k] + xb[k]];
        float s = __fmul_rn((in[k] & 1u) ? t0 : 0.f, nw[k]);
        s = __fmaf_rn((in[k] & 2u) ? t1 : 0.f, ne[k], s);
        s = __fmaf_rn((in[k] & 4u) ? t2 : 0.f, sw[k], s);
        s = __fmaf_rn((in[k] & 8u) ? t3 : 0.f, se[k], s);
        r[k] = s;
      }
    }
    ts::store4(a.out + (static_cast<size_t>(b) * a.C + c) * HW + p, nv, r);
  }
}

template <int MODE, int PAD, bool NEAREST>
__global__ void __launch_bounds__(kBwdThreads)
inverse_warp_bwd_kernel(const WarpArgs a) {
  __shared__ ts::Projection pr;
  const int b = blockIdx.z;
  if (MODE == 2) ts::load_projection(pr, a.K, a.inv_K, a.T, b, a.kdim, a.ikdim);
  const int H = a.H, W = a.W, Hi = a.Hi, Wi = a.Wi;
  const int HW = H * W;                                           // host: H * W < 2^31
  const int lane = threadIdx.x & (kBwdPixels - 1), slice = threadIdx.x / kBwdPixels;
  const bool live = blockIdx.x * kBwdPixels + lane < HW;           // the last workgroup's spare lanes redo its last pixel, write nothing
  const int p = live ? blockIdx.x * kBwdPixels + lane : HW - 1;
  const int y = p / W, x = p - y * W;
  const float Hm1 = static_cast<float>(H - 1), Wm1 = static_cast<float>(W - 1);
  const float Him1 = static_cast<float>(Hi - 1), Wim1 = static_cast<float>(Wi - 1);
  const float u = static_cast<float>(x), v = static_cast<float>(y);

  const float* mp = a.motion + static_cast<size_t>(b) * (MODE == 1 ? 2 : 1) * HW + p;
  const float m0 = mp[0];
  float X, Y, dsx = 0.f, dsy = 0.f;
  if (MODE == 2) {
    const ts::Projected o = ts::project_pixel(pr, u, v, m0, a.eps);
    X = o.sx; Y = o.sy;
    ts::project_pixel_ddepth(pr, u, v, o, a.eps, dsx, dsy);
  } else {
    X = __fadd_rn(u, m0);
    Y = MODE == 1 ? __fadd_rn(v, mp[HW]) : v;
  }
  const Taps t = taps_at<PAD, NEAREST>(X, Y, Hi, Wi, Hm1, Wm1, Him1, Wim1);
  const float nw = __fmul_rn(t.ww, t.wn), ne = __fmul_rn(t.we, t.wn), sw = __fmul_rn(t.ww, t.ws), se = __fmul_rn(t.we, t.ws);
  const int o0 = t.ra + t.xa, o1 = t.ra + t.xb, o2 = t.rb + t.xa, o3 = t.rb + t.xb;
  const bool want_motion = a.gmotion != nullptr && !NEAREST;

  const int c0 = blockIdx.y * a.cpc, c1 = min(a.C, c0 + a.cpc);
  const size_t HWi = static_cast<size_t>(Hi) * Wi;
  float gx = 0.f, gy = 0.f;
  for (int c = c0 + slice; c < c1; c += kBwdSlices) {              // wave `slice` takes every fourth channel of the range
    const size_t plane = static_cast<size_t>(b) * a.C + c;
    const float g = a.gout[plane * HW + p];
    if (a.out && live) {
      float* gi = a.out + plane * HWi;
      if (NEAREST) {
        if (t.in & 1u) unsafeAtomicAdd(gi + o0, g);
      } else {
        if (t.in & 1u) unsafeAtomicAdd(gi + o0, g * nw);
        if (t.in & 2u) unsafeAtomicAdd(gi + o1, g * ne);
        if (t.in & 4u) unsafeAtomicAdd(gi + o2, g * sw);
        if (t.in & 8u) unsafeAtomicAdd(gi + o3, g * se);
      }
    }
    if (want_motion) {
      const float* __restrict__ ic = a.img + plane * HWi;
      const float t0 = ic[o0], t1 = ic[o1], t2 = ic[o2], t3 = ic[o3];
      const float a0 = (t.in & 1u) ? t0 : 0.f, a1 = (t.in & 2u) ? t1 : 0.f, a2 = (t.in & 4u) ? t2 : 0.f, a3 = (t.in & 8u) ? t3 : 0.f;
      // d/d ix: nw -wn, ne +wn, sw -ws, se +ws;  d/d iy: nw -ww, ne -we, sw +ww, se +we
      gx += g * ((a1 - a0) * t.wn + (a3 - a2) * t.ws);
      gy += g * ((a2 - a0) * t.ww + (a3 - a1) * t.we);
    }
  }
  if (a.gmotion == nullptr) return;
  float* gm = a.gmotion + static_cast<size_t>(b) * (MODE == 1 ? 2 : 1) * HW + p;
  if (NEAREST) {                                                   // a step function of the position
    if (live && slice == 0) { gm[0] = 0.f; if (MODE == 1) gm[HW] = 0.f; }
    return;
  }
  // the four waves' partial sums, added by wave 0 in a fixed order: deterministic
  __shared__ float part[kBwdSlices][2][kBwdPixels];
  part[slice][0][lane] = gx;
  part[slice][1][lane] = gy;
  __syncthreads();
  if (slice != 0 || !live) return;
  gx = ((part[0][0][lane] + part[1][0][lane]) + part[2][0][lane]) + part[3][0][lane];
  gy = ((part[0][1][lane] + part[1][1][lane]) + part[2][1][lane]) + part[3][1][lane];
  // position -> source coordinate: the padding's own derivative, then (ni - 1) / (n - 1) of the two normalisations
  gx *= t.mx * (Wim1 / Wm1);
  gy *= t.my * (Him1 / Hm1);
  if (MODE == 0) gm[0] = gx;
  else if (MODE == 1) { gm[0] = gx; gm[HW] = gy; }
  else gm[0] = gx * dsx + gy * dsy;
}

template <bool BWD, int MODE, int PAD>
void launch_interp(bool nearest, dim3 grid, hipStream_t st, const WarpArgs& a) {
  ts::dispatch_bool(nearest, [&](auto N) {
    if constexpr (BWD) hipLaunchKernelGGL((inverse_warp_bwd_kernel<MODE, PAD, N()>), grid, dim3(kBwdThreads), 0, st, a);
    else hipLaunchKernelGGL((inverse_warp_fwd_kernel<MODE, PAD, N()>), grid, dim3(kFwdThreads), 0, st, a);
  });
}

template <bool BWD, int MODE>
void launch_pad(int pad, bool nearest, dim3 grid, hipStream_t st, const WarpArgs& a) {
  if (pad == ts::kPadZeros) launch_interp<BWD, MODE, ts::kPadZeros>(nearest, grid, st, a);
  else if (pad == ts::kPadBorder) launch_interp<BWD, MODE, ts::kPadBorder>(nearest, grid, st, a);
  else launch_interp<BWD, MODE, ts::kPadReflection>(nearest, grid, st, a);
}

template <bool BWD>
void launch_mode(int mode, int pad, bool nearest, dim3 grid, hipStream_t st, const WarpArgs& a) {
  if (mode == TS_WARP_DISPARITY) launch_pad<BWD, 0>(pad, nearest, grid, st, a);
  else if (mode == TS_WARP_FLOW) launch_pad<BWD, 1>(pad, nearest, grid, st, a);
  else launch_pad<BWD, 2>(pad, nearest, grid, st, a);
}

// sizes, then codes, then the pointers both directions share
int check_common(const char* op, const float* motion, const float* K, const float* inv_K, const float* T, int B, int C, int Hi, int Wi,
                 int H, int W, int mode, int interp, int pad, int k_dim, int inv_k_dim) {
  TS_REQUIRE(B > 0 && C > 0 && Hi > 0 && Wi > 0 && H > 0 && W > 0, TS_ERR_SHAPE, "%s: non-positive size", op);
  TS_REQUIRE(H >= 2 && W >= 2 && Hi >= 2 && Wi >= 2, TS_ERR_SHAPE,
             "%s: H, W, Hi, Wi must be >= 2 (the coordinates are divided by H - 1 and W - 1), got motion %dx%d, image %dx%d", op, H, W,
             Hi, Wi);
  TS_REQUIRE(mode == TS_WARP_DISPARITY || mode == TS_WARP_FLOW || mode == TS_WARP_DEPTH, TS_ERR_UNSUPPORTED, "%s: unknown mode %d", op, mode);
  TS_REQUIRE(interp != TS_WARP_BICUBIC, TS_ERR_UNSUPPORTED, "%s: bicubic interpolation is not built", op);
  TS_REQUIRE(interp == TS_WARP_BILINEAR || interp == TS_WARP_NEAREST, TS_ERR_UNSUPPORTED, "%s: unknown interpolation %d", op, interp);
  TS_REQUIRE(pad == TS_WARP_ZEROS || pad == TS_WARP_BORDER || pad == TS_WARP_REFLECTION, TS_ERR_UNSUPPORTED, "%s: unknown padding %d", op, pad);
  TS_REQUIRE(static_cast<long long>(H) * W < (1ll << 30) && static_cast<long long>(Hi) * Wi < (1ll << 30), TS_ERR_UNSUPPORTED,
             "%s: map too large", op);
  TS_REQUIRE(B <= 65535, TS_ERR_UNSUPPORTED, "%s: batch too large", op);
  TS_REQUIRE_PTR(motion);
  if (mode == TS_WARP_DEPTH) {
    TS_REQUIRE(K != nullptr, TS_ERR_NULL, "%s: depth mode needs K", op);
    TS_REQUIRE(T != nullptr, TS_ERR_NULL, "%s: depth mode needs T_target_to_source", op);
    TS_REQUIRE(inv_K != nullptr, TS_ERR_NULL, "%s: depth mode needs inv_K", op);
    TS_REQUIRE(k_dim == 3 || k_dim == 4, TS_ERR_SHAPE, "%s: K must be 3x3 or 4x4", op);
    TS_REQUIRE(inv_k_dim == 3 || inv_k_dim == 4, TS_ERR_SHAPE, "%s: inv_K must be 3x3 or 4x4", op);
  }
  return TS_OK;
}

// grid.y slices of the channel range: until the grid holds four workgroups per CU
int channels_per_slice(long long blocks_xz, int C) {
  const long long target = 4ll * ts::kNumCU;
  long long slices = (target + blocks_xz - 1) / blocks_xz;
  if (slices < 1) slices = 1;
  if (slices > C) slices = C;
  return static_cast<int>((C + slices - 1) / slices);
}

}  // namespace

extern "C" int ts_inverse_warp_fwd(const float* img, const float* motion, const float* K, const float* inv_K, const float* T, float* out,
                                   float* triangular_depth, float* src_pixel_coord, float* optical_flow, unsigned char* flow_mask,
                                   float* homo_points_3d, int B, int C, int Hi, int Wi, int H, int W, int mode, int interp, int pad,
                                   int k_dim, int inv_k_dim, float eps, void* stream) {
  if (int rc = check_common("inverse_warp_fwd", motion, K, inv_K, T, B, C, Hi, Wi, H, W, mode, interp, pad, k_dim, inv_k_dim)) return rc;
  TS_REQUIRE_PTR(img); TS_REQUIRE_PTR(out);
  WarpArgs a{};
  a.img = img; a.motion = motion; a.K = K; a.inv_K = inv_K; a.T = T; a.out = out;
  if (mode == TS_WARP_DEPTH) {
    a.tri = triangular_depth; a.coord = src_pixel_coord; a.flow = optical_flow; a.mask = flow_mask; a.homo = homo_points_3d;
  }
  a.B = B; a.C = C; a.Hi = Hi; a.Wi = Wi; a.H = H; a.W = W; a.kdim = k_dim; a.ikdim = inv_k_dim; a.eps = eps;
  const long long quads = static_cast<long long>(H) * ((W + 3) / 4);
  const long long bx = (quads + kFwdThreads - 1) / kFwdThreads;
  a.cpc = channels_per_slice(bx * B, C);
  const int slices = (C + a.cpc - 1) / a.cpc;
  TS_REQUIRE(slices <= 65535, TS_ERR_UNSUPPORTED, "inverse_warp_fwd: too many channels");
  launch_mode<false>(mode, pad, interp == TS_WARP_NEAREST, dim3(static_cast<unsigned>(bx), slices, B), ts::as_stream(stream), a);
  return ts::launched("inverse_warp_fwd_kernel");
}

extern "C" int ts_inverse_warp_bwd(const float* img, const float* motion, const float* K, const float* inv_K, const float* T,
                                   const float* grad_out, float* grad_img, float* grad_motion, int B, int C, int Hi, int Wi, int H, int W,
                                   int mode, int interp, int pad, int k_dim, int inv_k_dim, float eps, void* stream) {
  if (int rc = check_common("inverse_warp_bwd", motion, K, inv_K, T, B, C, Hi, Wi, H, W, mode, interp, pad, k_dim, inv_k_dim)) return rc;
  TS_REQUIRE_PTR(grad_out);
  TS_REQUIRE(grad_img != nullptr || grad_motion != nullptr, TS_ERR_NULL, "inverse_warp_bwd: no gradient selected");
  const bool nearest = interp == TS_WARP_NEAREST;
  if (grad_motion != nullptr && !nearest) TS_REQUIRE_PTR(img);
  WarpArgs a{};
  a.img = img; a.motion = motion; a.K = K; a.inv_K = inv_K; a.T = T; a.gout = grad_out; a.out = grad_img; a.gmotion = grad_motion;
  a.B = B; a.C = C; a.Hi = Hi; a.Wi = Wi; a.H = H; a.W = W; a.kdim = k_dim; a.ikdim = inv_k_dim; a.eps = eps;
  const long long bx = (static_cast<long long>(H) * W + kBwdPixels - 1) / kBwdPixels;
  a.cpc = grad_motion != nullptr ? C : channels_per_slice(bx * B, C);       // grad_motion: one workgroup sums every channel, in a fixed order
  const int slices = (C + a.cpc - 1) / a.cpc;
  TS_REQUIRE(slices <= 65535, TS_ERR_UNSUPPORTED, "inverse_warp_bwd: too many channels");
  launch_mode<true>(mode, pad, nearest, dim3(static_cast<unsigned>(bx), slices, B), ts::as_stream(stream), a);
  return ts::launched("inverse_warp_bwd_kernel");
}
