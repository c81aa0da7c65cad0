// Input frames prepared on the device, gfx950: uint8 frames in, the network's fp32 tensors out.
//
// The reference does this on the host for every frame (projects/TemporalStereo/video_inference.py:100-110 `read_image`;
// architecture/data/datasets/base.py:99-187 `do_transform`, :231-248 the intrinsics pyramid; video_inference.py:135-140
// `read_disparity`) and then uploads 4-byte floats:
//   ToTensor             v = float(byte) / 255, HWC -> CHW                                     ('color', t, side)
//   normalize            n = (v - mean[c]) / std[c], fp32, in that order
//   evaluation           F.interpolate(n, (H, W), bilinear, align_corners=True)   base.py:183  ('color_aug', t, side)
//   training             n[:, ch:ch+H, cw:cw+W], and the same window of v         base.py:155
//   K pyramid            rows 0 / 1 of K_norm times kw // 2**s / kh // 2**s, np.linalg.pinv in fp64, .float()
//   16-bit ground truth  (raw * (raw > 0)) / 256.0
//
// frames_prepare_kernel  one launch for the whole batch and both eyes.  A byte has 256 values and a channel 3: v and n are tables
//                        (256 + 3 x 256 floats) built once per workgroup in LDS with correctly rounded divisions, so no division is
//                        on the per-pixel path and every value has the bits torch's elementwise kernels give.  Normalise FIRST,
//                        then interpolate: the taps are taken on n (interpolating bytes and normalising after is another function).
//                        One lane = four horizontally adjacent output pixels of all three channels.
//                          copy form (same size, or a crop window with a per-image origin read from the device): 12 source bytes
//                            (three dwords where the address allows, bytes otherwise) -> a 16-byte store per channel and output;
//                          resize form: align-corners taps from bilinear.hpp (`ac_scale`, `lin_src`), any ratio, up or down; the
//                            `color` output (source size) is a second range of items of the same grid.
//                        Plain vector stores; no atomics, no scratch, no workspace.
// intrinsics_pyramid_kernel  one lane per (image, scale): the general 4x4 inverse by cofactors in fp64, rounded once to fp32 (the
//                        structural zeros of an intrinsics matrix come out as exact zeros: every term holds a zero factor).
// disp_u16_decode_kernel four pixels per lane: raw / scale where raw > 0, else 0; optionally the mask raw > 0 as bytes.
// The tables, the quad loads / stores and the 16-bit decode are those of frame_io.hpp, shared with augment.hip.
#include "bilinear.hpp"
#include "frame_io.hpp"

#include <climits>

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = ts::kNumCU * 8;

constexpr int F_CHW = TS_PREPARE_CHW;

struct PrepArgs {
  const unsigned char* src_l;   // [B,Hs,Ws,3] or [B,3,Hs,Ws]
  const unsigned char* src_r;   // same or NULL
  const int* crop;              // [B,2] (ch, cw) or NULL
  float* color_l;               // [B,3,Hc,Wc] with image stride color_stride, or NULL
  float* color_r;
  float* aug_l;                 // [B,3,H,W] with image stride aug_stride, or NULL
  float* aug_r;
  long long color_stride, aug_stride;
  int B, N, Hs, Ws, H, W;
  float mean[3], sd[3];
  float sh, sw;
};

using ts::ByteTables;
using ts::load_quad;
using ts::store4;

// one item of the copy form: four pixels of row y of an [Ho, Wo] window whose origin in the source is (oy, ox)
template <bool CHW>
__device__ __forceinline__ void copy_item(const PrepArgs& a, const ByteTables& t, long long it, int Ho, int Wo, bool with_aug) {
  const int per_row = (Wo + 3) >> 2;
  const int x0 = static_cast<int>(it % per_row) * 4;
  const long long r = it / per_row;
  const int y = static_cast<int>(r % Ho), n = static_cast<int>(r / Ho);
  const int eye = n >= a.B ? 1 : 0, b = n - eye * a.B;
  float* color = eye ? a.color_r : a.color_l;
  float* aug = with_aug ? (eye ? a.aug_r : a.aug_l) : nullptr;
  if (color == nullptr && aug == nullptr) return;
  int oy = 0, ox = 0;
  if (a.crop != nullptr) {      // an origin outside the image is clamped, never read out of bounds
    oy = min(max(a.crop[2 * b], 0), a.Hs - Ho);
    ox = min(max(a.crop[2 * b + 1], 0), a.Ws - Wo);
  }
  const int nv = min(4, Wo - x0);
  unsigned px[4][3];
  load_quad<CHW>(eye ? a.src_r : a.src_l, b, a.Hs, a.Ws, y + oy, x0 + ox, nv, px);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const size_t o = (static_cast<size_t>(c) * Ho + y) * Wo + x0;
    if (color != nullptr) {
      const float q[4] = {t.v[px[0][c]], t.v[px[1][c]], t.v[px[2][c]], t.v[px[3][c]]};
      store4(color + static_cast<size_t>(b) * a.color_stride + o, nv, q);
    }
    if (aug != nullptr) {
      const float q[4] = {t.n[c][px[0][c]], t.n[c][px[1][c]], t.n[c][px[2][c]], t.n[c][px[3][c]]};
      store4(aug + static_cast<size_t>(b) * a.aug_stride + o, nv, q);
    }
  }
}

template <bool CHW>
__device__ __forceinline__ unsigned src_byte(const unsigned char* __restrict__ src, int b, int Hs, int Ws, int y, int x, int c) {
  if constexpr (CHW) return src[((static_cast<size_t>(b) * 3 + c) * Hs + y) * Ws + x];
  else return src[((static_cast<size_t>(b) * Hs + y) * Ws + x) * 3 + c];
}

// one item of the resize form: four pixels of row y of color_aug [H, W]; the expressions of ts::rescaled on the normalised values
template <bool CHW>
__device__ __forceinline__ void resize_item(const PrepArgs& a, const ByteTables& t, long long it) {
  const int per_row = (a.W + 3) >> 2;
  const int x0 = static_cast<int>(it % per_row) * 4;
  const long long r = it / per_row;
  const int y = static_cast<int>(r % a.H), n = static_cast<int>(r / a.H);
  const int eye = n >= a.B ? 1 : 0, b = n - eye * a.B;
  float* aug = eye ? a.aug_r : a.aug_l;
  if (aug == nullptr) return;
  const unsigned char* src = eye ? a.src_r : a.src_l;
  const int nv = min(4, a.W - x0);
  int y0, y1;
  float ly;
  ts::lin_src(a.sh, y, a.Hs, y0, y1, ly);
  y0 = min(y0, a.Hs - 1); y1 = min(y1, a.Hs - 1);
  float q[3][4];
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const int x = min(x0 + v, a.W - 1);           // a lane's columns beyond the row repeat the last one and are not stored
    int xa, xb;
    float lx;
    ts::lin_src(a.sw, x, a.Ws, xa, xb, lx);
    xa = min(xa, a.Ws - 1); xb = min(xb, a.Ws - 1);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float e00 = t.n[c][src_byte<CHW>(src, b, a.Hs, a.Ws, y0, xa, c)], e01 = t.n[c][src_byte<CHW>(src, b, a.Hs, a.Ws, y0, xb, c)];
      const float e10 = t.n[c][src_byte<CHW>(src, b, a.Hs, a.Ws, y1, xa, c)], e11 = t.n[c][src_byte<CHW>(src, b, a.Hs, a.Ws, y1, xb, c)];
      const float top = (1.f - lx) * e00 + lx * e01;
      const float bot = (1.f - lx) * e10 + lx * e11;
      q[c][v] = (1.f - ly) * top + ly * bot;
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c)
    store4(aug + static_cast<size_t>(b) * a.aug_stride + (static_cast<size_t>(c) * a.H + y) * a.W + x0, nv, q[c]);
}

// RESIZE false: items = N x H x ceil(W / 4), both outputs from one read.
// RESIZE true:  the first aug_items items are color_aug [H, W], the rest color [Hs, Ws].
template <bool CHW, bool RESIZE>
__global__ void __launch_bounds__(kThreads) frames_prepare_kernel(PrepArgs a, long long aug_items, long long items) {
  __shared__ ByteTables t;
  ts::build_byte_tables(a.mean, a.sd, t);
  for (long long it = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x; it < items;
       it += static_cast<long long>(gridDim.x) * kThreads) {
    if constexpr (RESIZE) {
      if (it < aug_items) resize_item<CHW>(a, t, it);
      else copy_item<CHW>(a, t, it - aug_items, a.Hs, a.Ws, false);
    } else {
      copy_item<CHW>(a, t, it, a.H, a.W, true);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- intrinsics
template <class T>
__global__ void __launch_bounds__(64) intrinsics_pyramid_kernel(const T* __restrict__ kn, int B, int S, int kh, int kw,
                                                                float* __restrict__ K, float* __restrict__ invK) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * S) return;
  const int b = i / S, s = i - b * S;
  const T* p = kn + static_cast<size_t>(b) * 16;
  const double fw = static_cast<double>(kw >> s), fh = static_cast<double>(kh >> s);      // kw // 2**s, kh // 2**s
  double m[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const double v = static_cast<double>(p[k]);
    m[k] = k < 4 ? v * fw : (k < 8 ? v * fh : v);
  }
  // inverse by cofactors: the 2x2 minors of rows 0,1 (s*) and rows 2,3 (c*)
  const double s0 = m[0] * m[5] - m[4] * m[1], s1 = m[0] * m[6] - m[4] * m[2], s2 = m[0] * m[7] - m[4] * m[3];
  const double s3 = m[1] * m[6] - m[5] * m[2], s4 = m[1] * m[7] - m[5] * m[3], s5 = m[2] * m[7] - m[6] * m[3];
  const double c5 = m[10] * m[15] - m[14] * m[11], c4 = m[9] * m[15] - m[13] * m[11], c3 = m[9] * m[14] - m[13] * m[10];
  const double c2 = m[8] * m[15] - m[12] * m[11], c1 = m[8] * m[14] - m[12] * m[10], c0 = m[8] * m[13] - m[12] * m[9];
  const double det = s0 * c5 - s1 * c4 + s2 * c3 + s3 * c2 - s4 * c1 + s5 * c0;
  double r[16];
  r[0] = m[5] * c5 - m[6] * c4 + m[7] * c3;    r[1] = -m[1] * c5 + m[2] * c4 - m[3] * c3;
  r[2] = m[13] * s5 - m[14] * s4 + m[15] * s3; r[3] = -m[9] * s5 + m[10] * s4 - m[11] * s3;
  r[4] = -m[4] * c5 + m[6] * c2 - m[7] * c1;   r[5] = m[0] * c5 - m[2] * c2 + m[3] * c1;
  r[6] = -m[12] * s5 + m[14] * s2 - m[15] * s1; r[7] = m[8] * s5 - m[10] * s2 + m[11] * s1;
  r[8] = m[4] * c4 - m[5] * c2 + m[7] * c0;    r[9] = -m[0] * c4 + m[1] * c2 - m[3] * c0;
  r[10] = m[12] * s4 - m[13] * s2 + m[15] * s0; r[11] = -m[8] * s4 + m[9] * s2 - m[11] * s0;
  r[12] = -m[4] * c3 + m[5] * c1 - m[6] * c0;  r[13] = m[0] * c3 - m[1] * c1 + m[2] * c0;
  r[14] = -m[12] * s3 + m[13] * s1 - m[14] * s0; r[15] = m[8] * s3 - m[9] * s1 + m[10] * s0;
  float* ko = K + static_cast<size_t>(i) * 16;
  float* io = invK + static_cast<size_t>(i) * 16;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    ko[k] = static_cast<float>(m[k]);
    io[k] = static_cast<float>(r[k] / det);
  }
}

// ----------------------------------------------------------------------------------------------------------- 16-bit disparity
__global__ void __launch_bounds__(kThreads) disp_u16_decode_kernel(const unsigned short* __restrict__ raw, long long n, float scale,
                                                                   float* __restrict__ disp, unsigned char* __restrict__ valid) {
  const long long quads = (n + 3) >> 2;
  for (long long it = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x; it < quads;
       it += static_cast<long long>(gridDim.x) * kThreads) {
    const long long i0 = it * 4;
    const int nv = static_cast<int>(n - i0 < 4 ? n - i0 : 4);
    unsigned r[4];
    float q[4];
    ts::load_u16_quad(raw + i0, nv, r);
    ts::decode_u16_quad(r, scale, q);
    store4(disp + i0, nv, q);
    if (valid != nullptr) ts::store_valid4(valid + i0, nv, r);
  }
}

}  // namespace

extern "C" int ts_frames_prepare_fwd(const void* left, const void* right, int B, int Hs, int Ws, int flags, float mean0, float mean1,
                                     float mean2, float std0, float std1, float std2, int H, int W, const int* crop, float* color_l,
                                     float* color_r, long long color_stride, float* color_aug_l, float* color_aug_r,
                                     long long color_aug_stride, void* stream) {
  if (int rc = ts::frames_check_args("frames_prepare", "target", B, Hs, Ws, H, W, flags, {{"left", left}}, right, color_l, color_r,
                                     color_aug_l, color_aug_r, std0, std1, std2))
    return rc;
  const int N = right != nullptr ? 2 * B : B;
  const bool resize = crop == nullptr && (H != Hs || W != Ws);
  if (crop != nullptr)
    TS_REQUIRE(H <= Hs && W <= Ws, TS_ERR_SHAPE, "frames_prepare: a %dx%d crop window does not fit a %dx%d image", H, W, Hs, Ws);
  const long long big = static_cast<long long>(Hs) * Ws > static_cast<long long>(H) * W ? static_cast<long long>(Hs) * Ws
                                                                                         : static_cast<long long>(H) * W;
  TS_REQUIRE(static_cast<long long>(N) * big <= INT_MAX / 4, TS_ERR_SHAPE, "frames_prepare: more than 2^29-1 pixels");
  const int Hc = resize ? Hs : H, Wc = resize ? Ws : W;
  if (int rc = ts::frames_check_outputs("frames_prepare", Hc, Wc, H, W, color_l, color_r, color_stride, color_aug_l, color_aug_r,
                                        color_aug_stride, crop))
    return rc;

  PrepArgs a{};
  a.src_l = static_cast<const unsigned char*>(left); a.src_r = static_cast<const unsigned char*>(right);
  a.crop = crop;
  a.color_l = color_l; a.color_r = color_r; a.aug_l = color_aug_l; a.aug_r = color_aug_r;
  a.color_stride = color_stride; a.aug_stride = color_aug_stride;
  a.B = B; a.N = N; a.Hs = Hs; a.Ws = Ws; a.H = H; a.W = W;
  a.mean[0] = mean0; a.mean[1] = mean1; a.mean[2] = mean2; a.sd[0] = std0; a.sd[1] = std1; a.sd[2] = std2;
  a.sh = ts::ac_scale(Hs, H); a.sw = ts::ac_scale(Ws, W);
  const bool chw = (flags & F_CHW) != 0;
  const hipStream_t st = ts::as_stream(stream);
  long long aug_items = static_cast<long long>(N) * H * ((W + 3) / 4), items = aug_items;
  if (resize) {
    if (!(color_aug_l || color_aug_r)) aug_items = 0;
    items = aug_items + ((color_l || color_r) ? static_cast<long long>(N) * Hs * ((Ws + 3) / 4) : 0);
    const int nb = ts::grid_blocks(items, kThreads, kMaxBlocks);
    if (chw) hipLaunchKernelGGL((frames_prepare_kernel<true, true>), dim3(nb), dim3(kThreads), 0, st, a, aug_items, items);
    else hipLaunchKernelGGL((frames_prepare_kernel<false, true>), dim3(nb), dim3(kThreads), 0, st, a, aug_items, items);
  } else {
    const int nb = ts::grid_blocks(items, kThreads, kMaxBlocks);
    if (chw) hipLaunchKernelGGL((frames_prepare_kernel<true, false>), dim3(nb), dim3(kThreads), 0, st, a, aug_items, items);
    else hipLaunchKernelGGL((frames_prepare_kernel<false, false>), dim3(nb), dim3(kThreads), 0, st, a, aug_items, items);
  }
  return ts::launched("frames_prepare_kernel");
}

extern "C" int ts_intrinsics_pyramid_fwd(const void* K_norm, int is_fp64, int B, int kh, int kw, int S, float* K, float* inv_K,
                                         void* stream) {
  TS_REQUIRE(B > 0 && S > 0 && S <= 31 && kh > 0 && kw > 0 && B <= INT_MAX / 64, TS_ERR_SHAPE,
             "intrinsics_pyramid: bad size (B %d, S %d, kh %d, kw %d)", B, S, kh, kw);
  TS_REQUIRE(is_fp64 == 0 || is_fp64 == 1, TS_ERR_SHAPE, "intrinsics_pyramid: is_fp64 must be 0 or 1 (got %d)", is_fp64);
  TS_REQUIRE((kh >> (S - 1)) > 0 && (kw >> (S - 1)) > 0, TS_ERR_SHAPE,
             "intrinsics_pyramid: %d scales of %dx%d reach a zero size (a singular K)", S, kh, kw);
  TS_REQUIRE_PTR(K_norm); TS_REQUIRE_PTR(K); TS_REQUIRE_PTR(inv_K);
  TS_REQUIRE((reinterpret_cast<uintptr_t>(K_norm) & (is_fp64 ? 7u : 3u)) == 0, TS_ERR_ALIGN, "intrinsics_pyramid: K_norm misaligned");
  const int n = B * S, nb = (n + 63) / 64;
  const hipStream_t st = ts::as_stream(stream);
  if (is_fp64)
    hipLaunchKernelGGL(intrinsics_pyramid_kernel<double>, dim3(nb), dim3(64), 0, st, static_cast<const double*>(K_norm), B, S, kh, kw, K, inv_K);
  else
    hipLaunchKernelGGL(intrinsics_pyramid_kernel<float>, dim3(nb), dim3(64), 0, st, static_cast<const float*>(K_norm), B, S, kh, kw, K, inv_K);
  return ts::launched("intrinsics_pyramid_kernel");
}

extern "C" int ts_disp_u16_decode_fwd(const void* raw, int B, int H, int W, float scale, float* disp, void* valid, void* stream) {
  TS_REQUIRE(B > 0 && H > 0 && W > 0, TS_ERR_SHAPE, "disp_u16_decode: bad size (B %d, %dx%d)", B, H, W);
  TS_REQUIRE(static_cast<long long>(B) * H * W <= INT_MAX, TS_ERR_SHAPE, "disp_u16_decode: more than 2^31-1 pixels");
  TS_REQUIRE(scale > 0.f, TS_ERR_SHAPE, "disp_u16_decode: scale must be positive");
  TS_REQUIRE_PTR(raw); TS_REQUIRE_PTR(disp);
  TS_REQUIRE((reinterpret_cast<uintptr_t>(raw) & 1u) == 0, TS_ERR_ALIGN, "disp_u16_decode: raw not 2-byte aligned");
  TS_REQUIRE((reinterpret_cast<uintptr_t>(disp) & 3u) == 0, TS_ERR_ALIGN, "disp_u16_decode: disp not 4-byte aligned");
  const long long n = static_cast<long long>(B) * H * W;
  hipLaunchKernelGGL(disp_u16_decode_kernel, dim3(ts::grid_blocks((n + 3) / 4, kThreads, kMaxBlocks)), dim3(kThreads), 0, ts::as_stream(stream),
                     static_cast<const unsigned short*>(raw), n, scale, disp, static_cast<unsigned char*>(valid));
  return ts::launched("disp_u16_decode_kernel");
}
