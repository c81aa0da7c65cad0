// Training frames augmented on the device, gfx950: uint8 frames and one parameter table in, the training batch's fp32 tensors out.
//
// The reference does this on the host per image (architecture/data/datasets/base.py:65-187): torchvision's ColorJitter (brightness,
// contrast, saturation, hue in a random order) and adjust_gamma on the FULL PIL image, ToTensor, normalize, a random crop, and, on
// the right eye's color_aug, 2-4 rectangles of N(0, 0.1) noise (:157-173).  Here the random draws stay on the host (one table row per
// image and eye, include/ts_hip.h "Augmentation") and the pixels never leave the device:
//
// augment_stats_kernel   contrast blends towards the mean grey level of the WHOLE frame as it stands when contrast is applied, i.e.
//                        after the operations that precede it in that image's order, each with its uint8 rounding.  Grid (P, N):
//                        block (p, n) sums the grey bytes of slice p of image n into partial[n][p] (integers: exact, independent of
//                        the order of summation, so bit-reproducible; no atomics, nothing to zero).  A block whose image has no
//                        contrast operation returns at once, and the operations before contrast are the only ones evaluated.
// augment_apply_kernel   grid (x, N): the window's pixels only.  A block adds its image's P partials, m = int(sum / pixels + 0.5) with
//                        the division in double, and recomputes the chain per pixel from the source bytes: operations in the row's
//                        order, the row's 256-byte gamma table, then the normalisation tables of frame_io.hpp (ts::ByteTables: correctly
//                        rounded divisions, built once per block in LDS).  `color` is byte / 255 of the UN-augmented window.  One
//                        lane = four horizontally adjacent pixels of all three channels; 12 source bytes as three dwords where the
//                        address allows, one 16-byte store per channel and output.  A pixel inside one of the row's rectangles
//                        (the last one that holds it wins) is (n - mean[c]) / std[c] instead, n = 0.1 * Box-Muller of a
//                        Philox-4x32-10 draw keyed by the row's seed with the counter (column, row within the rectangle, channel,
//                        rectangle index): it depends on nothing else -- not on the launch geometry, the batch size, the image's
//                        position in the batch or the stride of the output.
// disp_u16_window_kernel raw / scale where raw > 0 of the window whose origin is the table's (ch, cw) of the LEFT eye's row.
//
// Arithmetic of the colour operations (PIL's, byte for byte; doubles only where PIL's C code computes in double):
//   grey          (19595 R + 38470 G + 7471 B + 0x8000) >> 16
//   blend         t = deg + f * (x - deg) in fp32, two roundings (never fused); 0 if t <= 0, 255 if t >= 255, else truncated
//   brightness    deg = 0;  contrast  deg = m;  saturation  deg = grey(pixel)
//   hue           RGB -> HSV bytes, H += shift (mod 256), HSV -> RGB bytes (the colorsys formulas of PIL's Convert.c)
#include "frame_io.hpp"

#include <climits>

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocksX = ts::kNumCU * 8;
constexpr int kRow = TS_AUGMENT_ROW_INTS;
constexpr int kHead = 32;                // the row's words before the gamma table
constexpr int kMaxParts = 128;           // slices of a frame in the statistics launch
constexpr int kStatPixels = 4096;        // pixels of a slice (at least)

// words of a table row (include/ts_hip.h)
constexpr int R_FLAGS = 0, R_ORDER = 1, R_BRIGHT = 2, R_CONTRAST = 3, R_SAT = 4, R_HUE = 5, R_CH = 6, R_CW = 7, R_NRECT = 8, R_RECT = 9,
              R_SEED = 25, R_GAMMA = 32;
constexpr int OP_BRIGHT = 0, OP_CONTRAST = 1, OP_SAT = 2, OP_HUE = 3;

struct AugArgs {
  const unsigned char* src_l;   // [B,Hs,Ws,3] or [B,3,Hs,Ws]
  const unsigned char* src_r;   // same or NULL
  const int* table;             // [eyes,B,kRow]
  unsigned long long* partial;  // [N,P]
  float* color_l;               // [B,3,H,W] with image stride color_stride, or NULL
  float* color_r;
  float* aug_l;                 // [B,3,H,W] with image stride aug_stride, or NULL
  float* aug_r;
  long long color_stride, aug_stride;
  int B, N, Hs, Ws, H, W, P;
  float mean[3], sd[3];
};

using ts::load_quad;
using ts::store4;

__device__ __forceinline__ int grey_of(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

__device__ __forceinline__ int blend(int deg, int x, float f) {
  const float t = __fadd_rn(static_cast<float>(deg), __fmul_rn(f, static_cast<float>(x - deg)));
  return t <= 0.f ? 0 : (t >= 255.f ? 255 : static_cast<int>(t));
}

__device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

__device__ __forceinline__ void hue_shift(int& r, int& g, int& b, int shift) {
  // RGB -> HSV bytes
  const int maxc = max(r, max(g, b)), minc = min(r, min(g, b));
  int H = 0, S = 0;
  const int V = maxc;
  if (minc != maxc) {
    const float cr = static_cast<float>(maxc - minc);
    const float s = __fdiv_rn(cr, static_cast<float>(maxc));
    const float rc = __fdiv_rn(static_cast<float>(maxc - r), cr), gc = __fdiv_rn(static_cast<float>(maxc - g), cr),
                bc = __fdiv_rn(static_cast<float>(maxc - b), cr);
    float h;
    if (r == maxc) h = __fsub_rn(bc, gc);
    else if (g == maxc) h = static_cast<float>(2.0 + static_cast<double>(rc) - static_cast<double>(bc));
    else h = static_cast<float>(4.0 + static_cast<double>(gc) - static_cast<double>(rc));
    const double w = static_cast<double>(h) / 6.0 + 1.0;          // in (0, 2): fmod(w, 1.0) is w - floor(w), exactly
    h = static_cast<float>(w - floor(w));
    H = clip8(static_cast<int>(static_cast<double>(h) * 255.0));
    S = clip8(static_cast<int>(static_cast<double>(s) * 255.0));
  }
  H = (H + shift) & 255;
  // HSV -> RGB bytes
  if (S == 0) {
    r = g = b = V;
    return;
  }
  const float fs = static_cast<float>(static_cast<double>(S) / 255.0);
  const double h6 = static_cast<double>(H) * 6.0 / 255.0;
  const int i = static_cast<int>(floor(h6));
  const float f = static_cast<float>(h6 - static_cast<double>(static_cast<float>(i)));
  const double dv = static_cast<double>(V), dfs = static_cast<double>(fs);
  const float fsf = __fmul_rn(fs, f);                             // float * float is a float product in C
  const int p = clip8(static_cast<int>(round(dv * (1.0 - dfs))));
  const int q = clip8(static_cast<int>(round(dv * (1.0 - static_cast<double>(fsf)))));
  const int t = clip8(static_cast<int>(round(dv * (1.0 - dfs * (1.0 - static_cast<double>(f))))));
  switch (i % 6) {
    case 0: r = V; g = t; b = p; break;
    case 1: r = q; g = V; b = p; break;
    case 2: r = p; g = V; b = t; break;
    case 3: r = p; g = q; b = V; break;
    case 4: r = t; g = p; b = V; break;
    default: r = V; g = p; b = q; break;
  }
}

// operations [0, count) of the row's order on one pixel; m: the mean grey level for contrast
__device__ __forceinline__ void chain(const int* __restrict__ row, int count, int m, int& r, int& g, int& b) {
  const unsigned order = static_cast<unsigned>(row[R_ORDER]);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (k >= count) break;
    const int op = (order >> (8 * k)) & 255u;
    if (op == OP_BRIGHT) {
      const float f = __int_as_float(row[R_BRIGHT]);
      r = blend(0, r, f); g = blend(0, g, f); b = blend(0, b, f);
    } else if (op == OP_CONTRAST) {
      const float f = __int_as_float(row[R_CONTRAST]);
      r = blend(m, r, f); g = blend(m, g, f); b = blend(m, b, f);
    } else if (op == OP_SAT) {
      const float f = __int_as_float(row[R_SAT]);
      const int y = grey_of(r, g, b);
      r = blend(y, r, f); g = blend(y, g, f); b = blend(y, b, f);
    } else if (op == OP_HUE) {
      hue_shift(r, g, b, row[R_HUE] & 255);
    }
  }
}

// position of contrast in the row's order, 4 when it is absent
__device__ __forceinline__ int contrast_at(const int* row) {
  const unsigned order = static_cast<unsigned>(row[R_ORDER]);
  for (int k = 0; k < 4; ++k)
    if (((order >> (8 * k)) & 255u) == static_cast<unsigned>(OP_CONTRAST)) return k;
  return 4;
}

// sum over the block; the result is valid in every lane
__device__ __forceinline__ unsigned long long block_sum(unsigned long long v, unsigned long long* red) {
#pragma unroll
  for (int o = ts::kWave / 2; o > 0; o >>= 1) v += __shfl_down(v, o, ts::kWave);
  __syncthreads();                                       // red may still be read from an earlier call
  if ((threadIdx.x & (ts::kWave - 1)) == 0) red[threadIdx.x / ts::kWave] = v;
  __syncthreads();
  unsigned long long s = 0;
#pragma unroll
  for (int w = 0; w < kThreads / ts::kWave; ++w) s += red[w];
  return s;
}

template <bool CHW>
__global__ void __launch_bounds__(kThreads) augment_stats_kernel(AugArgs a) {
  __shared__ int row[kHead];
  __shared__ unsigned long long red[kThreads / ts::kWave];
  const int n = blockIdx.y, p = blockIdx.x;
  if (threadIdx.x < kHead) row[threadIdx.x] = a.table[static_cast<size_t>(n) * kRow + threadIdx.x];
  __syncthreads();
  const int kc = contrast_at(row);
  if (kc == 4) return;                                   // this image's partials are never read
  const int eye = n >= a.B ? 1 : 0, b = n - eye * a.B;
  const unsigned char* src = eye ? a.src_r : a.src_l;
  const int pixels = a.Hs * a.Ws;
  const int quads = (pixels + 3) >> 2;
  const int per = (quads + a.P - 1) / a.P;               // quads of a slice
  const int q_end = min(quads, (p + 1) * per);
  unsigned sum = 0;                                      // at most 255 x 4 x ceil(per / 256): far below 2^32
  for (int q = p * per + threadIdx.x; q < q_end; q += kThreads) {
    const int nv = min(4, pixels - 4 * q);
    unsigned px[4][3];
    load_quad<CHW>(src, b, 1, pixels, 0, 4 * q, nv, px);  // the frame as one row of Hs x Ws pixels
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      if (v < nv) {
        int r = px[v][0], g = px[v][1], bl = px[v][2];
        chain(row, kc, 0, r, g, bl);
        sum += static_cast<unsigned>(grey_of(r, g, bl));
      }
    }
  }
  const unsigned long long total = block_sum(sum, red);
  if (threadIdx.x == 0) a.partial[static_cast<size_t>(n) * a.P + p] = total;
}

// ------------------------------------------------------------------------------------------------------------- occlusion noise
__device__ __forceinline__ void philox_round(unsigned (&c)[4], unsigned k0, unsigned k1) {
  const unsigned long long p0 = 0xD2511F53ull * c[0], p1 = 0xCD9E8D57ull * c[2];
  const unsigned hi0 = static_cast<unsigned>(p0 >> 32), lo0 = static_cast<unsigned>(p0);
  const unsigned hi1 = static_cast<unsigned>(p1 >> 32), lo1 = static_cast<unsigned>(p1);
  const unsigned n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
  c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
}

// one N(0, 0.1) value: Philox-4x32-10 of (x, y, channel, rectangle) under the image's seed, Box-Muller of its first two words
__device__ __forceinline__ float noise_at(unsigned seed_lo, unsigned seed_hi, unsigned x, unsigned y, unsigned ch, unsigned rect) {
  unsigned c[4] = {x, y, ch, rect};
  unsigned k0 = seed_lo, k1 = seed_hi;
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    philox_round(c, k0, k1);
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  const float u1 = (static_cast<float>(c[0] >> 8) + 0.5f) * 5.9604644775390625e-08f;      // (0, 1), exact in fp32
  const float u2 = (static_cast<float>(c[1] >> 8) + 0.5f) * 5.9604644775390625e-08f;
  return 0.1f * sqrtf(-2.f * __logf(u1)) * __cosf(6.28318530717958647692f * u2);
}

template <bool CHW>
__global__ void __launch_bounds__(kThreads) augment_apply_kernel(AugArgs a, int items) {
  __shared__ ts::ByteTables t;
  __shared__ int row[kHead];
  __shared__ unsigned char gam[256];
  __shared__ unsigned long long red[kThreads / ts::kWave];
  const int n = blockIdx.y;
  const int eye = n >= a.B ? 1 : 0, b = n - eye * a.B;
  const int* trow = a.table + static_cast<size_t>(n) * kRow;
  {
    const int i = threadIdx.x;                           // kThreads == 256: one byte value per lane
    if (i < kHead) row[i] = trow[i];
    gam[i] = static_cast<unsigned char>((static_cast<unsigned>(trow[R_GAMMA + (i >> 2)]) >> (8 * (i & 3))) & 255u);
  }
  ts::build_byte_tables(a.mean, a.sd, t);                // ends in the barrier that row[] and gam[] need too
  const bool with_gamma = (row[R_FLAGS] & TS_AUGMENT_GAMMA) != 0;
  const bool with_ops = static_cast<unsigned>(row[R_ORDER]) != 0x04040404u;
  int m = 0;
  if (contrast_at(row) < 4) {                            // uniform over the block
    const unsigned long long part = static_cast<int>(threadIdx.x) < a.P ? a.partial[static_cast<size_t>(n) * a.P + threadIdx.x] : 0ull;
    const unsigned long long total = block_sum(part, red);
    m = static_cast<int>(static_cast<double>(total) / static_cast<double>(a.Hs * a.Ws) + 0.5);
  }
  float* color = eye ? a.color_r : a.color_l;
  float* aug = eye ? a.aug_r : a.aug_l;
  if (color == nullptr && aug == nullptr) return;
  const unsigned char* src = eye ? a.src_r : a.src_l;
  const int oy = min(max(row[R_CH], 0), a.Hs - a.H), ox = min(max(row[R_CW], 0), a.Ws - a.W);   // clamped, never read out of bounds
  const int n_rect = min(max(row[R_NRECT], 0), TS_AUGMENT_MAX_RECTS);
  const unsigned seed_lo = static_cast<unsigned>(row[R_SEED]), seed_hi = static_cast<unsigned>(row[R_SEED + 1]);
  const int per_row = (a.W + 3) >> 2;
  for (int it = blockIdx.x * kThreads + threadIdx.x; it < items; it += gridDim.x * kThreads) {
    const int y = it / per_row, x0 = (it - y * per_row) * 4;
    const int nv = min(4, a.W - x0);
    unsigned px[4][3];
    load_quad<CHW>(src, b, a.Hs, a.Ws, y + oy, x0 + ox, nv, px);
    if (color != nullptr) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float q[4] = {t.v[px[0][c]], t.v[px[1][c]], t.v[px[2][c]], t.v[px[3][c]]};
        store4(color + static_cast<size_t>(b) * a.color_stride + (static_cast<size_t>(c) * a.H + y) * a.W + x0, nv, q);
      }
    }
    if (aug == nullptr) continue;
    // the rectangle of each pixel: the last one that holds it, -1 for none
    int hit[4] = {-1, -1, -1, -1};
    for (int k = 0; k < n_rect; ++k) {
      const int sh = row[R_RECT + 4 * k], sw = row[R_RECT + 4 * k + 1], oh = row[R_RECT + 4 * k + 2], ow = row[R_RECT + 4 * k + 3];
      if (y >= sh && y - sh < oh) {
#pragma unroll
        for (int v = 0; v < 4; ++v)
          if (x0 + v >= sw && x0 + v - sw < ow) hit[v] = k;
      }
    }
    float q[3][4];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      if (hit[v] >= 0) {
        const int k = hit[v];
        const unsigned ry = static_cast<unsigned>(y - row[R_RECT + 4 * k]), rx = static_cast<unsigned>(x0 + v - row[R_RECT + 4 * k + 1]);
#pragma unroll
        for (int c = 0; c < 3; ++c)
          q[c][v] = __fdiv_rn(__fsub_rn(noise_at(seed_lo, seed_hi, rx, ry, c, k), a.mean[c]), a.sd[c]);
      } else {
        int r = px[v][0], g = px[v][1], bl = px[v][2];
        if (with_ops) chain(row, 4, m, r, g, bl);
        if (with_gamma) {
          r = gam[r]; g = gam[g]; bl = gam[bl];
        }
        q[0][v] = t.n[0][r]; q[1][v] = t.n[1][g]; q[2][v] = t.n[2][bl];
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c)
      store4(aug + static_cast<size_t>(b) * a.aug_stride + (static_cast<size_t>(c) * a.H + y) * a.W + x0, nv, q[c]);
  }
}

// ----------------------------------------------------------------------------------------------- 16-bit disparity, the window
__global__ void __launch_bounds__(kThreads) disp_u16_window_kernel(const unsigned short* __restrict__ raw, const int* __restrict__ table,
                                                                   int Hs, int Ws, int H, int W, float scale, float* __restrict__ disp,
                                                                   unsigned char* __restrict__ valid, int items) {
  const int b = blockIdx.y;
  const int* row = table + static_cast<size_t>(b) * kRow;
  const int oy = min(max(row[R_CH], 0), Hs - H), ox = min(max(row[R_CW], 0), Ws - W);
  const int per_row = (W + 3) >> 2;
  for (int it = blockIdx.x * kThreads + threadIdx.x; it < items; it += gridDim.x * kThreads) {
    const int y = it / per_row, x0 = (it - y * per_row) * 4;
    const int nv = min(4, W - x0);
    const size_t o = (static_cast<size_t>(b) * H + y) * W + x0;
    unsigned r[4];
    float q[4];
    ts::load_u16_quad(raw + (static_cast<size_t>(b) * Hs + y + oy) * Ws + x0 + ox, nv, r);
    ts::decode_u16_quad(r, scale, q);
    store4(disp + o, nv, q);
    if (valid != nullptr) ts::store_valid4(valid + o, nv, r);
  }
}

int parts_for(int Hs, int Ws) {
  const long long pixels = static_cast<long long>(Hs) * Ws;
  long long p = (pixels + kStatPixels - 1) / kStatPixels;
  if (p > kMaxParts) p = kMaxParts;
  return static_cast<int>(p < 1 ? 1 : p);
}

}  // namespace

extern "C" size_t ts_frames_augment_workspace_bytes(int B, int Hs, int Ws) {
  if (B <= 0 || Hs <= 0 || Ws <= 0) return 0;
  return static_cast<size_t>(2) * B * parts_for(Hs, Ws) * sizeof(unsigned long long);
}

extern "C" int ts_frames_augment_fwd(const void* left, const void* right, int B, int Hs, int Ws, int flags, float mean0, float mean1,
                                     float mean2, float std0, float std1, float std2, int H, int W, const int* table, float* color_l,
                                     float* color_r, long long color_stride, float* color_aug_l, float* color_aug_r,
                                     long long color_aug_stride, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = ts::frames_check_args("frames_augment", "window", B, Hs, Ws, H, W, flags,
                                     {{"left", left}, {"table", table}, {"workspace", workspace}}, right, color_l, color_r, color_aug_l,
                                     color_aug_r, std0, std1, std2))
    return rc;
  TS_REQUIRE(H <= Hs && W <= Ws, TS_ERR_SHAPE, "frames_augment: a %dx%d window does not fit a %dx%d image", H, W, Hs, Ws);
  const int N = right != nullptr ? 2 * B : B;
  TS_REQUIRE(N <= 65535, TS_ERR_SHAPE, "frames_augment: a batch of %d", B);
  TS_REQUIRE(static_cast<long long>(N) * Hs * Ws <= INT_MAX / 4, TS_ERR_SHAPE, "frames_augment: more than 2^29-1 pixels");
  TS_REQUIRE(workspace_bytes >= ts_frames_augment_workspace_bytes(B, Hs, Ws), TS_ERR_SHAPE, "frames_augment: workspace of %zu bytes, %zu needed",
             workspace_bytes, ts_frames_augment_workspace_bytes(B, Hs, Ws));
  if (int rc = ts::frames_check_outputs("frames_augment", H, W, H, W, color_l, color_r, color_stride, color_aug_l, color_aug_r,
                                        color_aug_stride, table))
    return rc;
  TS_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0, TS_ERR_ALIGN, "frames_augment: workspace not 8-byte aligned");

  AugArgs a{};
  a.src_l = static_cast<const unsigned char*>(left); a.src_r = static_cast<const unsigned char*>(right);
  a.table = table; a.partial = static_cast<unsigned long long*>(workspace);
  a.color_l = color_l; a.color_r = color_r; a.aug_l = color_aug_l; a.aug_r = color_aug_r;
  a.color_stride = color_stride; a.aug_stride = color_aug_stride;
  a.B = B; a.N = N; a.Hs = Hs; a.Ws = Ws; a.H = H; a.W = W; a.P = parts_for(Hs, Ws);
  a.mean[0] = mean0; a.mean[1] = mean1; a.mean[2] = mean2; a.sd[0] = std0; a.sd[1] = std1; a.sd[2] = std2;
  const bool chw = (flags & TS_PREPARE_CHW) != 0;
  const hipStream_t st = ts::as_stream(stream);
  if (chw) hipLaunchKernelGGL(augment_stats_kernel<true>, dim3(a.P, N), dim3(kThreads), 0, st, a);
  else hipLaunchKernelGGL(augment_stats_kernel<false>, dim3(a.P, N), dim3(kThreads), 0, st, a);
  const int rc = ts::launched("augment_stats_kernel");
  if (rc != TS_OK) return rc;
  const int items = H * ((W + 3) / 4);
  const dim3 grid(ts::grid_blocks(items, kThreads, kMaxBlocksX), N);
  if (chw) hipLaunchKernelGGL(augment_apply_kernel<true>, grid, dim3(kThreads), 0, st, a, items);
  else hipLaunchKernelGGL(augment_apply_kernel<false>, grid, dim3(kThreads), 0, st, a, items);
  return ts::launched("augment_apply_kernel");
}

extern "C" int ts_disp_u16_window_fwd(const void* raw, int B, int Hs, int Ws, int H, int W, const int* table, float scale, float* disp,
                                      void* valid, void* stream) {
  TS_REQUIRE(B > 0 && Hs > 0 && Ws > 0 && H > 0 && W > 0, TS_ERR_SHAPE, "disp_u16_window: bad size (B %d, %dx%d, window %dx%d)", B, Hs, Ws, H, W);
  TS_REQUIRE(H <= Hs && W <= Ws, TS_ERR_SHAPE, "disp_u16_window: a %dx%d window does not fit a %dx%d map", H, W, Hs, Ws);
  TS_REQUIRE(static_cast<long long>(B) * Hs * Ws <= INT_MAX, TS_ERR_SHAPE, "disp_u16_window: more than 2^31-1 pixels");
  TS_REQUIRE(B <= 65535, TS_ERR_SHAPE, "disp_u16_window: a batch of %d", B);
  TS_REQUIRE(scale > 0.f, TS_ERR_SHAPE, "disp_u16_window: scale must be positive");
  TS_REQUIRE_PTR(raw); TS_REQUIRE_PTR(disp); TS_REQUIRE_PTR(table);
  TS_REQUIRE((reinterpret_cast<uintptr_t>(raw) & 1u) == 0, TS_ERR_ALIGN, "disp_u16_window: raw not 2-byte aligned");
  TS_REQUIRE((reinterpret_cast<uintptr_t>(disp) & 3u) == 0 && (reinterpret_cast<uintptr_t>(table) & 3u) == 0, TS_ERR_ALIGN,
             "disp_u16_window: disp / table not 4-byte aligned");
  const int items = H * ((W + 3) / 4);
  hipLaunchKernelGGL(disp_u16_window_kernel, dim3(ts::grid_blocks(items, kThreads, kMaxBlocksX), B), dim3(kThreads), 0, ts::as_stream(stream),
                     static_cast<const unsigned short*>(raw), table, Hs, Ws, H, W, scale, disp, static_cast<unsigned char*>(valid), items);
  return ts::launched("disp_u16_window_kernel");
}
