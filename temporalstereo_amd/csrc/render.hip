// Disparity and error colour maps and the 16-bit disparity map on the device, gfx950.
//
// The reference renders every frame with numpy on the host (projects/TemporalStereo/video_inference.py:169-227 `visualize`,
// TemporalStereo.py:488-622 `log_image`; architecture/utils/visualization/disparity_colormap.py):
//   resize               F.interpolate(d * Wg / w, (Hg, Wg), bilinear, align_corners=True)                video_inference.py:182
//   disp_to_color        t = d / max (fp32), s = #(t > cbins), r = (t - cbins[s]) / bins[s], colour = map[s] (1-r) + map[s+1] r;
//                        no clipping: t < 0 and t > 1 extrapolate the first / last segment                             :5-98
//   disp_err_to_color    both maps * 255, E = min(|e| / 3, |e| / gt / 0.05), ten closed classes, later ones win a shared end
//                        point, gt <= 0 stays black                                                                   :102-170
//   disp_err_to_colorbar err = |est - gt| * (gt > 0); the members of each of the six ranges (0,1] (1,2] (2,4] (4,12] (12,16]
//                        (16, max(192, max err)] are mapped onto their share of [0,1] between the range's own minimum and
//                        maximum (`revalue`), then matplotlib's jet (256 entries); with_bar adds a 50-row legend      :172-219
//   16-bit map           (d * 256).astype('uint16')                                                       video_inference.py:220
//
// Up to three launches per call (statistics, its finish, colours):
//   render_stats_kernel  (skipped when nothing data-dependent is asked for) one read of the estimate (full size, or the rescale of
//                        bilinear.hpp in registers) and of the ground truth; per image the NaN-propagating maxima (np.max) of the
//                        estimate, the ground truth and the error, and minimum / maximum / count of the error inside each range.
//                        The six ranges are found in ONE pass although the reference re-values the map in place range after
//                        range: every re-valued number is <= 1 and every later range starts at a bound >= 1, so no pixel a range
//                        has re-valued can enter a later one, and membership is a function of the original error alone.  The
//                        last range's upper bound needs the maximum, which the pass is still computing: when the maximum is a
//                        number every error above 16 is a member, when it is NaN (Python's max(192, nan) is 192) the members
//                        are (16, 192]; both variants are kept and the finish picks one.
//                        Per-workgroup partials, no atomics; render_stats_finish_kernel (one workgroup per image) reduces them
//                        in a fixed order.  Minima, maxima and integer counts are exact in any order: bit-identical run to run.
//   render_color_kernel  one lane per 4 horizontally adjacent pixels (row-aligned) or 1 pixel (ragged widths / unaligned pointers);
//                        the rescale is evaluated again in registers, every selected output is written with vector stores
//                        (fp32 HWC: three float4; uint8 HWC: three dwords; CHW: one float4 / dword per channel; 16-bit: 8 bytes).
//                        The legend rows H .. H+49 depend on the width only and are items of the same grid.
// Row loads and grid sizes: frame_io.hpp; the wave butterflies: reduce.hpp (both shared with evaluation.hip).
#include "bilinear.hpp"
#include "frame_io.hpp"
#include "reduce.hpp"

#include <climits>
#include <cmath>

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = ts::kNumCU * 8;
constexpr int kBarRows = 50;                    // error_bar_height (disparity_colormap.py:181)
constexpr int kRanges = 6;
constexpr int kVariants = kRanges + 1;          // the last range twice: (16, 192] and (16, inf]
constexpr int kPartial = 3 + 3 * kVariants;     // max est, max gt, max err, then min / max / count per variant
constexpr int kStats = TS_RENDER_STATS_FLOATS;  // per image, layout in include/ts_hip.h

// flag word of ts_disp_render_fwd (include/ts_hip.h)
constexpr int F_EST_COLOR = 1, F_GT_COLOR = 2, F_ERR_CLASS = 4, F_ERR_JET = 8, F_U16 = 16, F_UINT8 = 32, F_CHW = 64, F_BAR = 128,
              F_CLIP = 256, F_MAX_SHARED = 512, F_MAX_GIVEN = 1024, F_ALL = 2047;

// upper bounds of the ranges (the last one is data-dependent) and the share of [0,1] each is mapped onto    :189-190
__device__ __constant__ const float kBreak[kRanges] = {1.f, 2.f, 4.f, 12.f, 16.f, 192.f};
__device__ __constant__ const double kPoints[kRanges + 1] = {0.0, 0.25, 0.38, 0.66, 0.83, 0.95, 1.0};
// KITTI error classes: lower bounds (the reference compares the fp32 E with these float64 numbers) and colours / 255   :134-147
__device__ __constant__ const double kClassLo[10] = {0 / 3.0,   0.1875 / 3.0, 0.375 / 3.0, 0.75 / 3.0, 1.5 / 3.0,
                                                     3 / 3.0,   6 / 3.0,      12 / 3.0,    24 / 3.0,   48 / 3.0};
__device__ __constant__ const unsigned char kClassRGB[10][3] = {{49, 54, 149},   {69, 117, 180},  {116, 173, 209}, {171, 217, 233},
                                                                {224, 243, 248}, {254, 224, 144}, {253, 174, 97},  {244, 109, 67},
                                                                {215, 48, 39},   {165, 0, 38}};

struct RenderArgs {
  const float* est;        // [B,1,h,w]
  const float* gt;         // [B,1,Hg,Wg] or NULL
  const float* maxd;       // [B] or NULL
  const float* jet;        // [256][3]
  float* stats;            // [B][kStats]
  void* disp_color;
  void* err_class;
  void* err_jet;
  unsigned short* u16;
  int B, h, w, Hg, Wg;
  float sh, sw, vs, scale16;
  int flags;
};

using ts::nan_max;
using ts::store_rgb;

// V estimates of row y starting at column x0 of image b: read at full size, or rescaled in registers
template <int V>
__device__ __forceinline__ void load_est(const RenderArgs& a, int b, int y, int x0, float (&e)[V]) {
  if (a.h == a.Hg && a.w == a.Wg) {
    ts::load_row<V>(a.est + (static_cast<size_t>(b) * a.Hg + y) * a.Wg + x0, e);
  } else {
    const float* p = a.est + static_cast<size_t>(b) * a.h * a.w;
#pragma unroll
    for (int v = 0; v < V; ++v) e[v] = ts::rescaled(p, a.h, a.w, a.sh, a.sw, a.vs, y, x0 + v);
  }
}

// error_map of disp_err_to_colorbar (:182-183): |est - gt| * valid, literally (a non-finite estimate on an invalid pixel gives NaN)
__device__ __forceinline__ float bar_error(float e, float g) { return __fmul_rn(fabsf(__fsub_rn(e, g)), g > 0.f ? 1.f : 0.f); }

// ---------------------------------------------------------------------------------------------------------------- statistics
// what one lane, and then one workgroup, knows of an image: kPartial values in the layout of `partial`
struct RangeStats {
  float m3[3];                                    // NaN-propagating maxima of the estimate, the ground truth and the error
  float mn[kVariants], mx[kVariants];             // minimum / maximum of the error inside each range
  int cnt[kVariants];

  __device__ __forceinline__ void init() {
    m3[0] = m3[1] = m3[2] = -INFINITY;
#pragma unroll
    for (int k = 0; k < kVariants; ++k) {
      mn[k] = INFINITY; mx[k] = -INFINITY; cnt[k] = 0;
    }
  }

  // one error value into the ranges that hold it
  __device__ __forceinline__ void fold(float r) {
    float lo = 0.f;
#pragma unroll
    for (int k = 0; k < kVariants; ++k) {
      const float hi = k < kRanges ? kBreak[k] : INFINITY;
      if (k == kRanges) lo = kBreak[kRanges - 2];                     // the second variant of the last range starts at 16 too
      if (r > lo && r <= hi) {
        mn[k] = fminf(mn[k], r);
        mx[k] = fmaxf(mx[k], r);
        ++cnt[k];
      }
      lo = hi;
    }
  }

  // over the workgroup: shuffle trees per wave, then lane t < kPartial combines the four waves by kind into out[t]
  __device__ __forceinline__ void block_reduce(float* out) const {
    __shared__ float sf[kThreads / ts::kWave][kPartial];
    const int wave = threadIdx.x / ts::kWave, lane = threadIdx.x & (ts::kWave - 1);
    const float me = ts::wave_nan_max(m3[0]), mg = ts::wave_nan_max(m3[1]), mr = ts::wave_nan_max(m3[2]);
    if (lane == 0) {
      sf[wave][0] = me; sf[wave][1] = mg; sf[wave][2] = mr;
    }
#pragma unroll
    for (int k = 0; k < kVariants; ++k) {
      const float lo = ts::wave_min(mn[k]), hi = ts::wave_max(mx[k]);
      const int c = ts::wave_sum(cnt[k]);
      if (lane == 0) {
        sf[wave][3 + k] = lo;
        sf[wave][3 + kVariants + k] = hi;
        sf[wave][3 + 2 * kVariants + k] = __int_as_float(c);
      }
    }
    __syncthreads();
    const int t = threadIdx.x;
    if (t < kPartial) {
      float r;
      if (t < 3) r = nan_max(nan_max(sf[0][t], sf[1][t]), nan_max(sf[2][t], sf[3][t]));
      else if (t < 3 + kVariants) r = fminf(fminf(sf[0][t], sf[1][t]), fminf(sf[2][t], sf[3][t]));
      else if (t < 3 + 2 * kVariants) r = fmaxf(fmaxf(sf[0][t], sf[1][t]), fmaxf(sf[2][t], sf[3][t]));
      else r = __int_as_float(__float_as_int(sf[0][t]) + __float_as_int(sf[1][t]) + __float_as_int(sf[2][t]) + __float_as_int(sf[3][t]));
      out[t] = r;
    }
  }
};

// grid (workgroups per image, B).  partial [B][gridDim.x][kPartial] (counts as int bits)
template <int V>
__global__ void __launch_bounds__(kThreads) render_stats_kernel(RenderArgs a, float* __restrict__ partial) {
  const int b = blockIdx.y;
  RangeStats s;
  s.init();
  const int items = a.Hg * (a.Wg / V);          // V == 4 only when Wg % 4 == 0
  const int per_row = a.Wg / V;
  for (int it = blockIdx.x * kThreads + threadIdx.x; it < items; it += gridDim.x * kThreads) {
    const int y = it / per_row, x0 = (it - y * per_row) * V;
    float e[V], g[V];
    load_est<V>(a, b, y, x0, e);
#pragma unroll
    for (int v = 0; v < V; ++v) s.m3[0] = nan_max(s.m3[0], e[v]);
    if (a.gt != nullptr) {
      ts::load_row<V>(a.gt + (static_cast<size_t>(b) * a.Hg + y) * a.Wg + x0, g);
#pragma unroll
      for (int v = 0; v < V; ++v) {
        s.m3[1] = nan_max(s.m3[1], g[v]);
        const float r = bar_error(e[v], g[v]);
        s.m3[2] = nan_max(s.m3[2], r);
        s.fold(r);
      }
    }
  }
  s.block_reduce(partial + (static_cast<size_t>(b) * gridDim.x + blockIdx.x) * kPartial);
}

// one workgroup per image: lane t takes the partials t, t+256, ..., then shuffle trees and the four waves in order
__global__ void __launch_bounds__(kThreads) render_stats_finish_kernel(const float* __restrict__ partial, int nb, float* __restrict__ stats) {
  const int b = blockIdx.x;
  RangeStats s;
  s.init();
  for (int i = threadIdx.x; i < nb; i += kThreads) {
    const float* p = partial + (static_cast<size_t>(b) * nb + i) * kPartial;
#pragma unroll
    for (int k = 0; k < 3; ++k) s.m3[k] = nan_max(s.m3[k], p[k]);
#pragma unroll
    for (int k = 0; k < kVariants; ++k) {
      s.mn[k] = fminf(s.mn[k], p[3 + k]);
      s.mx[k] = fmaxf(s.mx[k], p[3 + kVariants + k]);
      s.cnt[k] += __float_as_int(p[3 + 2 * kVariants + k]);
    }
  }
  __shared__ float tot[kPartial];
  s.block_reduce(tot);
  const int t = threadIdx.x;
  __syncthreads();
  if (t < kStats) {
    const float maxerr = tot[2];
    const bool nan_err = maxerr != maxerr;
    const int last = nan_err ? kRanges - 1 : kRanges;                 // which variant of the last range holds its members
    float r = 0.f;
    if (t == 0) r = tot[0];
    else if (t == 1) r = tot[1];
    else if (t == 2) r = nan_max(tot[0], tot[1]);                     // np.max of cat(est, gt)                video_inference.py:201
    else if (t == 3) r = maxerr;
    else if (t == 4) r = (maxerr > 192.f) ? maxerr : 192.f;           // Python's max(192, maxvalue): 192 for a NaN           :189
    else if (t >= 8 && t < 8 + kRanges) r = tot[3 + (t - 8 == kRanges - 1 ? last : t - 8)];
    else if (t >= 16 && t < 16 + kRanges) r = tot[3 + kVariants + (t - 16 == kRanges - 1 ? last : t - 16)];
    else if (t >= 24 && t < 24 + kRanges) r = tot[3 + 2 * kVariants + (t - 24 == kRanges - 1 ? last : t - 24)];
    stats[static_cast<size_t>(b) * kStats + t] = r;
  }
}

// ------------------------------------------------------------------------------------------------------------------- colours
// disp_map (:5-66) of t = d / max.  The reference compares the fp32 t with float64 bin edges and interpolates in float64; here
// the comparison is the same (in float64) and the interpolation is fp32.  map[s] has the bits (R,G,B) = (s>>1, s>>2, s) & 1.
__device__ __forceinline__ void disp_color(float d, float mx, bool clip, float (&c)[3]) {
  constexpr double kEdge[6] = {0.114, 0.299, 0.413, 0.587, 0.701, 0.886};          // cumsum(bins) / 1000
  constexpr double kBins[7] = {114.0, 185.0, 114.0, 174.0, 114.0, 185.0, 114.0};
  const float t = __fdiv_rn(d, mx);
  const double td = static_cast<double>(t);
  int s = 0;
  float edge = 0.f, inv = static_cast<float>(1.0 / (kBins[0] / 1000.0));
#pragma unroll
  for (int k = 0; k < 6; ++k)
    if (td > kEdge[k]) {
      s = k + 1;
      edge = static_cast<float>(kEdge[k]);
      inv = static_cast<float>(1.0 / (kBins[k + 1] / 1000.0));
    }
  const float r = __fmul_rn(__fsub_rn(t, edge), inv), q = __fsub_rn(1.f, r);
  const int s1 = s + 1;
  const float a[3] = {static_cast<float>((s >> 1) & 1), static_cast<float>((s >> 2) & 1), static_cast<float>(s & 1)};
  const float b[3] = {static_cast<float>((s1 >> 1) & 1), static_cast<float>((s1 >> 2) & 1), static_cast<float>(s1 & 1)};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    float v = __fadd_rn(__fmul_rn(a[k], q), __fmul_rn(b[k], r));      // literal: 0 * inf and inf - inf give the reference's NaN
    if (clip) v = v < 0.f ? 0.f : (v > 1.f ? 1.f : v);                // np.clip keeps a NaN
    c[k] = v;
  }
}

// disp_err_to_color (:150-168) of one pixel
__device__ __forceinline__ void err_class_color(float e, float g, float (&c)[3]) {
  const float e255 = __fmul_rn(e, 255.f), g255 = __fmul_rn(g, 255.f);
  c[0] = c[1] = c[2] = 0.f;
  if (!(g255 > 0.f)) return;
  const float E = fabsf(__fsub_rn(e255, g255));
  const float rel = __fdiv_rn(__fdiv_rn(E, g255), 0.05f), ab = __fdiv_rn(E, 3.f);
  const float m = (rel != rel || ab != ab) ? __builtin_nanf("") : fminf(ab, rel);            // np.minimum propagates a NaN
  if (m != m) return;                                                                        // no class holds a NaN: black
  const double md = static_cast<double>(m);
  int cls = 0;
#pragma unroll
  for (int k = 1; k < 10; ++k) cls += md >= kClassLo[k] ? 1 : 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) c[k] = static_cast<float>(static_cast<double>(kClassRGB[cls][k]) / 255.0);
}

// the jet index of one pixel of disp_err_to_colorbar: revalue (:172-178) with the range's own minimum / maximum, then
// matplotlib's Colormap.__call__ on a float32 array (x * 256 truncated, x == 1 -> 255, above -> 255); -1: NaN, the `bad` colour
__device__ __forceinline__ int jet_index(float r, const float* __restrict__ st) {
  if (r != r) return -1;
  float x = r;
  if (r > 0.f) {
    int k = -1;
#pragma unroll
    for (int j = kRanges - 1; j >= 0; --j) {
      const float hi = j == kRanges - 1 ? st[4] : kBreak[j];
      if (r <= hi) k = j;
    }
    if (k >= 0) {
      const float mn = st[8 + k], mx = st[16 + k];
      const float q = __fdiv_rn(__fsub_rn(r, mn), __fadd_rn(__fsub_rn(mx, mn), 1e-7f));
      const double scale = __dsub_rn(kPoints[k + 1], kPoints[k]);
      x = static_cast<float>(__dadd_rn(__dmul_rn(static_cast<double>(q), scale), kPoints[k]));
      if (x != x) return -1;
    }
  }
  const float xi = __fmul_rn(x, 256.f);
  if (xi < 0.f) return 0;
  return xi >= 256.f ? 255 : static_cast<int>(xi);
}

// jet index of column x of the legend (:191, :207-212): six np.linspace pieces in float64, the width shared out as in num_bins
__device__ __forceinline__ int bar_index(int x, int W) {
  const int n8 = W / 8, n4 = W / 4;
  const int nb[kRanges] = {n8, n8, n4, n4, n8, W - (n4 + n4 + n8 + n8 + n8)};
  int j = x, k = 0;
#pragma unroll
  for (int i = 0; i < kRanges - 1; ++i)
    if (k == i && j >= nb[i]) {
      j -= nb[i];
      k = i + 1;
    }
  int n = nb[0];
#pragma unroll
  for (int i = 1; i < kRanges; ++i) n = k == i ? nb[i] : n;
  const double p0 = kPoints[k], p1 = kPoints[k + 1];
  double v = p0;
  if (n > 1) {
    const double step = __ddiv_rn(__dsub_rn(p1, p0), static_cast<double>(n - 1));
    v = j == n - 1 ? p1 : __dadd_rn(__dmul_rn(static_cast<double>(j), step), p0);
  }
  const double xi = __dmul_rn(v, 256.0);
  return xi >= 256.0 ? 255 : static_cast<int>(xi);
}

template <int V, bool U8>
__global__ void __launch_bounds__(kThreads) render_color_kernel(RenderArgs a) {
  __shared__ float sjet[256 * 3];
  const int flags = a.flags;
  if (flags & F_ERR_JET) {                                           // uniform: the whole workgroup stages the table or none does
    for (int i = threadIdx.x; i < 256 * 3; i += kThreads) sjet[i] = a.jet[i];
    __syncthreads();
  }
  const bool chw = (flags & F_CHW) != 0, clip = (flags & F_CLIP) != 0;
  const bool both = (flags & F_EST_COLOR) && (flags & F_GT_COLOR);
  const int disp_rows = both ? 2 * a.Hg : a.Hg;
  const int rows = a.Hg + (((flags & F_ERR_JET) && (flags & F_BAR)) ? kBarRows : 0);
  const int jet_rows = a.Hg + ((flags & F_BAR) ? kBarRows : 0);
  const int per_row = a.Wg / V;
  const long long items = static_cast<long long>(a.B) * rows * per_row;
  for (long long it = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x; it < items;
       it += static_cast<long long>(gridDim.x) * kThreads) {
    const int x0 = static_cast<int>(it % per_row) * V;
    const long long t = it / per_row;
    const int y = static_cast<int>(t % rows), b = static_cast<int>(t / rows);
    float c[V][3];
    if (y >= a.Hg) {                                                 // a legend row
#pragma unroll
      for (int v = 0; v < V; ++v) {
        const int i = bar_index(x0 + v, a.Wg);
        c[v][0] = sjet[3 * i]; c[v][1] = sjet[3 * i + 1]; c[v][2] = sjet[3 * i + 2];
      }
      store_rgb<V, U8>(a.err_jet, chw, jet_rows, a.Wg, b, y, x0, c);
      continue;
    }
    const float* st = a.stats + static_cast<size_t>(b) * kStats;
    float e[V], g[V];
    load_est<V>(a, b, y, x0, e);
    if (a.gt != nullptr) {
      ts::load_row<V>(a.gt + (static_cast<size_t>(b) * a.Hg + y) * a.Wg + x0, g);
    } else {
#pragma unroll
      for (int v = 0; v < V; ++v) g[v] = 0.f;
    }
    if (flags & (F_EST_COLOR | F_GT_COLOR)) {
      const int sel = (flags & F_MAX_SHARED) ? 2 : -1;
      if (flags & F_EST_COLOR) {
        const float mx = (flags & F_MAX_GIVEN) ? a.maxd[b] : st[sel < 0 ? 0 : sel];
#pragma unroll
        for (int v = 0; v < V; ++v) disp_color(e[v], mx, clip, c[v]);
        store_rgb<V, U8>(a.disp_color, chw, disp_rows, a.Wg, b, y, x0, c);
      }
      if (flags & F_GT_COLOR) {
        const float mx = (flags & F_MAX_GIVEN) ? a.maxd[b] : st[sel < 0 ? 1 : sel];
#pragma unroll
        for (int v = 0; v < V; ++v) disp_color(g[v], mx, clip, c[v]);
        store_rgb<V, U8>(a.disp_color, chw, disp_rows, a.Wg, b, both ? y + a.Hg : y, x0, c);
      }
    }
    if (flags & F_ERR_CLASS) {
#pragma unroll
      for (int v = 0; v < V; ++v) err_class_color(e[v], g[v], c[v]);
      store_rgb<V, U8>(a.err_class, chw, a.Hg, a.Wg, b, y, x0, c);
    }
    if (flags & F_ERR_JET) {
#pragma unroll
      for (int v = 0; v < V; ++v) {
        const int i = jet_index(bar_error(e[v], g[v]), st);
        c[v][0] = i < 0 ? 0.f : sjet[3 * i];
        c[v][1] = i < 0 ? 0.f : sjet[3 * i + 1];
        c[v][2] = i < 0 ? 0.f : sjet[3 * i + 2];
      }
      store_rgb<V, U8>(a.err_jet, chw, jet_rows, a.Wg, b, y, x0, c);
    }
    if (flags & F_U16) {
      unsigned q[V];
#pragma unroll
      for (int v = 0; v < V; ++v) {
        const float s = __fmul_rn(e[v], a.scale16);                  // truncation toward zero, saturated, NaN -> 0
        q[v] = !(s > 0.f) ? 0u : (s >= 65535.f ? 65535u : static_cast<unsigned>(s));
      }
      unsigned short* p = a.u16 + (static_cast<size_t>(b) * a.Hg + y) * a.Wg + x0;
      if constexpr (V == 4) *reinterpret_cast<uint2*>(p) = make_uint2(q[0] | (q[1] << 16), q[2] | (q[3] << 16));
      else p[0] = static_cast<unsigned short>(q[0]);
    }
  }
}

// statistics workgroups per image: ~1024 pixels each, the whole grid at most 4 per CU
int stats_blocks(int B, int Hg, int Wg) {
  return ts::grid_blocks(static_cast<long long>(Hg) * Wg, 4 * kThreads, (ts::kNumCU * 4 + B - 1) / B);
}

}  // namespace

extern "C" size_t ts_disp_render_workspace_bytes(int B, int Hg, int Wg) {
  if (B <= 0 || Hg <= 0 || Wg <= 0 || B > 65535) return 0;
  if (static_cast<long long>(B) * (Hg + kBarRows) * Wg > INT_MAX / 4) return 0;
  return ts::round_up(static_cast<size_t>(B) * stats_blocks(B, Hg, Wg) * kPartial * sizeof(float), 256);
}

extern "C" int ts_disp_render_fwd(const float* est, const float* gt, const float* max_disp, const float* jet, int B, int h, int w,
                                  int Hg, int Wg, int flags, float scale16, void* disp_color, void* err_class, void* err_jet,
                                  void* disp_u16, float* stats, void* workspace, void* stream) {
  TS_REQUIRE(B > 0 && B <= 65535 && Hg > 0 && Wg > 0 && h > 0 && w > 0, TS_ERR_SHAPE, "disp_render: bad size");
  TS_REQUIRE(static_cast<long long>(B) * (Hg + kBarRows) * Wg <= INT_MAX / 4, TS_ERR_SHAPE, "disp_render: more than 2^29-1 pixels");
  TS_REQUIRE(static_cast<long long>(h) * w <= INT_MAX, TS_ERR_SHAPE, "disp_render: estimate too large");
  TS_REQUIRE((flags & ~F_ALL) == 0, TS_ERR_SHAPE, "disp_render: unknown flags %d", flags);
  const int outs = flags & (F_EST_COLOR | F_GT_COLOR | F_ERR_CLASS | F_ERR_JET | F_U16);
  TS_REQUIRE(outs != 0, TS_ERR_SHAPE, "disp_render: no output selected");
  TS_REQUIRE(!((flags & F_MAX_SHARED) && (flags & F_MAX_GIVEN)), TS_ERR_SHAPE, "disp_render: shared and given maximum both set");
  TS_REQUIRE(!(flags & F_BAR) || (flags & F_ERR_JET), TS_ERR_SHAPE, "disp_render: the legend belongs to the jet error map");
  TS_REQUIRE_PTR(est);
  if (flags & (F_GT_COLOR | F_ERR_CLASS | F_ERR_JET | F_MAX_SHARED)) TS_REQUIRE_PTR(gt);
  if (flags & (F_EST_COLOR | F_GT_COLOR)) TS_REQUIRE_PTR(disp_color);
  if (flags & F_ERR_CLASS) TS_REQUIRE_PTR(err_class);
  if (flags & F_ERR_JET) {
    TS_REQUIRE_PTR(err_jet); TS_REQUIRE_PTR(jet);
  }
  if (flags & F_U16) {
    TS_REQUIRE_PTR(disp_u16);
    TS_REQUIRE((reinterpret_cast<uintptr_t>(disp_u16) & 1u) == 0, TS_ERR_ALIGN, "disp_render: disp_u16 not 2-byte aligned");
  }
  const bool colors = (flags & (F_EST_COLOR | F_GT_COLOR)) != 0;
  if (colors && (flags & F_MAX_GIVEN)) TS_REQUIRE_PTR(max_disp);
  const bool need_stats = (flags & F_ERR_JET) || (colors && !(flags & F_MAX_GIVEN));
  if (need_stats) {
    TS_REQUIRE_PTR(stats); TS_REQUIRE_PTR(workspace);
  }
  const bool u8 = (flags & F_UINT8) != 0;
  if (!u8)
    for (const void* p : {disp_color, err_class, err_jet})
      TS_REQUIRE((reinterpret_cast<uintptr_t>(p) & 3u) == 0, TS_ERR_ALIGN, "disp_render: fp32 output not 4-byte aligned");

  RenderArgs a{};
  a.est = est; a.gt = gt; a.maxd = max_disp; a.jet = jet; a.stats = stats;
  a.disp_color = disp_color; a.err_class = err_class; a.err_jet = err_jet; a.u16 = static_cast<unsigned short*>(disp_u16);
  a.B = B; a.h = h; a.w = w; a.Hg = Hg; a.Wg = Wg;
  a.sh = ts::ac_scale(h, Hg); a.sw = ts::ac_scale(w, Wg);
  a.vs = static_cast<float>(Wg) / static_cast<float>(w);                       // d * gw / pw (video_inference.py:182)
  a.scale16 = scale16; a.flags = flags;

  // four pixels per lane need whole rows of quads and 16-byte aligned rows of every map that is read or written as quads
  const bool same = h == Hg && w == Wg;
  bool vec_in = Wg % 4 == 0 && (!same || ts::aligned16(est)) && (gt == nullptr || ts::aligned16(gt));
  bool vec = vec_in;
  if (u8) {
    for (const void* p : {disp_color, err_class, err_jet}) vec = vec && (reinterpret_cast<uintptr_t>(p) & 3u) == 0;
  } else {
    for (const void* p : {disp_color, err_class, err_jet}) vec = vec && ts::aligned16(p);
  }
  vec = vec && (reinterpret_cast<uintptr_t>(disp_u16) & 7u) == 0;
  const hipStream_t st = ts::as_stream(stream);
  if (need_stats) {
    const int nb = stats_blocks(B, Hg, Wg);
    float* partial = static_cast<float*>(workspace);
    if (vec_in) hipLaunchKernelGGL(render_stats_kernel<4>, dim3(nb, B), dim3(kThreads), 0, st, a, partial);
    else hipLaunchKernelGGL(render_stats_kernel<1>, dim3(nb, B), dim3(kThreads), 0, st, a, partial);
    if (int rc = ts::launched("render_stats_kernel")) return rc;
    hipLaunchKernelGGL(render_stats_finish_kernel, dim3(B), dim3(kThreads), 0, st, partial, nb, stats);
    if (int rc = ts::launched("render_stats_finish_kernel")) return rc;
  }
  const int rows = Hg + (((flags & F_ERR_JET) && (flags & F_BAR)) ? kBarRows : 0);
  const long long items = static_cast<long long>(B) * rows * (Wg / (vec ? 4 : 1));
  const int nb = ts::grid_blocks(items, kThreads, kMaxBlocks);
  if (vec) {
    if (u8) hipLaunchKernelGGL((render_color_kernel<4, true>), dim3(nb), dim3(kThreads), 0, st, a);
    else hipLaunchKernelGGL((render_color_kernel<4, false>), dim3(nb), dim3(kThreads), 0, st, a);
  } else {
    if (u8) hipLaunchKernelGGL((render_color_kernel<1, true>), dim3(nb), dim3(kThreads), 0, st, a);
    else hipLaunchKernelGGL((render_color_kernel<1, false>), dim3(nb), dim3(kThreads), 0, st, a);
  }
  return ts::launched("render_color_kernel");
}
