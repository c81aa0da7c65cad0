// Optical-flow metrics, Middlebury flow colours, KITTI flow error classes and the KITTI 16-bit flow decode on the device, gfx950.
//
// The reference scores and draws every flow map with torch / numpy on the host:
//   flow_calc_error    valid = not (|gt_u| < 1e-12 and |gt_v| < 1e-12) [sparse], no NaN in gt, lb < rad < ub (strict),
//                      rad = sqrt(gt_u^2 + gt_v^2); err = sqrt((gt_u - est_u)^2 + (gt_v - est_v)^2) over the valid pixels;
//                      {1,2,3,5}px = #(err > t) / N * 100, epe = mean err, all 0 when N < 1      data/evaluation/flow_pixel_error.py:9-96
//   flow_to_color      unknown = |u| or |v| > 1e7 or NaN -> (0, 0), black; u, v / (max_rad + 2^-52), rad, a = atan2(-v, -u) / pi,
//                      fk = (a + 1) / 2 * 54 + 1 into the 55-entry colour wheel (k1 wraps to 1 at 56), then rad <= 1:
//                      1 - rad (1 - col), else 0.75 col                                   utils/visualization/flow_colormap.py:8-167
//   flow_err_to_color  E = sqrt(|gt - est|^2) * F_gt_val, ten closed classes, a later one wins a shared end point, F_gt_val == 0
//                      and NaN stay black                                                                                  :170-220
//   load_png           flow = (raw - 2^15) / 64, both components 0 where the third channel is 0        data/utils/load_flow.py:54-78
// The rescale of an estimate to the ground truth's size is this project's own (losses.rescale_to_full): align-corners bilinear
// (bilinear.hpp), then u * Wg / w and v * Hg / h.
//
// Every quantity that feeds a decision -- rad and err of the metrics, the radii of the colours, E of the classes -- is fp32 in the
// reference's operation order with every product, sum and square root rounded on its own (__fmul_rn / __fadd_rn, and
// __builtin_sqrtf, which is correctly rounded here; __fsqrt_rn is the approximate v_sqrt_f32), so the counts, the classes and the
// maxima are the reference's, bit for bit.  The library is built with -ffp-contract=on: none of these may fuse.
//
//   flow_metrics_kernel        one lane per 4 (row quads) or 1 ground-truth pixel(s), grid-stride over <= 1024 workgroups; per level
//                              the four integer counts and the fp64 sum of err; per-workgroup partials, no atomics
//   flow_metrics_finish_kernel one workgroup adds the partials in a fixed order and writes out[level][5]
//   flow_stats_kernel          (skipped when every maximum is given and no statistics are asked for) per image the maximum radius
//                              of est and of gt with unknown pixels as 0, and the members of the ten error classes
//   flow_stats_finish_kernel   one workgroup per image: maxima and integer counts, exact in any order
//   flow_color_kernel          est and / or gt through the colour wheel, the error classes; fp32 or uint8, HWC or CHW
//   flow_u16_decode_kernel     one lane per row quad: 24 source bytes in, two 16-byte stores and one packed dword out
// Maps are read in place through element strides (frame_io.hpp FlowMap): [B,2,H,W] or [B,H,W,2].
#include "bilinear.hpp"
#include "frame_io.hpp"
#include "reduce.hpp"

#include <climits>

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / ts::kWave;
constexpr int kMaxLevels = 4;
constexpr int kThr = 4;                                   // err > 1, 2, 3, 5
constexpr int kInts = 1 + kMaxLevels * kThr;              // N, then the counts per level x threshold
constexpr int kMetricBlocks = ts::kNumCU * 4;
constexpr int kColorBlocks = ts::kNumCU * 8;
constexpr int kClasses = 10;
constexpr int kStatWords = 2 + kClasses;                  // per-workgroup partial: max rad of est, of gt, the class counts (int bits)
constexpr int kStats = TS_FLOW_STATS_FLOATS;              // per image, layout in include/ts_hip.h
constexpr int kWheel = 55;                                // make_color_wheel: RY 15 + YG 6 + GC 4 + CB 11 + BM 13 + MR 6

constexpr int M_SPARSE = TS_FLOW_SPARSE, M_EST_HWC = TS_FLOW_EST_HWC, M_GT_HWC = TS_FLOW_GT_HWC;
constexpr int F_EST_COLOR = TS_FLOW_RENDER_EST_COLOR, F_GT_COLOR = TS_FLOW_RENDER_GT_COLOR, F_ERR_CLASS = TS_FLOW_RENDER_ERR_CLASS,
              F_STATS = TS_FLOW_RENDER_STATS, F_UINT8 = TS_FLOW_RENDER_UINT8, F_CHW = TS_FLOW_RENDER_CHW,
              F_MAX_SHARED = TS_FLOW_RENDER_MAX_SHARED, F_MAX_GIVEN = TS_FLOW_RENDER_MAX_GIVEN, F_EST_HWC = TS_FLOW_RENDER_EST_HWC,
              F_GT_HWC = TS_FLOW_RENDER_GT_HWC, F_ALL = 1023;

// lower bounds of the KITTI flow error classes (flow_colormap.py:185-196; all exact in fp32) and their colours
__device__ __constant__ const float kClassLo[kClasses] = {0.f, 0.1875f, 0.375f, 0.75f, 1.5f, 3.f, 6.f, 12.f, 24.f, 48.f};
__device__ __constant__ const unsigned char kClassRGB[kClasses][3] = {{49, 54, 149},   {69, 117, 180},  {116, 173, 209}, {171, 217, 233},
                                                                      {224, 243, 248}, {254, 224, 144}, {253, 174, 97},  {244, 109, 67},
                                                                      {215, 48, 39},   {165, 0, 38}};

// sqrt(a^2 + b^2) as numpy and torch evaluate it on fp32 arrays: two products, one sum, one square root, each rounded
__device__ __forceinline__ float radius(float a, float b) {
  return __builtin_sqrtf(__fadd_rn(__fmul_rn(a, a), __fmul_rn(b, b)));
}

// An estimate and the way it is read at the ground truth's size: as it is, or through the align-corners rescale
struct Level {
  ts::FlowMap m;
  float sh, sw, su, sv;            // source steps of the rescale; u * Wg / w, v * Hg / h
};

Level make_level(const float* p, int h, int w, bool hwc, int Hg, int Wg) {
  Level l{};
  l.m = ts::flow_map(p, h, w, hwc);
  l.sh = ts::ac_scale(h, Hg);
  l.sw = ts::ac_scale(w, Wg);
  l.su = static_cast<float>(Wg) / static_cast<float>(w);
  l.sv = static_cast<float>(Hg) / static_cast<float>(h);
  return l;
}

// (u, v) of V pixels of row y from column x0 of image b at the target size (Hg, Wg)
template <int V>
__device__ __forceinline__ void load_level(const Level& l, int Hg, int Wg, int b, int y, int x0, float (&u)[V], float (&v)[V]) {
  if (l.m.h == Hg && l.m.w == Wg) {
    ts::load_uv<V>(l.m, b, y, x0, u, v);
  } else {
    const float* p = l.m.p + b * l.m.sb;
#pragma unroll
    for (int i = 0; i < V; ++i) {
      u[i] = ts::rescaled_at<long long>(p, l.m.sy, l.m.sx, l.m.h, l.m.w, l.sh, l.sw, l.su, y, x0 + i);
      v[i] = ts::rescaled_at<long long>(p + l.m.sc, l.m.sy, l.m.sx, l.m.h, l.m.w, l.sh, l.sw, l.sv, y, x0 + i);
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------- metrics
struct MetricArgs {
  Level est[kMaxLevels];
  ts::FlowMap gt;
  int B, flags;
  float lb, ub;
};

__host__ __device__ constexpr int cnt_idx(int l, int k) { return 1 + l * kThr + k; }

// Workgroup totals of one lane's counts and sums: shuffle trees per wave, then lane v adds the four waves of value v in the
// fixed order ((w0 + w1) + w2) + w3 -- the fp64 totals are reproducible.  Slots of levels >= NL are literal zeros.
template <int NL>
__device__ __forceinline__ void metric_totals(const int (&ci)[kInts], const double (&cd)[kMaxLevels], int* ti, double* td) {
  __shared__ int si[kWaves][kInts];
  __shared__ double sd[kWaves][kMaxLevels];
  const int wave = threadIdx.x / ts::kWave, lane = threadIdx.x & (ts::kWave - 1);
  const int n = ts::wave_sum(ci[0]);
  if (lane == 0) si[wave][0] = n;
#pragma unroll
  for (int l = 0; l < kMaxLevels; ++l) {
#pragma unroll
    for (int k = 0; k < kThr; ++k) {
      const int a = l < NL ? ts::wave_sum(ci[cnt_idx(l, k)]) : 0;
      if (lane == 0) si[wave][cnt_idx(l, k)] = a;
    }
    const double d = l < NL ? ts::wave_sum(cd[l]) : 0.0;
    if (lane == 0) sd[wave][l] = d;
  }
  __syncthreads();
  const int t = threadIdx.x;
  if (t < kInts) ti[t] = si[0][t] + si[1][t] + si[2][t] + si[3][t];
  else if (t < kInts + kMaxLevels) td[t - kInts] = ((sd[0][t - kInts] + sd[1][t - kInts]) + sd[2][t - kInts]) + sd[3][t - kInts];
}

template <int NL, int V>
__global__ void __launch_bounds__(kThreads) flow_metrics_kernel(MetricArgs a, double* __restrict__ psum, int* __restrict__ pcnt) {
  int ci[kInts];
  double cd[kMaxLevels];
#pragma unroll
  for (int v = 0; v < kInts; ++v) ci[v] = 0;
#pragma unroll
  for (int v = 0; v < kMaxLevels; ++v) cd[v] = 0.0;
  const int Hg = a.gt.h, Wg = a.gt.w, per_row = Wg / V;
  const bool sparse = (a.flags & M_SPARSE) != 0;
  const long long items = static_cast<long long>(a.B) * Hg * per_row;
  for (long long it = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x; it < items;
       it += static_cast<long long>(gridDim.x) * kThreads) {
    const int x0 = static_cast<int>(it % per_row) * V;
    const long long t = it / per_row;
    const int y = static_cast<int>(t % Hg), b = static_cast<int>(t / Hg);
    float gu[V], gv[V], eu[NL][V], ev[NL][V];
    ts::load_uv<V>(a.gt, b, y, x0, gu, gv);
#pragma unroll
    for (int l = 0; l < NL; ++l) load_level<V>(a.est[l], Hg, Wg, b, y, x0, eu[l], ev[l]);
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const bool hole = fabsf(gu[v]) < 1e-12f && fabsf(gv[v]) < 1e-12f;               // zero_mask(gt_u) & zero_mask(gt_v)   :58
      const float rad = radius(gu[v], gv[v]);
      if (!(sparse && hole) && gu[v] == gu[v] && gv[v] == gv[v] && rad > a.lb && rad < a.ub) {
        ++ci[0];
#pragma unroll
        for (int l = 0; l < NL; ++l) {
          const float e = radius(__fsub_rn(gu[v], eu[l][v]), __fsub_rn(gv[v], ev[l][v]));
          ci[cnt_idx(l, 0)] += e > 1.f;
          ci[cnt_idx(l, 1)] += e > 2.f;
          ci[cnt_idx(l, 2)] += e > 3.f;
          ci[cnt_idx(l, 3)] += e > 5.f;
          cd[l] += static_cast<double>(e);
        }
      }
    }
  }
  metric_totals<NL>(ci, cd, pcnt + static_cast<size_t>(blockIdx.x) * kInts, psum + static_cast<size_t>(blockIdx.x) * kMaxLevels);
}

// one workgroup: lane t adds the partials t, t+256, ..., then the workgroup totals in their fixed order.
// out[l][k] in the reference's fp32 order: (float)count / (float)N * 100 and (float)(sum / N); 0 when N < 1.
__global__ void __launch_bounds__(kThreads)
flow_metrics_finish_kernel(const double* __restrict__ psum, const int* __restrict__ pcnt, int nb, int n_est, float* __restrict__ out) {
  int ci[kInts];                                      // totals fit: the entry point refuses more than 2^31-1 pixels
  double cd[kMaxLevels];
#pragma unroll
  for (int v = 0; v < kInts; ++v) ci[v] = 0;
#pragma unroll
  for (int v = 0; v < kMaxLevels; ++v) cd[v] = 0.0;
  for (int i = threadIdx.x; i < nb; i += kThreads) {
#pragma unroll
    for (int v = 0; v < kInts; ++v) ci[v] += pcnt[static_cast<size_t>(i) * kInts + v];
#pragma unroll
    for (int v = 0; v < kMaxLevels; ++v) cd[v] += psum[static_cast<size_t>(i) * kMaxLevels + v];
  }
  __shared__ int ti[kInts];
  __shared__ double td[kMaxLevels];
  metric_totals<kMaxLevels>(ci, cd, ti, td);
  __syncthreads();
  const int t = threadIdx.x;
  if (t < n_est * 5) {
    const int l = t / 5, k = t % 5;
    const int N = ti[0];
    float r = 0.f;
    if (N >= 1) {
      if (k < kThr) r = __fmul_rn(__fdiv_rn(static_cast<float>(ti[cnt_idx(l, k)]), static_cast<float>(N)), 100.f);
      else r = static_cast<float>(td[l] / static_cast<double>(N));
    }
    out[t] = r;
  }
}

template <int NL>
void launch_metrics(bool vec, int nb, hipStream_t st, const MetricArgs& a, double* psum, int* pcnt) {
  if (vec) hipLaunchKernelGGL((flow_metrics_kernel<NL, 4>), dim3(nb), dim3(kThreads), 0, st, a, psum, pcnt);
  else hipLaunchKernelGGL((flow_metrics_kernel<NL, 1>), dim3(nb), dim3(kThreads), 0, st, a, psum, pcnt);
}

// metrics workgroups for n ground-truth pixels: ~1024 pixels each, at most 4 per CU (a grid-stride loop takes the rest)
int metric_blocks(long long n) { return ts::grid_blocks(n, 4 * kThreads, kMetricBlocks); }
size_t partial_sum_bytes(int nb) { return ts::round_up(static_cast<size_t>(nb) * kMaxLevels * sizeof(double), 256); }

// ----------------------------------------------------------------------------------------------------------------- rendering
struct RenderArgs {
  Level est;                // read at (Hg, Wg)
  ts::FlowMap gt;           // p NULL when no selected output needs it
  const float* val;         // F_gt_val [B,Hg,Wg] or NULL
  const float* maxr;        // [B] or NULL
  const float* wheel;       // [55][3], 0..255
  float* stats;             // [B][kStats]
  void* color;
  void* err;
  int B, Hg, Wg, flags;
};

__device__ __forceinline__ bool unknown(float u, float v) {                              // idxUnknow                       :70
  return fabsf(u) > 1e7f || fabsf(v) > 1e7f || u != u || v != v;
}

// the radius of a pixel as flow_max_rad sees it: unknown pixels count as (0, 0)
__device__ __forceinline__ float known_radius(float u, float v) { return unknown(u, v) ? 0.f : radius(u, v); }

// E of flow_err_to_color (:198-203) and its class, -1: black (F_gt_val == 0, a NaN, or a negative product)
__device__ __forceinline__ int err_class(float eu, float ev, float gu, float gv, bool has_val, float val) {
  float E = radius(__fsub_rn(gu, eu), __fsub_rn(gv, ev));
  if (has_val) {
    E = __fmul_rn(E, val);
    if (val == 0.f) return -1;
  }
  if (!(E >= 0.f)) return -1;
  int cls = 0;
#pragma unroll
  for (int k = 1; k < kClasses; ++k) cls += E >= kClassLo[k] ? 1 : 0;                    // closed ends, the later class wins
  return cls;
}

// flow_color (:80-140) of one pixel.  maxr: the maximum radius; given: it came from the caller (then "inside" is decided on the
// normalised radius as the reference does; a maximum taken from the data decides it on the unnormalised radius r <= maxr, r
// computed as the reduction computed it, so that the brightest pixel cannot leave the disc through the rounding of u / maxr).
// The angle is evaluated in fp64 and rounded once: the correctly rounded fp32 atan2 up to double rounding, with the true signs
// of -v and -u (the wheel does not close: at u > 0 the colour jumps with the sign of v, signed zeros included).
__device__ __forceinline__ void wheel_color(float u, float v, float maxr, bool given, const float* __restrict__ wheel, float (&c)[3]) {
  c[0] = c[1] = c[2] = 0.f;
  if (unknown(u, v)) return;
  const float r0 = radius(u, v);
  const float den = __fadd_rn(maxr, 0x1p-52f);
  const float un = __fdiv_rn(u, den), vn = __fdiv_rn(v, den);
  const float rad = radius(un, vn);
  const float ang = static_cast<float>(atan2(static_cast<double>(-vn), static_cast<double>(-un)));
  const float a = __fdiv_rn(ang, 3.14159274101257324f);
  const float fk = __fadd_rn(__fmul_rn(__fmul_rn(__fadd_rn(a, 1.f), 0.5f), static_cast<float>(kWheel - 1)), 1.f);
  const int k0 = fk >= 1.f ? (fk < static_cast<float>(kWheel) ? static_cast<int>(fk) : kWheel) : 1;       // a NaN reads entry 1
  const int k1 = k0 == kWheel ? 1 : k0 + 1;
  const float f = __fsub_rn(fk, static_cast<float>(k0)), g = __fsub_rn(1.f, f);
  const bool inside = given ? rad <= 1.f : r0 <= maxr;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float col = __fadd_rn(__fmul_rn(g, wheel[3 * (k0 - 1) + k]), __fmul_rn(f, wheel[3 * (k1 - 1) + k]));
    c[k] = inside ? __fsub_rn(1.f, __fmul_rn(rad, __fsub_rn(1.f, col))) : __fmul_rn(col, 0.75f);
  }
}

// over the workgroup: lane t < kStatWords combines the four waves of value t by kind into out[t] (counts as int bits)
__device__ __forceinline__ void stats_reduce(float me, float mg, const int (&cnt)[kClasses], float* out) {
  __shared__ float sf[kWaves][kStatWords];
  const int wave = threadIdx.x / ts::kWave, lane = threadIdx.x & (ts::kWave - 1);
  me = ts::wave_max(me);
  mg = ts::wave_max(mg);
  if (lane == 0) {
    sf[wave][0] = me; sf[wave][1] = mg;
  }
#pragma unroll
  for (int k = 0; k < kClasses; ++k) {
    const int n = ts::wave_sum(cnt[k]);
    if (lane == 0) sf[wave][2 + k] = __int_as_float(n);
  }
  __syncthreads();
  const int t = threadIdx.x;
  if (t < 2) out[t] = fmaxf(fmaxf(sf[0][t], sf[1][t]), fmaxf(sf[2][t], sf[3][t]));
  else if (t < kStatWords)
    out[t] = __int_as_float(__float_as_int(sf[0][t]) + __float_as_int(sf[1][t]) + __float_as_int(sf[2][t]) + __float_as_int(sf[3][t]));
}

// grid (workgroups per image, B).  partial [B][gridDim.x][kStatWords]
template <int V>
__global__ void __launch_bounds__(kThreads) flow_stats_kernel(RenderArgs a, float* __restrict__ partial) {
  const int b = blockIdx.y;
  float me = 0.f, mg = 0.f;                            // radii are >= 0, so max(-1, np.max(rad)) is the maximum itself
  int cnt[kClasses];
#pragma unroll
  for (int k = 0; k < kClasses; ++k) cnt[k] = 0;
  const int per_row = a.Wg / V, items = a.Hg * per_row;
  for (int it = blockIdx.x * kThreads + threadIdx.x; it < items; it += gridDim.x * kThreads) {
    const int y = it / per_row, x0 = (it - y * per_row) * V;
    float eu[V], ev[V], gu[V], gv[V], val[V];
    load_level<V>(a.est, a.Hg, a.Wg, b, y, x0, eu, ev);
#pragma unroll
    for (int v = 0; v < V; ++v) me = fmaxf(me, known_radius(eu[v], ev[v]));
    if (a.gt.p != nullptr) {
      ts::load_uv<V>(a.gt, b, y, x0, gu, gv);
      if (a.val != nullptr) ts::load_row<V>(a.val + (static_cast<size_t>(b) * a.Hg + y) * a.Wg + x0, val);
#pragma unroll
      for (int v = 0; v < V; ++v) {
        mg = fmaxf(mg, known_radius(gu[v], gv[v]));
        const int cls = err_class(eu[v], ev[v], gu[v], gv[v], a.val != nullptr, a.val != nullptr ? val[v] : 1.f);
#pragma unroll
        for (int k = 0; k < kClasses; ++k) cnt[k] += cls == k;
      }
    }
  }
  stats_reduce(me, mg, cnt, partial + (static_cast<size_t>(b) * gridDim.x + blockIdx.x) * kStatWords);
}

// one workgroup per image: lane t takes the partials t, t+256, ...; maxima and integer sums are exact in any order
__global__ void __launch_bounds__(kThreads) flow_stats_finish_kernel(const float* __restrict__ partial, int nb, float* __restrict__ stats) {
  const int b = blockIdx.x;
  float me = 0.f, mg = 0.f;
  int cnt[kClasses];
#pragma unroll
  for (int k = 0; k < kClasses; ++k) cnt[k] = 0;
  for (int i = threadIdx.x; i < nb; i += kThreads) {
    const float* p = partial + (static_cast<size_t>(b) * nb + i) * kStatWords;
    me = fmaxf(me, p[0]);
    mg = fmaxf(mg, p[1]);
#pragma unroll
    for (int k = 0; k < kClasses; ++k) cnt[k] += __float_as_int(p[2 + k]);
  }
  __shared__ float tot[kStatWords];
  stats_reduce(me, mg, cnt, tot);
  __syncthreads();
  const int t = threadIdx.x;
  if (t < kStats) {
    float r = 0.f;
    if (t < 2) r = tot[t];
    else if (t == 2) r = fmaxf(tot[0], tot[1]);
    else if (t >= 4 && t < 4 + kClasses) r = tot[2 + t - 4];
    stats[static_cast<size_t>(b) * kStats + t] = r;
  }
}

template <int V, bool U8>
__global__ void __launch_bounds__(kThreads) flow_color_kernel(RenderArgs a) {
  __shared__ float wheel[kWheel * 3];
  const int flags = a.flags;
  const bool colors = (flags & (F_EST_COLOR | F_GT_COLOR)) != 0;
  if (colors) {                                                      // uniform: the whole workgroup stages the table or none does
    for (int i = threadIdx.x; i < kWheel * 3; i += kThreads) wheel[i] = __fdiv_rn(a.wheel[i], 255.f);
    __syncthreads();
  }
  const bool chw = (flags & F_CHW) != 0, given = (flags & F_MAX_GIVEN) != 0;
  const bool both = (flags & F_EST_COLOR) && (flags & F_GT_COLOR);
  const int rows = both ? 2 * a.Hg : a.Hg;
  const int per_row = a.Wg / V;
  const long long items = static_cast<long long>(a.B) * a.Hg * per_row;
  for (long long it = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x; it < items;
       it += static_cast<long long>(gridDim.x) * kThreads) {
    const int x0 = static_cast<int>(it % per_row) * V;
    const long long t = it / per_row;
    const int y = static_cast<int>(t % a.Hg), b = static_cast<int>(t / a.Hg);
    float eu[V], ev[V], gu[V], gv[V], c[V][3];
    load_level<V>(a.est, a.Hg, a.Wg, b, y, x0, eu, ev);
    if (a.gt.p != nullptr) {
      ts::load_uv<V>(a.gt, b, y, x0, gu, gv);
    } else {
#pragma unroll
      for (int v = 0; v < V; ++v) gu[v] = gv[v] = 0.f;
    }
    if (colors) {
      const float* st = a.stats + static_cast<size_t>(b) * kStats;
      const bool shared = (flags & F_MAX_SHARED) != 0;
      if (flags & F_EST_COLOR) {
        const float mx = given ? a.maxr[b] : st[shared ? 2 : 0];
#pragma unroll
        for (int v = 0; v < V; ++v) wheel_color(eu[v], ev[v], mx, given, wheel, c[v]);
        ts::store_rgb<V, U8>(a.color, chw, rows, a.Wg, b, y, x0, c);
      }
      if (flags & F_GT_COLOR) {
        const float mx = given ? a.maxr[b] : st[shared ? 2 : 1];
#pragma unroll
        for (int v = 0; v < V; ++v) wheel_color(gu[v], gv[v], mx, given, wheel, c[v]);
        ts::store_rgb<V, U8>(a.color, chw, rows, a.Wg, b, both ? y + a.Hg : y, x0, c);
      }
    }
    if (flags & F_ERR_CLASS) {
      float val[V];
      if (a.val != nullptr) ts::load_row<V>(a.val + (static_cast<size_t>(b) * a.Hg + y) * a.Wg + x0, val);
#pragma unroll
      for (int v = 0; v < V; ++v) {
        const int cls = err_class(eu[v], ev[v], gu[v], gv[v], a.val != nullptr, a.val != nullptr ? val[v] : 1.f);
#pragma unroll
        for (int k = 0; k < 3; ++k) c[v][k] = cls < 0 ? 0.f : __fdiv_rn(static_cast<float>(kClassRGB[cls][k]), 255.f);
      }
      ts::store_rgb<V, U8>(a.err, chw, a.Hg, a.Wg, b, y, x0, c);
    }
  }
}

// statistics workgroups per image: ~1024 pixels each, the whole grid at most 4 per CU
int stats_blocks(int B, int Hg, int Wg) {
  return ts::grid_blocks(static_cast<long long>(Hg) * Wg, 4 * kThreads, (ts::kNumCU * 4 + B - 1) / B);
}

// -------------------------------------------------------------------------------------------------------------------- decode
// the three 16-bit channels of nv <= 4 adjacent pixels of row y from column x0 of image b: ch[c][v]
template <bool CHW>
__device__ __forceinline__ void load_u16_rgb(const unsigned short* __restrict__ raw, int b, int H, int W, int y, int x0, int nv,
                                             unsigned (&ch)[3][4]) {
  if constexpr (CHW) {
#pragma unroll
    for (int c = 0; c < 3; ++c) ts::load_u16_quad(raw + ((static_cast<size_t>(b) * 3 + c) * H + y) * W + x0, nv, ch[c]);
  } else {
    const unsigned short* p = raw + ((static_cast<size_t>(b) * H + y) * W + x0) * 3;
    unsigned q[3][4];                                               // the 3 nv interleaved values, four at a time
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int left = 3 * nv - 4 * k;
      ts::load_u16_quad(p + 4 * k, left < 0 ? 0 : (left > 4 ? 4 : left), q[k]);
    }
#pragma unroll
    for (int i = 0; i < 12; ++i) ch[i % 3][i / 3] = q[i / 4][i % 4];
  }
}

// grid-stride over the row quads of the batch
template <bool CHW>
__global__ void __launch_bounds__(kThreads)
flow_u16_decode_kernel(const unsigned short* __restrict__ raw, int B, int H, int W, float* __restrict__ flow,
                       unsigned char* __restrict__ valid) {
  const int per_row = (W + 3) / 4;
  const long long items = static_cast<long long>(B) * H * per_row;
  for (long long it = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x; it < items;
       it += static_cast<long long>(gridDim.x) * kThreads) {
    const int x0 = static_cast<int>(it % per_row) * 4;
    const long long t = it / per_row;
    const int y = static_cast<int>(t % H), b = static_cast<int>(t / H);
    const int nv = W - x0 < 4 ? W - x0 : 4;
    unsigned ch[3][4];
    load_u16_rgb<CHW>(raw, b, H, W, y, x0, nv, ch);
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      float q[4];
#pragma unroll
      for (int v = 0; v < 4; ++v)                                   // (raw - 2^15) / 64: an integer times a power of two, exact
        q[v] = ch[2][v] != 0u ? __fmul_rn(static_cast<float>(static_cast<int>(ch[c][v]) - 32768), 0.015625f) : 0.f;
      ts::store4(flow + ((static_cast<size_t>(b) * 2 + c) * H + y) * W + x0, nv, q);
    }
    if (valid != nullptr) ts::store_valid4(valid + (static_cast<size_t>(b) * H + y) * W + x0, nv, ch[2]);
  }
}

}  // namespace

extern "C" size_t ts_flow_metrics_workspace_bytes(int B, int Hg, int Wg) {
  if (B <= 0 || Hg <= 0 || Wg <= 0) return 0;
  const long long n = static_cast<long long>(B) * Hg * Wg;
  if (n > INT_MAX / 2) return 0;
  const int nb = metric_blocks(n);
  return partial_sum_bytes(nb) + ts::round_up(static_cast<size_t>(nb) * kInts * sizeof(int), 256);
}

extern "C" int ts_flow_metrics_fwd(const float* est0, const float* est1, const float* est2, const float* est3, int n_est, int h0,
                                   int w0, int h1, int w1, int h2, int w2, int h3, int w3, const float* gt, int B, int Hg, int Wg,
                                   float lb, float ub, int flags, float* out, void* workspace, void* stream) {
  TS_REQUIRE(n_est >= 1 && n_est <= kMaxLevels, TS_ERR_SHAPE, "flow_metrics: n_est must be 1..4 (got %d)", n_est);
  TS_REQUIRE(B > 0 && Hg > 0 && Wg > 0, TS_ERR_SHAPE, "flow_metrics: bad ground-truth size");
  TS_REQUIRE(static_cast<long long>(B) * Hg * Wg <= INT_MAX / 2, TS_ERR_SHAPE, "flow_metrics: more than 2^30-1 pixels");
  TS_REQUIRE((flags & ~(M_SPARSE | M_EST_HWC | M_GT_HWC)) == 0, TS_ERR_SHAPE, "flow_metrics: unknown flags %d", flags);
  const float* est[kMaxLevels] = {est0, est1, est2, est3};
  const int hs[kMaxLevels] = {h0, h1, h2, h3}, ws[kMaxLevels] = {w0, w1, w2, w3};
  MetricArgs a{};
  a.gt = ts::flow_map(gt, Hg, Wg, (flags & M_GT_HWC) != 0);
  bool vec = ts::flow_quads_ok(a.gt);
  for (int l = 0; l < n_est; ++l) {
    TS_REQUIRE(est[l] != nullptr, TS_ERR_NULL, "flow_metrics: est%d is NULL", l);
    TS_REQUIRE(hs[l] > 0 && ws[l] > 0 && static_cast<long long>(B) * hs[l] * ws[l] <= INT_MAX / 2, TS_ERR_SHAPE,
               "flow_metrics: bad size of level %d", l);
    TS_REQUIRE((reinterpret_cast<uintptr_t>(est[l]) & 3u) == 0, TS_ERR_ALIGN, "flow_metrics: est%d not 4-byte aligned", l);
    a.est[l] = make_level(est[l], hs[l], ws[l], (flags & M_EST_HWC) != 0, Hg, Wg);
    if (hs[l] == Hg && ws[l] == Wg) vec = vec && ts::flow_quads_ok(a.est[l].m);
  }
  TS_REQUIRE_PTR(gt); TS_REQUIRE_PTR(out); TS_REQUIRE_PTR(workspace);
  TS_REQUIRE((reinterpret_cast<uintptr_t>(gt) & 3u) == 0 && (reinterpret_cast<uintptr_t>(out) & 3u) == 0, TS_ERR_ALIGN,
             "flow_metrics: gt / out not 4-byte aligned");
  TS_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0, TS_ERR_ALIGN, "flow_metrics: workspace not 8-byte aligned");
  a.B = B; a.flags = flags; a.lb = lb; a.ub = ub;
  const int nb = metric_blocks(static_cast<long long>(B) * Hg * Wg);
  double* psum = reinterpret_cast<double*>(workspace);
  int* pcnt = reinterpret_cast<int*>(reinterpret_cast<char*>(workspace) + partial_sum_bytes(nb));
  const hipStream_t st = ts::as_stream(stream);
  switch (n_est) {
    case 1: launch_metrics<1>(vec, nb, st, a, psum, pcnt); break;
    case 2: launch_metrics<2>(vec, nb, st, a, psum, pcnt); break;
    case 3: launch_metrics<3>(vec, nb, st, a, psum, pcnt); break;
    default: launch_metrics<4>(vec, nb, st, a, psum, pcnt); break;
  }
  if (int rc = ts::launched("flow_metrics_kernel")) return rc;
  hipLaunchKernelGGL(flow_metrics_finish_kernel, dim3(1), dim3(kThreads), 0, st, psum, pcnt, nb, n_est, out);
  return ts::launched("flow_metrics_finish_kernel");
}

extern "C" size_t ts_flow_render_workspace_bytes(int B, int Hg, int Wg) {
  if (B <= 0 || Hg <= 0 || Wg <= 0 || B > 65535) return 0;
  if (static_cast<long long>(B) * Hg * Wg > INT_MAX / 8) return 0;
  return ts::round_up(static_cast<size_t>(B) * stats_blocks(B, Hg, Wg) * kStatWords * sizeof(float), 256);
}

extern "C" int ts_flow_render_fwd(const float* est, const float* gt, const float* gt_val, const float* max_rad, const float* wheel,
                                  int B, int h, int w, int Hg, int Wg, int flags, void* flow_color, void* err_class, float* stats,
                                  void* workspace, void* stream) {
  TS_REQUIRE(B > 0 && B <= 65535 && Hg > 0 && Wg > 0 && h > 0 && w > 0, TS_ERR_SHAPE, "flow_render: bad size");
  TS_REQUIRE(static_cast<long long>(B) * Hg * Wg <= INT_MAX / 8, TS_ERR_SHAPE, "flow_render: more than 2^28-1 pixels");
  TS_REQUIRE(static_cast<long long>(B) * h * w <= INT_MAX / 2, TS_ERR_SHAPE, "flow_render: estimate too large");
  TS_REQUIRE((flags & ~F_ALL) == 0, TS_ERR_SHAPE, "flow_render: unknown flags %d", flags);
  const bool colors = (flags & (F_EST_COLOR | F_GT_COLOR)) != 0, classes = (flags & F_ERR_CLASS) != 0;
  TS_REQUIRE(colors || classes || (flags & F_STATS), TS_ERR_SHAPE, "flow_render: no output selected");
  TS_REQUIRE(!((flags & F_MAX_SHARED) && (flags & F_MAX_GIVEN)), TS_ERR_SHAPE, "flow_render: shared and given maximum both set");
  TS_REQUIRE_PTR(est);
  if (flags & (F_GT_COLOR | F_ERR_CLASS | F_MAX_SHARED)) TS_REQUIRE_PTR(gt);
  TS_REQUIRE(gt != nullptr || gt_val == nullptr, TS_ERR_NULL, "flow_render: a validity map without a ground truth");
  if (colors) {
    TS_REQUIRE_PTR(flow_color); TS_REQUIRE_PTR(wheel);
    if (flags & F_MAX_GIVEN) TS_REQUIRE_PTR(max_rad);
  }
  if (classes) TS_REQUIRE_PTR(err_class);
  const bool need_stats = (flags & F_STATS) || (colors && !(flags & F_MAX_GIVEN));
  if (need_stats) {
    TS_REQUIRE_PTR(stats); TS_REQUIRE_PTR(workspace);
  }
  for (const void* p : {static_cast<const void*>(est), static_cast<const void*>(gt), static_cast<const void*>(gt_val),
                        static_cast<const void*>(max_rad), static_cast<const void*>(wheel), static_cast<const void*>(stats),
                        static_cast<const void*>(workspace)})
    TS_REQUIRE((reinterpret_cast<uintptr_t>(p) & 3u) == 0, TS_ERR_ALIGN, "flow_render: an fp32 pointer is not 4-byte aligned");
  const bool u8 = (flags & F_UINT8) != 0;
  if (!u8)
    for (const void* p : {flow_color, err_class})
      TS_REQUIRE((reinterpret_cast<uintptr_t>(p) & 3u) == 0, TS_ERR_ALIGN, "flow_render: fp32 output not 4-byte aligned");

  RenderArgs a{};
  a.est = make_level(est, h, w, (flags & F_EST_HWC) != 0, Hg, Wg);
  a.gt = ts::flow_map(gt, Hg, Wg, (flags & F_GT_HWC) != 0);
  a.val = gt_val; a.maxr = max_rad; a.wheel = wheel; a.stats = stats;
  a.color = colors ? flow_color : nullptr; a.err = classes ? err_class : nullptr;
  a.B = B; a.Hg = Hg; a.Wg = Wg; a.flags = flags;

  // four pixels per lane need whole rows of quads and 16-byte aligned rows of every map that is read or written as quads
  const bool same = h == Hg && w == Wg;
  const bool vec_in = Wg % 4 == 0 && (!same || ts::flow_quads_ok(a.est.m)) && ts::flow_quads_ok(a.gt) && ts::aligned16(gt_val);
  bool vec = vec_in;
  for (const void* p : {a.color, a.err}) vec = vec && (u8 ? (reinterpret_cast<uintptr_t>(p) & 3u) == 0 : ts::aligned16(p));
  const hipStream_t st = ts::as_stream(stream);
  if (need_stats) {
    const int nb = stats_blocks(B, Hg, Wg);
    float* partial = static_cast<float*>(workspace);
    if (vec_in) hipLaunchKernelGGL(flow_stats_kernel<4>, dim3(nb, B), dim3(kThreads), 0, st, a, partial);
    else hipLaunchKernelGGL(flow_stats_kernel<1>, dim3(nb, B), dim3(kThreads), 0, st, a, partial);
    if (int rc = ts::launched("flow_stats_kernel")) return rc;
    hipLaunchKernelGGL(flow_stats_finish_kernel, dim3(B), dim3(kThreads), 0, st, partial, nb, stats);
    if (int rc = ts::launched("flow_stats_finish_kernel")) return rc;
  }
  if (!colors && !classes) return TS_OK;
  const long long items = static_cast<long long>(B) * Hg * (Wg / (vec ? 4 : 1));
  const int nb = ts::grid_blocks(items, kThreads, kColorBlocks);
  if (vec) {
    if (u8) hipLaunchKernelGGL((flow_color_kernel<4, true>), dim3(nb), dim3(kThreads), 0, st, a);
    else hipLaunchKernelGGL((flow_color_kernel<4, false>), dim3(nb), dim3(kThreads), 0, st, a);
  } else {
    if (u8) hipLaunchKernelGGL((flow_color_kernel<1, true>), dim3(nb), dim3(kThreads), 0, st, a);
    else hipLaunchKernelGGL((flow_color_kernel<1, false>), dim3(nb), dim3(kThreads), 0, st, a);
  }
  return ts::launched("flow_color_kernel");
}

extern "C" int ts_flow_u16_decode_fwd(const void* raw, int B, int H, int W, int flags, float* flow, void* valid, void* stream) {
  TS_REQUIRE(B > 0 && H > 0 && W > 0, TS_ERR_SHAPE, "flow_u16_decode: bad size (B %d, %dx%d)", B, H, W);
  TS_REQUIRE(static_cast<long long>(B) * H * W <= INT_MAX / 4, TS_ERR_SHAPE, "flow_u16_decode: more than 2^29-1 pixels");
  TS_REQUIRE((flags & ~TS_FLOW_U16_CHW) == 0, TS_ERR_SHAPE, "flow_u16_decode: unknown flags %d", flags);
  TS_REQUIRE_PTR(raw); TS_REQUIRE_PTR(flow);
  TS_REQUIRE((reinterpret_cast<uintptr_t>(raw) & 1u) == 0, TS_ERR_ALIGN, "flow_u16_decode: raw not 2-byte aligned");
  TS_REQUIRE((reinterpret_cast<uintptr_t>(flow) & 3u) == 0, TS_ERR_ALIGN, "flow_u16_decode: flow not 4-byte aligned");
  const long long items = static_cast<long long>(B) * H * ((W + 3) / 4);
  const int nb = ts::grid_blocks(items, kThreads, kColorBlocks);
  const unsigned short* r = static_cast<const unsigned short*>(raw);
  if (flags & TS_FLOW_U16_CHW)
    hipLaunchKernelGGL(flow_u16_decode_kernel<true>, dim3(nb), dim3(kThreads), 0, ts::as_stream(stream), r, B, H, W, flow,
                       static_cast<unsigned char*>(valid));
  else
    hipLaunchKernelGGL(flow_u16_decode_kernel<false>, dim3(nb), dim3(kThreads), 0, ts::as_stream(stream), r, B, H, W, flow,
                       static_cast<unsigned char*>(valid));
  return ts::launched("flow_u16_decode_kernel");
}
