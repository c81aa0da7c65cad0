// Disparity evaluation of the validation / test steps on the device, gfx950.
//
// The reference scores every returned disparity on the CPU (projects/TemporalStereo/TemporalStereo.py:170-214, log_metric :463-486):
//   resize      F.interpolate(d * Wg / w, (Hg, Wg), bilinear, align_corners=True)                              :183
//   calc_error  valid = gt > lb, gt < ub (strict, each only when given); |gt - est| over the valid pixels;
//               {1,2,3,5}px = #(|e| > t) / N * 100, epe = mean |e|, all 0 when N < 1      data/evaluation/pixel_error.py:6-71
//   occlusion   w = inverse_warp(gt_right, -gt_left): grid_sample(bilinear, zeros, align_corners) of gt_right at
//               (x - gt_left, y) through the normalise / unnormalise round trip       modeling/layers/inverse_warp.py:48-72
//               occ = |w - gt_left| > 1 or |w| < 1e-6; calc_error(est * m, gt * m) for m = occ and m = 1 - occ  eval.py:45-105
// Note the split is literal: a pixel outside the split enters calc_error as gt' = 0, est' = est * 0, so it is masked out when
// lb >= 0 and counted with error 0 (NaN for a non-finite est) when lb is None or negative.
//
// Two launches per call, for up to four levels:
//   disp_metrics_kernel   one lane per 4 (row-aligned, 16-byte loads) or 1 ground-truth pixel(s), grid-stride over <= 1024
//                         workgroups.  Per pixel: gt, the occlusion bit (once, shared by every level), every level's estimate
//                         (read directly at full size, else the rescale of bilinear.hpp evaluated in registers), and per
//                         level x split the integer counts and the fp64 sum of |e|.  Per-workgroup partials, no atomics.
//   disp_metrics_finish   one workgroup adds the partials in a fixed order (counts exact, fp64 sums deterministic) and writes
//                         out[level][split][5] = {1px, 2px, 3px, 5px, epe}, split = all / occ / noc.
// Row loads and grid sizes: frame_io.hpp; the wave butterflies: reduce.hpp (both shared with render.hip).
#include "bilinear.hpp"
#include "frame_io.hpp"
#include "reduce.hpp"

#include <climits>

namespace {

constexpr int kMaxLevels = 4;
constexpr int kSplits = 3;                                      // all, occ, noc
constexpr int kThr = 4;                                         // |e| > 1, 2, 3, 5
constexpr int kInts = kSplits + kMaxLevels * kSplits * kThr;    // N per split (it does not depend on the level), then the counts
constexpr int kDoubles = kMaxLevels * kSplits;                  // sum |e| per level x split
constexpr int kThreads = 256;
constexpr int kMaxBlocks = ts::kNumCU * 4;

__host__ __device__ constexpr int cnt_idx(int l, int s, int k) { return kSplits + (l * kSplits + s) * kThr + k; }

struct Levels {
  const float* est[kMaxLevels];
  int h[kMaxLevels], w[kMaxLevels];
  float sh[kMaxLevels], sw[kMaxLevels], vs[kMaxLevels];
};

// metrics workgroups for n ground-truth pixels: ~1024 pixels each, at most 4 per CU (a grid-stride loop takes the rest)
int metric_blocks(long long n) { return ts::grid_blocks(n, 4 * kThreads, kMaxBlocks); }

// value of gt_right at the tap (xx, yy) of grid_sample's zero padding: 0 outside the map
__device__ __forceinline__ float tap(const float* __restrict__ gr, int Hg, int Wg, float xx, float yy) {
  const bool in = xx > -1.f && xx < static_cast<float>(Wg) && yy > -1.f && yy < static_cast<float>(Hg);
  return in ? gr[static_cast<size_t>(static_cast<int>(yy)) * Wg + static_cast<int>(xx)] : 0.f;
}

// occlusion bit of eval.py:82-89 at (y, x).  The coordinate round trip X -> 2X/(W-1)-1 -> (X'+1)*((W-1)/2) is not an identity in
// fp32 (nor is it for Y, so a tap row can be y-1 with weight ~1), so every step is rounded on its own, in the order of torch's CPU
// grid_sample; that kernel then accumulates the four taps as a chain of fused multiply-adds (measured against torch on the CPU).
__device__ __forceinline__ bool occluded(const float* __restrict__ gr, int Hg, int Wg, int y, int x, float g) {
  const float X = __fsub_rn(static_cast<float>(x), g);                                   // pixel x + (-gt_left)
  const float xn = __fsub_rn(__fdiv_rn(__fmul_rn(2.f, X), static_cast<float>(Wg - 1)), 1.f);
  const float yn = __fsub_rn(__fdiv_rn(__fmul_rn(2.f, static_cast<float>(y)), static_cast<float>(Hg - 1)), 1.f);
  const float ix = __fmul_rn(__fadd_rn(xn, 1.f), static_cast<float>(Wg - 1) * 0.5f);
  const float iy = __fmul_rn(__fadd_rn(yn, 1.f), static_cast<float>(Hg - 1) * 0.5f);
  const float xw = floorf(ix), yt = floorf(iy);
  const float we = __fsub_rn(ix, xw), ww = __fsub_rn(1.f, we);
  const float ws = __fsub_rn(iy, yt), wn = __fsub_rn(1.f, ws);
  float r = __fmul_rn(tap(gr, Hg, Wg, xw, yt), __fmul_rn(wn, ww));
  r = __fmaf_rn(tap(gr, Hg, Wg, xw + 1.f, yt), __fmul_rn(wn, we), r);
  r = __fmaf_rn(tap(gr, Hg, Wg, xw, yt + 1.f), __fmul_rn(ws, ww), r);
  r = __fmaf_rn(tap(gr, Hg, Wg, xw + 1.f, yt + 1.f), __fmul_rn(ws, we), r);
  return fabsf(__fsub_rn(r, g)) > 1.f || fabsf(r) < 1e-6f;
}

// Workgroup totals of one lane's kInts counts and kDoubles sums: shuffle trees per wave, then lane v (kInts + v) adds the four
// waves of count (sum) v in the fixed order ((w0 + w1) + w2) + w3 into ti[v] (td[v]) -- the fp64 totals are reproducible.
// Only the slots of levels < NL and splits < S are read; the others are literal zeros.
template <int NL, int S>
__device__ __forceinline__ void block_totals(const int (&ci)[kInts], const double (&cd)[kDoubles], int* ti, double* td) {
  __shared__ int si[kThreads / ts::kWave][kInts];
  __shared__ double sd[kThreads / ts::kWave][kDoubles];
  const int wave = threadIdx.x / ts::kWave, lane = threadIdx.x & (ts::kWave - 1);
#pragma unroll
  for (int s = 0; s < kSplits; ++s) {
    const int a = s < S ? ts::wave_sum(ci[s]) : 0;
    if (lane == 0) si[wave][s] = a;
  }
#pragma unroll
  for (int l = 0; l < kMaxLevels; ++l)
#pragma unroll
    for (int s = 0; s < kSplits; ++s) {
      const bool used = l < NL && s < S;
#pragma unroll
      for (int k = 0; k < kThr; ++k) {
        const int a = used ? ts::wave_sum(ci[cnt_idx(l, s, k)]) : 0;
        if (lane == 0) si[wave][cnt_idx(l, s, k)] = a;
      }
      const double d = used ? ts::wave_sum(cd[l * kSplits + s]) : 0.0;
      if (lane == 0) sd[wave][l * kSplits + s] = d;
    }
  __syncthreads();
  const int t = threadIdx.x;
  if (t < kInts) ti[t] = si[0][t] + si[1][t] + si[2][t] + si[3][t];
  else if (t < kInts + kDoubles) td[t - kInts] = ((sd[0][t - kInts] + sd[1][t - kInts]) + sd[2][t - kInts]) + sd[3][t - kInts];
}

// NL levels, OCC: gt_right given (three splits, else only `all`), V pixels per lane (4: row-aligned float4 loads)
template <int NL, bool OCC, int V>
__global__ void __launch_bounds__(kThreads)
disp_metrics_kernel(Levels lv, const float* __restrict__ gt, const float* __restrict__ gtr, int B, int Hg, int Wg, float lb,
                    float ub, int flags, double* __restrict__ psum, int* __restrict__ pcnt) {
  constexpr int S = OCC ? kSplits : 1;
  int ci[kInts];                                      // N per split, then the counts per level x split x threshold
  double cd[kDoubles];                                // sum |e| per level x split
#pragma unroll
  for (int v = 0; v < kInts; ++v) ci[v] = 0;
#pragma unroll
  for (int v = 0; v < kDoubles; ++v) cd[v] = 0.0;
  const bool use_lb = (flags & 1) != 0, use_ub = (flags & 2) != 0;
  const long long HW = static_cast<long long>(Hg) * Wg;
  const long long items = static_cast<long long>(B) * HW / V;
  for (long long it = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x; it < items;
       it += static_cast<long long>(gridDim.x) * kThreads) {
    const long long i = it * V;
    const int x0 = static_cast<int>(i % Wg);
    const long long t = i / Wg;
    const int y = static_cast<int>(t % Hg), b = static_cast<int>(t / Hg);
    float g[V], e[NL][V];
    ts::load_row<V>(gt + i, g);
#pragma unroll
    for (int l = 0; l < NL; ++l) {
      if (lv.h[l] == Hg && lv.w[l] == Wg) {
        ts::load_row<V>(lv.est[l] + i, e[l]);
      } else {
        const float* p = lv.est[l] + static_cast<size_t>(b) * lv.h[l] * lv.w[l];
#pragma unroll
        for (int v = 0; v < V; ++v) e[l][v] = ts::rescaled(p, lv.h[l], lv.w[l], lv.sh[l], lv.sw[l], lv.vs[l], y, x0 + v);
      }
    }
#pragma unroll
    for (int v = 0; v < V; ++v) {
      bool occ = false;
      if constexpr (OCC) occ = occluded(gtr + static_cast<size_t>(b) * HW, Hg, Wg, y, x0 + v, g[v]);
#pragma unroll
      for (int s = 0; s < S; ++s) {
        const bool in = s == 0 || (s == 1 ? occ : !occ);
        const float gs = in ? g[v] : g[v] * 0.f;             // gt * m of eval.py:91-101 (NaN / inf stay non-finite)
        if ((!use_lb || gs > lb) && (!use_ub || gs < ub)) {
          ++ci[s];
#pragma unroll
          for (int l = 0; l < NL; ++l) {
            const float a = fabsf(gs - (in ? e[l][v] : e[l][v] * 0.f));
            ci[cnt_idx(l, s, 0)] += a > 1.f;
            ci[cnt_idx(l, s, 1)] += a > 2.f;
            ci[cnt_idx(l, s, 2)] += a > 3.f;
            ci[cnt_idx(l, s, 3)] += a > 5.f;
            cd[l * kSplits + s] += static_cast<double>(a);
          }
        }
      }
    }
  }
  block_totals<NL, S>(ci, cd, pcnt + static_cast<size_t>(blockIdx.x) * kInts, psum + static_cast<size_t>(blockIdx.x) * kDoubles);
}

// one workgroup: lane t adds the partials t, t+256, ... of every value (all loads independent: one memory latency per 256
// partials, not one per value), then the workgroup totals in their fixed order, so the fp64 sums are reproducible.
// out[l][s][k] in the reference's fp32 order: (float)count / (float)N * 100 and (float)(sum / N); 0 when N < 1.
__global__ void __launch_bounds__(kThreads)
disp_metrics_finish_kernel(const double* __restrict__ psum, const int* __restrict__ pcnt, int nb, int n_est, int splits,
                           float* __restrict__ out) {
  int ci[kInts];                                      // totals fit: the entry point refuses more than 2^31-1 pixels
  double cd[kDoubles];
#pragma unroll
  for (int v = 0; v < kInts; ++v) ci[v] = 0;
#pragma unroll
  for (int v = 0; v < kDoubles; ++v) cd[v] = 0.0;
  for (int i = threadIdx.x; i < nb; i += kThreads) {
#pragma unroll
    for (int v = 0; v < kInts; ++v) ci[v] += pcnt[static_cast<size_t>(i) * kInts + v];
#pragma unroll
    for (int v = 0; v < kDoubles; ++v) cd[v] += psum[static_cast<size_t>(i) * kDoubles + v];
  }
  __shared__ int ti[kInts];
  __shared__ double td[kDoubles];
  block_totals<kMaxLevels, kSplits>(ci, cd, ti, td);
  __syncthreads();
  const int t = threadIdx.x;
  if (t < n_est * kSplits * 5) {
    const int l = t / (kSplits * 5), s = (t / 5) % kSplits, k = t % 5;
    const int N = ti[s];
    float r = 0.f;
    if (s < splits && N >= 1) {
      if (k < kThr) r = __fmul_rn(__fdiv_rn(static_cast<float>(ti[cnt_idx(l, s, k)]), static_cast<float>(N)), 100.f);
      else r = static_cast<float>(td[l * kSplits + s] / static_cast<double>(N));
    }
    out[t] = r;
  }
}

template <int NL, bool OCC>
void launch_metrics(bool vec, int nb, hipStream_t st, const Levels& lv, const float* gt, const float* gtr, int B, int Hg, int Wg,
                    float lb, float ub, int flags, double* psum, int* pcnt) {
  if (vec)
    hipLaunchKernelGGL((disp_metrics_kernel<NL, OCC, 4>), dim3(nb), dim3(kThreads), 0, st, lv, gt, gtr, B, Hg, Wg, lb, ub, flags,
                       psum, pcnt);
  else
    hipLaunchKernelGGL((disp_metrics_kernel<NL, OCC, 1>), dim3(nb), dim3(kThreads), 0, st, lv, gt, gtr, B, Hg, Wg, lb, ub, flags,
                       psum, pcnt);
}

template <int NL>
void launch_metrics(bool occ, bool vec, int nb, hipStream_t st, const Levels& lv, const float* gt, const float* gtr, int B, int Hg,
                    int Wg, float lb, float ub, int flags, double* psum, int* pcnt) {
  if (occ) launch_metrics<NL, true>(vec, nb, st, lv, gt, gtr, B, Hg, Wg, lb, ub, flags, psum, pcnt);
  else launch_metrics<NL, false>(vec, nb, st, lv, gt, gtr, B, Hg, Wg, lb, ub, flags, psum, pcnt);
}

size_t partial_sum_bytes(int nb) { return ts::round_up(static_cast<size_t>(nb) * kDoubles * sizeof(double), 256); }

}  // namespace

extern "C" size_t ts_disp_metrics_workspace_bytes(int B, int Hg, int Wg) {
  if (B <= 0 || Hg <= 0 || Wg <= 0) return 0;
  const long long n = static_cast<long long>(B) * Hg * Wg;
  if (n > INT_MAX) return 0;
  const int nb = metric_blocks(n);
  return partial_sum_bytes(nb) + ts::round_up(static_cast<size_t>(nb) * kInts * sizeof(int), 256);
}

extern "C" int ts_disp_metrics_fwd(const float* est0, const float* est1, const float* est2, const float* est3, int n_est, int h0,
                                   int w0, int h1, int w1, int h2, int w2, int h3, int w3, const float* gt, const float* gt_right,
                                   int B, int Hg, int Wg, float lb, float ub, int flags, float* out, void* workspace,
                                   void* stream) {
  TS_REQUIRE(n_est >= 1 && n_est <= kMaxLevels, TS_ERR_SHAPE, "disp_metrics: n_est must be 1..4 (got %d)", n_est);
  TS_REQUIRE(B > 0 && Hg > 0 && Wg > 0, TS_ERR_SHAPE, "disp_metrics: bad ground-truth size");
  TS_REQUIRE(static_cast<long long>(B) * Hg * Wg <= INT_MAX, TS_ERR_SHAPE, "disp_metrics: more than 2^31-1 pixels");
  TS_REQUIRE(gt_right == nullptr || (Hg >= 2 && Wg >= 2), TS_ERR_SHAPE,
             "disp_metrics: the occlusion warp needs Hg, Wg >= 2 (it divides by H-1 and W-1)");
  TS_REQUIRE((flags & ~3) == 0, TS_ERR_SHAPE, "disp_metrics: unknown flags %d", flags);
  const float* est[kMaxLevels] = {est0, est1, est2, est3};
  const int hs[kMaxLevels] = {h0, h1, h2, h3}, ws[kMaxLevels] = {w0, w1, w2, w3};
  Levels lv{};
  bool vec = (Wg % 4 == 0) && ts::aligned16(gt);
  for (int l = 0; l < n_est; ++l) {
    TS_REQUIRE(est[l] != nullptr, TS_ERR_NULL, "disp_metrics: est%d is NULL", l);
    TS_REQUIRE(hs[l] > 0 && ws[l] > 0, TS_ERR_SHAPE, "disp_metrics: bad size of level %d", l);
    lv.est[l] = est[l];
    lv.h[l] = hs[l];
    lv.w[l] = ws[l];
    lv.sh[l] = ts::ac_scale(hs[l], Hg);
    lv.sw[l] = ts::ac_scale(ws[l], Wg);
    lv.vs[l] = static_cast<float>(Wg) / static_cast<float>(ws[l]);       // d * gw / d.shape[-1] (TemporalStereo.py:183)
    if (hs[l] == Hg && ws[l] == Wg) vec = vec && ts::aligned16(est[l]);
  }
  TS_REQUIRE_PTR(gt); TS_REQUIRE_PTR(out); TS_REQUIRE_PTR(workspace);
  const long long n = static_cast<long long>(B) * Hg * Wg;
  const int nb = metric_blocks(n);
  double* psum = reinterpret_cast<double*>(workspace);
  int* pcnt = reinterpret_cast<int*>(reinterpret_cast<char*>(workspace) + partial_sum_bytes(nb));
  const hipStream_t st = ts::as_stream(stream);
  const bool occ = gt_right != nullptr;
  switch (n_est) {
    case 1: launch_metrics<1>(occ, vec, nb, st, lv, gt, gt_right, B, Hg, Wg, lb, ub, flags, psum, pcnt); break;
    case 2: launch_metrics<2>(occ, vec, nb, st, lv, gt, gt_right, B, Hg, Wg, lb, ub, flags, psum, pcnt); break;
    case 3: launch_metrics<3>(occ, vec, nb, st, lv, gt, gt_right, B, Hg, Wg, lb, ub, flags, psum, pcnt); break;
    default: launch_metrics<4>(occ, vec, nb, st, lv, gt, gt_right, B, Hg, Wg, lb, ub, flags, psum, pcnt); break;
  }
  if (int rc = ts::launched("disp_metrics_kernel")) return rc;
  hipLaunchKernelGGL(disp_metrics_finish_kernel, dim3(1), dim3(kThreads), 0, st, psum, pcnt, nb, n_est, occ ? kSplits : 1, out);
  return ts::launched("disp_metrics_finish_kernel");
}
