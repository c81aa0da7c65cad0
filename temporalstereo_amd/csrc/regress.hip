// K4 -- disparity regression for gfx950 (MI355X).
//
//   K4a  top-k soft-argmax with learned per-candidate offset
//        replaces predict_disp()  architecture/modeling/aggregation/TemporalStereo/coarse.py:69-75
//        (== fine.py:70-76, precise.py:61-67): topk -> softmax -> gather(sample+offset) -> sum.
//   K4b  full soft-argmin / argmin over D
//        replaces SOFTARGMIN.forward  architecture/modeling/prediction/soft_argmin.py:38-59 and
//        ARGMIN.forward  architecture/modeling/prediction/argmin.py:35-46.
//
// Layout is [B, D, H, W] with W contiguous, so consecutive lanes own consecutive pixels and every
// load of a candidate plane is a coalesced row segment; the D axis is a stride of H*W.  K4a keeps
// its k best candidates in registers (D <= 14 in the shipped configs).  K4b splits the D axis of a
// pixel over 4 lanes (16 pixels x 4 slices per wavefront) and merges the online-softmax partials
// (max, sum, weighted sum) with wavefront shuffles, which quarters the serial chain at D=192.
// All of it is HBM-bound: inputs read once, outputs written once.
#include "regress_tails.hpp"
#include "ts_common.hpp"

namespace {

constexpr int KMAX = 8;

// ---------------------------------------------------------------------------------------- K4a
template <int K>
__global__ void __launch_bounds__(256)
topk_softargmax_fwd(const float* __restrict__ cost, const float* __restrict__ samp, const float* __restrict__ off,
                    float* __restrict__ disp, float* __restrict__ tdisp, float* __restrict__ tcost,
                    int* __restrict__ tidx, int B, int D, int HW) {
  const long long n = static_cast<long long>(B) * HW;
  for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < n;
       i += static_cast<long long>(gridDim.x) * blockDim.x) {
    const int b = static_cast<int>(i / HW);
    const int p = static_cast<int>(i - static_cast<long long>(b) * HW);
    const size_t base = static_cast<size_t>(b) * D * HW + p;
    float bc[K], td[K];
    int bi[K];
    const float acc = ts_tail::topk_softargmax_pixel<K>(cost + base, samp + base, off + base, D, HW, bc, bi, td);
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const size_t ko = (static_cast<size_t>(b) * K + j) * HW + p;
      tdisp[ko] = td[j];
      tcost[ko] = bc[j];
      if (tidx) tidx[ko] = bi[j];
    }
    disp[i] = acc;
  }
}

// grads of (disp, topk_disp, topk_cost) -> grads of (cost, sample (+offset: same tensor))
template <int K>
__global__ void __launch_bounds__(256)
topk_softargmax_bwd(const float* __restrict__ tdisp, const float* __restrict__ tcost, const int* __restrict__ tidx,
                    const float* __restrict__ disp, const float* __restrict__ gdisp, const float* __restrict__ gtd,
                    const float* __restrict__ gtc, float* __restrict__ gcost, float* __restrict__ gsamp,
                    int B, int D, int HW) {
  const long long n = static_cast<long long>(B) * HW;
  for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < n;
       i += static_cast<long long>(gridDim.x) * blockDim.x) {
    const int b = static_cast<int>(i / HW);
    const int p = static_cast<int>(i - static_cast<long long>(b) * HW);
    const size_t base = static_cast<size_t>(b) * D * HW + p;
    for (int d = 0; d < D; ++d) {
      if (gcost) gcost[base + static_cast<size_t>(d) * HW] = 0.f;
      if (gsamp) gsamp[base + static_cast<size_t>(d) * HW] = 0.f;
    }
    float c[K], td[K], w[K], den = 0.f;
    int idx[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const size_t ko = (static_cast<size_t>(b) * K + j) * HW + p;
      c[j] = tcost[ko]; td[j] = tdisp[ko]; idx[j] = tidx[ko];
    }
#pragma unroll
    for (int j = 0; j < K; ++j) { w[j] = expf(c[j] - c[0]); den += w[j]; }
    const float g = gdisp ? gdisp[i] : 0.f;
    const float dv = disp[i];
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const size_t ko = (static_cast<size_t>(b) * K + j) * HW + p;
      const float pj = w[j] / den;
      const size_t o = base + static_cast<size_t>(idx[j]) * HW;
      if (gcost) gcost[o] = g * pj * (td[j] - dv) + (gtc ? gtc[ko] : 0.f);
      if (gsamp) gsamp[o] = g * pj + (gtd ? gtd[ko] : 0.f);
    }
  }
}

// ---------------------------------------------------------------------------------------- K4a + K5
// topk_softargmax_fwd followed by convex_upsample_kernel (pyramid_ops.hip, the form with the next level's candidates) as ONE launch:
// the disparity at level resolution and the top-k planes are not results of the coarse and fine levels, and two launches of ~4 us on
// grids of 8-32 workgroups are mostly launch latency on the pass's critical chain.  A workgroup owns RT x RT level pixels: it
// regresses them and their one-pixel halo into LDS (outside the map: the zero the select of the 9-tap kernel produces), then every
// thread combines the nine taps of its output pixels.  The logits do not depend on the regression: they are requested first.
constexpr int RT = 8;

template <int K>
__global__ void __launch_bounds__(256)
regress_convex_upsample_fwd(const float* __restrict__ cost, const float* __restrict__ samp, const float* __restrict__ off,
                            const float* __restrict__ mask, float* __restrict__ out, float* __restrict__ low,
                            float* __restrict__ high, float* __restrict__ cand, int D, int H, int W, int r, float disp_scale,
                            float range, int coff, int ctot) {
  constexpr int HT = RT + 2;
  __shared__ float sd[HT * HT];
  const int tiles_x = (W + RT - 1) / RT;
  const int ty0 = static_cast<int>(blockIdx.x / tiles_x) * RT, tx0 = static_cast<int>(blockIdx.x % tiles_x) * RT;
  const int b = blockIdx.y;
  const int HW = H * W, Ho = H * r, Wo = W * r;
  const int E = RT * r, n_out = E * E;                     // output pixels of the tile: E x E
  const size_t kstride = static_cast<size_t>(r) * r * HW;
  const float* mb = mask + static_cast<size_t>(b) * 9 * kstride;
  // output pixel t of the tile -> (oy, ox), its level pixel (y, x) and sub-position; false: outside the map
  auto place = [&](int t, int& oy, int& ox, int& y, int& x, const float*& mp) {
    const int ly = t / E, lx = t - ly * E;
    oy = ty0 * r + ly; ox = tx0 * r + lx;
    y = oy / r; x = ox / r;
    const int ry = oy - y * r, rx = ox - x * r;
    mp = mb + static_cast<size_t>(ry * r + rx) * HW + static_cast<size_t>(y) * W + x;
    return t < n_out && oy < Ho && ox < Wo;
  };
  float m[9], mx = 0.f;
  int oy, ox, y, x;
  const float* mp;
  bool ok = place(threadIdx.x, oy, ox, y, x, mp);
  if (ok) mx = ts_tail::convex_logits(mp, kstride, m);
  for (int q = threadIdx.x; q < HT * HT; q += blockDim.x) {
    const int hy = ty0 - 1 + q / HT, hx = tx0 - 1 + q % HT;
    float d = 0.f;
    if (hy >= 0 && hy < H && hx >= 0 && hx < W) {
      const size_t base = static_cast<size_t>(b) * D * HW + static_cast<size_t>(hy) * W + hx;
      float bc[K], td[K];
      int bi[K];
      d = ts_tail::topk_softargmax_pixel<K>(cost + base, samp + base, off + base, D, HW, bc, bi, td);
    }
    sd[q] = d;
  }
  __syncthreads();
  const size_t HWo = static_cast<size_t>(Ho) * Wo;
  for (int t = threadIdx.x; t < n_out; t += blockDim.x) {
    if (t != static_cast<int>(threadIdx.x)) {
      ok = place(t, oy, ox, y, x, mp);
      if (ok) mx = ts_tail::convex_logits(mp, kstride, m);
    }
    if (!ok) continue;
    const float dup = ts_tail::convex_combine(m, mx, [&](int k) {
      const int yy = y + k / 3 - 1, xx = x + k % 3 - 1;
      const float dv = sd[(yy - ty0 + 1) * HT + (xx - tx0 + 1)];
      return ts_tail::convex_tap_value(dv, yy >= 0 && yy < H && xx >= 0 && xx < W, disp_scale);
    });
    const size_t o = static_cast<size_t>(b) * HWo + static_cast<size_t>(oy) * Wo + ox;
    out[o] = dup;
    ts_tail::convex_store_range(dup, range, low + o, high + o,
                                cand + (static_cast<size_t>(b) * ctot + coff) * HWo + static_cast<size_t>(oy) * Wo + ox, HWo);
  }
}

// ---------------------------------------------------------------------------------------- K4a + memory resize
// topk_softargmax_fwd followed by resize_bilinear_pair_kernel (pyramid_ops.hip) of its top-k planes to half size, as ONE launch (the
// 1/4 level: only the half-size maps are kept as the next frame's memory, precise.py:100-103).  The resize is align_corners: output
// (oy, ox) reads source rows floor(s) and floor(s) + 1 with s = oy (H - 1) / (H/2 - 1) in [2 oy, 2 oy + 1] -- NOT the 2x2 mean of its
// own quad, the row below and the column to the right belong to the neighbours.  So a workgroup owns HQ x HQ outputs, regresses
// the 2 HQ x 2 HQ pixels under them plus one row below and one column to the right (320 threads, 289 pixels) into LDS, writes the
// disparity of the pixels it owns, and interpolates from LDS with resize_bilinear_pair_kernel's own expression.  The host entry
// verifies the index range for the given size before it launches (ts_topk_softargmax_half_fwd).
constexpr int HQ = 8, HF = 2 * HQ + 1;

template <int K>
__global__ void __launch_bounds__(320)
topk_softargmax_half_fwd(const float* __restrict__ cost, const float* __restrict__ samp, const float* __restrict__ off,
                         float* __restrict__ disp, float* __restrict__ mem_s, float* __restrict__ mem_c, int D, int H, int W,
                         float sh, float sw, float vs0, float vs1) {
  __shared__ float s_td[K][HF * HF], s_tc[K][HF * HF];
  const int Ho = H / 2, Wo = W / 2, HW = H * W;
  const int tiles_x = (Wo + HQ - 1) / HQ;
  const int oy0 = static_cast<int>(blockIdx.x / tiles_x) * HQ, ox0 = static_cast<int>(blockIdx.x % tiles_x) * HQ;
  const int b = blockIdx.y;
  for (int q = threadIdx.x; q < HF * HF; q += blockDim.x) {
    const int ly = q / HF, lx = q - ly * HF;
    const int y = 2 * oy0 + ly, x = 2 * ox0 + lx;
    float bc[K], td[K];
    int bi[K];
#pragma unroll
    for (int j = 0; j < K; ++j) { bc[j] = 0.f; td[j] = 0.f; }
    if (y < H && x < W) {
      const size_t base = static_cast<size_t>(b) * D * HW + static_cast<size_t>(y) * W + x;
      const float acc = ts_tail::topk_softargmax_pixel<K>(cost + base, samp + base, off + base, D, HW, bc, bi, td);
      if (ly < 2 * HQ && lx < 2 * HQ) disp[static_cast<size_t>(b) * HW + static_cast<size_t>(y) * W + x] = acc;
    }
#pragma unroll
    for (int j = 0; j < K; ++j) { s_td[j][q] = td[j]; s_tc[j][q] = bc[j]; }
  }
  __syncthreads();
  for (int t = threadIdx.x; t < HQ * HQ * K * 2; t += blockDim.x) {
    const int lxo = t % HQ;
    int r = t / HQ;
    const int lyo = r % HQ;
    r /= HQ;
    const int j = r % K, which = r / K;
    const int oy = oy0 + lyo, ox = ox0 + lxo;
    if (oy >= Ho || ox >= Wo) continue;
    int y0, y1, xa, xb;
    float ly, lx;
    ts_tail::lin_src(sh, oy, H, y0, y1, ly);
    ts_tail::lin_src(sw, ox, W, xa, xb, lx);
    // tile-local; the clamp only keeps a read inside the tile (the host has checked that it changes nothing)
    y0 = min(max(y0 - 2 * oy0, 0), HF - 1); y1 = min(max(y1 - 2 * oy0, 0), HF - 1);
    xa = min(max(xa - 2 * ox0, 0), HF - 1); xb = min(max(xb - 2 * ox0, 0), HF - 1);
    const float* s = which ? s_tc[j] : s_td[j];
    const float v = ts_tail::bilinear_value(s[y0 * HF + xa], s[y0 * HF + xb], s[y1 * HF + xa], s[y1 * HF + xb], ly, lx, which ? vs1 : vs0);
    (which ? mem_c : mem_s)[((static_cast<size_t>(b) * K + j) * Ho + oy) * Wo + ox] = v;
  }
}

// whether every output index o < out_size of an align_corners resize in_size -> out_size = in_size / 2 reads sources 2 o .. 2 o + 2
// (the device's own arithmetic: one fp32 multiply, truncation)
bool half_resize_in_reach(int in_size, int out_size) {
  const float scale = out_size > 1 ? static_cast<float>(in_size - 1) / static_cast<float>(out_size - 1) : 0.f;
  for (int o = 0; o < out_size; ++o) {
    const int i0 = static_cast<int>(scale * static_cast<float>(o));
    const int i1 = i0 + ((i0 < in_size - 1) ? 1 : 0);
    if (i0 < 2 * o || i1 > 2 * o + 2) return false;
  }
  return true;
}

// ---------------------------------------------------------------------------------------- K4b
// One wavefront = 16 consecutive pixels x 4 slices of the D axis.
struct Partial { float m, s, ws; };   // running max, sum exp, sum exp*sample

__device__ __forceinline__ Partial merge(Partial a, Partial b) {
  const float m = fmaxf(a.m, b.m);
  const float ea = (a.m == -INFINITY) ? 0.f : expf(a.m - m);
  const float eb = (b.m == -INFINITY) ? 0.f : expf(b.m - m);
  return Partial{m, a.s * ea + b.s * eb, a.ws * ea + b.ws * eb};
}

template <bool NORMALIZE>
__global__ void __launch_bounds__(256)
soft_argmin_fwd(const float* __restrict__ cost, const float* __restrict__ samp, float* __restrict__ disp,
                float temperature, int B, int D, int HW) {
  const int lane = threadIdx.x & 63;
  const int slice = lane >> 4;                 // 0..3
  const long long wave = (static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  const long long nwave = (static_cast<long long>(gridDim.x) * blockDim.x) >> 6;
  const long long npix = static_cast<long long>(B) * HW;
  for (long long p0 = wave * 16; p0 < npix; p0 += nwave * 16) {
    const long long i = p0 + (lane & 15);
    const bool ok = i < npix;
    const int b = ok ? static_cast<int>(i / HW) : 0;
    const int p = ok ? static_cast<int>(i - static_cast<long long>(b) * HW) : 0;
    const size_t base = static_cast<size_t>(b) * D * HW + p;
    Partial a{-INFINITY, 0.f, 0.f};
    float lin = 0.f;
    if (ok) {
      for (int d = slice; d < D; d += 4) {
        const float c = cost[base + static_cast<size_t>(d) * HW] * temperature;
        const float sv = samp[base + static_cast<size_t>(d) * HW];
        if constexpr (NORMALIZE) {
          a = merge(a, Partial{c, 1.f, sv});
        } else {
          lin += c * sv;
        }
      }
    }
    if constexpr (NORMALIZE) {
      // wavefront-shuffle reduction across the 4 slices of a pixel (lanes l, l^16, l^32, l^48)
#pragma unroll
      for (int s = 16; s <= 32; s <<= 1) {
        Partial o{__shfl_xor(a.m, s), __shfl_xor(a.s, s), __shfl_xor(a.ws, s)};
        a = merge(a, o);
      }
      if (ok && slice == 0) disp[i] = a.ws / a.s;
    } else {
      lin += __shfl_xor(lin, 16);
      lin += __shfl_xor(lin, 32);
      if (ok && slice == 0) disp[i] = lin;
    }
  }
}

template <bool NORMALIZE>
__global__ void __launch_bounds__(256)
soft_argmin_bwd(const float* __restrict__ cost, const float* __restrict__ samp, const float* __restrict__ disp,
                const float* __restrict__ gdisp, float* __restrict__ gcost, float* __restrict__ gsamp,
                float temperature, int B, int D, int HW) {
  const long long n = static_cast<long long>(B) * HW;
  for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < n;
       i += static_cast<long long>(gridDim.x) * blockDim.x) {
    const int b = static_cast<int>(i / HW);
    const int p = static_cast<int>(i - static_cast<long long>(b) * HW);
    const size_t base = static_cast<size_t>(b) * D * HW + p;
    const float g = gdisp[i];
    if constexpr (NORMALIZE) {
      float m = -INFINITY, s = 0.f;
      for (int d = 0; d < D; ++d) {
        const float c = cost[base + static_cast<size_t>(d) * HW] * temperature;
        const float mn = fmaxf(m, c);
        s = s * expf(m - mn) + expf(c - mn);
        m = mn;
      }
      const float dv = disp[i];
      for (int d = 0; d < D; ++d) {
        const size_t o = base + static_cast<size_t>(d) * HW;
        const float pd = expf(cost[o] * temperature - m) / s;
        if (gcost) gcost[o] = g * temperature * pd * (samp[o] - dv);
        if (gsamp) gsamp[o] = g * pd;
      }
    } else {
      for (int d = 0; d < D; ++d) {
        const size_t o = base + static_cast<size_t>(d) * HW;
        if (gcost) gcost[o] = g * temperature * samp[o];
        if (gsamp) gsamp[o] = g * temperature * cost[o];
      }
    }
  }
}

__global__ void __launch_bounds__(256)
argmax_select_fwd(const float* __restrict__ cost, const float* __restrict__ samp, float* __restrict__ disp,
                  int* __restrict__ idx, int B, int D, int HW) {
  const long long n = static_cast<long long>(B) * HW;
  for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < n;
       i += static_cast<long long>(gridDim.x) * blockDim.x) {
    const int b = static_cast<int>(i / HW);
    const int p = static_cast<int>(i - static_cast<long long>(b) * HW);
    const size_t base = static_cast<size_t>(b) * D * HW + p;
    float best = -INFINITY;
    int bi = 0;
    for (int d = 0; d < D; ++d) {
      const float c = cost[base + static_cast<size_t>(d) * HW];
      if (c > best) { best = c; bi = d; }
    }
    disp[i] = samp[base + static_cast<size_t>(bi) * HW];
    if (idx) idx[i] = bi;
  }
}

int check_bdhw(int B, int D, int H, int W, const char* who) {
  TS_REQUIRE(B > 0 && D > 0 && H > 0 && W > 0, TS_ERR_SHAPE, "%s: non-positive size", who);
  TS_REQUIRE(static_cast<long long>(H) * W < (1ll << 31), TS_ERR_UNSUPPORTED, "%s: plane too large", who);
  return TS_OK;
}

unsigned grid_for(long long n, int threads) {
  long long blocks = (n + threads - 1) / threads;
  const long long cap = static_cast<long long>(ts::kNumCU) * 8;
  if (blocks > cap) blocks = cap;
  if (blocks < 1) blocks = 1;
  return static_cast<unsigned>(blocks);
}

}  // namespace

extern "C" int ts_topk_softargmax_fwd(const float* cost, const float* sample, const float* offset, float* disp,
                                      float* topk_disp, float* topk_cost, int* topk_index,
                                      int B, int D, int H, int W, int k, void* stream) {
  if (int rc = check_bdhw(B, D, H, W, "topk_softargmax")) return rc;
  TS_REQUIRE(k >= 1 && k <= KMAX && k <= D, TS_ERR_UNSUPPORTED, "topk_softargmax: k=%d outside 1..min(%d, D)", k, KMAX);
  TS_REQUIRE_PTR(cost); TS_REQUIRE_PTR(sample); TS_REQUIRE_PTR(offset);
  TS_REQUIRE_PTR(disp); TS_REQUIRE_PTR(topk_disp); TS_REQUIRE_PTR(topk_cost);
  const int HW = H * W;
  const dim3 grid(grid_for(static_cast<long long>(B) * HW, 256));
  hipStream_t st = ts::as_stream(stream);
#define TS_CASE(KK)                                                                                     \
  case KK:                                                                                              \
    hipLaunchKernelGGL(topk_softargmax_fwd<KK>, grid, dim3(256), 0, st, cost, sample, offset, disp,      \
                       topk_disp, topk_cost, topk_index, B, D, HW);                                     \
    break;
  switch (k) { TS_CASE(1) TS_CASE(2) TS_CASE(3) TS_CASE(4) TS_CASE(5) TS_CASE(6) TS_CASE(7) TS_CASE(8) }
#undef TS_CASE
  return ts::launched("topk_softargmax_fwd");
}

// ts_topk_softargmax_fwd + ts_convex_upsample_candidates_fwd on its disparity, as one launch (nothing at level resolution is written)
extern "C" int ts_regress_convex_upsample_fwd(const float* cost, const float* sample, const float* offset, const float* mask,
                                              float* out, float* low, float* high, float* candidates, int B, int D, int H, int W,
                                              int k, int factor, float disp_scale, float range, int channel_offset,
                                              int channels_total, void* stream) {
  if (int rc = check_bdhw(B, D, H, W, "regress_convex_upsample")) return rc;
  TS_REQUIRE(k >= 1 && k <= KMAX && k <= D, TS_ERR_UNSUPPORTED, "regress_convex_upsample: k=%d outside 1..min(%d, D)", k, KMAX);
  TS_REQUIRE(factor >= 1, TS_ERR_SHAPE, "regress_convex_upsample: bad factor");
  TS_REQUIRE(channel_offset >= 0 && channel_offset + 5 <= channels_total, TS_ERR_SHAPE, "regress_convex_upsample: bad channel slice");
  TS_REQUIRE(factor <= 8 && B <= 65535 && static_cast<long long>(H) * W * factor * factor < (1ll << 31), TS_ERR_UNSUPPORTED,
             "regress_convex_upsample: factor, batch or upsampled plane too large");
  TS_REQUIRE_PTR(cost); TS_REQUIRE_PTR(sample); TS_REQUIRE_PTR(offset); TS_REQUIRE_PTR(mask);
  TS_REQUIRE_PTR(out); TS_REQUIRE_PTR(low); TS_REQUIRE_PTR(high); TS_REQUIRE_PTR(candidates);
  const dim3 grid(static_cast<unsigned>(((H + RT - 1) / RT) * ((W + RT - 1) / RT)), static_cast<unsigned>(B));
  hipStream_t st = ts::as_stream(stream);
#define TS_CASE(KK)                                                                                                       \
  case KK:                                                                                                                \
    hipLaunchKernelGGL(regress_convex_upsample_fwd<KK>, grid, dim3(256), 0, st, cost, sample, offset, mask, out, low, high, \
                       candidates, D, H, W, factor, disp_scale, range, channel_offset, channels_total);                   \
    break;
  switch (k) { TS_CASE(1) TS_CASE(2) TS_CASE(3) TS_CASE(4) TS_CASE(5) TS_CASE(6) TS_CASE(7) TS_CASE(8) }
#undef TS_CASE
  return ts::launched("regress_convex_upsample_fwd");
}

// ts_topk_softargmax_fwd + ts_resize_bilinear_pair_fwd of its top-k planes to (H/2, W/2) with value scales 0.5 and 1, as one launch
extern "C" int ts_topk_softargmax_half_fwd(const float* cost, const float* sample, const float* offset, float* disp,
                                           float* mem_sample, float* mem_cost, int B, int D, int H, int W, int k, void* stream) {
  if (int rc = check_bdhw(B, D, H, W, "topk_softargmax_half")) return rc;
  TS_REQUIRE(k >= 1 && k <= KMAX && k <= D, TS_ERR_UNSUPPORTED, "topk_softargmax_half: k=%d outside 1..min(%d, D)", k, KMAX);
  TS_REQUIRE(H % 2 == 0 && W % 2 == 0, TS_ERR_UNSUPPORTED, "topk_softargmax_half: odd size %d x %d", H, W);
  TS_REQUIRE(B <= 65535 && half_resize_in_reach(H, H / 2) && half_resize_in_reach(W, W / 2), TS_ERR_UNSUPPORTED,
             "topk_softargmax_half: batch or size beyond the tile's reach");
  TS_REQUIRE_PTR(cost); TS_REQUIRE_PTR(sample); TS_REQUIRE_PTR(offset);
  TS_REQUIRE_PTR(disp); TS_REQUIRE_PTR(mem_sample); TS_REQUIRE_PTR(mem_cost);
  const int Ho = H / 2, Wo = W / 2;
  const float sh = Ho > 1 ? static_cast<float>(H - 1) / static_cast<float>(Ho - 1) : 0.f;      // ts_resize_bilinear_pair_fwd's scales
  const float sw = Wo > 1 ? static_cast<float>(W - 1) / static_cast<float>(Wo - 1) : 0.f;
  const dim3 grid(static_cast<unsigned>(((Ho + HQ - 1) / HQ) * ((Wo + HQ - 1) / HQ)), static_cast<unsigned>(B));
  hipStream_t st = ts::as_stream(stream);
#define TS_CASE(KK)                                                                                                     \
  case KK:                                                                                                              \
    hipLaunchKernelGGL(topk_softargmax_half_fwd<KK>, grid, dim3(320), 0, st, cost, sample, offset, disp, mem_sample,     \
                       mem_cost, D, H, W, sh, sw, 0.5f, 1.f);                                                            \
    break;
  switch (k) { TS_CASE(1) TS_CASE(2) TS_CASE(3) TS_CASE(4) TS_CASE(5) TS_CASE(6) TS_CASE(7) TS_CASE(8) }
#undef TS_CASE
  return ts::launched("topk_softargmax_half_fwd");
}

extern "C" int ts_topk_softargmax_bwd(const float* topk_disp, const float* topk_cost, const int* topk_index,
                                      const float* disp, const float* grad_disp, const float* grad_topk_disp,
                                      const float* grad_topk_cost, float* grad_cost, float* grad_sample,
                                      int B, int D, int H, int W, int k, void* stream) {
  if (int rc = check_bdhw(B, D, H, W, "topk_softargmax_bwd")) return rc;
  TS_REQUIRE(k >= 1 && k <= KMAX && k <= D, TS_ERR_UNSUPPORTED, "topk_softargmax_bwd: k=%d outside 1..min(%d, D)", k, KMAX);
  TS_REQUIRE_PTR(topk_disp); TS_REQUIRE_PTR(topk_cost); TS_REQUIRE_PTR(topk_index); TS_REQUIRE_PTR(disp);
  const int HW = H * W;
  const dim3 grid(grid_for(static_cast<long long>(B) * HW, 256));
  hipStream_t st = ts::as_stream(stream);
#define TS_CASE(KK)                                                                                      \
  case KK:                                                                                               \
    hipLaunchKernelGGL(topk_softargmax_bwd<KK>, grid, dim3(256), 0, st, topk_disp, topk_cost, topk_index, \
                       disp, grad_disp, grad_topk_disp, grad_topk_cost, grad_cost, grad_sample, B, D, HW); \
    break;
  switch (k) { TS_CASE(1) TS_CASE(2) TS_CASE(3) TS_CASE(4) TS_CASE(5) TS_CASE(6) TS_CASE(7) TS_CASE(8) }
#undef TS_CASE
  return ts::launched("topk_softargmax_bwd");
}

extern "C" int ts_softargmin_fwd(const float* cost, const float* sample, float* disp, float temperature,
                                 int normalize, int B, int D, int H, int W, void* stream) {
  if (int rc = check_bdhw(B, D, H, W, "softargmin")) return rc;
  TS_REQUIRE_PTR(cost); TS_REQUIRE_PTR(sample); TS_REQUIRE_PTR(disp);
  const int HW = H * W;
  const long long nthreads = (static_cast<long long>(B) * HW + 15) / 16 * 64;    // 4 lanes per pixel
  const dim3 grid(grid_for(nthreads, 256));
  hipStream_t st = ts::as_stream(stream);
  if (normalize) hipLaunchKernelGGL(soft_argmin_fwd<true>, grid, dim3(256), 0, st, cost, sample, disp, temperature, B, D, HW);
  else hipLaunchKernelGGL(soft_argmin_fwd<false>, grid, dim3(256), 0, st, cost, sample, disp, temperature, B, D, HW);
  return ts::launched("softargmin_fwd");
}

extern "C" int ts_softargmin_bwd(const float* cost, const float* sample, const float* disp, const float* grad_disp,
                                 float* grad_cost, float* grad_sample, float temperature, int normalize,
                                 int B, int D, int H, int W, void* stream) {
  if (int rc = check_bdhw(B, D, H, W, "softargmin_bwd")) return rc;
  TS_REQUIRE_PTR(cost); TS_REQUIRE_PTR(sample); TS_REQUIRE_PTR(disp); TS_REQUIRE_PTR(grad_disp);
  const int HW = H * W;
  const dim3 grid(grid_for(static_cast<long long>(B) * HW, 256));
  hipStream_t st = ts::as_stream(stream);
  if (normalize) hipLaunchKernelGGL(soft_argmin_bwd<true>, grid, dim3(256), 0, st, cost, sample, disp, grad_disp, grad_cost, grad_sample, temperature, B, D, HW);
  else hipLaunchKernelGGL(soft_argmin_bwd<false>, grid, dim3(256), 0, st, cost, sample, disp, grad_disp, grad_cost, grad_sample, temperature, B, D, HW);
  return ts::launched("softargmin_bwd");
}

extern "C" int ts_argmax_select_fwd(const float* cost, const float* sample, float* disp, int* index,
                                    int B, int D, int H, int W, void* stream) {
  if (int rc = check_bdhw(B, D, H, W, "argmax_select")) return rc;
  TS_REQUIRE_PTR(cost); TS_REQUIRE_PTR(sample); TS_REQUIRE_PTR(disp);
  const int HW = H * W;
  hipLaunchKernelGGL(argmax_select_fwd, dim3(grid_for(static_cast<long long>(B) * HW, 256)), dim3(256), 0,
                     ts::as_stream(stream), cost, sample, disp, index, B, D, HW);
  return ts::launched("argmax_select_fwd");
}
