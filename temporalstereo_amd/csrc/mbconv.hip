// MemoryInvertedResidual (reference: architecture/modeling/backbone/TemporalStereo.py:165-218): the encoder's inverted-residual block
// with the per-frame feature memory spliced into its input, fp32 throughout, no atomics.
//
//   x = silu(bn1(conv_pw(cat([memory, input[:, mc:]], 1))))        expand_kernel      the concatenation is never written
//   x = silu(bn2(conv_dw(x))), plane_sum = sum_hw(x)               depthwise_kernel   3x3, stride 1, padding 1
//   g = sigmoid(conv_expand(silu(conv_reduce(plane_sum / HW))))    se_gate_kernel
//   y = input + bn3(conv_pwl(x * g))                               project_kernel     the gated map is never written
//
// expand_kernel<MT> and project_kernel<MT> are conv_pw1.hpp's pointwise convolution (geometry, staging, pitches and the blocked
// summation: there).  expand reads input channels [0, mc) from `memory` and [mc, C) from `input`, each in place through its own batch /
// channel strides (memory NULL: `input` alone); epilogue silu(sum * scale + shift).  project multiplies channel ci of batch element b by
// gate[b, ci] while it stages; epilogue sum * scale + shift + residual, the residual through its own strides.
//
// depthwise_kernel: one workgroup per (b, c) plane -- the encoder's planes are tiny (34 x 60, 17 x 30) and its channels many (512 to
// 1632), so the planes fill the chip (1024 to 13056 workgroups) and a plane's sum is finished inside its workgroup, with no second
// step.  The workgroup walks the plane in tiles of kDR rows x kDC columns in row-major tile order; a tile is staged with its halo in
// LDS (zeros outside the plane), the interior in 16-byte pieces when every plane row starts 16-byte aligned, and a thread takes outputs
// tid, tid + 256, ... of the tile in row-major order.  plane_sum: a thread sums ITS outputs in that order, the 64 lanes of a wave go
// through the xor butterfly of reduce.hpp, the four waves are added in order -- which thread holds which pixel depends on (H, W) alone,
// so a plane's sum has the same bits whatever B and C are.  With the taps flipped and no epilogue the kernel is the input gradient.
// depthwise_wgrad_kernel: one workgroup per channel; it walks b, then the tiles, staging x as above and reading dy once from global
// memory; a thread keeps nine partial sums, finished as plane_sum is.
//
// se_gate_kernel: the step is a few hundred thousand multiply-adds and all latency.  A workgroup per batch element and slice of 256
// gate channels: each puts the means in LDS and computes EVERY reduce row (a wave carries 4 rows at once -- lanes over the channels in
// ascending order, then the butterfly -- with 32 loads per lane in flight), then a thread takes one expand row as one ascending chain.
// The reduce step is repeated by the slices of a batch element (Cmid / 256 times: 444 KB from L2 at the widest) rather than made a
// launch of its own.
#include "conv_pw1.hpp"
#include "reduce.hpp"

namespace {

constexpr int kMaxC = 512;                   // the block's width (expand's Cin, project's Cout) and the squeeze width Cr
constexpr int kMaxMid = 2048;                // the expanded width
constexpr int kFlush = 8;                    // chunks (256 input channels) per block of the blocked summation
constexpr int kDR = 8, kDC = 64;             // depthwise tile
constexpr int kDP = kDC + 8;                 // LDS row pitch: the interior starts at column 4 (16-byte aligned), halos at 3 and 4 + width
using node::kGridCap;
using node::kMaxAxis;
using ts::strides_ok;

// ---------------------------------------------------------------------------------------------------------------- pointwise
struct Expand {
  pw1::Geom g;              // Cin: C, rows: Cmid
  const float* mem;         // source of channels [0, mc)
  const float* inp;         // source of channels [mc, C)
  node::Affine<ACT_SILU, 0> ep;      // silu(sum * scale + shift), never a residual
  int mc;
  long long mem_bs, mem_cs, in_bs, in_cs;

  // the lambda holds copies of what it uses, never `this`: a store through y then cannot be taken to change a field
  __device__ __forceinline__ auto source(int b) const {
    return [pm = mem + b * mem_bs, pi = inp + b * in_bs, mc = mc, mem_cs = mem_cs, in_cs = in_cs](int gc, long long p) {
      return gc < mc ? pm[gc * mem_cs + p] : pi[gc * in_cs + p];
    };
  }
  __device__ __forceinline__ auto sink(int b, long long p) const { return ep.writer(b, p); }
};

using Project = pw1::Project<true>;      // Cin: Cmid, rows: C; the gate is [B][Cmid]

template <int MT>
__global__ void __launch_bounds__(256) expand_kernel(const Expand p) { pw1::conv_tile<MT, kFlush>(p); }
template <int MT>
__global__ void __launch_bounds__(256) project_kernel(const Project p) { pw1::conv_tile<MT, kFlush>(p); }

// the block's envelope, and the pointwise core's plane limit
int check_block(const char* who, int C, int Cmid, long long HW) {
  TS_REQUIRE(C <= kMaxC && Cmid <= kMaxMid, TS_ERR_UNSUPPORTED, "%s: C = %d above %d or Cmid = %d above %d", who, C, kMaxC, Cmid, kMaxMid);
  return pw1::check_plane(who, HW);
}

// ---------------------------------------------------------------------------------------------------------------- depthwise
// the sum of a workgroup's 256 values in a fixed order, valid in every thread: butterfly per wave, then the four waves in order
__device__ __forceinline__ float block_sum(float v, float* s4) {
  v = ts::wave_sum(v);
  __syncthreads();                                               // s4 may still be read from the previous call
  if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((s4[0] + s4[1]) + s4[2]) + s4[3];
}

// rows y0 - 1 .. y0 + kDR, columns x0 - 1 .. x0 + wt of a plane into sT, zeros outside the plane; ends with a barrier
template <bool VEC>
__device__ __forceinline__ void stage_tile(float* sT, const float* __restrict__ plane, int H, int W, int y0, int x0, int wt) {
  const int tid = threadIdx.x;
  __syncthreads();                                               // the previous tile has been read
  if constexpr (VEC) {                                           // W, x0 and so wt are multiples of 4, every plane row 16-byte aligned
    const int q4 = wt >> 2;
    for (int i = tid; i < (kDR + 2) * q4; i += 256) {
      const int row = i / q4, q = i - row * q4, gy = y0 - 1 + row;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (gy >= 0 && gy < H) v = *reinterpret_cast<const float4*>(plane + static_cast<long long>(gy) * W + x0 + 4 * q);
      *reinterpret_cast<float4*>(sT + row * kDP + 4 + 4 * q) = v;
    }
  } else {
    for (int i = tid; i < (kDR + 2) * wt; i += 256) {
      const int row = i / wt, col = i - row * wt, gy = y0 - 1 + row;
      sT[row * kDP + 4 + col] = (gy >= 0 && gy < H) ? plane[static_cast<long long>(gy) * W + x0 + col] : 0.f;
    }
  }
  if (tid < 2 * (kDR + 2)) {                                     // the two halo columns
    const int row = tid >> 1, right = tid & 1, gy = y0 - 1 + row, gx = right ? x0 + wt : x0 - 1;
    sT[row * kDP + (right ? 4 + wt : 3)] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? plane[static_cast<long long>(gy) * W + gx] : 0.f;
  }
  __syncthreads();
}

template <bool VEC>
__global__ void __launch_bounds__(256) depthwise_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                        const float* __restrict__ scale, const float* __restrict__ shift,
                                                        float* __restrict__ y, float* __restrict__ plane_sum, int C, int H, int W, int act,
                                                        int flip, long long x_bs, long long x_cs, long long y_bs, long long y_cs) {
  __shared__ __attribute__((aligned(16))) float sT[(kDR + 2) * kDP];
  __shared__ float s4[4];
  const int b = blockIdx.x / C, c = blockIdx.x - b * C;
  const float* px = x + b * x_bs + c * x_cs;
  float* py = y + b * y_bs + c * y_cs;
  float k[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) k[t] = w[c * 9 + (flip ? 8 - t : t)];
  const float sc = scale ? scale[c] : 1.f, sh = shift ? shift[c] : 0.f;
  float total = 0.f;
  for (int y0 = 0; y0 < H; y0 += kDR) {
    const int ht = min(kDR, H - y0);
    for (int x0 = 0; x0 < W; x0 += kDC) {
      const int wt = min(kDC, W - x0);
      stage_tile<VEC>(sT, px, H, W, y0, x0, wt);
      for (int i = threadIdx.x; i < ht * wt; i += 256) {
        const int r = i / wt, col = i - r * wt;
        const float* s = sT + r * kDP + 3 + col;                 // the tap (0, 0) of output (r, col)
        float v = 0.f;
#pragma unroll
        for (int t = 0; t < 9; ++t) v = fmaf(k[t], s[(t / 3) * kDP + t % 3], v);
        v = fmaf(v, sc, sh);
        if (act == ACT_SILU) v = silu_fast(v);
        py[static_cast<long long>(y0 + r) * W + x0 + col] = v;
        total += v;
      }
    }
  }
  if (plane_sum) {
    total = block_sum(total, s4);
    if (threadIdx.x == 0) plane_sum[blockIdx.x] = total;
  }
}

template <bool VEC>
__global__ void __launch_bounds__(256) depthwise_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                              float* __restrict__ dw, int B, int H, int W, long long x_bs, long long x_cs,
                                                              long long dy_bs, long long dy_cs) {
  __shared__ __attribute__((aligned(16))) float sT[(kDR + 2) * kDP];
  __shared__ float s4[4];
  const int c = blockIdx.x;
  float acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) acc[t] = 0.f;
  for (int b = 0; b < B; ++b) {
    const float* px = x + b * x_bs + c * x_cs;
    const float* pg = dy + b * dy_bs + c * dy_cs;
    for (int y0 = 0; y0 < H; y0 += kDR) {
      const int ht = min(kDR, H - y0);
      for (int x0 = 0; x0 < W; x0 += kDC) {
        const int wt = min(kDC, W - x0);
        stage_tile<VEC>(sT, px, H, W, y0, x0, wt);
        for (int i = threadIdx.x; i < ht * wt; i += 256) {
          const int r = i / wt, col = i - r * wt;
          const float* s = sT + r * kDP + 3 + col;
          const float g = pg[static_cast<long long>(y0 + r) * W + x0 + col];
#pragma unroll
          for (int t = 0; t < 9; ++t) acc[t] = fmaf(g, s[(t / 3) * kDP + t % 3], acc[t]);
        }
      }
    }
  }
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    const float v = block_sum(acc[t], s4);
    if (threadIdx.x == 0) dw[c * 9 + t] = v;
  }
}

// every plane row starts 16-byte aligned: the 16-byte staging form
inline bool rows_aligned(const float* p, int W, long long bs, long long cs) {
  return ts::aligned16(p) && W % 4 == 0 && bs % 4 == 0 && cs % 4 == 0;
}

// ---------------------------------------------------------------------------------------------------------------- squeeze-excite
constexpr int kGateRows = 4;                 // reduce rows a wave carries at once
constexpr int kGateAhead = 8;                // loads per row (reduce) or per thread (expand) issued together

// Every load of a step that can be in flight is: the step is 222 k multiply-adds at the widest and nothing but dependent round trips
// to memory, on a grid of a few workgroups.  A group of kGateAhead loads is
// unconditional (an index past the end is clamped and its term multiplied by zero), so the compiler can issue the group before the
// first use.  V4: rows are read in 16-byte pieces (the row length a multiple of 4 and the base aligned); the summation order of a row
// then differs from the scalar form's, and depends on the shape alone.
template <bool V4>
__device__ __forceinline__ void gate_reduce(const float* __restrict__ w_reduce, const float* __restrict__ b_reduce, const float* sMean,
                                            float* sRed, int Cmid, int Cr, int wave, int lane) {
  constexpr int E = V4 ? 4 : 1;
  const int n = Cmid / E;                                        // pieces of a row
  for (int jb = wave * kGateRows; jb < Cr; jb += 4 * kGateRows) {
    const float* wr[kGateRows];
    float v[kGateRows];
#pragma unroll
    for (int r = 0; r < kGateRows; ++r) {
      wr[r] = w_reduce + static_cast<long long>(min(jb + r, Cr - 1)) * Cmid;      // a row past the last is the last again, and dropped
      v[r] = 0.f;
    }
    for (int i0 = lane; i0 < n; i0 += 64 * kGateAhead) {
#pragma unroll
      for (int k = 0; k < kGateAhead; ++k) {
        const int i = i0 + 64 * k, ic = min(i, n - 1);
        const float live = i < n ? 1.f : 0.f;
        if constexpr (V4) {
          const float4 m = *reinterpret_cast<const float4*>(sMean + 4 * ic);
#pragma unroll
          for (int r = 0; r < kGateRows; ++r) {
            const float4 w = *reinterpret_cast<const float4*>(wr[r] + 4 * ic);
            v[r] = fmaf(w.w * live, m.w, fmaf(w.z * live, m.z, fmaf(w.y * live, m.y, fmaf(w.x * live, m.x, v[r]))));
          }
        } else {
          const float m = sMean[ic];
#pragma unroll
          for (int r = 0; r < kGateRows; ++r) v[r] = fmaf(wr[r][ic] * live, m, v[r]);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < kGateRows; ++r) {
      const float s = ts::wave_sum(v[r]);
      if (lane == 0 && jb + r < Cr) sRed[jb + r] = silu_fast(s + b_reduce[jb + r]);
    }
  }
}

template <bool V4>
__device__ __forceinline__ float gate_expand(const float* __restrict__ we, const float* sRed, int Cr) {
  constexpr int E = V4 ? 4 : 1;
  const int n = Cr / E;
  float v = 0.f;
  for (int i0 = 0; i0 < n; i0 += kGateAhead) {
#pragma unroll
    for (int k = 0; k < kGateAhead; ++k) {
      const int i = i0 + k, ic = min(i, n - 1);
      const float live = i < n ? 1.f : 0.f;
      if constexpr (V4) {
        const float4 w = *reinterpret_cast<const float4*>(we + 4 * ic);
        const float4 m = *reinterpret_cast<const float4*>(sRed + 4 * ic);
        v = fmaf(w.w * live, m.w, fmaf(w.z * live, m.z, fmaf(w.y * live, m.y, fmaf(w.x * live, m.x, v))));
      } else {
        v = fmaf(we[ic] * live, sRed[ic], v);
      }
    }
  }
  return v;
}

__global__ void __launch_bounds__(256) se_gate_kernel(const float* __restrict__ plane_sum, const float* __restrict__ w_reduce,
                                                      const float* __restrict__ b_reduce, const float* __restrict__ w_expand,
                                                      const float* __restrict__ b_expand, float* __restrict__ gate, int Cmid, int Cr,
                                                      int slices, int vec_reduce, int vec_expand, float inv_hw) {
  __shared__ __attribute__((aligned(16))) float sMean[kMaxMid];
  __shared__ __attribute__((aligned(16))) float sRed[kMaxC];
  const int b = blockIdx.x / slices, slice = blockIdx.x - b * slices;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  for (int c = tid; c < Cmid; c += 256) sMean[c] = plane_sum[static_cast<long long>(b) * Cmid + c] * inv_hw;
  __syncthreads();
  if (vec_reduce) gate_reduce<true>(w_reduce, b_reduce, sMean, sRed, Cmid, Cr, wave, lane);
  else gate_reduce<false>(w_reduce, b_reduce, sMean, sRed, Cmid, Cr, wave, lane);
  __syncthreads();
  const int c = slice * 256 + tid;
  if (c < Cmid) {
    const float* we = w_expand + static_cast<long long>(c) * Cr;
    const float v = vec_expand ? gate_expand<true>(we, sRed, Cr) : gate_expand<false>(we, sRed, Cr);
    gate[static_cast<long long>(b) * Cmid + c] = sigmoid_fast(v + b_expand[c]);
  }
}

}  // namespace

extern "C" size_t ts_mbconv_weight_bytes(int Cin, int Cout) {
  if (Cin <= 0 || Cout <= 0 || Cin > kMaxMid || Cout > kMaxMid) return 0;
  return pw1::image_floats(Cin, Cout) * sizeof(float);
}

extern "C" int ts_mbconv_weight_layout(const float* w, float* w_l, int Cin, int Cout, void* stream) {
  TS_REQUIRE(Cin > 0 && Cout > 0, TS_ERR_SHAPE, "mbconv_weight_layout: non-positive size");
  TS_REQUIRE(Cin <= kMaxMid && Cout <= kMaxMid, TS_ERR_UNSUPPORTED, "mbconv_weight_layout: Cin=%d / Cout=%d above %d", Cin, Cout, kMaxMid);
  TS_REQUIRE_PTR(w); TS_REQUIRE_PTR(w_l);
  TS_REQUIRE_ALIGNED(w_l);
  return pw1::weight_layout(w, w_l, Cin, Cout, kGridCap, ts::as_stream(stream), "mbconv_weight_layout_kernel");
}

extern "C" int ts_mbconv_expand_fwd(const float* memory, const float* input, const float* w_l, const float* scale, const float* shift,
                                    float* y, int B, int C, int mc, int Cmid, int H, int W, long long mem_bstride, long long mem_cstride,
                                    long long in_bstride, long long in_cstride, long long y_bstride, long long y_cstride, void* stream) {
  const char* who = "mbconv_expand_fwd";
  TS_REQUIRE(B > 0 && C > 0 && Cmid > 0 && H > 0 && W > 0 && mc >= 0 && mc <= C, TS_ERR_SHAPE, "%s: non-positive size or mc outside [0, C]", who);
  const long long HW = static_cast<long long>(H) * W;
  const int seam = memory ? mc : 0;                              // no memory: the first frame reads `input` alone
  const node::Operand M{"memory", memory, seam, HW, mem_bstride, mem_cstride, node::IN}, I{"input", input, C, HW, in_bstride, in_cstride, node::IN},
      Y{"y", y, Cmid, HW, y_bstride, y_cstride, node::OUT};
  Expand p;
  p.mem = memory; p.inp = input; p.mc = seam;
  p.mem_bs = mem_bstride; p.mem_cs = mem_cstride; p.in_bs = in_bstride; p.in_cs = in_cstride;
  p.ep = {scale, shift, ACT_SILU, {nullptr, 0, 0}, {y, y_bstride, y_cstride}};
  // as the decoder: a grid of fewer than two workgroups per compute unit is cut finer along the rows
  return node::launch(
      who, "mbconv_expand_kernel", B, {M, I, Y}, {}, w_l, {B, H, W}, [&] { return check_block(who, C, Cmid, HW); },
      [&] { p.g = pw1::geom(w_l, C, Cmid, HW); return pw1::launch_rule(p.g, B, 2ull * ts::kNumCU); },      // the geometry behind the envelope and the axes
      [&](auto MT, dim3 grid) { hipLaunchKernelGGL((expand_kernel<MT()>), grid, dim3(256), 0, ts::as_stream(stream), p); });
}

extern "C" int ts_mbconv_project_fwd(const float* x, const float* gate, const float* w_l, const float* scale, const float* shift,
                                     const float* residual, float* y, int B, int Cmid, int C, int H, int W, long long x_bstride,
                                     long long x_cstride, long long r_bstride, long long r_cstride, long long y_bstride,
                                     long long y_cstride, void* stream) {
  const char* who = "mbconv_project_fwd";
  TS_REQUIRE(B > 0 && C > 0 && Cmid > 0 && H > 0 && W > 0, TS_ERR_SHAPE, "%s: non-positive size", who);
  const long long HW = static_cast<long long>(H) * W;
  const node::Operand X{"x", x, Cmid, HW, x_bstride, x_cstride, node::IN}, R{"residual", residual, C, HW, r_bstride, r_cstride, node::RES},
      Y{"y", y, C, HW, y_bstride, y_cstride, node::OUT};
  Project p;
  p.x = X.plane(); p.gate = gate;
  p.ep = {scale, shift, ACT_NONE, R.plane(), {y, y_bstride, y_cstride}};
  return node::launch(
      who, "mbconv_project_kernel", B, {R, X, Y}, {{"gate", gate}}, w_l, {B, H, W}, [&] { return check_block(who, C, Cmid, HW); },
      [&] { p.g = pw1::geom(w_l, Cmid, C, HW); return pw1::launch_rule(p.g, B, 2ull * ts::kNumCU); },
      [&](auto MT, dim3 grid) { hipLaunchKernelGGL((project_kernel<MT()>), grid, dim3(256), 0, ts::as_stream(stream), p); });
}

extern "C" int ts_depthwise3x3_fwd(const float* x, const float* w, const float* scale, const float* shift, float* y, float* plane_sum,
                                   int B, int C, int H, int W, int act, int flip, long long x_bstride, long long x_cstride,
                                   long long y_bstride, long long y_cstride, void* stream) {
  TS_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, TS_ERR_SHAPE, "depthwise3x3_fwd: non-positive size");
  TS_REQUIRE(act == ACT_NONE || act == ACT_SILU, TS_ERR_SHAPE, "depthwise3x3_fwd: unknown activation %d", act);
  TS_REQUIRE(flip == 0 || flip == 1, TS_ERR_SHAPE, "depthwise3x3_fwd: flip must be 0 or 1");
  const long long HW = static_cast<long long>(H) * W;
  TS_REQUIRE(strides_ok(B, C, HW, x_bstride, x_cstride), TS_ERR_SHAPE, "depthwise3x3_fwd: x strides %lld / %lld overlap", x_bstride,
             x_cstride);
  TS_REQUIRE(strides_ok(B, C, HW, y_bstride, y_cstride), TS_ERR_SHAPE, "depthwise3x3_fwd: y strides %lld / %lld overlap", y_bstride,
             y_cstride);
  TS_REQUIRE(B < kMaxAxis && C < kMaxAxis && H < kMaxAxis && W < kMaxAxis, TS_ERR_UNSUPPORTED, "depthwise3x3_fwd: an axis of 2^20 or more");
  const unsigned blocks = corr::grid_blocks(static_cast<unsigned long long>(B) * C);
  TS_REQUIRE(blocks != 0, TS_ERR_UNSUPPORTED, "depthwise3x3_fwd: grid too large");
  TS_REQUIRE_PTR(x); TS_REQUIRE_PTR(w); TS_REQUIRE_PTR(y);
  if (int rc = node::check_overlap("depthwise3x3_fwd", B, {{"x", x, C, HW, x_bstride, x_cstride, node::IN}, {"y", y, C, HW, y_bstride, y_cstride, node::OUT}}))
    return rc;
  ts::dispatch_bool(rows_aligned(x, W, x_bstride, x_cstride), [&](auto VEC) {
    hipLaunchKernelGGL(depthwise_kernel<VEC()>, dim3(blocks), dim3(256), 0, ts::as_stream(stream), x, w, scale, shift, y, plane_sum, C, H,
                       W, act, flip, x_bstride, x_cstride, y_bstride, y_cstride);
  });
  return ts::launched("depthwise_kernel");
}

extern "C" int ts_depthwise3x3_bwd_weight(const float* x, const float* dy, float* dw, int B, int C, int H, int W, long long x_bstride,
                                          long long x_cstride, long long dy_bstride, long long dy_cstride, void* stream) {
  TS_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, TS_ERR_SHAPE, "depthwise3x3_bwd_weight: non-positive size");
  const long long HW = static_cast<long long>(H) * W;
  TS_REQUIRE(strides_ok(B, C, HW, x_bstride, x_cstride), TS_ERR_SHAPE, "depthwise3x3_bwd_weight: x strides %lld / %lld overlap", x_bstride,
             x_cstride);
  TS_REQUIRE(strides_ok(B, C, HW, dy_bstride, dy_cstride), TS_ERR_SHAPE, "depthwise3x3_bwd_weight: dy strides %lld / %lld overlap",
             dy_bstride, dy_cstride);
  TS_REQUIRE(B < kMaxAxis && C < kMaxAxis && H < kMaxAxis && W < kMaxAxis, TS_ERR_UNSUPPORTED,
             "depthwise3x3_bwd_weight: an axis of 2^20 or more");
  TS_REQUIRE_PTR(x); TS_REQUIRE_PTR(dy); TS_REQUIRE_PTR(dw);
  ts::dispatch_bool(rows_aligned(x, W, x_bstride, x_cstride), [&](auto VEC) {
    hipLaunchKernelGGL(depthwise_wgrad_kernel<VEC()>, dim3(C), dim3(256), 0, ts::as_stream(stream), x, dy, dw, B, H, W, x_bstride,
                       x_cstride, dy_bstride, dy_cstride);
  });
  return ts::launched("depthwise_wgrad_kernel");
}

extern "C" int ts_se_gate_fwd(const float* plane_sum, const float* w_reduce, const float* b_reduce, const float* w_expand,
                              const float* b_expand, float* gate, int B, int Cmid, int Cr, float inv_hw, void* stream) {
  TS_REQUIRE(B > 0 && Cmid > 0 && Cr > 0, TS_ERR_SHAPE, "se_gate_fwd: non-positive size");
  TS_REQUIRE(Cmid <= kMaxMid && Cr <= kMaxC && B < kMaxAxis, TS_ERR_UNSUPPORTED, "se_gate_fwd: Cmid = %d above %d, Cr = %d above %d or a batch of 2^20 or more",
             Cmid, kMaxMid, Cr, kMaxC);
  TS_REQUIRE_PTR(plane_sum); TS_REQUIRE_PTR(w_reduce); TS_REQUIRE_PTR(b_reduce); TS_REQUIRE_PTR(w_expand); TS_REQUIRE_PTR(b_expand);
  TS_REQUIRE_PTR(gate);
  const int slices = (Cmid + 255) / 256;
  hipLaunchKernelGGL(se_gate_kernel, dim3(static_cast<unsigned>(B) * slices), dim3(256), 0, ts::as_stream(stream), plane_sum, w_reduce,
                     b_reduce, w_expand, b_expand, gate, Cmid, Cr, slices, Cmid % 4 == 0 && ts::aligned16(w_reduce),
                     Cr % 4 == 0 && ts::aligned16(w_expand), inv_hw);
  return ts::launched("se_gate_kernel");
}
