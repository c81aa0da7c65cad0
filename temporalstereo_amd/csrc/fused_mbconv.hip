// The encoder's large planes (reference: architecture/modeling/backbone/TemporalStereo.py:62-70,105-113 -- the stem, block0's ConvBnAct
// members and the fused-MBConv (EdgeResidual) members of block1 and block2 of timm's efficientnetv2_rw_s), fp32 throughout, no atomics.
//
//   y = act(conv3x3(x, stride s, padding 1) * scale + shift) (+ residual)        conv3x3_kernel<MT, S>      s = 1 | 2
//   y = conv1x1(x) * scale + shift (+ residual)                                  fused_project_kernel<MT>
//
// A ConvBnAct and the stem are the first alone; a fused block is the first (the 3x3 expansion, BatchNorm, SiLU: it writes the mid map)
// and then the second (the 1x1 projection, BatchNorm, the residual).  The residual of the first is added AFTER the activation (the
// ConvBnAct order) and is taken for s = 1 only.
//
// conv3x3_kernel<MT, 1> is conv_hw3.hpp's 3x3 convolution (geometry, staging, pitches and the blocked summation: there) with a plain
// reader: channel gc of `x` in place through its batch / channel strides.
//
// conv3x3_kernel<MT, 2> is THE SAME core, untouched, in the phase form.  A stride-2 3x3 convolution of x [Cin, H, W] is a stride-1 3x3
// convolution over 4 Cin phase channels on the output plane (ceil(H / 2), ceil(W / 2)):
//     phase channel gc = 4 c + 2 py + px,      its value at (gy, gx) is x[c, 2 gy + py, 2 gx + px]   (zero past H or W: odd sizes)
// Output (oy, ox) reads input rows 2 oy - 1, 2 oy, 2 oy + 1: row 2 oy - 1 is phase 1 at gy = oy - 1, row 2 oy is phase 0 at gy = oy and
// row 2 oy + 1 is phase 1 at gy = oy.  So along an axis phase 0 carries the centre weight on the tap at offset 0, phase 1 carries the
// first weight on the tap at offset -1 and the last weight on the tap at offset 0; the taps at offset +1 are zero.  The weight image
// (conv3x3_weight_layout_kernel) is written in that order, zeros included, and the reader maps gc -> (c, py, px) and reads x in place.
// The core predicates a read on the OUTPUT plane alone, so the reader itself answers zero where 2 gy + py >= H or 2 gx + px >= W.
// K is four times the true length (27 of 108, 216 of 864 and 432 of 1728 products are real in the three strided layers of the
// encoder): the price of leaving the core as it is, paid on its three smallest layers.
//
// Summation.  Both strides run the core with FLUSH = 4, the decoder's: the accumulators are added into a second set every four chunks
// (32 core channels, 288 products).  Up to 32 core channels -- the stem (12 phase channels), block0 (24) and a stride-1 expansion
// of 24 channels -- that is ONE chain (no flush is reached; tot = 0 is added once); above, a chain of 288 products, then a chain of
// blocks: 48 and 64 channels at stride 1 are two blocks, 24 and 48 at stride 2 (96 and 192 phase channels) three and six.
// The projection is conv_pw1.hpp's core with FLUSH = 8 (mbconv.hip's): chains of 256 products, then a chain of blocks; Cmid = 96, 192
// and 256 are one chain.  An output's chains run over the channels in order whatever MT, `groups` and the batch are.
#include "conv_pw1.hpp"

namespace {

constexpr int kMaxC = 512;                   // the 3x3's core channels (Cin at stride 1, 4 Cin at stride 2) and its Cout; the projection's Cout
constexpr int kMaxMid = 2048;                // the projection's Cin
constexpr int kFlush3 = 4;                   // the 3x3: chunks (32 core channels, 288 products) per block of the blocked summation
constexpr int kFlush1 = 8;                   // the 1x1: chunks (256 input channels) per block
using node::pitch_for;

inline int core_channels(int Cin, int stride) { return stride == 2 ? 4 * Cin : Cin; }

template <int S>
struct Conv3 {
  hw3::Geom g;              // Cin: core channels; H, W: the OUTPUT plane; rows: Cout
  node::Plane<const float> x;      // [B,Cin,Hin,Win]
  node::Affine<> ep;        // act(sum * scale + shift) + residual [B,Cout,H,W]
  int Hin, Win;

  // the lambda holds copies of what it uses, never `this`: a store through y then cannot be taken to change a field
  __device__ __forceinline__ auto source(int b) const {
    return [px = x.at(b, 0), x_cs = x.cs, Hin = Hin, Win = Win](int gc, int gy, int gx) {
      if constexpr (S == 1) {
        (void)Hin;
        return px[gc * x_cs + hw3::pixel_at(gy, gx, Win)];
      } else {
        const int iy = 2 * gy + ((gc >> 1) & 1), ix = 2 * gx + (gc & 1);       // inside the output plane: both non-negative
        return (iy < Hin && ix < Win) ? px[(gc >> 2) * x_cs + hw3::pixel_at(iy, ix, Win)] : 0.f;
      }
    };
  }
  __device__ __forceinline__ auto sink(int b, int gy, int gx) const { return ep.writer(b, hw3::pixel_at(gy, gx, g.W)); }
};

using Project = pw1::Project<false>;     // Cin: Cmid, rows: Cout

template <int MT, int S>
__global__ void __launch_bounds__(256) conv3x3_kernel(const Conv3<S> p) { hw3::conv_tile<MT, kFlush3>(p); }
template <int MT>
__global__ void __launch_bounds__(256) fused_project_kernel(const Project p) { pw1::conv_tile<MT, kFlush1>(p); }

// the weight of tap t (0..2: offsets -1, 0, +1) of a phase along one axis, as an index into the 3 framework weights, or -1: zero
__device__ __forceinline__ int phase_tap(int phase, int t) { return phase == 0 ? (t == 1 ? 1 : -1) : (t == 0 ? 0 : t == 1 ? 2 : -1); }

// w [rows][Cin][3][3] -> hw3's [chunk][tap][8][pitch] over the core channels; stride 2: the phase order, zeros included
__global__ void __launch_bounds__(256) conv3x3_weight_layout_kernel(const float* __restrict__ w, float* __restrict__ out, int Cin, int rows,
                                                                    int stride, int pitch, int total) {
  const int Cc = stride == 2 ? 4 * Cin : Cin;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const int col = i % pitch, k = i / pitch;
    const int c = k % hw3::kCK, tap = (k / hw3::kCK) % 9, gc = (k / hw3::kKC) * hw3::kCK + c;
    float v = 0.f;
    if (gc < Cc && col < rows) {
      int ci = gc, at = tap;
      if (stride == 2) {
        const int ky = phase_tap((gc >> 1) & 1, tap / 3), kx = phase_tap(gc & 1, tap % 3);
        ci = gc >> 2;
        at = (ky < 0 || kx < 0) ? -1 : ky * 3 + kx;
      }
      if (at >= 0) v = w[(static_cast<size_t>(col) * Cin + ci) * 9 + at];
    }
    out[i] = v;
  }
}

}  // namespace

extern "C" size_t ts_conv3x3_s_weight_bytes(int Cin, int Cout, int stride) {
  if (Cin <= 0 || Cout <= 0 || (stride != 1 && stride != 2) || Cin > kMaxC || core_channels(Cin, stride) > kMaxC || Cout > kMaxC) return 0;
  return hw3::image_floats(core_channels(Cin, stride), pitch_for(Cout)) * sizeof(float);
}

extern "C" int ts_conv3x3_s_weight_layout(const float* w, float* w_l, int Cin, int Cout, int stride, void* stream) {
  TS_REQUIRE(Cin > 0 && Cout > 0, TS_ERR_SHAPE, "conv3x3_s_weight_layout: non-positive size");
  TS_REQUIRE(stride == 1 || stride == 2, TS_ERR_SHAPE, "conv3x3_s_weight_layout: stride %d is neither 1 nor 2", stride);
  TS_REQUIRE(Cin <= kMaxC && core_channels(Cin, stride) <= kMaxC && Cout <= kMaxC, TS_ERR_UNSUPPORTED,
             "conv3x3_s_weight_layout: %d core channels (Cin = %d, stride %d) / Cout = %d above %d", core_channels(Cin, stride), Cin, stride, Cout, kMaxC);
  TS_REQUIRE_PTR(w); TS_REQUIRE_PTR(w_l);
  TS_REQUIRE_ALIGNED(w_l);
  const int pitch = pitch_for(Cout);
  const size_t total = hw3::image_floats(core_channels(Cin, stride), pitch);           // at most 64 x 72 x 512
  hipLaunchKernelGGL(conv3x3_weight_layout_kernel, dim3(ts::blocks_for(static_cast<long long>(total), node::kGridCap)), dim3(256), 0,
                     ts::as_stream(stream), w, w_l, Cin, Cout, stride, pitch, static_cast<int>(total));
  return ts::launched("conv3x3_weight_layout_kernel");
}

extern "C" int ts_conv3x3_s_fwd(const float* x, const float* w_l, const float* scale, const float* shift, const float* residual, float* y,
                                int B, int Cin, int Cout, int H, int W, int stride, int act, long long x_bstride, long long x_cstride,
                                long long r_bstride, long long r_cstride, long long y_bstride, long long y_cstride, void* stream) {
  TS_REQUIRE(B > 0 && Cin > 0 && Cout > 0 && H > 0 && W > 0, TS_ERR_SHAPE, "conv3x3_s_fwd: non-positive size");
  TS_REQUIRE(stride == 1 || stride == 2, TS_ERR_SHAPE, "conv3x3_s_fwd: stride %d is neither 1 nor 2", stride);
  TS_REQUIRE(act == ACT_NONE || act == ACT_SILU, TS_ERR_SHAPE, "conv3x3_s_fwd: unknown activation %d", act);
  TS_REQUIRE(residual == nullptr || stride == 1, TS_ERR_SHAPE, "conv3x3_s_fwd: a residual is taken at stride 1 only");
  const char* who = "conv3x3_s_fwd";
  const int Ho = (H + stride - 1) / stride, Wo = (W + stride - 1) / stride;
  const long long HW = static_cast<long long>(H) * W, HWo = static_cast<long long>(Ho) * Wo;
  const int Cc = core_channels(Cin <= kMaxC ? Cin : kMaxC + 1, stride);
  const node::Operand X{"x", x, Cin, HW, x_bstride, x_cstride, node::IN},
      R{"residual", residual, residual ? Cout : 0, HWo, r_bstride, r_cstride, node::RES}, Y{"y", y, Cout, HWo, y_bstride, y_cstride, node::OUT};
  hw3::Geom g;
  auto envelope = [&] {
    TS_REQUIRE(Cc <= kMaxC && Cout <= kMaxC, TS_ERR_UNSUPPORTED, "%s: %d core channels (Cin = %d, stride %d) / Cout = %d above %d", who, Cc, Cin, stride,
               Cout, kMaxC);
    return TS_OK;
  };
  // as the decoder: fewer than two workgroups per compute unit are cut finer along the rows
  auto rule = [&] {          // the geometry behind the envelope and the axes
    g = hw3::geom(w_l, Cc, Cout, Ho, Wo, pitch_for(Cout));
    return hw3::launch_rule(g, B, 2ull * ts::kNumCU);
  };
  auto run = [&](auto S) {
    return node::launch(who, "conv3x3_kernel", B, {R, X, Y}, {}, w_l, {B, H, W}, envelope, rule, [&](auto MT, dim3 grid) {
      const Conv3<S()> p{g, X.plane(), {scale, shift, act, R.plane(), {y, y_bstride, y_cstride}}, H, W};
      hipLaunchKernelGGL((conv3x3_kernel<MT(), S()>), grid, dim3(256), 0, ts::as_stream(stream), p);
    });
  };
  return stride == 1 ? run(std::integral_constant<int, 1>{}) : run(std::integral_constant<int, 2>{});
}

extern "C" int ts_fused_project_fwd(const float* x, const float* w_l, const float* scale, const float* shift, const float* residual,
                                    float* y, int B, int Cmid, int Cout, int H, int W, long long x_bstride, long long x_cstride,
                                    long long r_bstride, long long r_cstride, long long y_bstride, long long y_cstride, void* stream) {
  const char* who = "fused_project_fwd";
  TS_REQUIRE(B > 0 && Cmid > 0 && Cout > 0 && H > 0 && W > 0, TS_ERR_SHAPE, "%s: non-positive size", who);
  const long long HW = static_cast<long long>(H) * W;
  const node::Operand X{"x", x, Cmid, HW, x_bstride, x_cstride, node::IN},
      R{"residual", residual, residual ? Cout : 0, HW, r_bstride, r_cstride, node::RES}, Y{"y", y, Cout, HW, y_bstride, y_cstride, node::OUT};
  Project p;
  p.x = X.plane(); p.gate = nullptr;
  p.ep = {scale, shift, ACT_NONE, R.plane(), {y, y_bstride, y_cstride}};
  auto envelope = [&] {
    TS_REQUIRE(Cout <= kMaxC && Cmid <= kMaxMid, TS_ERR_UNSUPPORTED, "%s: Cout = %d above %d or Cmid = %d above %d", who, Cout, kMaxC, Cmid, kMaxMid);
    return pw1::check_plane(who, HW);
  };
  return node::launch(
      who, "fused_project_kernel", B, {R, X, Y}, {}, w_l, {B, H, W}, envelope,
      [&] { p.g = pw1::geom(w_l, Cmid, Cout, HW); return pw1::launch_rule(p.g, B, 2ull * ts::kNumCU); },
      [&](auto MT, dim3 grid) { hipLaunchKernelGGL((fused_project_kernel<MT()>), grid, dim3(256), 0, ts::as_stream(stream), p); });
}
