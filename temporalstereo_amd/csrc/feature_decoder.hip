// FeatureDecoder (reference: architecture/modeling/backbone/TemporalStereo.py:78-90,125-138): the backbone's three-level decoder -- seven
// 3x3 convolutions, three align-corners bilinear resizes, three concatenations -- fp32 throughout.
//
//   x16 = deconv32_16(cat([resize(conv32(x32)), x16]))   x8 = deconv16_8(cat([resize(x16), x8]))   x4 = deconv8_4(cat([resize(x8), x4]))
//
// decoder_conv_kernel<MT> is conv_hw3.hpp's 3x3 convolution (geometry, staging, pitches and the blocked summation: there) whose
// input channels come from TWO tensors, neither written anywhere first: channels [0, Cu) are `up` [B,Cu,h,w] read THROUGH the
// align-corners bilinear resize to (H, W) (ts::lin_src, the coordinates of every other resize of the library; the four taps are
// combined while the halo tile is staged), channels [Cu, Cu + Cs) are `skip` [B,Cs,H,W] read in place.  The convolution's zero
// padding applies to the resized map: a halo position outside (H, W) is staged as 0.  Cu = 0 is the plain wide convolution.
// The accumulators are flushed every kFlush chunks: K reaches 4608 here.
// Epilogue: act(y * scale + shift), act 0 none | 1 silu_fast; scale / shift may be NULL (1 / 0).
//
// resize_bilinear_bwd_kernel is the adjoint of the align-corners resize as a GATHER: a coarse pixel sums, rows then columns in
// ascending order, the fine pixels whose two source indices (ts::lin_src again, evaluated per candidate: the forward's own
// predicate) include it.  No atomics: bit-reproducible.
#include "bilinear.hpp"
#include "conv_hw3.hpp"

namespace {

constexpr int kMaxC = 512;                   // Cu + Cs and Cout
constexpr int kFlush = 4;                    // chunks (32 input channels, 288 products) per block of the blocked summation
using node::kGridCap;
using node::kMaxAxis;
using node::pitch_for;
using ts::strides_ok;

struct Dec {
  hw3::Geom g;              // rows: Cout
  const float* up;          // source of channels [0, Cu), [B,Cu,h,w], read through the resize
  const float* skip;        // source of channels [Cu, Cu + Cs), [B,Cs,H,W]
  node::Affine<> ep;        // act(sum * scale + shift), no residual
  int Cu, h, w_in;
  float sh, sw;             // source steps of the resize
  long long up_bs, up_cs, skip_bs, skip_cs;

  // the lambda holds copies of what it uses, never `this`: a store through y then cannot be taken to change a field
  __device__ __forceinline__ auto source(int b) const {
    return [pu = up + b * up_bs, ps = skip + b * skip_bs, Cu = Cu, up_cs = up_cs, skip_cs = skip_cs, h = h, w_in = w_in, sh = sh, sw = sw,
            W = g.W](int gc, int gy, int gx) {
      if (gc < Cu) return ts::rescaled_at<long long>(pu + gc * up_cs, w_in, 1, h, w_in, sh, sw, 1.f, gy, gx);
      return ps[(gc - Cu) * skip_cs + hw3::pixel_at(gy, gx, W)];
    };
  }
  __device__ __forceinline__ auto sink(int b, int gy, int gx) const { return ep.writer(b, hw3::pixel_at(gy, gx, g.W)); }
};

template <int MT>
__global__ void __launch_bounds__(256) decoder_conv_kernel(const Dec p) { hw3::conv_tile<MT, kFlush>(p); }

// candidate fine indices whose source interval can touch coarse index c: [lo, hi], one more on either side than the real range
__device__ __forceinline__ void fine_range(float scale, int c, int out_size, int& lo, int& hi) {
  lo = 0; hi = out_size - 1;
  if (scale > 0.f) {
    const float inv = 1.f / scale;
    const float a = (static_cast<float>(c) - 1.f) * inv - 1.f, e = (static_cast<float>(c) + 1.f) * inv + 2.f;
    lo = a > 0.f ? static_cast<int>(a) : 0;
    if (e < static_cast<float>(out_size - 1)) hi = static_cast<int>(e);
  }
}

// weight with which fine index `dst` reads coarse index c in the forward pass (0: it does not)
__device__ __forceinline__ float tap_weight(float scale, int dst, int in_size, int c) {
  int i0, i1;
  float l1;
  ts::lin_src(scale, dst, in_size, i0, i1, l1);
  return (i0 == c ? 1.f - l1 : 0.f) + (i1 == c ? l1 : 0.f);
}

__global__ void __launch_bounds__(256) resize_bilinear_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, int B, int C,
                                                                  int h, int w, int H, int W, float sh, float sw, long long dy_bs,
                                                                  long long dy_cs, long long dx_bs, long long dx_cs) {
  const long long hw = static_cast<long long>(h) * w, total = static_cast<long long>(B) * C * hw;
  for (long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x; i < total; i += static_cast<long long>(gridDim.x) * 256) {
    const long long bc = i / hw, pix = i - bc * hw;
    const int b = static_cast<int>(bc / C), c = static_cast<int>(bc % C);
    const int y = static_cast<int>(pix / w), x = static_cast<int>(pix - static_cast<long long>(y) * w);
    int ylo, yhi, xlo, xhi;
    fine_range(sh, y, H, ylo, yhi);
    fine_range(sw, x, W, xlo, xhi);
    const float* g = dy + b * dy_bs + c * dy_cs;
    float acc = 0.f;
    for (int oy = ylo; oy <= yhi; ++oy) {
      const float wy = tap_weight(sh, oy, h, y);
      if (wy == 0.f) continue;
      const float* grow = g + static_cast<long long>(oy) * W;
      float rsum = 0.f;
      for (int ox = xlo; ox <= xhi; ++ox) {
        const float wx = tap_weight(sw, ox, w, x);
        if (wx != 0.f) rsum = fmaf(wx, grow[ox], rsum);
      }
      acc = fmaf(wy, rsum, acc);
    }
    dx[b * dx_bs + c * dx_cs + pix] = acc;
  }
}

}  // namespace

extern "C" size_t ts_decoder_weight_bytes(int Cin, int Cout) {
  if (Cin <= 0 || Cout <= 0 || Cin > kMaxC || Cout > kMaxC) return 0;
  return hw3::image_floats(Cin, pitch_for(Cout)) * sizeof(float);
}

extern "C" int ts_decoder_weight_layout(const float* w, float* w_l, int Cin, int Cout, void* stream) {
  TS_REQUIRE(Cin > 0 && Cout > 0, TS_ERR_SHAPE, "decoder_weight_layout: non-positive size");
  TS_REQUIRE(Cin <= kMaxC && Cout <= kMaxC, TS_ERR_UNSUPPORTED, "decoder_weight_layout: Cin=%d / Cout=%d above %d", Cin, Cout, kMaxC);
  TS_REQUIRE_PTR(w); TS_REQUIRE_PTR(w_l);
  TS_REQUIRE_ALIGNED(w_l);
  hw3::WeightImages im;          // one weight, one image
  im.wa = w; im.ra = Cout; im.wb = nullptr; im.rb = 0; im.p0 = pitch_for(Cout);
  im.wc = nullptr; im.rc = 0; im.p1 = 0;
  return hw3::weight_layout(im, w_l, Cin, kGridCap, ts::as_stream(stream), "decoder_weight_layout_kernel");
}

extern "C" int ts_decoder_conv_fwd(const float* up, const float* skip, const float* w_l, const float* scale, const float* shift, float* y,
                                   int B, int Cu, int Cs, int Cout, int h, int w, int H, int W, int act, long long up_bstride,
                                   long long up_cstride, long long skip_bstride, long long skip_cstride, long long y_bstride,
                                   long long y_cstride, void* stream) {
  const char* who = "decoder_conv_fwd";
  TS_REQUIRE(B > 0 && Cu >= 0 && Cs > 0 && Cout > 0 && H > 0 && W > 0 && (Cu == 0 || (h > 0 && w > 0)), TS_ERR_SHAPE, "%s: non-positive size", who);
  TS_REQUIRE(act == ACT_NONE || act == ACT_SILU, TS_ERR_SHAPE, "%s: unknown activation %d", who, act);
  const long long HW = static_cast<long long>(H) * W;
  const node::Operand U{"up", up, Cu, static_cast<long long>(h) * w, up_bstride, up_cstride, node::IN},
      S{"skip", skip, Cs, HW, skip_bstride, skip_cstride, node::IN}, Y{"y", y, Cout, HW, y_bstride, y_cstride, node::OUT};
  Dec p;
  p.up = up; p.skip = skip;
  p.Cu = Cu; p.h = Cu ? h : 1; p.w_in = Cu ? w : 1;
  p.sh = ts::ac_scale(p.h, H); p.sw = ts::ac_scale(p.w_in, W);
  p.up_bs = up_bstride; p.up_cs = up_cstride; p.skip_bs = skip_bstride; p.skip_cs = skip_cstride;
  p.ep = {scale, shift, act, {nullptr, 0, 0}, {y, y_bstride, y_cstride}};
  auto envelope = [&] {
    TS_REQUIRE(Cu + Cs <= kMaxC && Cout <= kMaxC, TS_ERR_UNSUPPORTED, "%s: Cu + Cs = %d / Cout = %d above %d", who, Cu + Cs, Cout, kMaxC);
    return TS_OK;
  };
  // A grid of fewer than two workgroups per compute unit is cut finer along the rows (hw3::launch_rule): a lone workgroup has nothing
  // to hide its staging behind (measured at 1, 2 and 4 per compute unit: batch 2 of the 544 x 960 decoder 1385 / 1218 / 1187 us,
  // batch 8 3194 / 3175 / 3239 us).
  return node::launch(
      who, "decoder_conv_kernel", B, {U, S, Y}, {}, w_l, {B, H, W, h, w}, envelope,
      [&] {          // the geometry behind the envelope and the axes
        p.g = hw3::geom(w_l, Cu + Cs, Cout, H, W, pitch_for(Cout));
        return hw3::launch_rule(p.g, B, 2ull * ts::kNumCU);
      },
      [&](auto MT, dim3 grid) { hipLaunchKernelGGL((decoder_conv_kernel<MT()>), grid, dim3(256), 0, ts::as_stream(stream), p); });
}

extern "C" int ts_resize_bilinear_bwd(const float* dy, float* dx, int B, int C, int h, int w, int H, int W, long long dy_bstride,
                                      long long dy_cstride, long long dx_bstride, long long dx_cstride, void* stream) {
  TS_REQUIRE(B > 0 && C > 0 && h > 0 && w > 0 && H > 0 && W > 0, TS_ERR_SHAPE, "resize_bilinear_bwd: non-positive size");
  TS_REQUIRE(strides_ok(B, C, static_cast<long long>(H) * W, dy_bstride, dy_cstride), TS_ERR_SHAPE,
             "resize_bilinear_bwd: dy strides %lld / %lld overlap", dy_bstride, dy_cstride);
  TS_REQUIRE(strides_ok(B, C, static_cast<long long>(h) * w, dx_bstride, dx_cstride), TS_ERR_SHAPE,
             "resize_bilinear_bwd: dx strides %lld / %lld overlap", dx_bstride, dx_cstride);
  TS_REQUIRE(B < kMaxAxis && C < kMaxAxis && h < kMaxAxis && w < kMaxAxis && H < kMaxAxis && W < kMaxAxis, TS_ERR_UNSUPPORTED,
             "resize_bilinear_bwd: an axis of 2^20 or more");
  TS_REQUIRE_PTR(dy); TS_REQUIRE_PTR(dx);
  hipLaunchKernelGGL(resize_bilinear_bwd_kernel, dim3(ts::blocks_for(static_cast<long long>(B) * C * h * w, kGridCap)), dim3(256), 0,
                     ts::as_stream(stream), dy, dx, B, C, h, w, H, W, ts::ac_scale(h, H), ts::ac_scale(w, W), dy_bstride, dy_cstride,
                     dx_bstride, dx_cstride);
  return ts::launched("resize_bilinear_bwd_kernel");
}
