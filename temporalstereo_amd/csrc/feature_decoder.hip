// FeatureDecoder (reference: architecture/modeling/backbone/TemporalStereo.py:78-90,125-138): the backbone's three-level decoder -- seven
// 3x3 convolutions, three align-corners bilinear resizes, three concatenations -- fp32 throughout.
//
//   x16 = deconv32_16(cat([resize(conv32(x32)), x16]))   x8 = deconv16_8(cat([resize(x16), x8]))   x4 = deconv8_4(cat([resize(x8), x4]))
//
// decoder_conv_kernel<MT> is one implicit-GEMM 3x3 convolution (stride 1, padding 1) on v_mfma_f32_16x16x4_f32 -- bitwise an fmaf
// chain -- whose input channels come from TWO tensors, neither written anywhere first: channels [0, Cu) are `up` [B,Cu,h,w] read
// THROUGH the align-corners bilinear resize to (H, W) (ts::lin_src, the coordinates of every other resize of the library; the four
// taps are combined while the halo tile is staged), channels [Cu, Cu + Cs) are `skip` [B,Cs,H,W] read in place.  The convolution's
// zero padding applies to the resized map: a halo position outside (H, W) is staged as 0.  Cu = 0 is the plain wide convolution.
// The geometry is conv_gru.hip's: a workgroup (4 waves) owns a 2 x 32 pixel tile and MT blocks of 16 output rows, a wave 16 pixels
// of one tile row and MT accumulators; output channels beyond 16 MT are tiled over the grid (neighbouring workgroups share the input
// tile, so the second and later read it from L2).  K runs over chunks of 8 input channels x 9 taps, k = tap * 8 + channel inside a
// chunk; the B operand is read straight from the staged halo tile (4 x 34 per channel), no im2col image.  The source seam may fall
// anywhere in a chunk: the source is chosen per staged channel.  Every global read is predicated on row, column and channel.
// K reaches 4608 here, and one fp32 fmaf chain of that length sits at four times the error of the framework's blocked sums: the
// accumulators are added into a second set every kFlush chunks (a chain of 288 products, then a chain of at most 16 blocks).  An
// output's chains run over the input channels in order whatever MT is, so the bits do not depend on the launch geometry.
// Epilogue: act(y * scale + shift), act 0 none | 1 silu_fast; scale / shift may be NULL (1 / 0).
// Weights are pre-laid by decoder_weight_layout_kernel as [chunk][tap][8][rows padded] (zero rows / channels included).
//
// resize_bilinear_bwd_kernel is the adjoint of the align-corners resize as a GATHER: a coarse pixel sums, rows then columns in
// ascending order, the fine pixels whose two source indices (ts::lin_src again, evaluated per candidate: the forward's own
// predicate) include it.  No atomics: bit-reproducible.
#include "bilinear.hpp"
#include "conv_common.hpp"

namespace {

constexpr int kCK = 8;                       // input channels per staged chunk
constexpr int kKC = kCK * 9;                 // contraction elements per chunk
constexpr int kTR = 2, kTW = 32;             // pixel tile
constexpr int kRowP = 36;                    // halo row pitch (34 columns staged)
constexpr int kChP = (kTR + 2) * kRowP;      // 144 == 16 mod 32: the two kq of a lane half land on disjoint banks
constexpr int kMaxC = 512;                   // Cu + Cs and Cout
constexpr int kFlush = 4;                    // chunks (32 input channels, 288 products) per block of the blocked summation
constexpr int kMaxAxis = 1 << 20;

constexpr int w_pitch(int mt) { return (mt * 16) % 32 == 16 ? mt * 16 : mt * 16 + 16; }
inline int mt_for(int rows) { return rows <= 16 ? 1 : rows <= 32 ? 2 : rows <= 64 ? 4 : 8; }
inline int pitch_for(int rows) { return rows <= 64 ? 64 : (rows + 127) / 128 * 128; }      // whole workgroups of any MT
inline int chunks_for(int Cin) { return (Cin + kCK - 1) / kCK; }
inline size_t weight_floats(int Cin, int Cout) { return static_cast<size_t>(chunks_for(Cin)) * kKC * pitch_for(Cout); }

struct Dec {
  const float* up;          // source of channels [0, Cu), [B,Cu,h,w], read through the resize
  const float* skip;        // source of channels [Cu, Cu + Cs), [B,Cs,H,W]
  const float* w;           // [chunks][9][8][rp]
  const float* scale;
  const float* shift;
  float* y;
  int Cu, Cs, Cout, h, w_in, H, W, tiles_x, tiles_y;
  int rp, groups, act;
  float sh, sw;             // source steps of the resize
  long long up_bs, up_cs, skip_bs, skip_cs, y_bs, y_cs;
};

template <int MT>
__global__ void __launch_bounds__(256) decoder_conv_kernel(const Dec p) {
  constexpr int PW = w_pitch(MT);
  constexpr int kHalo = (kTR + 2) * (kTW + 2);                  // staged values per channel
  __shared__ __attribute__((aligned(16))) float sW[kKC * PW];
  __shared__ float sX[kCK * kChP];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 15, kq = lane >> 4;
  unsigned blk = blockIdx.x;
  const int rg = blk % p.groups; blk /= p.groups;               // neighbours share the input tile
  const int tx = blk % p.tiles_x; blk /= p.tiles_x;
  const int ty = blk % p.tiles_y;
  const int b = blk / p.tiles_y;
  const int x0 = tx * kTW, y0 = ty * kTR;
  const int Cin = p.Cu + p.Cs;
  const float* pu = p.up + b * p.up_bs;
  const float* ps = p.skip + b * p.skip_bs;
  const float* pw = p.w + rg * (16 * MT);
  const int pr = wave >> 1, pc = (wave & 1) * 16 + j;

  v4f acc[MT], tot[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t] = tot[t] = v4f{0.f, 0.f, 0.f, 0.f};

  const int nchunks = (Cin + kCK - 1) / kCK;
  for (int ch = 0; ch < nchunks; ++ch) {
    if (ch != 0 && ch % kFlush == 0) {                           // blocked summation: a chain of 288 products, then a chain of blocks
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        tot[t] += acc[t];
        acc[t] = v4f{0.f, 0.f, 0.f, 0.f};
      }
    }
    __syncthreads();                                             // the previous chunk has been read
    for (int i = tid; i < kKC * 4 * MT; i += 256) {              // this workgroup's columns of the chunk's 72 weight rows, 16 bytes a piece
      const int row = i / (4 * MT), seg = i % (4 * MT);
      *reinterpret_cast<float4*>(sW + row * PW + seg * 4) =
          *reinterpret_cast<const float4*>(pw + (static_cast<size_t>(ch) * kKC + row) * p.rp + seg * 4);
    }
    for (int i = tid; i < kCK * kHalo; i += 256) {               // halo tile, 8 channels x 4 rows x 34 columns
      const int c = i / kHalo, rem = i - c * kHalo;
      const int row = rem / (kTW + 2), col = rem - row * (kTW + 2);
      const int gc = ch * kCK + c, gy = y0 - 1 + row, gx = x0 - 1 + col;
      float v = 0.f;
      if (gc < Cin && gy >= 0 && gy < p.H && gx >= 0 && gx < p.W) {      // every read predicated on channel, row and column
        if (gc < p.Cu) v = ts::rescaled_at<long long>(pu + gc * p.up_cs, p.w_in, 1, p.h, p.w_in, p.sh, p.sw, 1.f, gy, gx);
        else v = ps[(gc - p.Cu) * p.skip_cs + static_cast<long long>(gy) * p.W + gx];
      }
      sX[c * kChP + row * kRowP + col] = v;
    }
    __syncthreads();
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int c = half * 4 + kq;
        const float bv = sX[c * kChP + (pr + tap / 3) * kRowP + pc + tap % 3];
        const float* wrow = sW + (tap * kCK + c) * PW + j;
#pragma unroll
        for (int t = 0; t < MT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wrow[16 * t], bv, acc[t], 0, 0, 0);
      }
    }
  }

  // epilogue: the lane holds rows 16 (MT rg + t) + 4 kq + r of pixel (y0 + pr, x0 + pc)
  const int gy = y0 + pr, gx = x0 + pc;
  if (gy >= p.H || gx >= p.W) return;
  float* py = p.y + b * p.y_bs + static_cast<long long>(gy) * p.W + gx;
#pragma unroll
  for (int t = 0; t < MT; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * (MT * rg + t) + 4 * kq + r;
      if (row >= p.Cout) continue;
      float v = tot[t][r] + acc[t][r];
      if (p.scale) v *= p.scale[row];
      if (p.shift) v += p.shift[row];
      py[row * p.y_cs] = p.act == ACT_SILU ? silu_fast(v) : v;
    }
  }
}

// w [Cout][Cin][3][3] (the framework's, contiguous) -> [chunk][tap][8][pitch]
__global__ void __launch_bounds__(256) decoder_weight_layout_kernel(const float* __restrict__ w, float* __restrict__ out, int Cin,
                                                                    int Cout, int pitch, int total) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const int col = i % pitch, k = i / pitch;
    const int c = k % kCK, tap = (k / kCK) % 9, ci = (k / kKC) * kCK + c;
    out[i] = (ci < Cin && col < Cout) ? w[(static_cast<size_t>(col) * Cin + ci) * 9 + tap] : 0.f;
  }
}

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

unsigned blocks_for(long long items) {
  long long n = (items + 255) / 256;
  if (n > 4096) n = 4096;
  return static_cast<unsigned>(n < 1 ? 1 : n);
}

bool strides_ok(int B, int C, long long vol, long long bs, long long cs) {
  if (C == 0) return true;
  return cs >= vol && (B == 1 || bs >= cs * (C - 1) + vol);
}

}  // namespace

extern "C" size_t ts_decoder_weight_bytes(int Cin, int Cout) {
  if (Cin <= 0 || Cout <= 0 || Cin > kMaxC || Cout > kMaxC) return 0;
  return weight_floats(Cin, Cout) * sizeof(float);
}

extern "C" int ts_decoder_weight_layout(const float* w, float* w_l, int Cin, int Cout, void* stream) {
  TS_REQUIRE(Cin > 0 && Cout > 0, TS_ERR_SHAPE, "decoder_weight_layout: non-positive size");
  TS_REQUIRE(Cin <= kMaxC && Cout <= kMaxC, TS_ERR_UNSUPPORTED, "decoder_weight_layout: Cin=%d / Cout=%d above %d", Cin, Cout, kMaxC);
  TS_REQUIRE_PTR(w); TS_REQUIRE_PTR(w_l);
  TS_REQUIRE_ALIGNED(w_l);
  const int total = static_cast<int>(weight_floats(Cin, Cout));          // at most 64 x 72 x 512
  hipLaunchKernelGGL(decoder_weight_layout_kernel, dim3(blocks_for(total)), dim3(256), 0, ts::as_stream(stream), w, w_l, Cin, Cout,
                     pitch_for(Cout), total);
  return ts::launched("decoder_weight_layout_kernel");
}

extern "C" int ts_decoder_conv_fwd(const float* up, const float* skip, const float* w_l, const float* scale, const float* shift, float* y,
                                   int B, int Cu, int Cs, int Cout, int h, int w, int H, int W, int act, long long up_bstride,
                                   long long up_cstride, long long skip_bstride, long long skip_cstride, long long y_bstride,
                                   long long y_cstride, void* stream) {
  TS_REQUIRE(B > 0 && Cu >= 0 && Cs > 0 && Cout > 0 && H > 0 && W > 0 && (Cu == 0 || (h > 0 && w > 0)), TS_ERR_SHAPE,
             "decoder_conv_fwd: non-positive size");
  TS_REQUIRE(act == ACT_NONE || act == ACT_SILU, TS_ERR_SHAPE, "decoder_conv_fwd: unknown activation %d", act);
  const long long HW = static_cast<long long>(H) * W;
  TS_REQUIRE(strides_ok(B, Cu, static_cast<long long>(h) * w, up_bstride, up_cstride), TS_ERR_SHAPE,
             "decoder_conv_fwd: up strides %lld / %lld overlap", up_bstride, up_cstride);
  TS_REQUIRE(strides_ok(B, Cs, HW, skip_bstride, skip_cstride), TS_ERR_SHAPE, "decoder_conv_fwd: skip strides %lld / %lld overlap",
             skip_bstride, skip_cstride);
  TS_REQUIRE(strides_ok(B, Cout, HW, y_bstride, y_cstride), TS_ERR_SHAPE, "decoder_conv_fwd: y strides %lld / %lld overlap", y_bstride,
             y_cstride);
  TS_REQUIRE(Cu + Cs <= kMaxC && Cout <= kMaxC, TS_ERR_UNSUPPORTED, "decoder_conv_fwd: Cu + Cs = %d / Cout = %d above %d", Cu + Cs, Cout, kMaxC);
  TS_REQUIRE(B < kMaxAxis && H < kMaxAxis && W < kMaxAxis && h < kMaxAxis && w < kMaxAxis, TS_ERR_UNSUPPORTED,
             "decoder_conv_fwd: an axis of 2^20 or more");
  Dec p;
  p.tiles_x = (W + kTW - 1) / kTW; p.tiles_y = (H + kTR - 1) / kTR;
  // MT blocks of 16 output rows per workgroup, `groups` workgroups along the rows.  A grid of fewer than two workgroups per compute
  // unit is cut finer along the rows: a lone workgroup has nothing to hide its staging behind (measured at 1, 2 and 4 per compute unit:
  // batch 2 of the 544 x 960 decoder 1385 / 1218 / 1187 us, batch 8 3194 / 3175 / 3239 us).  An output's chains do not depend on MT.
  int mt = mt_for(Cout);
  const unsigned long long tiles = static_cast<unsigned long long>(p.tiles_x) * p.tiles_y * B;
  auto groups = [&](int m) { return (Cout + 16 * m - 1) / (16 * m); };
  while (mt > 1 && tiles * groups(mt) < 2ull * ts::kNumCU) mt /= 2;
  p.groups = groups(mt);
  const unsigned long long nblocks = tiles * p.groups;
  TS_REQUIRE(nblocks < 0x7fffffffull, TS_ERR_UNSUPPORTED, "decoder_conv_fwd: grid too large");
  if (Cu > 0) TS_REQUIRE_PTR(up);
  TS_REQUIRE_PTR(skip);
  TS_REQUIRE_PTR(w_l); TS_REQUIRE_PTR(y);
  TS_REQUIRE_ALIGNED(w_l);
  p.up = up; p.skip = skip; p.w = w_l; p.scale = scale; p.shift = shift; p.y = y;
  p.Cu = Cu; p.Cs = Cs; p.Cout = Cout; p.h = Cu ? h : 1; p.w_in = Cu ? w : 1; p.H = H; p.W = W; p.act = act;
  p.rp = pitch_for(Cout);
  p.sh = ts::ac_scale(p.h, H); p.sw = ts::ac_scale(p.w_in, W);
  p.up_bs = up_bstride; p.up_cs = up_cstride; p.skip_bs = skip_bstride; p.skip_cs = skip_cstride; p.y_bs = y_bstride; p.y_cs = y_cstride;
  const dim3 grid(static_cast<unsigned>(nblocks));
  hipStream_t st = ts::as_stream(stream);
  switch (mt) {
    case 1: hipLaunchKernelGGL((decoder_conv_kernel<1>), grid, dim3(256), 0, st, p); break;
    case 2: hipLaunchKernelGGL((decoder_conv_kernel<2>), grid, dim3(256), 0, st, p); break;
    case 4: hipLaunchKernelGGL((decoder_conv_kernel<4>), grid, dim3(256), 0, st, p); break;
    default: hipLaunchKernelGGL((decoder_conv_kernel<8>), grid, dim3(256), 0, st, p); break;
  }
  return ts::launched("decoder_conv_kernel");
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
  hipLaunchKernelGGL(resize_bilinear_bwd_kernel, dim3(blocks_for(static_cast<long long>(B) * C * h * w)), dim3(256), 0,
                     ts::as_stream(stream), dy, dx, B, C, h, w, H, W, ts::ac_scale(h, H), ts::ac_scale(w, W), dy_bstride, dy_cstride,
                     dx_bstride, dx_cstride);
  return ts::launched("resize_bilinear_bwd_kernel");
}
