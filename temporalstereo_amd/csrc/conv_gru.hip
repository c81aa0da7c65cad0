// ConvGRU (reference: architecture/modeling/layers/conv_gru.py:4-28): the gated recurrent cell as two launches, fp32 throughout.
//
//   z = sigmoid(convz([h, x]))   r = sigmoid(convr([h, x]))   q = tanh(convq([r*h, x]))   hidden = (1 - z) * h + z * q
//
// gru_conv_kernel<MT, GATES> is one implicit-GEMM 3x3 convolution (padding 1) on v_mfma_f32_16x16x4_f32 -- bitwise an fmaf chain, so a
// recurrence keeps fp32 rounding -- whose input channels come from TWO tensors read in place: channels [0, Ch) from `a` (h, or r*h),
// channels [Ch, Ch + Cx) from x, each with its own batch / channel strides.  No concatenation is written.
//   GATES:  2 Ch output rows (z rows, then r rows); epilogue bias + sigmoid; stores z, r*h and (training only) r.
//   !GATES: Ch output rows; epilogue bias + tanh, reads z and h at the output pixel, stores hidden and (training only) q.
// A workgroup (4 waves) owns a 2 x 32 pixel tile and MT blocks of 16 output rows: every row where the grid fills the chip, fewer rows
// per workgroup and more workgroups along the rows where it would not (launch_conv).  A wave owns 16 pixels of one tile row and holds
// MT accumulators.  K runs over chunks of 8 input channels x 9 taps; inside a chunk k = tap * 8 + channel, so a k-step of 4 has a
// compile-time tap and the lane's kq picks the channel: the B operand is read straight from the staged halo tile (4 x 34 per channel),
// no im2col image.  The source seam may fall anywhere in a chunk: the source is chosen per staged channel.  Every global read is
// predicated on row, column and channel; the zero padding is what staging writes for the others.  An output's fmaf chain runs over
// the input channels in order whatever MT is, so the bits do not depend on the launch geometry.
// Staging is the plain form -- load, store, barrier, MFMAs -- and the workgroups resident on a compute unit (3 to 8) hide one another's
// loads.  Two forms that keep a chunk in registers (loads issued together before the barrier; the next chunk loaded under the current
// chunk's MFMAs) were measured and were 4-25 % slower at every benched shape: 90-117 VGPRs instead of 48-51, fewer resident waves.
// Weights are pre-laid by gru_weight_layout_kernel as [chunk][tap][8][rows padded to 64] per convolution (zero rows / channels
// included), so a chunk's weights are 72 row segments of 64 MT bytes.  LDS pitches follow corr_common.hpp: a [k][columns] image wants
// pitch == 16 mod 32.
//
// Backward: the convolutions' gradients run on ts_conv3d_hw_bwd_data / ts_conv3d_hw_bwd_weight (D = 1); the three element kernels
// here carry the gates' derivatives and the sums into dh / dx.  No atomics anywhere: bit-reproducible.
#include "corr_common.hpp"

namespace {

using corr::v4f;

constexpr int kCK = 8;                       // input channels per staged chunk
constexpr int kKC = kCK * 9;                 // contraction elements per chunk
constexpr int kTR = 2, kTW = 32;             // pixel tile
constexpr int kRowP = 36;                    // halo row pitch (34 columns staged)
constexpr int kChP = (kTR + 2) * kRowP;      // 144 == 16 mod 32: the two kq of a lane half land on disjoint banks
constexpr int kMaxC = 64;

constexpr int w_pitch(int mt) { return (mt * 16) % 32 == 16 ? mt * 16 : mt * 16 + 16; }
inline int mt_for(int rows) { return rows <= 16 ? 1 : rows <= 32 ? 2 : rows <= 64 ? 4 : 8; }      // 16-row blocks a workgroup holds, before the grid is looked at
inline int pitch_for(int rows) { return (rows + 63) / 64 * 64; }                  // global pitch of a weight row: whole workgroups of any MT
inline int chunks_for(int Ch, int Cx) { return (Ch + Cx + kCK - 1) / kCK; }

__device__ __forceinline__ float rcp_newton(float d) {
  const float r = __builtin_amdgcn_rcpf(d);
  return fmaf(fmaf(-d, r, 1.f), r, r);
}
// 1 / (1 + e^-v) on v_exp_f32 + v_rcp_f32 + one Newton step (conv_common.hpp silu_fast).  Whole float range: below v = -88.7 e^-v is inf,
// the reciprocal 0 and the Newton step inf * 0 -- the unrefined 0 is kept there.  d >= 1 and the refined quotient is one rounding of
// r (2 - d r) <= 1 / d, so the result lies in [0, 1].  NaN stays NaN.
__device__ __forceinline__ float sigmoid_fast(float v) {
  const float d = 1.f + __builtin_amdgcn_exp2f(v * -1.4426950408889634f);
  const float r = __builtin_amdgcn_rcpf(d);
  const float rn = fmaf(fmaf(-d, r, 1.f), r, r);
  return d < 3.0e38f ? rn : r;
}
// tanh(v) = sign(v) (1 - e) / (1 + e), e = e^(-2|v|) in [0, 1]: the denominator stays in [1, 2] (no overflow anywhere; 2|v| = inf gives
// e = 0), both factors are <= 1, so |result| <= 1.
__device__ __forceinline__ float tanh_fast(float v) {
  const float e = __builtin_amdgcn_exp2f(fabsf(v) * -2.8853900817779268f);
  return copysignf((1.f - e) * rcp_newton(1.f + e), v);
}

struct Gru {
  const float* a;           // source of channels [0, Ch): h (gates) or r*h (candidate)
  const float* x;           // source of channels [Ch, Ch + Cx)
  const float* w;           // [chunks][9][8][rp]
  const float* b0;          // bias of rows [0, Ch)
  const float* b1;          // bias of rows [Ch, 2 Ch) (gates)
  const float* h;           // the hidden state the epilogue reads
  const float* zin;         // candidate: z
  float* o0;                // gates: z          candidate: hidden
  float* o1;                // gates: r * h      candidate: q or NULL
  float* o2;                // gates: r or NULL
  int Ch, Cx, H, W, tiles_x, tiles_y;
  int rp, groups;           // pitch of a weight row in global memory (rows padded to 64); workgroups along the output rows
  long long a_bs, a_cs, x_bs, x_cs, h_bs, h_cs;
};

template <int MT, bool GATES>
__global__ void __launch_bounds__(256) gru_conv_kernel(const Gru p) {
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
  const int Cin = p.Ch + p.Cx;
  const long long HW = static_cast<long long>(p.H) * p.W;
  const float* pa = p.a + b * p.a_bs;
  const float* px = p.x + b * p.x_bs;
  const float* pw = p.w + rg * (16 * MT);
  const int pr = wave >> 1, pc = (wave & 1) * 16 + j;

  v4f acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t] = v4f{0.f, 0.f, 0.f, 0.f};

  const int nchunks = (Cin + kCK - 1) / kCK;
  for (int ch = 0; ch < nchunks; ++ch) {
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
        const long long pix = static_cast<long long>(gy) * p.W + gx;
        v = gc < p.Ch ? pa[gc * p.a_cs + pix] : px[(gc - p.Ch) * p.x_cs + pix];
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
  const long long pix = static_cast<long long>(gy) * p.W + gx;
  const int rows = GATES ? 2 * p.Ch : p.Ch;
  const float* ph = p.h + b * p.h_bs + pix;
  const long long ob = static_cast<long long>(b) * p.Ch * HW + pix;
#pragma unroll
  for (int t = 0; t < MT; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * (MT * rg + t) + 4 * kq + r;
      if (row >= rows) continue;
      if (GATES) {
        if (row < p.Ch) {
          p.o0[ob + row * HW] = sigmoid_fast(acc[t][r] + p.b0[row]);
        } else {
          const int c = row - p.Ch;
          const float g = sigmoid_fast(acc[t][r] + p.b1[c]);
          if (p.o2) p.o2[ob + c * HW] = g;
          p.o1[ob + c * HW] = g * ph[c * p.h_cs];
        }
      } else {
        const float q = tanh_fast(acc[t][r] + p.b0[row]);
        const float z = p.zin[ob + row * HW], hv = ph[row * p.h_cs];
        if (p.o1) p.o1[ob + row * HW] = q;
        p.o0[ob + row * HW] = (1.f - z) * hv + z * q;
      }
    }
  }
}

// [chunk][tap][8][pitch] images of the gate weights ([wz rows | wr rows]) and, behind them, of the candidate weights;
// w* are the framework's [Ch][Ch + Cx][3][3].
__global__ void __launch_bounds__(256) gru_weight_layout_kernel(const float* __restrict__ wz, const float* __restrict__ wr,
                                                                const float* __restrict__ wq, float* __restrict__ out, int Ch, int Cin,
                                                                int pg, int pq, int nchunks) {
  const int ng = nchunks * kKC * pg, total = ng + nchunks * kKC * pq;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const bool gates = i < ng;
    const int e = gates ? i : i - ng, pitch = gates ? pg : pq;
    const int col = e % pitch, k = e / pitch;
    const int c = k % kCK, tap = (k / kCK) % 9, ci = (k / kKC) * kCK + c;
    float v = 0.f;
    if (ci < Cin) {
      const int at = ci * 9 + tap;
      if (gates) {
        if (col < Ch) v = wz[static_cast<size_t>(col) * Cin * 9 + at];
        else if (col < 2 * Ch) v = wr[static_cast<size_t>(col - Ch) * Cin * 9 + at];
      } else if (col < Ch) {
        v = wq[static_cast<size_t>(col) * Cin * 9 + at];
      }
    }
    out[i] = v;
  }
}

// element kernels of the backward pass: [B][Ch][N] planes, dense unless strides are given
struct Idx {
  int b, c;
  long long n;
};
__device__ __forceinline__ Idx split_index(long long i, int Ch, long long N) {
  const long long bc = i / N;
  return Idx{static_cast<int>(bc / Ch), static_cast<int>(bc % Ch), i - bc * N};
}

// (a) through the blend and the tanh: dq_pre = dout z (1 - q^2), dz_pre = dout (q - h) z (1 - z), dh = dout (1 - z)
__global__ void __launch_bounds__(256) gru_gate_bwd_a_kernel(const float* __restrict__ dout, const float* __restrict__ z,
                                                             const float* __restrict__ q, const float* __restrict__ h,
                                                             float* __restrict__ dq_pre, float* __restrict__ dz_pre, float* __restrict__ dh,
                                                             int B, int Ch, long long N, long long h_bs, long long h_cs, long long dz_bs,
                                                             long long dz_cs) {
  const long long total = static_cast<long long>(B) * Ch * N;
  for (long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x; i < total; i += static_cast<long long>(gridDim.x) * 256) {
    const Idx ix = split_index(i, Ch, N);
    const float g = dout[i], zv = z[i], qv = q[i], hv = h[ix.b * h_bs + ix.c * h_cs + ix.n];
    dq_pre[i] = g * zv * (1.f - qv * qv);
    dz_pre[ix.b * dz_bs + ix.c * dz_cs + ix.n] = g * (qv - hv) * zv * (1.f - zv);
    dh[i] = g * (1.f - zv);
  }
}

// (b) through r * h and the reset gate's sigmoid: dr_pre = d_rh h r (1 - r), dh += d_rh r
__global__ void __launch_bounds__(256) gru_gate_bwd_b_kernel(const float* __restrict__ d_rh, const float* __restrict__ r,
                                                             const float* __restrict__ h, float* __restrict__ dr_pre, float* __restrict__ dh,
                                                             int B, int Ch, long long N, long long drh_bs, long long drh_cs,
                                                             long long h_bs, long long h_cs, long long dr_bs, long long dr_cs) {
  const long long total = static_cast<long long>(B) * Ch * N;
  for (long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x; i < total; i += static_cast<long long>(gridDim.x) * 256) {
    const Idx ix = split_index(i, Ch, N);
    const float g = d_rh[ix.b * drh_bs + ix.c * drh_cs + ix.n], rv = r[i], hv = h[ix.b * h_bs + ix.c * h_cs + ix.n];
    dr_pre[ix.b * dr_bs + ix.c * dr_cs + ix.n] = g * hv * rv * (1.f - rv);
    dh[i] += g * rv;
  }
}

// (c) the input gradients of the two convolutions, [B][Ch + Cx][N] each, into dh (+=, first Ch channels of the gates' one) and
// dx (= the x channels of both)
__global__ void __launch_bounds__(256) gru_grad_sum_kernel(const float* __restrict__ dcat_g, const float* __restrict__ dcat_q,
                                                           float* __restrict__ dh, float* __restrict__ dx, int B, int Ch, int Cx,
                                                           long long N) {
  const int C = Ch + Cx;
  const long long total = static_cast<long long>(B) * C * N;
  for (long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x; i < total; i += static_cast<long long>(gridDim.x) * 256) {
    const Idx ix = split_index(i, C, N);
    if (ix.c < Ch) dh[(static_cast<long long>(ix.b) * Ch + ix.c) * N + ix.n] += dcat_g[i];
    else if (dx) dx[(static_cast<long long>(ix.b) * Cx + ix.c - Ch) * N + ix.n] = dcat_g[i] + dcat_q[i];
  }
}

unsigned blocks_for(long long items) {
  long long n = (items + 255) / 256;
  if (n > 2048) n = 2048;
  return static_cast<unsigned>(n < 1 ? 1 : n);
}

bool strides_ok(int B, int C, long long vol, long long bs, long long cs) {
  return cs >= vol && (B == 1 || bs >= cs * (C - 1) + vol);
}

// sizes (TS_ERR_SHAPE), then the envelope (TS_ERR_UNSUPPORTED)
int check_cell(const char* who, int B, int Ch, int Cx, int H, int W) {
  TS_REQUIRE(B > 0 && Ch > 0 && Cx > 0 && H > 0 && W > 0, TS_ERR_SHAPE, "%s: non-positive size", who);
  TS_REQUIRE(Ch <= kMaxC && Cx <= kMaxC, TS_ERR_UNSUPPORTED, "%s: Ch=%d / Cx=%d above %d", who, Ch, Cx, kMaxC);
  TS_REQUIRE(B < (1 << 20) && H < (1 << 20) && W < (1 << 20), TS_ERR_UNSUPPORTED, "%s: an axis of 2^20 or more", who);
  const unsigned long long blocks = static_cast<unsigned long long>((W + kTW - 1) / kTW) * ((H + kTR - 1) / kTR) * B * 8;      // at most 8 row groups
  TS_REQUIRE(corr::grid_blocks(blocks) != 0, TS_ERR_UNSUPPORTED, "%s: grid too large", who);
  return TS_OK;
}
int check_planes(const char* who, int B, int Ch, long long N) {
  TS_REQUIRE(B > 0 && Ch > 0 && N > 0, TS_ERR_SHAPE, "%s: non-positive size", who);
  TS_REQUIRE(Ch <= kMaxC, TS_ERR_UNSUPPORTED, "%s: Ch=%d above %d", who, Ch, kMaxC);
  TS_REQUIRE(B < (1 << 20) && N < (1ll << 40), TS_ERR_UNSUPPORTED, "%s: an axis of 2^20 or more", who);
  return TS_OK;
}

// MT blocks of 16 output rows per workgroup, `groups` workgroups along the rows.  A grid that leaves compute units idle is cut finer
// along the rows (the input tile is then staged by more workgroups, from L2).  The fmaf chain of an output does not depend on MT.
template <bool GATES>
int launch_conv(Gru& p, int rows, int B, hipStream_t st, const char* what) {
  int mt = mt_for(rows);
  const unsigned long long tiles = static_cast<unsigned long long>(p.tiles_x) * p.tiles_y * B;
  auto groups = [&](int m) { return (rows + 16 * m - 1) / (16 * m); };
  while (mt > 1 && tiles * groups(mt) < static_cast<unsigned long long>(ts::kNumCU)) mt /= 2;
  p.groups = groups(mt);
  p.rp = pitch_for(rows);
  const unsigned blocks = corr::grid_blocks(tiles * p.groups);
  TS_REQUIRE(blocks != 0, TS_ERR_UNSUPPORTED, "%s: grid too large", what);
  const dim3 grid(blocks);
  switch (mt) {
    case 1: hipLaunchKernelGGL((gru_conv_kernel<1, GATES>), grid, dim3(256), 0, st, p); break;
    case 2: hipLaunchKernelGGL((gru_conv_kernel<2, GATES>), grid, dim3(256), 0, st, p); break;
    case 4: hipLaunchKernelGGL((gru_conv_kernel<4, GATES>), grid, dim3(256), 0, st, p); break;
    default:
      if constexpr (GATES) hipLaunchKernelGGL((gru_conv_kernel<8, true>), grid, dim3(256), 0, st, p);      // 65 .. 128 rows: the gates alone
      break;
  }
  return ts::launched(what);
}

size_t gates_floats(int Ch, int Cx) { return static_cast<size_t>(chunks_for(Ch, Cx)) * kKC * pitch_for(2 * Ch); }
size_t cand_floats(int Ch, int Cx) { return static_cast<size_t>(chunks_for(Ch, Cx)) * kKC * pitch_for(Ch); }

}  // namespace

extern "C" size_t ts_conv_gru_weight_bytes(int Ch, int Cx) {
  if (Ch <= 0 || Cx <= 0 || Ch > kMaxC || Cx > kMaxC) return 0;
  return (gates_floats(Ch, Cx) + cand_floats(Ch, Cx)) * sizeof(float);
}

extern "C" int ts_conv_gru_weight_layout(const float* wz, const float* wr, const float* wq, float* w_l, int Ch, int Cx, void* stream) {
  TS_REQUIRE(Ch > 0 && Cx > 0, TS_ERR_SHAPE, "conv_gru_weight_layout: non-positive size");
  TS_REQUIRE(Ch <= kMaxC && Cx <= kMaxC, TS_ERR_UNSUPPORTED, "conv_gru_weight_layout: Ch=%d / Cx=%d above %d", Ch, Cx, kMaxC);
  TS_REQUIRE_PTR(wz); TS_REQUIRE_PTR(wr); TS_REQUIRE_PTR(wq); TS_REQUIRE_PTR(w_l);
  TS_REQUIRE_ALIGNED(w_l);
  const long long total = static_cast<long long>(gates_floats(Ch, Cx) + cand_floats(Ch, Cx));
  hipLaunchKernelGGL(gru_weight_layout_kernel, dim3(blocks_for(total)), dim3(256), 0, ts::as_stream(stream), wz, wr, wq, w_l, Ch, Ch + Cx,
                     pitch_for(2 * Ch), pitch_for(Ch), chunks_for(Ch, Cx));
  return ts::launched("gru_weight_layout_kernel");
}

extern "C" int ts_conv_gru_gates_fwd(const float* h, const float* x, const float* w_l, const float* bz, const float* br, float* z,
                                     float* rh, float* r, int B, int Ch, int Cx, int H, int W, long long h_bstride, long long h_cstride,
                                     long long x_bstride, long long x_cstride, void* stream) {
  if (int rc = check_cell("conv_gru_gates_fwd", B, Ch, Cx, H, W)) return rc;
  const long long HW = static_cast<long long>(H) * W;
  TS_REQUIRE(strides_ok(B, Ch, HW, h_bstride, h_cstride), TS_ERR_SHAPE, "conv_gru_gates_fwd: h strides %lld / %lld overlap", h_bstride, h_cstride);
  TS_REQUIRE(strides_ok(B, Cx, HW, x_bstride, x_cstride), TS_ERR_SHAPE, "conv_gru_gates_fwd: x strides %lld / %lld overlap", x_bstride, x_cstride);
  TS_REQUIRE_PTR(h); TS_REQUIRE_PTR(x); TS_REQUIRE_PTR(w_l); TS_REQUIRE_PTR(bz); TS_REQUIRE_PTR(br); TS_REQUIRE_PTR(z); TS_REQUIRE_PTR(rh);
  TS_REQUIRE_ALIGNED(w_l);
  Gru p;
  p.a = h; p.x = x; p.w = w_l; p.b0 = bz; p.b1 = br; p.h = h; p.zin = nullptr; p.o0 = z; p.o1 = rh; p.o2 = r;
  p.Ch = Ch; p.Cx = Cx; p.H = H; p.W = W; p.tiles_x = (W + kTW - 1) / kTW; p.tiles_y = (H + kTR - 1) / kTR;
  p.a_bs = h_bstride; p.a_cs = h_cstride; p.x_bs = x_bstride; p.x_cs = x_cstride; p.h_bs = h_bstride; p.h_cs = h_cstride;
  return launch_conv<true>(p, 2 * Ch, B, ts::as_stream(stream), "gru_conv_kernel<gates>");
}

extern "C" int ts_conv_gru_out_fwd(const float* rh, const float* x, const float* w_l, const float* bq, const float* z, const float* h,
                                   float* out, float* q, int B, int Ch, int Cx, int H, int W, long long h_bstride, long long h_cstride,
                                   long long x_bstride, long long x_cstride, void* stream) {
  if (int rc = check_cell("conv_gru_out_fwd", B, Ch, Cx, H, W)) return rc;
  const long long HW = static_cast<long long>(H) * W;
  TS_REQUIRE(strides_ok(B, Ch, HW, h_bstride, h_cstride), TS_ERR_SHAPE, "conv_gru_out_fwd: h strides %lld / %lld overlap", h_bstride, h_cstride);
  TS_REQUIRE(strides_ok(B, Cx, HW, x_bstride, x_cstride), TS_ERR_SHAPE, "conv_gru_out_fwd: x strides %lld / %lld overlap", x_bstride, x_cstride);
  TS_REQUIRE_PTR(rh); TS_REQUIRE_PTR(x); TS_REQUIRE_PTR(w_l); TS_REQUIRE_PTR(bq); TS_REQUIRE_PTR(z); TS_REQUIRE_PTR(h); TS_REQUIRE_PTR(out);
  TS_REQUIRE_ALIGNED(w_l);
  Gru p;
  p.a = rh; p.x = x; p.w = w_l + gates_floats(Ch, Cx); p.b0 = bq; p.b1 = nullptr; p.h = h; p.zin = z; p.o0 = out; p.o1 = q; p.o2 = nullptr;
  p.Ch = Ch; p.Cx = Cx; p.H = H; p.W = W; p.tiles_x = (W + kTW - 1) / kTW; p.tiles_y = (H + kTR - 1) / kTR;
  p.a_bs = Ch * HW; p.a_cs = HW; p.x_bs = x_bstride; p.x_cs = x_cstride; p.h_bs = h_bstride; p.h_cs = h_cstride;
  return launch_conv<false>(p, Ch, B, ts::as_stream(stream), "gru_conv_kernel<out>");
}

extern "C" int ts_conv_gru_gate_bwd_a(const float* dout, const float* z, const float* q, const float* h, float* dq_pre, float* dz_pre,
                                      float* dh, int B, int Ch, long long N, long long h_bstride, long long h_cstride,
                                      long long dz_bstride, long long dz_cstride, void* stream) {
  if (int rc = check_planes("conv_gru_gate_bwd_a", B, Ch, N)) return rc;
  TS_REQUIRE(strides_ok(B, Ch, N, h_bstride, h_cstride), TS_ERR_SHAPE, "conv_gru_gate_bwd_a: h strides %lld / %lld overlap", h_bstride, h_cstride);
  TS_REQUIRE(strides_ok(B, Ch, N, dz_bstride, dz_cstride), TS_ERR_SHAPE, "conv_gru_gate_bwd_a: dz_pre strides %lld / %lld overlap", dz_bstride, dz_cstride);
  TS_REQUIRE_PTR(dout); TS_REQUIRE_PTR(z); TS_REQUIRE_PTR(q); TS_REQUIRE_PTR(h); TS_REQUIRE_PTR(dq_pre); TS_REQUIRE_PTR(dz_pre); TS_REQUIRE_PTR(dh);
  hipLaunchKernelGGL(gru_gate_bwd_a_kernel, dim3(blocks_for(static_cast<long long>(B) * Ch * N)), dim3(256), 0, ts::as_stream(stream), dout, z,
                     q, h, dq_pre, dz_pre, dh, B, Ch, N, h_bstride, h_cstride, dz_bstride, dz_cstride);
  return ts::launched("gru_gate_bwd_a_kernel");
}

extern "C" int ts_conv_gru_gate_bwd_b(const float* d_rh, const float* r, const float* h, float* dr_pre, float* dh, int B, int Ch,
                                      long long N, long long drh_bstride, long long drh_cstride, long long h_bstride, long long h_cstride,
                                      long long dr_bstride, long long dr_cstride, void* stream) {
  if (int rc = check_planes("conv_gru_gate_bwd_b", B, Ch, N)) return rc;
  TS_REQUIRE(strides_ok(B, Ch, N, drh_bstride, drh_cstride), TS_ERR_SHAPE, "conv_gru_gate_bwd_b: d_rh strides %lld / %lld overlap", drh_bstride, drh_cstride);
  TS_REQUIRE(strides_ok(B, Ch, N, h_bstride, h_cstride), TS_ERR_SHAPE, "conv_gru_gate_bwd_b: h strides %lld / %lld overlap", h_bstride, h_cstride);
  TS_REQUIRE(strides_ok(B, Ch, N, dr_bstride, dr_cstride), TS_ERR_SHAPE, "conv_gru_gate_bwd_b: dr_pre strides %lld / %lld overlap", dr_bstride, dr_cstride);
  TS_REQUIRE_PTR(d_rh); TS_REQUIRE_PTR(r); TS_REQUIRE_PTR(h); TS_REQUIRE_PTR(dr_pre); TS_REQUIRE_PTR(dh);
  hipLaunchKernelGGL(gru_gate_bwd_b_kernel, dim3(blocks_for(static_cast<long long>(B) * Ch * N)), dim3(256), 0, ts::as_stream(stream), d_rh, r,
                     h, dr_pre, dh, B, Ch, N, drh_bstride, drh_cstride, h_bstride, h_cstride, dr_bstride, dr_cstride);
  return ts::launched("gru_gate_bwd_b_kernel");
}

extern "C" int ts_conv_gru_grad_sum(const float* dcat_g, const float* dcat_q, float* dh, float* dx, int B, int Ch, int Cx, long long N,
                                    void* stream) {
  if (int rc = check_planes("conv_gru_grad_sum", B, Ch, N)) return rc;
  TS_REQUIRE(Cx > 0, TS_ERR_SHAPE, "conv_gru_grad_sum: non-positive size");
  TS_REQUIRE(Cx <= kMaxC, TS_ERR_UNSUPPORTED, "conv_gru_grad_sum: Cx=%d above %d", Cx, kMaxC);
  TS_REQUIRE_PTR(dcat_g); TS_REQUIRE_PTR(dcat_q); TS_REQUIRE_PTR(dh);
  hipLaunchKernelGGL(gru_grad_sum_kernel, dim3(blocks_for(static_cast<long long>(B) * (Ch + Cx) * N)), dim3(256), 0, ts::as_stream(stream),
                     dcat_g, dcat_q, dh, dx, B, Ch, Cx, N);
  return ts::launched("gru_grad_sum_kernel");
}
