// ConvGRU (reference: architecture/modeling/layers/conv_gru.py:4-28): the gated recurrent cell as two launches, fp32 throughout.
//
//   z = sigmoid(convz([h, x]))   r = sigmoid(convr([h, x]))   q = tanh(convq([r*h, x]))   hidden = (1 - z) * h + z * q
//
// gru_conv_kernel<MT, GATES> is conv_hw3.hpp's 3x3 convolution (geometry, staging and pitches: there) with ONE fmaf chain per output
// -- a recurrence keeps fp32 rounding -- whose input channels come from TWO tensors read in place: channels [0, Ch) from `a` (h, or
// r*h), channels [Ch, Ch + Cx) from x, each with its own batch / channel strides.  No concatenation is written.
//   GATES:  2 Ch output rows (z rows, then r rows); epilogue bias + sigmoid; stores z, r*h and (training only) r.
//   !GATES: Ch output rows; epilogue bias + tanh, reads z and h at the output pixel, stores hidden and (training only) q.
// The weights of both convolutions are laid out by one launch: the gate image ([wz rows | wr rows]) and, behind it, the candidate's,
// each with its rows padded to 64.
//
// Backward: the convolutions' gradients run on ts_conv3d_hw_bwd_data / ts_conv3d_hw_bwd_weight (D = 1); the three element kernels
// here carry the gates' derivatives and the sums into dh / dx.  No atomics anywhere: bit-reproducible.
#include "conv_hw3.hpp"

namespace {

constexpr int kMaxC = 64;
constexpr int kElemGridCap = 2048;           // blocks of the grid-stride element kernels of the backward pass
using node::pitch_for;                       // (the gates' 2 Ch <= 128 rows: 64 or 128)
using ts::strides_ok;

template <bool GATES>
struct Gru {
  hw3::Geom g;              // rows: 2 Ch (gates) or Ch (candidate)
  const float* a;           // source of channels [0, Ch): h (gates) or r*h (candidate)
  const float* x;           // source of channels [Ch, Ch + Cx)
  const float* b0;          // bias of rows [0, Ch)
  const float* b1;          // bias of rows [Ch, 2 Ch) (gates)
  const float* h;           // the hidden state the epilogue reads
  const float* zin;         // candidate: z
  float* o0;                // gates: z          candidate: hidden
  float* o1;                // gates: r * h      candidate: q or NULL
  float* o2;                // gates: r or NULL
  int Ch;
  long long a_bs, a_cs, x_bs, x_cs, h_bs, h_cs;

  // the lambdas hold copies of what they use, never `this`: a store through o0 / o1 / o2 then cannot be taken to change a field
  __device__ __forceinline__ auto source(int b) const {
    return [pa = a + b * a_bs, px = x + b * x_bs, Ch = Ch, a_cs = a_cs, x_cs = x_cs, W = g.W](int gc, int gy, int gx) {
      const long long pix = hw3::pixel_at(gy, gx, W);
      return gc < Ch ? pa[gc * a_cs + pix] : px[(gc - Ch) * x_cs + pix];          // the seam may fall anywhere in a chunk
    };
  }
  __device__ __forceinline__ auto sink(int b, int gy, int gx) const {
    const long long HW = static_cast<long long>(g.H) * g.W, pix = hw3::pixel_at(gy, gx, g.W);
    return [HW, ph = h + b * h_bs + pix, ob = static_cast<long long>(b) * Ch * HW + pix, h_cs = h_cs, Ch = Ch, b0 = b0, b1 = b1, zin = zin,
            o0 = o0, o1 = o1, o2 = o2](int row, float sum) {
      if (GATES) {
        if (row < Ch) {
          o0[ob + row * HW] = sigmoid_fast(sum + b0[row]);
        } else {
          const int c = row - Ch;
          const float gate = sigmoid_fast(sum + b1[c]);
          if (o2) o2[ob + c * HW] = gate;
          o1[ob + c * HW] = gate * ph[c * h_cs];
        }
      } else {
        const long long at = ob + row * HW;
        const float q = tanh_fast(sum + b0[row]);
        const float z = zin[at], hv = ph[row * h_cs];
        if (o1) o1[at] = q;
        o0[at] = (1.f - z) * hv + z * q;
      }
    };
  }
};

template <int MT, bool GATES>
__global__ void __launch_bounds__(256) gru_conv_kernel(const Gru<GATES> p) { hw3::conv_tile<MT, 0>(p); }

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

// sizes (TS_ERR_SHAPE), then the envelope (TS_ERR_UNSUPPORTED)
int check_planes(const char* who, int B, int Ch, long long N) {
  TS_REQUIRE(B > 0 && Ch > 0 && N > 0, TS_ERR_SHAPE, "%s: non-positive size", who);
  TS_REQUIRE(Ch <= kMaxC, TS_ERR_UNSUPPORTED, "%s: Ch=%d above %d", who, Ch, kMaxC);
  TS_REQUIRE(B < node::kMaxAxis && N < (1ll << 40), TS_ERR_UNSUPPORTED, "%s: an axis of 2^20 or more", who);
  return TS_OK;
}

size_t gates_floats(int Ch, int Cx) { return hw3::image_floats(Ch + Cx, pitch_for(2 * Ch)); }
size_t cand_floats(int Ch, int Cx) { return hw3::image_floats(Ch + Cx, pitch_for(Ch)); }

// One convolution of the cell, p filled but for its geometry: h and x are the strided operands (the outputs are dense and the cell's own),
// `dense` the other required pointers.  The grid is cut along the rows until every compute unit has a workgroup (hw3::launch_rule).
template <bool GATES>
int launch_conv(const char* who, const char* kernel, Gru<GATES>& p, const float* w_l, std::initializer_list<node::Pointer> dense, int B, int Cx,
                int H, int W, hipStream_t st) {
  const int Ch = p.Ch;
  TS_REQUIRE(B > 0 && Ch > 0 && Cx > 0 && H > 0 && W > 0, TS_ERR_SHAPE, "%s: non-positive size", who);
  const long long HW = static_cast<long long>(H) * W;
  auto envelope = [&] {
    TS_REQUIRE(Ch <= kMaxC && Cx <= kMaxC, TS_ERR_UNSUPPORTED, "%s: Ch=%d / Cx=%d above %d", who, Ch, Cx, kMaxC);
    return TS_OK;
  };
  return node::launch(
      who, kernel, B, {{"h", p.h, Ch, HW, p.h_bs, p.h_cs, node::IN}, {"x", p.x, Cx, HW, p.x_bs, p.x_cs, node::IN}}, dense, w_l, {B, H, W}, envelope,
      [&] {          // behind the envelope and the axes; the candidate's image lies behind the gates'
        const int rows = GATES ? 2 * Ch : Ch;
        p.g = hw3::geom(GATES ? w_l : w_l + gates_floats(Ch, Cx), Ch + Cx, rows, H, W, pitch_for(rows));
        return hw3::launch_rule(p.g, B, ts::kNumCU);
      },
      [&](auto MT, dim3 grid) {
        if constexpr (GATES || MT() < 8)          // 65 .. 128 rows: the gates alone
          hipLaunchKernelGGL((gru_conv_kernel<MT(), GATES>), grid, dim3(256), 0, st, p);
      });
}

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
  hw3::WeightImages im;          // [wz | wr] at the gates' pitch, then wq at the candidate's: one launch
  im.wa = wz; im.ra = Ch; im.wb = wr; im.rb = Ch; im.p0 = pitch_for(2 * Ch);
  im.wc = wq; im.rc = Ch; im.p1 = pitch_for(Ch);
  return hw3::weight_layout(im, w_l, Ch + Cx, node::kGridCap, ts::as_stream(stream), "gru_weight_layout_kernel");
}

extern "C" int ts_conv_gru_gates_fwd(const float* h, const float* x, const float* w_l, const float* bz, const float* br, float* z,
                                     float* rh, float* r, int B, int Ch, int Cx, int H, int W, long long h_bstride, long long h_cstride,
                                     long long x_bstride, long long x_cstride, void* stream) {
  Gru<true> p;
  p.a = h; p.x = x; p.b0 = bz; p.b1 = br; p.h = h; p.zin = nullptr; p.o0 = z; p.o1 = rh; p.o2 = r; p.Ch = Ch;
  p.a_bs = h_bstride; p.a_cs = h_cstride; p.x_bs = x_bstride; p.x_cs = x_cstride; p.h_bs = h_bstride; p.h_cs = h_cstride;
  return launch_conv("conv_gru_gates_fwd", "gru_conv_kernel<gates>", p, w_l, {{"bz", bz}, {"br", br}, {"z", z}, {"rh", rh}}, B, Cx, H, W,
                     ts::as_stream(stream));
}

extern "C" int ts_conv_gru_out_fwd(const float* rh, const float* x, const float* w_l, const float* bq, const float* z, const float* h,
                                   float* out, float* q, int B, int Ch, int Cx, int H, int W, long long h_bstride, long long h_cstride,
                                   long long x_bstride, long long x_cstride, void* stream) {
  const long long HW = static_cast<long long>(H) * W;
  Gru<false> p;
  p.a = rh; p.x = x; p.b0 = bq; p.b1 = nullptr; p.h = h; p.zin = z; p.o0 = out; p.o1 = q; p.o2 = nullptr; p.Ch = Ch;
  p.a_bs = Ch * HW; p.a_cs = HW; p.x_bs = x_bstride; p.x_cs = x_cstride; p.h_bs = h_bstride; p.h_cs = h_cstride;
  return launch_conv("conv_gru_out_fwd", "gru_conv_kernel<out>", p, w_l, {{"rh", rh}, {"bq", bq}, {"z", z}, {"out", out}}, B, Cx, H, W,
                     ts::as_stream(stream));
}

extern "C" int ts_conv_gru_gate_bwd_a(const float* dout, const float* z, const float* q, const float* h, float* dq_pre, float* dz_pre,
                                      float* dh, int B, int Ch, long long N, long long h_bstride, long long h_cstride,
                                      long long dz_bstride, long long dz_cstride, void* stream) {
  if (int rc = check_planes("conv_gru_gate_bwd_a", B, Ch, N)) return rc;
  TS_REQUIRE(strides_ok(B, Ch, N, h_bstride, h_cstride), TS_ERR_SHAPE, "conv_gru_gate_bwd_a: h strides %lld / %lld overlap", h_bstride, h_cstride);
  TS_REQUIRE(strides_ok(B, Ch, N, dz_bstride, dz_cstride), TS_ERR_SHAPE, "conv_gru_gate_bwd_a: dz_pre strides %lld / %lld overlap", dz_bstride, dz_cstride);
  TS_REQUIRE_PTR(dout); TS_REQUIRE_PTR(z); TS_REQUIRE_PTR(q); TS_REQUIRE_PTR(h); TS_REQUIRE_PTR(dq_pre); TS_REQUIRE_PTR(dz_pre); TS_REQUIRE_PTR(dh);
  hipLaunchKernelGGL(gru_gate_bwd_a_kernel, dim3(ts::blocks_for(static_cast<long long>(B) * Ch * N, kElemGridCap)), dim3(256), 0, ts::as_stream(stream), dout, z,
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
  hipLaunchKernelGGL(gru_gate_bwd_b_kernel, dim3(ts::blocks_for(static_cast<long long>(B) * Ch * N, kElemGridCap)), dim3(256), 0, ts::as_stream(stream), d_rh, r,
                     h, dr_pre, dh, B, Ch, N, drh_bstride, drh_cstride, h_bstride, h_cstride, dr_bstride, dr_cstride);
  return ts::launched("gru_gate_bwd_b_kernel");
}

extern "C" int ts_conv_gru_grad_sum(const float* dcat_g, const float* dcat_q, float* dh, float* dx, int B, int Ch, int Cx, long long N,
                                    void* stream) {
  if (int rc = check_planes("conv_gru_grad_sum", B, Ch, N)) return rc;
  TS_REQUIRE(Cx > 0, TS_ERR_SHAPE, "conv_gru_grad_sum: non-positive size");
  TS_REQUIRE(Cx <= kMaxC, TS_ERR_UNSUPPORTED, "conv_gru_grad_sum: Cx=%d above %d", Cx, kMaxC);
  TS_REQUIRE_PTR(dcat_g); TS_REQUIRE_PTR(dcat_q); TS_REQUIRE_PTR(dh);
  hipLaunchKernelGGL(gru_grad_sum_kernel, dim3(ts::blocks_for(static_cast<long long>(B) * (Ch + Cx) * N, kElemGridCap)), dim3(256), 0, ts::as_stream(stream),
                     dcat_g, dcat_q, dh, dx, B, Ch, Cx, N);
  return ts::launched("gru_grad_sum_kernel");
}
