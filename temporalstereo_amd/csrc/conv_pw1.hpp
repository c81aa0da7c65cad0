// The pointwise (1x1) fp32-MFMA convolution core of mbconv.hip (expand_kernel, project_kernel): per batch element the GEMM
// [rows x Cin] . [Cin x H W] on v_mfma_f32_16x16x4_f32 -- bitwise an fmaf chain -- built as conv_hw3.hpp is: the input channels a caller
// reads from wherever they lie (two strided tensors with a seam; one tensor times a per-channel gate) and the sums a caller finishes
// (scale / shift / SiLU; scale / shift / residual).  Everything between the two is here, with no branch on which caller it serves.
//
// Geometry.  A plane is dense, so a pixel is its flat index p in [0, H W).  A workgroup (4 waves) owns kTP = 64 consecutive pixels and
// MT blocks of 16 output rows; output rows beyond 16 MT are tiled over the grid as `groups` workgroups per pixel tile, neighbours in the
// grid, so the second and later read the input tile from L2.  A wave owns 16 pixels and holds MT accumulators.  K runs over chunks of
// kCK = 32 input channels; a k-step of 4 takes channel 4 q + kq of the chunk from the lane's kq.  The seam of a caller's sources may fall
// anywhere in a chunk: the reader is called per staged value.  Channel and pixel are clamped HERE and zero is what staging writes for a
// value past either end: a reader is only ever called with gc < Cin, 0 <= p < H W.
// Weights are pre-laid by pw1::weight_layout as [Cin rounded up to 32][pitch] -- the transpose, zero rows / channels included -- so a
// chunk's weights are 32 row segments of 64 MT bytes; `pitch` (Geom::rp) holds whole workgroups of any MT.
// LDS: sW [32][w_pitch(MT)] and sX [32][kXP]; the pitches are == 16 mod 32 (corr_common.hpp: the two kq of a lane half land on disjoint
// banks).  Staging is split -- a chunk's loads are issued up to four chunks ahead of its MFMAs (conv_tile) -- where hw3 keeps the plain
// form: there the resident workgroups hide one another's loads, here the grids are too small for that.
//
// Summation.  The accumulators are added into a second set every FLUSH chunks and the sum is tot + acc: a chain of 32 FLUSH products,
// then a chain of blocks (K reaches 1632 in the encoder: with FLUSH = 8, chains of 256, then at most 7 blocks).  An output's chains run
// over the input channels in order whatever MT, `groups` and the batch are: the bits do not depend on the launch geometry.
//
// A problem type P has
//   pw1::Geom g;
//   source(b)     -> a reader (gc, p) -> float of batch element b;
//   sink(b, p)    -> a writer (row, sum) of output pixel p of batch element b, called for row < g.rows only.
#pragma once
#include "conv_hw3.hpp"

namespace pw1 {

using corr::v4f;
using hw3::w_pitch;
using node::pitch_for;

constexpr int kCK = 32;                      // input channels per staged chunk
constexpr int kTP = 64;                      // pixels per workgroup
constexpr int kXP = kTP + 16;                // 80 == 16 mod 32

inline int chunks_for(int Cin) { return (Cin + kCK - 1) / kCK; }
inline size_t image_floats(int Cin, int rows) { return static_cast<size_t>(chunks_for(Cin)) * kCK * pitch_for(rows); }

struct Geom {
  const float* w;           // [chunks * 32][rp]
  int Cin, rows;            // input channels, output rows
  long long N;              // pixels of a plane
  int tiles;                // pixel tiles of a plane
  int rp, groups;           // pitch of a weight row in global memory; workgroups along the output rows
};

inline Geom geom(const float* w, int Cin, int rows, long long N) {
  return Geom{w, Cin, rows, N, static_cast<int>((N + kTP - 1) / kTP), pitch_for(rows), 0};
}

template <int MT, int FLUSH, class P>
__device__ __forceinline__ void conv_tile(const P& p) {
  static_assert(FLUSH > 0, "the pointwise core sums in blocks");
  constexpr int PW = w_pitch(MT);
  __shared__ __attribute__((aligned(16))) float sW[kCK * PW];
  __shared__ float sX[kCK * kXP];
  const Geom& g = p.g;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 15, kq = lane >> 4;
  unsigned blk = blockIdx.x;
  const int rg = blk % g.groups; blk /= g.groups;               // neighbours share the input tile
  const int tile = blk % g.tiles;
  const int b = blk / g.tiles;
  const long long p0 = static_cast<long long>(tile) * kTP;
  const auto src = p.source(b);
  const float* pw = g.w + rg * (16 * MT);

  v4f acc[MT], tot[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t] = tot[t] = v4f{0.f, 0.f, 0.f, 0.f};

  // Staging in two halves (issue early, write late), D chunks deep: the global loads of chunk ch + D go to registers while chunks
  // ch .. ch + D - 1 are staged and multiplied, and are written to LDS behind the barrier that ends the chunk before them.  The encoder's
  // grids are small and its K long (a 17 x 30 project is 272 workgroups of 51 chunks at MT = 1, eight MFMAs per wave and chunk), so a
  // workgroup has neither neighbours on its compute unit nor arithmetic of its own to hide a load behind.  D = 4 where the registers
  // are there (MT <= 2), 2 at MT = 4, 1 at MT = 8.  The arithmetic and its order are the plain form's.
  constexpr int D = MT <= 2 ? 4 : MT == 4 ? 2 : 1;
  constexpr int XN = kCK * kTP / 256;                            // staged input values per thread and chunk
  constexpr int WN = (kCK * 4 * MT + 255) / 256;                 // staged 16-byte weight pieces per thread and chunk
  float xr[D][XN];
  v4f wr[D][WN];                                                 // (the ext-vector type: an array of HIP's float4 went to scratch)
  const int px = tid & (kTP - 1), c0 = tid / kTP;                // a wave per channel row of the input tile
  const long long gp_in = p0 + px;
  auto fetch = [&](int ch, float (&x)[XN], v4f (&w)[WN]) {
#pragma unroll
    for (int n = 0; n < XN; ++n) {                               // every load unconditional, so the loads in flight can be counted: a
      const int gc = ch * kCK + c0 + n * (256 / kTP);            // channel or pixel past the end reads the last one and is dropped
      const float v = src(min(gc, g.Cin - 1), min(gp_in, g.N - 1));
      x[n] = (gc < g.Cin && gp_in < g.N) ? v : 0.f;
    }
#pragma unroll
    for (int n = 0; n < WN; ++n) {
      const int i = min(tid + n * 256, kCK * 4 * MT - 1);        // this workgroup's columns of the chunk's 32 weight rows, 16 bytes a piece
      const int row = i / (4 * MT), seg = i % (4 * MT);          // (MT = 1: the upper half of the threads reads the last piece again, and drops it)
      w[n] = *reinterpret_cast<const v4f*>(pw + (static_cast<size_t>(ch) * kCK + row) * g.rp + seg * 4);
    }
  };

  const int nchunks = (g.Cin + kCK - 1) / kCK;
#pragma unroll
  for (int d = 0; d < D; ++d) fetch(min(d, nchunks - 1), xr[d], wr[d]);
  for (int ch0 = 0; ch0 < nchunks; ch0 += D) {
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const int ch = ch0 + d;
      if (ch >= nchunks) break;
      if (ch != 0 && ch % FLUSH == 0) {                          // blocked summation: a chain of FLUSH x 32 products, then a chain of blocks
#pragma unroll
        for (int t = 0; t < MT; ++t) {
          tot[t] += acc[t];
          acc[t] = v4f{0.f, 0.f, 0.f, 0.f};
        }
      }
      __syncthreads();                                           // the previous chunk has been read
#pragma unroll
      for (int n = 0; n < XN; ++n) sX[(c0 + n * (256 / kTP)) * kXP + px] = xr[d][n];
#pragma unroll
      for (int n = 0; n < WN; ++n) {
        const int i = tid + n * 256;
        if (i < kCK * 4 * MT) *reinterpret_cast<v4f*>(sW + (i / (4 * MT)) * PW + (i % (4 * MT)) * 4) = wr[d][n];
      }
      __syncthreads();
      fetch(min(ch + D, nchunks - 1), xr[d], wr[d]);             // in flight under the next D chunks (past the end: the last chunk again, dropped)
      const float* xcol = sX + wave * 16 + j;
#pragma unroll
      for (int q = 0; q < kCK / 4; ++q) {
        const int k = 4 * q + kq;
        const float bv = xcol[k * kXP];
        const float* wrow = sW + k * PW + j;
#pragma unroll
        for (int t = 0; t < MT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wrow[16 * t], bv, acc[t], 0, 0, 0);
      }
    }
  }

  // epilogue: the lane holds rows 16 (MT rg + t) + 4 kq + r of pixel p0 + 16 wave + j
  const long long gp = p0 + wave * 16 + j;
  if (gp >= g.N) return;
  const auto out = p.sink(b, gp);
#pragma unroll
  for (int t = 0; t < MT; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * (MT * rg + t) + 4 * kq + r;
      if (row < g.rows) out(row, tot[t][r] + acc[t][r]);
    }
  }
}

namespace {
// w [rows][Cin] (the framework's 1x1 weight, contiguous) -> [Cin rounded up to 32][pitch], zeros past the weight's own rows / channels
__global__ void __launch_bounds__(256) weight_layout_kernel(const float* __restrict__ w, float* __restrict__ out, int Cin, int rows,
                                                            int pitch, int total) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const int col = i % pitch, ci = i / pitch;
    out[i] = (ci < Cin && col < rows) ? w[static_cast<size_t>(col) * Cin + ci] : 0.f;
  }
}

int weight_layout(const float* w, float* out, int Cin, int rows, int cap, hipStream_t st, const char* what) {
  const size_t total = image_floats(Cin, rows);                  // at most 2048 x 2048
  hipLaunchKernelGGL(weight_layout_kernel, dim3(ts::blocks_for(static_cast<long long>(total), cap)), dim3(256), 0, st, w, out, Cin, rows,
                     pitch_for(rows), static_cast<int>(total));
  return ts::launched(what);
}
}  // namespace

// The launch rule, hw3's: MT blocks of 16 output rows per workgroup, halved while the grid holds fewer than min_blocks workgroups.
// Sets g.groups; returns MT and the blocks of the 1-D grid (0: they do not fit one).
inline hw3::Launch launch_rule(Geom& g, int B, unsigned long long min_blocks) {
  int mt = hw3::mt_for(g.rows);
  const unsigned long long tiles = static_cast<unsigned long long>(g.tiles) * B;
  auto groups = [&](int m) { return (g.rows + 16 * m - 1) / (16 * m); };
  while (mt > 1 && tiles * groups(mt) < min_blocks) mt /= 2;
  g.groups = groups(mt);
  return hw3::Launch{mt, corr::grid_blocks(tiles * g.groups)};
}

// The pointwise projection: channel gc of `x` in place through its strides -- GATED: times gate[b, gc] ([B][Cin]) while it is staged,
// so a gated map is never written -- finished by the affine epilogue.
template <bool GATED>
struct Project {
  Geom g;
  node::Plane<const float> x;
  const float* gate;
  node::Affine<ACT_NONE, GATED ? 1 : node::kRuntime> ep;      // no activation; the gated use always has a residual

  __device__ __forceinline__ auto source(int b) const {
    return [px = x.at(b, 0), pg = GATED ? gate + static_cast<long long>(b) * g.Cin : nullptr, x_cs = x.cs](int gc, long long p) {
      (void)pg;
      if constexpr (GATED) return px[gc * x_cs + p] * pg[gc];
      else return px[gc * x_cs + p];
    };
  }
  __device__ __forceinline__ auto sink(int b, long long p) const { return ep.writer(b, p); }
};

// a plane's pixels are one 32-bit count here
inline int check_plane(const char* who, long long N) {
  TS_REQUIRE(N <= 0x7fffffffll, TS_ERR_UNSUPPORTED, "%s: a plane of 2^31 pixels or more", who);
  return TS_OK;
}

}  // namespace pw1
