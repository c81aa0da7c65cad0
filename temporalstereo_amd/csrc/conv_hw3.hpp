// The 3x3 fp32-MFMA convolution core of conv_gru.hip (gru_conv_kernel) and feature_decoder.hip (decoder_conv_kernel): one
// implicit-GEMM 3x3 convolution (stride 1, padding 1) on v_mfma_f32_16x16x4_f32 -- bitwise an fmaf chain -- whose input channels a
// caller reads from wherever they lie (two strided tensors; one tensor through a resize and one in place) and whose sums a caller
// finishes (gates, blend, scale / shift / activation).  Everything between the two is here, with no branch on which caller it serves.
//
// Geometry.  A workgroup (4 waves) owns a 2 x 32 pixel tile and MT blocks of 16 output rows; output rows beyond 16 MT are tiled over
// the grid as `groups` workgroups per pixel tile, neighbours in the grid, so the second and later read the input tile from L2.  A wave
// owns 16 pixels of one tile row and holds MT accumulators.  K runs over chunks of 8 input channels x 9 taps; inside a chunk
// k = tap * 8 + channel, so a k-step of 4 has a compile-time tap and the lane's kq picks the channel: the B operand is read straight
// from the staged halo tile (4 x 34 per channel), no im2col image.  A caller's source seam may fall anywhere in a chunk: the reader is
// called per staged value.  Every read is predicated HERE on channel, row and column, and the zero padding is what staging writes
// for the others: a reader is only ever called with gc < Cin, 0 <= gy < H, 0 <= gx < W.
// Weights are pre-laid by weight_layout_kernel as [chunk][tap][8][pitch] (zero rows / channels included), so a chunk's weights are 72
// row segments of 64 MT bytes; `pitch` (Geom::rp) is the caller's and holds whole workgroups of any MT.
// LDS: two arrays per instantiation, sW [72][w_pitch(MT)] and sX [8][kChP].  The pitches follow corr_common.hpp: a [k][columns] image
// wants pitch == 16 mod 32, so the two kq of a lane half land on disjoint banks (kChP = 144; w_pitch pads 32 | 16 MT by 16).
// Staging is the plain form -- load, store, barrier, MFMAs -- and the workgroups resident on a compute unit (3 to 8) hide one another's
// loads.  Two forms that keep a chunk in registers (loads issued together before the barrier; the next chunk loaded under the current
// chunk's MFMAs) were measured on the GRU and were 4-25 % slower at every benched shape: 90-117 VGPRs instead of 48-51, fewer resident
// waves.
//
// Summation.  FLUSH = 0: one fmaf chain per output over all input channels in order (the GRU: a recurrence keeps fp32 rounding, and
// its Ch + Cx <= 128 channels stay ONE chain -- tests and fixtures hold its bits).  FLUSH = n: the accumulators are added into a
// second set every n chunks and the sum is tot + acc (the decoder, n = 4: K reaches 4608 there, and one fp32 chain of that length sits
// at four times the error of the framework's blocked sums; this is a chain of 288 products, then a chain of at most 16 blocks).
// FLUSH = 0 compiles the second set away.  Either way an output's chains run over the input channels in order whatever MT and
// `groups` are: the bits do not depend on the launch geometry.
//
// A problem type P has
//   hw3::Geom g;
//   source(b)         -> a reader (gc, gy, gx) -> float of batch element b;
//   sink(b, gy, gx)   -> a writer (row, sum) of output pixel (gy, gx) of batch element b, called for row < g.rows only.
#pragma once
#include "conv_node.hpp"
#include "corr_common.hpp"

namespace hw3 {

using corr::v4f;
using node::dispatch_mt;
using node::Launch;

constexpr int kCK = 8;                       // input channels per staged chunk
constexpr int kKC = kCK * 9;                 // contraction elements per chunk
constexpr int kTR = 2, kTW = 32;             // pixel tile
constexpr int kRowP = 36;                    // halo row pitch (34 columns staged)
constexpr int kChP = (kTR + 2) * kRowP;      // 144 == 16 mod 32

constexpr int w_pitch(int mt) { return (mt * 16) % 32 == 16 ? mt * 16 : mt * 16 + 16; }
inline int mt_for(int rows) { return rows <= 16 ? 1 : rows <= 32 ? 2 : rows <= 64 ? 4 : 8; }      // 16-row blocks a workgroup holds, before the grid is looked at
inline int chunks_for(int Cin) { return (Cin + kCK - 1) / kCK; }

struct Geom {
  const float* w;           // [chunks][9][8][rp]
  int Cin, rows;            // input channels, output rows
  int H, W, tiles_x, tiles_y;
  int rp, groups;           // pitch of a weight row in global memory; workgroups along the output rows
};

inline int tiles_x(int W) { return (W + kTW - 1) / kTW; }
inline int tiles_y(int H) { return (H + kTR - 1) / kTR; }
inline Geom geom(const float* w, int Cin, int rows, int H, int W, int rp) {
  return Geom{w, Cin, rows, H, W, tiles_x(W), tiles_y(H), rp, 0};
}

// gy * W + gx of a pixel a reader or writer is called with: all three are non-negative there, so the product is one unsigned
// 32 x 32 -> 64 bit multiply-add (the signed form costs a second one per staged value)
__device__ __forceinline__ long long pixel_at(int gy, int gx, int W) {
  return static_cast<long long>(static_cast<unsigned long long>(static_cast<unsigned>(gy)) * static_cast<unsigned>(W) + static_cast<unsigned>(gx));
}

template <int MT, int FLUSH, class P>
__device__ __forceinline__ void conv_tile(const P& p) {
  constexpr int PW = w_pitch(MT);
  constexpr int kHalo = (kTR + 2) * (kTW + 2);                  // staged values per channel
  __shared__ __attribute__((aligned(16))) float sW[kKC * PW];
  __shared__ float sX[kCK * kChP];
  const Geom& g = p.g;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 15, kq = lane >> 4;
  unsigned blk = blockIdx.x;
  const int rg = blk % g.groups; blk /= g.groups;               // neighbours share the input tile
  const int tx = blk % g.tiles_x; blk /= g.tiles_x;
  const int ty = blk % g.tiles_y;
  const int b = blk / g.tiles_y;
  const int x0 = tx * kTW, y0 = ty * kTR;
  const auto src = p.source(b);
  const float* pw = g.w + rg * (16 * MT);
  const int pr = wave >> 1, pc = (wave & 1) * 16 + j;

  v4f acc[MT], tot[FLUSH ? MT : 1];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t] = v4f{0.f, 0.f, 0.f, 0.f};
  if constexpr (FLUSH != 0) {
#pragma unroll
    for (int t = 0; t < MT; ++t) tot[t] = v4f{0.f, 0.f, 0.f, 0.f};
  }

  const int nchunks = (g.Cin + kCK - 1) / kCK;
  for (int ch = 0; ch < nchunks; ++ch) {
    if constexpr (FLUSH != 0) {
      if (ch != 0 && ch % FLUSH == 0) {                          // blocked summation: a chain of FLUSH x 72 products, then a chain of blocks
#pragma unroll
        for (int t = 0; t < MT; ++t) {
          tot[t] += acc[t];
          acc[t] = v4f{0.f, 0.f, 0.f, 0.f};
        }
      }
    }
    __syncthreads();                                             // the previous chunk has been read
    for (int i = tid; i < kKC * 4 * MT; i += 256) {              // this workgroup's columns of the chunk's 72 weight rows, 16 bytes a piece
      const int row = i / (4 * MT), seg = i % (4 * MT);
      *reinterpret_cast<float4*>(sW + row * PW + seg * 4) =
          *reinterpret_cast<const float4*>(pw + (static_cast<size_t>(ch) * kKC + row) * g.rp + seg * 4);
    }
    for (int i = tid; i < kCK * kHalo; i += 256) {               // halo tile, 8 channels x 4 rows x 34 columns
      const int c = i / kHalo, rem = i - c * kHalo;
      const int row = rem / (kTW + 2), col = rem - row * (kTW + 2);
      const int gc = ch * kCK + c, gy = y0 - 1 + row, gx = x0 - 1 + col;
      float v = 0.f;
      if (gc < g.Cin && gy >= 0 && gy < g.H && gx >= 0 && gx < g.W) v = src(gc, gy, gx);
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
  if (gy >= g.H || gx >= g.W) return;
  const auto out = p.sink(b, gy, gx);
#pragma unroll
  for (int t = 0; t < MT; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * (MT * rg + t) + 4 * kq + r;
      if (row >= g.rows) continue;
      if constexpr (FLUSH != 0) out(row, tot[t][r] + acc[t][r]);
      else out(row, acc[t][r]);
    }
  }
}

// [chunk][tap][8][pitch] images of framework weights [rows][Cin][3][3].  The first image holds wa's rows and, below them, wb's
// (rb may be 0) at pitch p0; behind it an optional second image (p1 != 0) holds wc's rows at pitch p1.  Rows and channels past the
// weights' own are written as zeros.
struct WeightImages {
  const float* wa; const float* wb;      // first image: ra rows of wa, then rb rows of wb
  int ra, rb, p0;
  const float* wc;                       // second image: rc rows of wc; absent when p1 == 0
  int rc, p1;
};
inline size_t image_floats(int Cin, int pitch) { return static_cast<size_t>(chunks_for(Cin)) * kKC * pitch; }

namespace {
// One grid-stride pass over both images, one element per iteration.  MANY = false is the one-weight case (wa alone, one image):
// wb and the second image are compiled away, so the pitch is uniform, and its division with it.
template <bool MANY>
__global__ void __launch_bounds__(256) weight_layout_kernel(const WeightImages s, float* __restrict__ out, int Cin, int n0, int total) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const bool first = !MANY || i < n0;
    const int e = first ? i : i - n0, pitch = first ? s.p0 : s.p1;
    const int col = e % pitch, k = e / pitch;
    const int c = k % kCK, tap = (k / kCK) % 9, ci = (k / kKC) * kCK + c;
    float v = 0.f;
    if (ci < Cin) {
      const int at = ci * 9 + tap;
      if (first) {
        if (col < s.ra) v = s.wa[static_cast<size_t>(col) * Cin * 9 + at];
        else if (MANY && col < s.ra + s.rb) v = s.wb[static_cast<size_t>(col - s.ra) * Cin * 9 + at];
      } else if (col < s.rc) {
        v = s.wc[static_cast<size_t>(col) * Cin * 9 + at];
      }
    }
    out[i] = v;
  }
}

// one launch for all images; `cap` is the caller's grid cap (ts::blocks_for)
int weight_layout(const WeightImages& s, float* out, int Cin, int cap, hipStream_t st, const char* what) {
  const size_t n0 = image_floats(Cin, s.p0), total = n0 + image_floats(Cin, s.p1);          // at most 64 x 72 x 512
  const dim3 grid(ts::blocks_for(static_cast<long long>(total), cap));
  ts::dispatch_bool(s.rb != 0 || s.p1 != 0, [&](auto MANY) {
    hipLaunchKernelGGL(weight_layout_kernel<MANY()>, grid, dim3(256), 0, st, s, out, Cin, static_cast<int>(n0), static_cast<int>(total));
  });
  return ts::launched(what);
}
}  // namespace

// The launch rule: MT blocks of 16 output rows per workgroup, `groups` workgroups along the rows.  Start at mt_for(rows) and halve MT
// while the grid holds fewer than min_blocks workgroups: a grid that leaves compute units idle is cut finer along the rows (the input
// tile is then staged by more workgroups, from L2).  Sets g.groups; returns MT and the blocks of the 1-D grid (0: they do not fit one).
inline Launch launch_rule(Geom& g, int B, unsigned long long min_blocks) {
  int mt = mt_for(g.rows);
  const unsigned long long tiles = static_cast<unsigned long long>(g.tiles_x) * g.tiles_y * B;
  auto groups = [&](int m) { return (g.rows + 16 * m - 1) / (16 * m); };
  while (mt > 1 && tiles * groups(mt) < min_blocks) mt /= 2;
  g.groups = groups(mt);
  return Launch{mt, corr::grid_blocks(tiles * g.groups)};
}

}  // namespace hw3
