// FlowCorrBlock: the RAFT all-pairs correlation pyramid for optical flow and its windowed lookup (reference architecture/modeling/
// aggregation/utils/raft_corr.py:71-160: three [HW,C]x[C,HW] matmuls and their combine, three avg_pool2d over a [B*HW, 1, H, W]
// tensor, num_levels grid_sample calls and the permutes between them -- every intermediate the size of the [B*HW, HW] volume).
//
// Closed form.  fmap1, fmap2 [B,C,H,W], coords [B,2,H,W] (channel 0 = x, 1 = y, at level-0 scale), L levels, radius r, K = 2r+1;
// N = H*W, n and m number the pixels of frame 1 and frame 2 row-major, H_i = H >> i, W_i = W >> i, S = sqrt(C) rounded to fp32.
//   P_0[b,n,m] = (f1_n . f1_m - 2 f1_n . f2_m + f2_n . f2_m) / S         (FULL Gram matrices, not squared norms: the reference's
//              = (f1_n . D_m - D_n . f2_m) / S,  D = f1 - f2               arithmetic; evaluated here as ONE contraction of length 2C)
//   P_i[b,n]   = avg_pool2d(P_{i-1}[b,n] as an H_{i-1} x W_{i-1} image, 2, 2)   (from the ROUNDED level below; an odd last row or
//                column is dropped)
//   out[b, i K^2 + a K + bb, y, x] = bilinear(P_i[b,n], xs, ys), zeros outside,  xs = x_t / 2^i + (a - r), ys = y_t / 2^i + (bb - r),
//   (x_t, y_t) = coords[b,:,y,x]: the FIRST window index moves x (the meshgrid(dy, dx) quirk of raft_corr.py:97-103).
// bilinear_sampler normalises by W_i - 1, H_i - 1 and grid_sample(align_corners=True) undoes it: flow_position() takes those fp32
// steps in the reference's order, every one rounded on its own.  Every level needs H_i >= 2 and W_i >= 2 (the division).
//
// Data layout.  ONE pyramid buffer: level i is [B*N][H_i*W_i] contiguous at float offset B*N * sum_{l<i} H_l W_l (level_offsets;
// the Python side slices the same way).  Row b*N + n of every level belongs to source pixel n alone: the lookup reads only its own
// L rows, and the backward's owner writes them without any atomic.
//
// ts_flow_corr_pyramid_fwd   a workgroup owns FS = 32 source pixels n and an 8-row by 32-column PATCH of target pixels, aligned to
//   8 = 2^(4-1) in both directions.  16-channel chunks are staged in LDS as 32 rows of the length-2C contraction (f1_n | -D_n against
//   D_m | f2_m), v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulation), a wave 16 sources by 128 targets.  The tile is
//   divided by S into LDS, leaves as 128-byte runs along x', and levels 1..L-1 are pooled from the tile in LDS level by level
//   (8 >> 3 == 1: at most 4 levels): level 0 is never read back.
// ts_flow_corr_lookup_fwd    a lane owns one (pixel, level, a): K taps along y of its own row, stores coalesced along x.
// ts_flow_corr_lookup_bwd    a wave owns one pixel.  The taps of a level are one cell apart, so they touch a window of at most
//   cw = 2r + 4 cells per axis; the bilinear weight of tap (a, bb) on cell (mx, my) is wx_a(mx) wy_bb(my).  A lane owns one
//   (level, cell) and GATHERS the taps that fall on it in tap order (no atomic, neither in LDS nor in global memory; the same order
//   every run).  Then the wave writes the pixel's rows once: folded into the level-0 cotangent by the pooling chain's own backward,
//   G[m] = ((g_3[m>>3] / 4 + g_2[m>>2]) / 4 + g_1[m>>1]) / 4 + g_0[m]  (fold = 1), or level by level in the pyramid's layout
//   (fold = 0, the gradient with respect to a free pyramid).  grad_coords: a lane per tap, reduced over the wave in a fixed order.
// ts_flow_corr_pyramid_bwd   per batch, G [N,N]:  grad_f1 = ((G + G^T) f1 - 2 G f2) / S,  grad_f2 = ((G + G^T) f2 - 2 G^T f1) / S, as
//   grad[c][n] = sum_m G[n,m] U[c][m] + sum_m G[m,n] V[c][m]  (U = f1 - 2 f2, V = f1;  resp. U = f2, V = f2 - 2 f1): a workgroup owns
//   64 channels by 64 pixels, 32-wide slices of the contraction staged in LDS, the same MFMA; every output is written once.  A
//   cotangent that still has its levels (levels > 1) is folded while it is staged.
#include <cmath>

#include "corr_common.hpp"

namespace {

using namespace corr;

constexpr int FS = 32;             // source pixels per workgroup
constexpr int PH = 8, PW = 32;     // the patch of target pixels
constexpr int FT = PH * PW;        // 256 targets: one per thread
static_assert(FT == 256, "a workgroup of 256 threads stages and stores one target each");
constexpr int FKC = RKC / 2;       // channels per staged chunk: 16 rows of f1 | D, 16 rows of -D | f2
// LDS pitches by the bank arithmetic of corr_common.hpp.  Not measured.
constexpr int FPA = 48;            // [k][32 sources]: 48 == 16 mod 32
constexpr int FPB = 272;           // [k][256 targets]: 272 == 16 mod 32
constexpr int FPO = 260;           // output tile [32][256]: 4 * 260 == 16 mod 32
constexpr int FPL = 84;            // pooled levels of a source: 4x16 + 2x8 + 1x4 cells
constexpr int FPK = 80;            // backward, [k][64 pixels]: 80 == 16 mod 32
constexpr int BT = 64;             // backward tile edge: channels and pixels per workgroup
constexpr int kFlowMaxLevels = 4;  // 8 >> 3 == 1: the deepest level an 8-row patch still pools by itself

struct Flow : Levels {             // off[i]: float offset of level i in the pyramid buffer
  int B, C, H, W, L, r;
};

void level_offsets(Flow& p) {
  corr::level_offsets(p, static_cast<size_t>(p.B) * p.H * p.W, [&](int i) { return (p.H >> i) * (p.W >> i); });
}

// Position of tap k of level i along one axis (size D_i, Dm1 = D_i - 1): c / 2^i, + (k - r), * 2 / (D_i - 1) - 1, then grid_sample's
// ((g + 1) / 2) * (D_i - 1).  The clamp keeps the conversion to int defined: every position it moves has both taps outside either
// way (a non-finite coordinate lands on -2).
__device__ __forceinline__ float flow_position(float c, int i, int k, int r, float Dm1) {
  float t = __fmul_rn(c, pow2_neg(i));
  t = __fadd_rn(t, static_cast<float>(k - r));
  const float g = __fsub_rn(__fdiv_rn(__fmul_rn(2.f, t), Dm1), 1.f);
  const float pos = __fmul_rn(__fdiv_rn(__fadd_rn(g, 1.f), 2.f), Dm1);
  return fminf(fmaxf(pos, -2.f), Dm1 + 2.f);
}

// ------------------------------------------------------------------------------------------------------------- pyramid, forward
__global__ void __launch_bounds__(256)
flow_pyramid_fwd_kernel(const float* __restrict__ f1, const float* __restrict__ f2, float* __restrict__ pyr, const Flow p,
                        float sqrtC, int nsb, int pyb, int pxb) {
  __shared__ __attribute__((aligned(16))) float lds[RKC * FPA + RKC * FPB];     // both operand images; afterwards the output tile [32][FPO]
  __shared__ __attribute__((aligned(16))) float sP[FS * FPL];                   // pooled levels: level 1 at column 0, 2 at 64, 3 at 80
  static_assert(FS * FPO <= RKC * FPA + RKC * FPB, "the output tile lives over the operand images");
  float* sA = lds;
  float* sB = lds + RKC * FPA;
  float* sO = lds;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 15, kq = lane >> 4;
  long long blk = blockIdx.x;
  const int bx = static_cast<int>(blk % pxb); blk /= pxb;
  const int by = static_cast<int>(blk % pyb); blk /= pyb;
  const int sb = static_cast<int>(blk % nsb);
  const int b = static_cast<int>(blk / nsb);
  const size_t N = static_cast<size_t>(p.H) * p.W;
  const size_t n0 = static_cast<size_t>(sb) * FS;
  const int y0 = by * PH, x0 = bx * PW;
  const float* F1 = f1 + static_cast<size_t>(b) * p.C * N;
  const float* F2 = f2 + static_cast<size_t>(b) * p.C * N;
  // sources: column tid & 31, channel rows tid >> 5 and + 8;  targets: one per thread, (tid >> 5, tid & 31) of the patch
  const int col = tid & 31, cb = tid >> 5;
  const bool okA = n0 + col < N;
  const size_t na = okA ? n0 + col : 0;
  const int ty = y0 + (tid >> 5), tx = x0 + (tid & 31);
  const bool okB = ty < p.H && tx < p.W;
  const size_t mb = okB ? static_cast<size_t>(ty) * p.W + tx : 0;
  v4f acc[8];
#pragma unroll
  for (int t = 0; t < 8; ++t) acc[t] = v4f{0.f, 0.f, 0.f, 0.f};

#pragma unroll 1
  for (int c0 = 0; c0 < p.C; c0 += FKC) {
    __syncthreads();                       // the previous chunk's fragments have been read
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const int kk = cb + 8 * m, c = c0 + kk;
      const bool ok = c < p.C && okA;
      const size_t o = static_cast<size_t>(ok ? c : 0) * N + na;
      const float v1 = F1[o], v2 = F2[o];
      sA[kk * FPA + col] = ok ? v1 : 0.f;
      sA[(FKC + kk) * FPA + col] = ok ? __fsub_rn(v2, v1) : 0.f;
    }
#pragma unroll 4
    for (int kk = 0; kk < FKC; ++kk) {
      const int c = c0 + kk;
      const bool ok = c < p.C && okB;
      const size_t o = static_cast<size_t>(ok ? c : 0) * N + mb;
      const float v1 = F1[o], v2 = F2[o];
      sB[kk * FPB + tid] = ok ? __fsub_rn(v1, v2) : 0.f;
      sB[(FKC + kk) * FPB + tid] = ok ? v2 : 0.f;
    }
    __syncthreads();
    // rows past C are zeros: every chunk runs its eight steps
    mfma_chunk<FPA, FPB, 8>(acc, sA, 16 * (wave & 1), sB, 128 * (wave >> 1), RKC / 4, j, kq);
  }
  // ---- the tile, divided by sqrt(C), into LDS: a lane of an accumulator holds target j of four sources
  __syncthreads();
  store_tile<FPO, 8>(sO, acc, 16 * (wave & 1), 128 * (wave >> 1), sqrtC, j, kq);
  __syncthreads();
  // ---- level 0: a wave store is two 128-byte runs of one source's row
  const size_t row0 = static_cast<size_t>(b) * N + n0;
  for (int rr = 0; rr < FS; ++rr)
    if (n0 + rr < N && okB) pyr[(row0 + rr) * N + mb] = sO[rr * FPO + tid];
  // ---- levels 1..L-1, each from the rounded level below: the four cells in avg_pool2d's order
  const float* src = sO;
  int spitch = FPO, sw = PW, doff = 0;
  for (int i = 1; i < p.L; ++i) {
    const int hi = PH >> i, wi = PW >> i, cells = hi * wi, Hi = p.H >> i, Wi = p.W >> i;
    const size_t Ni = static_cast<size_t>(Hi) * Wi;
    float* dst = sP + doff;
    float* lvl = pyr + p.off[i];
    for (int idx = tid; idx < FS * cells; idx += 256) {
      const int rr = idx / cells, cc = idx - rr * cells, cy = cc / wi, cx = cc - cy * wi;
      const float* s = src + rr * spitch + 2 * cy * sw + 2 * cx;
      const float v = (((s[0] + s[1]) + s[sw]) + s[sw + 1]) * 0.25f;
      dst[rr * FPL + cc] = v;
      const int gy = (y0 >> i) + cy, gx = (x0 >> i) + cx;
      if (n0 + rr < N && gy < Hi && gx < Wi) lvl[(row0 + rr) * Ni + static_cast<size_t>(gy) * Wi + gx] = v;
    }
    __syncthreads();
    src = dst;
    spitch = FPL;
    sw = wi;
    doff += cells;
  }
}

// -------------------------------------------------------------------------------------------------------------- lookup, forward
// The bilinear sample of one row (an Hi x Wi image) at (ix, iy), zeros outside, weights and order as grid_sample's.
__device__ __forceinline__ float flow_sample(const float* __restrict__ rowp, int Hi, int Wi, float ix, float iy) {
  const float xf = floorf(ix), yf = floorf(iy);
  const int x0 = static_cast<int>(xf), y0 = static_cast<int>(yf);
  const float wx1 = __fsub_rn(ix, xf), wx0 = __fsub_rn(__fadd_rn(xf, 1.f), ix);
  const float wy1 = __fsub_rn(iy, yf), wy0 = __fsub_rn(__fadd_rn(yf, 1.f), iy);
  const bool inx0 = x0 >= 0 && x0 < Wi, inx1 = x0 + 1 >= 0 && x0 + 1 < Wi;
  const bool iny0 = y0 >= 0 && y0 < Hi, iny1 = y0 + 1 >= 0 && y0 + 1 < Hi;
  const int xa = min(max(x0, 0), Wi - 1), xb = min(max(x0 + 1, 0), Wi - 1);
  const int ya = min(max(y0, 0), Hi - 1), yb = min(max(y0 + 1, 0), Hi - 1);
  const float l00 = rowp[ya * Wi + xa], l01 = rowp[ya * Wi + xb], l10 = rowp[yb * Wi + xa], l11 = rowp[yb * Wi + xb];
  const float nw = (iny0 && inx0) ? l00 : 0.f, ne = (iny0 && inx1) ? l01 : 0.f;
  const float sw = (iny1 && inx0) ? l10 : 0.f, se = (iny1 && inx1) ? l11 : 0.f;
  return nw * __fmul_rn(wx0, wy0) + ne * __fmul_rn(wx1, wy0) + sw * __fmul_rn(wx0, wy1) + se * __fmul_rn(wx1, wy1);
}

__global__ void __launch_bounds__(256)
flow_lookup_fwd_kernel(const float* __restrict__ pyr, const float* __restrict__ coords, float* __restrict__ out, const Flow p) {
  const int K = 2 * p.r + 1;
  const long long total = static_cast<long long>(p.B) * p.L * K * p.H * p.W;
  const long long idx = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int x = static_cast<int>(idx % p.W);
  long long t = idx / p.W;
  const int y = static_cast<int>(t % p.H); t /= p.H;
  const int a = static_cast<int>(t % K); t /= K;
  const int i = static_cast<int>(t % p.L), b = static_cast<int>(t / p.L);
  const size_t N = static_cast<size_t>(p.H) * p.W;
  const size_t yx = static_cast<size_t>(y) * p.W + x, pix = static_cast<size_t>(b) * N + yx;
  const float cx = coords[static_cast<size_t>(b) * 2 * N + yx], cy = coords[(static_cast<size_t>(b) * 2 + 1) * N + yx];
  const int Hi = p.H >> i, Wi = p.W >> i;
  const float* rowp = pyr + p.off[i] + pix * (static_cast<size_t>(Hi) * Wi);
  const float ix = flow_position(cx, i, a, p.r, static_cast<float>(Wi - 1));
  float* op = out + (static_cast<size_t>(b) * p.L * K * K + (static_cast<size_t>(i) * K + a) * K) * N + yx;
  for (int bb = 0; bb < K; ++bb) {
    const float iy = flow_position(cy, i, bb, p.r, static_cast<float>(Hi - 1));
    op[static_cast<size_t>(bb) * N] = flow_sample(rowp, Hi, Wi, ix, iy);
  }
}

// ------------------------------------------------------------------------------------------------------------- lookup, backward
__global__ void __launch_bounds__(256)
flow_lookup_bwd_kernel(const float* __restrict__ pyr, const float* __restrict__ coords, const float* __restrict__ go,
                       float* __restrict__ gcoords, float* __restrict__ gpyr, const Flow p, int cw, int fold) {
  // per wave: [L][cw*cw] cell sums, then per (level, axis, tap) the first cell (int) and its two weights, then per (level, axis)
  // the first cell of the window (int)
  extern __shared__ __attribute__((aligned(16))) float flow_lds[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const size_t N = static_cast<size_t>(p.H) * p.W, npix = static_cast<size_t>(p.B) * N;
  const size_t pix_raw = static_cast<size_t>(blockIdx.x) * 4 + wave;
  const bool live = pix_raw < npix;                                      // a wave past the end works on the last pixel and stores nothing
  const size_t pix = live ? pix_raw : npix - 1;
  const int b = static_cast<int>(pix / N);
  const size_t yx = pix - static_cast<size_t>(b) * N;
  const int K = 2 * p.r + 1, K2 = K * K, ntap = p.L * K2, cw2 = cw * cw;
  float* my = flow_lds + wave * (p.L * cw2 + p.L * 2 * K * 3 + p.L * 2);
  float* tab = my + p.L * cw2;                                           // [L][2][K][3]
  int* first = reinterpret_cast<int*>(tab + p.L * 2 * K * 3);            // [L][2]
  const float cx = coords[static_cast<size_t>(b) * 2 * N + yx], cy = coords[(static_cast<size_t>(b) * 2 + 1) * N + yx];
  const float* gop = go + static_cast<size_t>(b) * ntap * N + yx;        // + channel * N

  // ---- the taps' positions along each axis: first cell and the weights of it and of the next
  for (int e = lane; e < p.L * 2 * K; e += 64) {
    const int i = e / (2 * K), ax = (e / K) & 1, k = e % K;
    const int Di = (ax ? p.H : p.W) >> i;
    const float pos = flow_position(ax ? cy : cx, i, k, p.r, static_cast<float>(Di - 1));
    const float f = floorf(pos);
    float* te = tab + e * 3;
    reinterpret_cast<int*>(te)[0] = static_cast<int>(f);
    te[1] = __fsub_rn(__fadd_rn(f, 1.f), pos);
    te[2] = __fsub_rn(pos, f);
    if (k == 0) first[i * 2 + ax] = static_cast<int>(f);
  }
  __syncthreads();
  // ---- a lane per (level, cell): the taps that fall on the cell, gathered in tap order (only when the pyramid's cotangent is wanted)
  for (int e = lane; gpyr != nullptr && e < p.L * cw2; e += 64) {
    const int i = e / cw2, jj = e - i * cw2, jy = jj / cw, jx = jj - jy * cw;
    const int Hi = p.H >> i, Wi = p.W >> i;
    const int mx = first[i * 2] + jx, myy = first[i * 2 + 1] + jy;
    float s = 0.f;
    if (mx >= 0 && mx < Wi && myy >= 0 && myy < Hi) {                    // a cell outside the image: zero padding, dropped
      const float* tx = tab + (i * 2) * K * 3;
      const float* ty = tab + (i * 2 + 1) * K * 3;
      for (int a = 0; a < K; ++a) {
        const int xa = reinterpret_cast<const int*>(tx + a * 3)[0];
        if (xa != mx && xa + 1 != mx) continue;
        const float wxa = xa == mx ? tx[a * 3 + 1] : tx[a * 3 + 2];
        for (int bb = 0; bb < K; ++bb) {
          const int yb = reinterpret_cast<const int*>(ty + bb * 3)[0];
          if (yb != myy && yb + 1 != myy) continue;
          const float wyb = yb == myy ? ty[bb * 3 + 1] : ty[bb * 3 + 2];
          s += gop[static_cast<size_t>(i * K2 + a * K + bb) * N] * __fmul_rn(wxa, wyb);
        }
      }
    }
    my[e] = s;
  }
  // ---- grad_coords: a lane per tap, d out / d x_t = g * d bilinear / d ix * 2^-i (the normalisation and its inverse cancel)
  if (gcoords != nullptr) {
    float px = 0.f, py = 0.f;
    for (int tt = lane; tt < ntap; tt += 64) {
      const int i = tt / K2, ab = tt - i * K2, a = ab / K, bb = ab - a * K;
      const int Hi = p.H >> i, Wi = p.W >> i;
      const float* tx = tab + ((i * 2) * K + a) * 3;
      const float* ty = tab + ((i * 2 + 1) * K + bb) * 3;
      const int x0 = reinterpret_cast<const int*>(tx)[0], y0 = reinterpret_cast<const int*>(ty)[0];
      const float* rowp = pyr + p.off[i] + pix * (static_cast<size_t>(Hi) * Wi);
      const bool inx0 = x0 >= 0 && x0 < Wi, inx1 = x0 + 1 >= 0 && x0 + 1 < Wi;
      const bool iny0 = y0 >= 0 && y0 < Hi, iny1 = y0 + 1 >= 0 && y0 + 1 < Hi;
      const int xa = min(max(x0, 0), Wi - 1), xb = min(max(x0 + 1, 0), Wi - 1);
      const int ya = min(max(y0, 0), Hi - 1), yb = min(max(y0 + 1, 0), Hi - 1);
      const float l00 = rowp[ya * Wi + xa], l01 = rowp[ya * Wi + xb], l10 = rowp[yb * Wi + xa], l11 = rowp[yb * Wi + xb];
      const float nw = (iny0 && inx0) ? l00 : 0.f, ne = (iny0 && inx1) ? l01 : 0.f;
      const float sw = (iny1 && inx0) ? l10 : 0.f, se = (iny1 && inx1) ? l11 : 0.f;
      const float g = gop[static_cast<size_t>(tt) * N] * pow2_neg(i);
      px += g * ((ne - nw) * ty[1] + (se - sw) * ty[2]);
      py += g * ((sw - nw) * tx[1] + (se - ne) * tx[2]);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      px += __shfl_xor(px, o);
      py += __shfl_xor(py, o);
    }
    if (lane == 0 && live) {
      gcoords[static_cast<size_t>(b) * 2 * N + yx] = px;
      gcoords[(static_cast<size_t>(b) * 2 + 1) * N + yx] = py;
    }
  }
  __syncthreads();
  if (gpyr == nullptr || !live) return;
  // ---- the pixel's row(s), written once
  if (fold) {
    float* grow = gpyr + pix * N;
    for (int yy = 0; yy < p.H; ++yy)
      for (int xx = lane; xx < p.W; xx += 64) {
        float v = 0.f;
        for (int i = p.L - 1; i >= 0; --i) {
          const int cyi = yy >> i, cxi = xx >> i, jy = cyi - first[i * 2 + 1], jx = cxi - first[i * 2];
          const bool in = cyi < (p.H >> i) && cxi < (p.W >> i) && jy >= 0 && jy < cw && jx >= 0 && jx < cw;
          const float c = my[i * cw2 + min(max(jy, 0), cw - 1) * cw + min(max(jx, 0), cw - 1)];
          v += in ? c : 0.f;
          if (i > 0) v *= 0.25f;
        }
        grow[static_cast<size_t>(yy) * p.W + xx] = v;
      }
  } else {
    for (int i = 0; i < p.L; ++i) {
      const int Hi = p.H >> i, Wi = p.W >> i;
      float* grow = gpyr + p.off[i] + pix * (static_cast<size_t>(Hi) * Wi);
      for (int yy = 0; yy < Hi; ++yy)
        for (int xx = lane; xx < Wi; xx += 64) {
          const int jy = yy - first[i * 2 + 1], jx = xx - first[i * 2];
          const bool in = jy >= 0 && jy < cw && jx >= 0 && jx < cw;
          const float c = my[i * cw2 + min(max(jy, 0), cw - 1) * cw + min(max(jx, 0), cw - 1)];
          grow[static_cast<size_t>(yy) * Wi + xx] = in ? c : 0.f;
        }
    }
  }
}

// ------------------------------------------------------------------------------------------------------------ pyramid, backward
// Element (n, m) of batch b's level-0 cotangent: of a cotangent that still has its levels, the pooling chain's backward.
__device__ __forceinline__ float flow_cotangent0(const float* __restrict__ gpyr, const Flow& p, size_t brow, size_t n, size_t m) {
  const size_t N = static_cast<size_t>(p.H) * p.W;
  if (p.L == 1) return gpyr[(brow + n) * N + m];
  const int yy = static_cast<int>(m / p.W), xx = static_cast<int>(m - static_cast<size_t>(yy) * p.W);
  float v = 0.f;
  for (int i = p.L - 1; i >= 1; --i) {
    const int Hi = p.H >> i, Wi = p.W >> i, cy = yy >> i, cx = xx >> i;
    const float c = gpyr[p.off[i] + (brow + n) * (static_cast<size_t>(Hi) * Wi) + static_cast<size_t>(min(cy, Hi - 1)) * Wi + min(cx, Wi - 1)];
    v = (v + ((cy < Hi && cx < Wi) ? c : 0.f)) * 0.25f;
  }
  return v + gpyr[(brow + n) * N + m];
}

// grad[c][n] = (sum_m G[n,m] U[c][m] + sum_m G[m,n] V[c][m]) / S.  SECOND = false: Fa = fmap1, Fb = fmap2, U = Fa - 2 Fb, V = Fa
// (grad_fmap1); true: Fa = fmap2, Fb = fmap1, U = Fa, V = Fa - 2 Fb (grad_fmap2).  M = 16 channels per wave, 64 pixels in four tiles.
template <bool SECOND>
__global__ void __launch_bounds__(256)
flow_pyramid_bwd_kernel(const float* __restrict__ gpyr, const float* __restrict__ Fa, const float* __restrict__ Fb,
                        float* __restrict__ grad, const Flow p, float sqrtC, int strips, int cgroups) {
  __shared__ __attribute__((aligned(16))) float sU[BT * RPM];            // [channel][k]
  __shared__ __attribute__((aligned(16))) float sV[BT * RPM];            // [channel][k]
  __shared__ __attribute__((aligned(16))) float sGr[BT * RPM];           // [pixel n][k]: G[n, k]
  __shared__ __attribute__((aligned(16))) float sGc[RKC * FPK];          // [k][pixel n]: G[k, n]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 15, kq = lane >> 4;
  long long blk = blockIdx.x;
  const int sp = static_cast<int>(blk % strips); blk /= strips;
  const int cg = static_cast<int>(blk % cgroups);
  const int b = static_cast<int>(blk / cgroups);
  const size_t N = static_cast<size_t>(p.H) * p.W, brow = static_cast<size_t>(b) * N;
  const size_t pos0 = static_cast<size_t>(sp) * BT;
  const int c0 = cg * BT;
  const float* A = Fa + static_cast<size_t>(b) * p.C * N;
  const float* Bm = Fb + static_cast<size_t>(b) * p.C * N;
  v4f acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = v4f{0.f, 0.f, 0.f, 0.f};

#pragma unroll 1
  for (size_t k0 = 0; k0 < N; k0 += RKC) {
    __syncthreads();
    {
      const int kk = tid & 31;
      const size_t k = k0 + kk;
#pragma unroll
      for (int m = 0; m < 8; ++m) {
        const int cc = (tid >> 5) + 8 * m, c = c0 + cc;
        const bool ok = c < p.C && k < N;
        const size_t o = static_cast<size_t>(ok ? c : 0) * N + (ok ? k : 0);
        const float va = A[o], vb = Bm[o], mix = __fsub_rn(va, __fmul_rn(2.f, vb));
        sU[cc * RPM + kk] = ok ? (SECOND ? va : mix) : 0.f;
        sV[cc * RPM + kk] = ok ? (SECOND ? mix : va) : 0.f;
      }
#pragma unroll
      for (int m = 0; m < 8; ++m) {
        const int pp = (tid >> 5) + 8 * m;
        const size_t pos = pos0 + pp;
        const bool ok = pos < N && k < N;
        const float v = flow_cotangent0(gpyr, p, brow, ok ? pos : 0, ok ? k : 0);
        sGr[pp * RPM + kk] = ok ? v : 0.f;
      }
    }
    {
      const int pp = tid & 63;
      const size_t pos = pos0 + pp;
#pragma unroll
      for (int m = 0; m < 8; ++m) {
        const int kk = (tid >> 6) + 4 * m;
        const size_t k = k0 + kk;
        const bool ok = pos < N && k < N;
        const float v = flow_cotangent0(gpyr, p, brow, ok ? k : 0, ok ? pos : 0);
        sGc[kk * FPK + pp] = ok ? v : 0.f;
      }
    }
    __syncthreads();
    const int ksteps = static_cast<int>(min(static_cast<size_t>(RKC / 4), (N - k0 + 3) / 4));
#pragma unroll
    for (int q = 0; q < RKC / 4; ++q) {
      if (q < ksteps) {
        const float au = sU[(16 * wave + j) * RPM + 4 * q + kq], av = sV[(16 * wave + j) * RPM + 4 * q + kq];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(au, sGr[(16 * t + j) * RPM + 4 * q + kq], acc[t], 0, 0, 0);
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, sGc[(4 * q + kq) * FPK + 16 * t + j], acc[t], 0, 0, 0);
        }
      }
    }
  }
  // a lane of an accumulator holds pixel j of four channels: 64-byte runs along the image
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int c = c0 + 16 * wave + 4 * kq + r;
      const size_t pos = pos0 + 16 * t + j;
      if (c < p.C && pos < N) grad[(static_cast<size_t>(b) * p.C + c) * N + pos] = __fdiv_rn(acc[t][r], sqrtC);
    }
}

int check(const Flow& p, bool with_c, bool with_r) {
  TS_REQUIRE(p.B > 0 && p.H > 0 && p.W > 0 && (!with_c || p.C > 0), TS_ERR_SHAPE, "flow_corr: non-positive size");
  TS_REQUIRE(p.L >= 1, TS_ERR_SHAPE, "flow_corr: num_levels = %d, need >= 1", p.L);
  TS_REQUIRE(!with_r || p.r >= 0, TS_ERR_SHAPE, "flow_corr: radius = %d, need >= 0", p.r);
  TS_REQUIRE(p.L <= kFlowMaxLevels, TS_ERR_UNSUPPORTED,
             "flow_corr: num_levels = %d, this build pools at most %d levels (from an %d-row patch of the level-0 tile)", p.L,
             kFlowMaxLevels, PH);
  TS_REQUIRE(!with_r || p.r <= 1024, TS_ERR_UNSUPPORTED, "flow_corr: radius = %d, this build takes at most 1024", p.r);
  for (int i = 0; i < p.L; ++i)
    TS_REQUIRE((p.H >> i) >= 2 && (p.W >> i) >= 2, TS_ERR_SHAPE,
               "flow_corr: level %d of a %d x %d map is %d x %d, need >= 2 x 2 (the lookup divides by H_i - 1 and W_i - 1)", i, p.H, p.W,
               p.H >> i, p.W >> i);
  TS_REQUIRE(static_cast<unsigned long long>(p.H) * p.W < 0x7fffffffull, TS_ERR_UNSUPPORTED, "flow_corr: H * W does not fit an int");
  return TS_OK;
}

}  // namespace

extern "C" int ts_flow_corr_pyramid_fwd(const float* fmap1, const float* fmap2, float* pyramid, int B, int C, int H, int W,
                                        int num_levels, void* stream) {
  Flow p{{}, B, C, H, W, num_levels, 0};
  if (int rc = check(p, true, false)) return rc;
  TS_REQUIRE_PTR(fmap1); TS_REQUIRE_PTR(fmap2); TS_REQUIRE_PTR(pyramid);
  level_offsets(p);
  const unsigned long long N = static_cast<unsigned long long>(H) * W;
  const int nsb = static_cast<int>((N + FS - 1) / FS), pyb = (H + PH - 1) / PH, pxb = (W + PW - 1) / PW;
  const unsigned blocks = grid_blocks(static_cast<unsigned long long>(B) * nsb * pyb * pxb);
  TS_REQUIRE(blocks != 0, TS_ERR_UNSUPPORTED, "flow_corr_pyramid_fwd: grid too large");
  hipLaunchKernelGGL(flow_pyramid_fwd_kernel, dim3(blocks), dim3(256), 0, ts::as_stream(stream), fmap1, fmap2, pyramid, p,
                     sqrtf(static_cast<float>(C)), nsb, pyb, pxb);
  return ts::launched("flow_pyramid_fwd_kernel");
}

extern "C" int ts_flow_corr_lookup_fwd(const float* pyramid, const float* coords, float* out, int B, int H, int W, int num_levels,
                                       int radius, void* stream) {
  Flow p{{}, B, 0, H, W, num_levels, radius};
  if (int rc = check(p, false, true)) return rc;
  TS_REQUIRE_PTR(pyramid); TS_REQUIRE_PTR(coords); TS_REQUIRE_PTR(out);
  level_offsets(p);
  const unsigned long long total = static_cast<unsigned long long>(B) * num_levels * (2 * radius + 1) * H * W;
  const unsigned blocks = grid_blocks((total + 255) / 256);
  TS_REQUIRE(blocks != 0, TS_ERR_UNSUPPORTED, "flow_corr_lookup_fwd: grid too large");
  hipLaunchKernelGGL(flow_lookup_fwd_kernel, dim3(blocks), dim3(256), 0, ts::as_stream(stream), pyramid, coords, out, p);
  return ts::launched("flow_lookup_fwd_kernel");
}

extern "C" int ts_flow_corr_lookup_bwd(const float* pyramid, const float* coords, const float* grad_out, float* grad_coords,
                                       float* grad_pyramid, int B, int H, int W, int num_levels, int radius, int fold, void* stream) {
  Flow p{{}, B, 0, H, W, num_levels, radius};
  if (int rc = check(p, false, true)) return rc;
  TS_REQUIRE_PTR(coords); TS_REQUIRE_PTR(grad_out);
  TS_REQUIRE(grad_coords != nullptr || grad_pyramid != nullptr, TS_ERR_NULL, "flow_corr_lookup_bwd: grad_coords and grad_pyramid are both NULL");
  if (grad_coords != nullptr) TS_REQUIRE_PTR(pyramid);
  level_offsets(p);
  // cells a level's taps can touch along an axis: the taps lie one cell apart, so their floors span 2r + 1 cells, the right tap of
  // the last one more, and the rounding of a position may move a floor by one: 2r + 3, and one spare
  const int cw = 2 * radius + 4, K = 2 * radius + 1;
  const size_t shm = 4 * static_cast<size_t>(num_levels) * (static_cast<size_t>(cw) * cw + 6 * K + 2) * sizeof(float);
  TS_REQUIRE(shm <= 64 * 1024, TS_ERR_UNSUPPORTED, "flow_corr_lookup_bwd: radius = %d needs %zu bytes of LDS", radius, shm);
  const unsigned long long npix = static_cast<unsigned long long>(B) * H * W;
  const unsigned blocks = grid_blocks((npix + 3) / 4);
  TS_REQUIRE(blocks != 0, TS_ERR_UNSUPPORTED, "flow_corr_lookup_bwd: grid too large");
  hipLaunchKernelGGL(flow_lookup_bwd_kernel, dim3(blocks), dim3(256), shm, ts::as_stream(stream), pyramid, coords, grad_out,
                     grad_coords, grad_pyramid, p, cw, fold != 0);
  return ts::launched("flow_lookup_bwd_kernel");
}

extern "C" int ts_flow_corr_pyramid_bwd(const float* grad_pyramid, const float* fmap1, const float* fmap2, float* grad_fmap1,
                                        float* grad_fmap2, int B, int C, int H, int W, int levels, void* stream) {
  Flow p{{}, B, C, H, W, levels, 0};
  if (int rc = check(p, true, false)) return rc;
  TS_REQUIRE_PTR(grad_pyramid); TS_REQUIRE_PTR(fmap1); TS_REQUIRE_PTR(fmap2);
  TS_REQUIRE(grad_fmap1 != nullptr || grad_fmap2 != nullptr, TS_ERR_NULL, "flow_corr_pyramid_bwd: grad_fmap1 and grad_fmap2 are both NULL");
  level_offsets(p);
  const unsigned long long N = static_cast<unsigned long long>(H) * W;
  const int strips = static_cast<int>((N + BT - 1) / BT), cgroups = (C + BT - 1) / BT;
  const unsigned blocks = grid_blocks(static_cast<unsigned long long>(B) * strips * cgroups);
  TS_REQUIRE(blocks != 0, TS_ERR_UNSUPPORTED, "flow_corr_pyramid_bwd: grid too large");
  const float sc = sqrtf(static_cast<float>(C));
  hipStream_t st = ts::as_stream(stream);
  if (grad_fmap1 != nullptr) {
    hipLaunchKernelGGL(flow_pyramid_bwd_kernel<false>, dim3(blocks), dim3(256), 0, st, grad_pyramid, fmap1, fmap2, grad_fmap1, p, sc, strips, cgroups);
    if (int rc = ts::launched("flow_pyramid_bwd_kernel<fmap1>")) return rc;
  }
  if (grad_fmap2 != nullptr) {
    hipLaunchKernelGGL(flow_pyramid_bwd_kernel<true>, dim3(blocks), dim3(256), 0, st, grad_pyramid, fmap2, fmap1, grad_fmap2, p, sc, strips, cgroups);
    if (int rc = ts::launched("flow_pyramid_bwd_kernel<fmap2>")) return rc;
  }
  return TS_OK;
}
