// CorrBlock: the RAFT-Stereo correlation pyramid and its windowed lookup (reference architecture/modeling/aggregation/utils/
// raft_corr.py:4-67: matmul, three avg_pool2d, four grid_sample over a [B*H*W, 1, 1, W] tensor, and the permutes between them).
//
// Closed form.  fmap1, fmap2 [B,C,H,W], disp [B,1,H,W], L levels, radius r; n = (b*H + y)*W + x numbers the pixels, W_i = W >> i.
//   P_0[n][x'] = sum_c fmap1[b,c,y,x] * fmap2[b,c,y,x'] / sqrt(C)                (sqrt and the division in fp32)
//   P_i[n][m]  = (P_{i-1}[n][2m] + P_{i-1}[n][2m+1]) / 2,  m < W_i               (from the ROUNDED level below; an odd tail is dropped)
//   out[b, i*(2r+1)+k, y, x] = (1 - 2^-(i+1)) * lerp0(P_i[n][:], xp),
//   xp = ((x - disp[n]) / 2^i + (k - r)) * W_i / (W - 1) - 0.5,   lerp0 = linear interpolation, zeros outside [0, W_i - 1].
// Both quirks are the reference's: x is normalised with the level-0 W - 1 but un-normalised by grid_sample(align_corners=False) at
// the level's width, and the y coordinate -1 is divided by 2^i with x, so the one-row image is sampled at y = -2^-(i+1) -- the
// row above it is outside: hence the level weights 0.5, 0.75, 0.875, 0.9375.  raft_position() takes the fp32 steps in the
// reference's order, every one rounded on its own.
//
// Data layout.  ONE pyramid buffer of N * sum_i W_i floats, N = B*H*W: level i is [N][W_i] contiguous at float offset
// N * (W_0 + ... + W_{i-1}) (level_offsets below; the Python side slices the same way).  Row n of every level belongs to pixel n
// alone: the lookup reads only its own L rows, and the backward's owner writes them without any atomic.
//
// ts_raft_corr_pyramid_fwd   a workgroup owns a 64 (x) by 64 (x') tile of one image row's Gram matrix: 32-channel chunks of both
//   strips staged in LDS, v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulation), wave w the 16 pixels w.  The tile is
//   divided by sqrt(C) into LDS, leaves as 256-byte runs along x', and levels 1..L-1 are pooled from the tile in LDS level by
//   level (64 is a multiple of 2^(L-1) for L <= 7): level 0 is never read back.
// ts_raft_corr_lookup_fwd    a lane owns one (pixel, level): 2r+1 taps of its own row, stores coalesced along x.
// ts_raft_corr_lookup_bwd    a wave owns one pixel.  The taps of a level touch a window of at most cw = floor(2r W/(W-1)) + 4
//   adjacent cells of the level's row; a lane owns one (level, cell) and GATHERS the taps that fall on it in tap order (no atomic,
//   neither in LDS nor in global memory; the same order every run).  Then the wave writes the pixel's row once: folded,
//   G[x'] = g_0[x'] + sum_i 2^-i g_i[x' >> i] evaluated as the pooling chain's own backward ((.. + g_2) / 2 + g_1) / 2 + g_0
//   (fold = 1, what the build's backward wants), or level by level in the pyramid's layout (fold = 0, the gradient with respect
//   to a free pyramid).  grad_disp: a lane per tap, reduced over the wave in a fixed order.
// ts_raft_corr_pyramid_bwd   grad_fmap1[c][x] = sum_x' G[x][x'] fmap2[c][x'] / sqrt(C), grad_fmap2[c][x'] = sum_x G[x][x'] fmap1[c][x]
//   / sqrt(C): a workgroup owns 64 channels by 64 positions of one image row, 32-wide slices of the contraction staged in LDS, the
//   same MFMA; every output is written once (deterministic).  A cotangent that still has its levels (levels > 1) is folded while it
//   is staged.
#include <cmath>

#include "corr_common.hpp"

namespace {

using namespace corr;          // v4f, RKC, RPM, kMaxLevels, Levels, pow2_neg, mfma_chunk, store_tile, grid_blocks

constexpr int RT = 64;           // tile edge: pixels x and x' per workgroup
// LDS pitches by the bank arithmetic of corr_common.hpp (RPM, the pitch of a [64][k] operand image, is there).  Not measured.
constexpr int RPK = 80;          // pitch of a [k][64] operand image: bank 16 kq + j (80 == 16 mod 32), disjoint within a half
constexpr int RPO = 68;          // pitch of the output tile: a store of the accumulators hits bank 16 kq + j (4 * 68 == 16 mod 32)

struct Raft : Levels {           // off[i]: float offset of level i in the pyramid buffer
  int B, C, H, W, L, r;
};

void level_offsets(Raft& p) {
  corr::level_offsets(p, static_cast<size_t>(p.B) * p.H * p.W, [&](int i) { return p.W >> i; });
}

// Position of tap k of level i in the level's row, the reference's fp32 sequence: x - d, / 2^i, + (k - r), * 2 / (W - 1) - 1, then
// grid_sample's ((g + 1) * W_i - 1) / 2.  The clamp keeps the conversion to int defined: every position it moves has both taps
// outside the row either way (a non-finite disparity lands on -2).
__device__ __forceinline__ float raft_position(int x, float d, int i, int k, int r, float Wm1, float Wi) {
  float t = __fsub_rn(static_cast<float>(x), d);
  t = __fmul_rn(t, pow2_neg(i));
  t = __fadd_rn(t, static_cast<float>(k - r));
  const float g = __fsub_rn(__fdiv_rn(__fmul_rn(2.f, t), Wm1), 1.f);
  const float ix = __fdiv_rn(__fsub_rn(__fmul_rn(__fadd_rn(g, 1.f), Wi), 1.f), 2.f);
  return fminf(fmaxf(ix, -2.f), Wi + 1.f);
}

// ------------------------------------------------------------------------------------------------------------- pyramid, forward
__global__ void __launch_bounds__(256)
raft_pyramid_fwd_kernel(const float* __restrict__ f1, const float* __restrict__ f2, float* __restrict__ pyr, const Raft p,
                        float sqrtC, int strips) {
  __shared__ __attribute__((aligned(16))) float lds[2 * RKC * RPK];     // both strips of a chunk; afterwards the output tile [64][RPO]
  __shared__ __attribute__((aligned(16))) float sP[RT * RT];            // pooled levels [64][64]: level i >= 1 at column 64 - (128 >> i)
  static_assert(RT * RPO <= 2 * RKC * RPK, "the output tile lives over the input strips");
  float* sA = lds;
  float* sB = lds + RKC * RPK;
  float* sO = lds;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 15, kq = lane >> 4;
  long long blk = blockIdx.x;
  const int sp = static_cast<int>(blk % strips); blk /= strips;
  const int sx = static_cast<int>(blk % strips);
  const size_t row = static_cast<size_t>(blk / strips);                 // b * H + y
  const int b = static_cast<int>(row / p.H), y = static_cast<int>(row % p.H);
  const int x0 = sx * RT, xp0 = sp * RT;
  const size_t HW = static_cast<size_t>(p.H) * p.W;
  const float* A = f1 + static_cast<size_t>(b) * p.C * HW + static_cast<size_t>(y) * p.W;
  const float* Bm = f2 + static_cast<size_t>(b) * p.C * HW + static_cast<size_t>(y) * p.W;
  const int col = tid & 63, cb = tid >> 6;
  const bool okA = x0 + col < p.W, okB = xp0 + col < p.W;
  const int ca = okA ? x0 + col : 0, cbm = okB ? xp0 + col : 0;
  v4f acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = v4f{0.f, 0.f, 0.f, 0.f};

#pragma unroll 1
  for (int c0 = 0; c0 < p.C; c0 += RKC) {
    __syncthreads();                       // the previous chunk's fragments have been read
#pragma unroll
    for (int m = 0; m < RKC / 4; ++m) {
      const int c = c0 + cb + 4 * m;
      const bool okc = c < p.C;
      const size_t co = static_cast<size_t>(okc ? c : 0) * HW;
      const float va = A[co + ca], vb = Bm[co + cbm];
      sA[(cb + 4 * m) * RPK + col] = (okc && okA) ? va : 0.f;
      sB[(cb + 4 * m) * RPK + col] = (okc && okB) ? vb : 0.f;
    }
    __syncthreads();
    const int ksteps = min(RKC / 4, (p.C - c0 + 3) / 4);
    mfma_chunk<RPK, RPK, 4>(acc, sA, 16 * wave, sB, 0, ksteps, j, kq);
  }
  // ---- the tile, divided by sqrt(C), into LDS: a lane of an accumulator holds x' = j of four pixels
  __syncthreads();
  store_tile<RPO, 4>(sO, acc, 16 * wave, 0, sqrtC, j, kq);
  __syncthreads();
  // ---- level 0: a wave store is one pixel's 64 consecutive x'
  const size_t n0 = row * p.W + x0;
#pragma unroll 4
  for (int m = 0; m < RT / 4; ++m) {
    const int rr = cb + 4 * m;
    if (x0 + rr < p.W && okB) pyr[(n0 + rr) * p.W + xp0 + col] = sO[rr * RPO + col];
  }
  // ---- levels 1..L-1, each from the rounded level below
  const float* src = sO;
  int spitch = RPO;
  for (int i = 1; i < p.L; ++i) {
    const int wi = RT >> i, Wi = p.W >> i, cbase = xp0 >> i;
    float* dst = sP + (RT - (2 * RT >> i));
    float* lvl = pyr + p.off[i];
    for (int idx = tid; idx < RT * wi; idx += 256) {
      const int rr = idx >> (6 - i), m = idx & (wi - 1);
      const float v = (src[rr * spitch + 2 * m] + src[rr * spitch + 2 * m + 1]) * 0.5f;
      dst[rr * RT + m] = v;
      if (x0 + rr < p.W && cbase + m < Wi) lvl[(n0 + rr) * Wi + cbase + m] = v;
    }
    __syncthreads();
    src = dst;
    spitch = RT;
  }
}

// -------------------------------------------------------------------------------------------------------------- lookup, forward
__global__ void __launch_bounds__(256)
raft_lookup_fwd_kernel(const float* __restrict__ pyr, const float* __restrict__ disp, float* __restrict__ out, const Raft p) {
  const long long total = static_cast<long long>(p.B) * p.L * p.H * p.W;
  const long long idx = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int x = static_cast<int>(idx % p.W);
  long long t = idx / p.W;
  const int y = static_cast<int>(t % p.H); t /= p.H;
  const int i = static_cast<int>(t % p.L), b = static_cast<int>(t / p.L);
  const size_t HW = static_cast<size_t>(p.H) * p.W;
  const size_t pix = static_cast<size_t>(b) * HW + static_cast<size_t>(y) * p.W + x;
  const float d = disp[pix];
  const int Wi = p.W >> i, K = 2 * p.r + 1;
  const float Wif = static_cast<float>(Wi), Wm1 = static_cast<float>(p.W - 1), wy = 1.f - pow2_neg(i + 1);
  const float* rowp = pyr + p.off[i] + pix * Wi;
  float* op = out + (static_cast<size_t>(b) * p.L * K + static_cast<size_t>(i) * K) * HW + static_cast<size_t>(y) * p.W + x;
  for (int k = 0; k < K; ++k) {
    const float ix = raft_position(x, d, i, k, p.r, Wm1, Wif);
    const float ixf = floorf(ix);
    const int ix0 = static_cast<int>(ixf);
    const float w0 = __fmul_rn(__fsub_rn(__fadd_rn(ixf, 1.f), ix), wy), w1 = __fmul_rn(__fsub_rn(ix, ixf), wy);
    const float l0 = rowp[min(max(ix0, 0), Wi - 1)], l1 = rowp[min(max(ix0 + 1, 0), Wi - 1)];
    const float v0 = (ix0 >= 0 && ix0 < Wi) ? l0 : 0.f, v1 = (ix0 + 1 >= 0 && ix0 + 1 < Wi) ? l1 : 0.f;
    op[static_cast<size_t>(k) * HW] = v0 * w0 + v1 * w1;
  }
}

// ------------------------------------------------------------------------------------------------------------- lookup, backward
__global__ void __launch_bounds__(256)
raft_lookup_bwd_kernel(const float* __restrict__ pyr, const float* __restrict__ disp, const float* __restrict__ go,
                       float* __restrict__ gdisp, float* __restrict__ gpyr, const Raft p, int cw, int fold) {
  extern __shared__ __attribute__((aligned(16))) float cells_all[];      // per wave: [L][cw] cell sums, then [L] first cells (int)
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const size_t npix = static_cast<size_t>(p.B) * p.H * p.W;
  const size_t pix_raw = static_cast<size_t>(blockIdx.x) * 4 + wave;
  const bool live = pix_raw < npix;                                      // a wave past the end works on the last pixel and stores nothing
  const size_t pix = live ? pix_raw : npix - 1;
  const size_t HW = static_cast<size_t>(p.H) * p.W;
  const int x = static_cast<int>(pix % p.W), y = static_cast<int>((pix / p.W) % p.H), b = static_cast<int>(pix / HW);
  const int K = 2 * p.r + 1, ntap = p.L * K;
  const float d = disp[pix], Wm1 = static_cast<float>(p.W - 1);
  float* my = cells_all + wave * (p.L * cw + p.L);
  int* first = reinterpret_cast<int*>(my + p.L * cw);
  const float* gop = go + static_cast<size_t>(b) * ntap * HW + static_cast<size_t>(y) * p.W + x;      // + channel * HW

  // ---- a lane per (level, cell): the taps that fall on the cell, gathered in tap order (only when the pyramid's cotangent is wanted)
  for (int e = lane; gpyr != nullptr && e < p.L * cw; e += 64) {
    const int i = e / cw, jj = e - i * cw, Wi = p.W >> i;
    const float Wif = static_cast<float>(Wi), wy = 1.f - pow2_neg(i + 1);
    const int m0 = static_cast<int>(floorf(raft_position(x, d, i, 0, p.r, Wm1, Wif)));
    const int m = m0 + jj;
    float s = 0.f;
    for (int k = 0; k < K; ++k) {
      const float ix = raft_position(x, d, i, k, p.r, Wm1, Wif);
      const float ixf = floorf(ix);
      const int ix0 = static_cast<int>(ixf);
      const float w0 = __fmul_rn(__fsub_rn(__fadd_rn(ixf, 1.f), ix), wy), w1 = __fmul_rn(__fsub_rn(ix, ixf), wy);
      const float g = gop[static_cast<size_t>(i * K + k) * HW];
      s += (ix0 == m ? g * w0 : 0.f) + (ix0 + 1 == m ? g * w1 : 0.f);
    }
    my[e] = (m >= 0 && m < Wi) ? s : 0.f;                                // a cell outside the row: zero padding, dropped
    if (jj == 0) first[i] = m0;
  }
  // ---- grad_disp: a lane per tap, d out / d disp = g * wy * (v1 - v0) * d ix / d disp, d ix / d disp = -W_i / (2^i (W - 1))
  if (gdisp != nullptr) {
    float part = 0.f;
    for (int tt = lane; tt < ntap; tt += 64) {
      const int i = tt / K, k = tt - i * K, Wi = p.W >> i;
      const float Wif = static_cast<float>(Wi), wy = 1.f - pow2_neg(i + 1);
      const float ix = raft_position(x, d, i, k, p.r, Wm1, Wif);
      const int ix0 = static_cast<int>(floorf(ix));
      const float* rowp = pyr + p.off[i] + pix * Wi;
      const float l0 = rowp[min(max(ix0, 0), Wi - 1)], l1 = rowp[min(max(ix0 + 1, 0), Wi - 1)];
      const float v0 = (ix0 >= 0 && ix0 < Wi) ? l0 : 0.f, v1 = (ix0 + 1 >= 0 && ix0 + 1 < Wi) ? l1 : 0.f;
      const float dscale = -(Wif * pow2_neg(i)) / Wm1;
      part += gop[static_cast<size_t>(tt) * HW] * wy * (v1 - v0) * dscale;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) part += __shfl_xor(part, o);
    if (lane == 0 && live) gdisp[pix] = part;
  }
  __syncthreads();
  if (gpyr == nullptr || !live) return;
  // ---- the pixel's row(s), written once
  if (fold) {
    float* grow = gpyr + pix * p.W;
    for (int xp = lane; xp < p.W; xp += 64) {
      float v = 0.f;
      for (int i = p.L - 1; i >= 1; --i) {
        const int m = xp >> i, jj = m - first[i];
        const float c = my[i * cw + min(max(jj, 0), cw - 1)];
        v = (v + ((m < (p.W >> i) && jj >= 0 && jj < cw) ? c : 0.f)) * 0.5f;
      }
      const int jj = xp - first[0];
      const float c = my[min(max(jj, 0), cw - 1)];
      grow[xp] = v + ((jj >= 0 && jj < cw) ? c : 0.f);
    }
  } else {
    for (int i = 0; i < p.L; ++i) {
      const int Wi = p.W >> i;
      float* grow = gpyr + p.off[i] + pix * Wi;
      for (int m = lane; m < Wi; m += 64) {
        const int jj = m - first[i];
        const float c = my[i * cw + min(max(jj, 0), cw - 1)];
        grow[m] = (jj >= 0 && jj < cw) ? c : 0.f;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------------------ pyramid, backward
// Element (n, xp) of the level-0 cotangent: of a cotangent that still has its levels, the pooling chain's backward.
__device__ __forceinline__ float cotangent0(const float* __restrict__ gpyr, const Raft& p, size_t n, int xp) {
  float v = 0.f;
  for (int i = p.L - 1; i >= 1; --i) {
    const int Wi = p.W >> i, m = xp >> i;
    const float c = gpyr[p.off[i] + n * Wi + min(m, Wi - 1)];
    v = (v + (m < Wi ? c : 0.f)) * 0.5f;
  }
  return v + gpyr[n * p.W + xp];
}

// SECOND = false: grad_fmap1[c][x] = sum_x' G[x][x'] F[c][x'] (F = fmap2); true: grad_fmap2[c][x'] = sum_x G[x][x'] F[c][x] (F = fmap1).
// M = 16 channels per wave, N = 64 positions in four tiles, the contraction in 32-wide slices.
template <bool SECOND>
__global__ void __launch_bounds__(256)
raft_pyramid_bwd_kernel(const float* __restrict__ gpyr, const float* __restrict__ F, float* __restrict__ grad, const Raft p,
                        float sqrtC, int strips, int cgroups) {
  __shared__ __attribute__((aligned(16))) float sF[RT * RPM];                               // [channel][k]
  __shared__ __attribute__((aligned(16))) float sG[SECOND ? RKC * RPK : RT * RPM];          // [k][position] resp. [position][k]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 15, kq = lane >> 4;
  long long blk = blockIdx.x;
  const int sp = static_cast<int>(blk % strips); blk /= strips;
  const int cg = static_cast<int>(blk % cgroups);
  const size_t row = static_cast<size_t>(blk / cgroups);                 // b * H + y
  const int b = static_cast<int>(row / p.H), y = static_cast<int>(row % p.H);
  const int pos0 = sp * RT, c0 = cg * RT;
  const size_t HW = static_cast<size_t>(p.H) * p.W;
  const float* Fr = F + static_cast<size_t>(b) * p.C * HW + static_cast<size_t>(y) * p.W;
  const size_t nrow = row * p.W;
  v4f acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = v4f{0.f, 0.f, 0.f, 0.f};

#pragma unroll 1
  for (int k0 = 0; k0 < p.W; k0 += RKC) {
    __syncthreads();
    {
      const int kk = tid & 31, k = k0 + kk;
#pragma unroll
      for (int m = 0; m < 8; ++m) {
        const int cc = (tid >> 5) + 8 * m, c = c0 + cc;
        const bool ok = c < p.C && k < p.W;
        const float v = Fr[static_cast<size_t>(ok ? c : 0) * HW + (ok ? k : 0)];
        sF[cc * RPM + kk] = ok ? v : 0.f;
      }
      if (!SECOND) {
#pragma unroll
        for (int m = 0; m < 8; ++m) {
          const int pp = (tid >> 5) + 8 * m, pos = pos0 + pp;
          const bool ok = pos < p.W && k < p.W;
          const float v = cotangent0(gpyr, p, nrow + (ok ? pos : 0), ok ? k : 0);
          sG[pp * RPM + kk] = ok ? v : 0.f;
        }
      }
    }
    if (SECOND) {
      const int pp = tid & 63, pos = pos0 + pp;
#pragma unroll
      for (int m = 0; m < 8; ++m) {
        const int kk = (tid >> 6) + 4 * m, k = k0 + kk;
        const bool ok = pos < p.W && k < p.W;
        const float v = cotangent0(gpyr, p, nrow + (ok ? k : 0), ok ? pos : 0);
        sG[kk * RPK + pp] = ok ? v : 0.f;
      }
    }
    __syncthreads();
    const int ksteps = min(RKC / 4, (p.W - k0 + 3) / 4);
#pragma unroll
    for (int q = 0; q < RKC / 4; ++q) {
      if (q < ksteps) {
        const float a = sF[(16 * wave + j) * RPM + 4 * q + kq];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const float bv = SECOND ? sG[(4 * q + kq) * RPK + 16 * t + j] : sG[(16 * t + j) * RPM + 4 * q + kq];
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bv, acc[t], 0, 0, 0);
        }
      }
    }
  }
  // a lane of an accumulator holds position j of four channels: 64-byte runs along the row
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int c = c0 + 16 * wave + 4 * kq + r, pos = pos0 + 16 * t + j;
      if (c < p.C && pos < p.W)
        grad[(static_cast<size_t>(b) * p.C + c) * HW + static_cast<size_t>(y) * p.W + pos] = __fdiv_rn(acc[t][r], sqrtC);
    }
}

int check(const Raft& p, bool with_c, bool with_r) {
  TS_REQUIRE(p.B > 0 && p.H > 0 && p.W > 0 && (!with_c || p.C > 0), TS_ERR_SHAPE, "raft_corr: non-positive size");
  TS_REQUIRE(p.W >= 2, TS_ERR_SHAPE, "raft_corr: W = %d, need W >= 2 (the lookup divides by W - 1)", p.W);
  TS_REQUIRE(p.L >= 1, TS_ERR_SHAPE, "raft_corr: num_levels = %d, need >= 1", p.L);
  TS_REQUIRE(!with_r || p.r >= 0, TS_ERR_SHAPE, "raft_corr: radius = %d, need >= 0", p.r);
  TS_REQUIRE(p.L <= kMaxLevels, TS_ERR_UNSUPPORTED, "raft_corr: num_levels = %d, this build pools at most %d levels", p.L, kMaxLevels);
  TS_REQUIRE(!with_r || p.r <= 1024, TS_ERR_UNSUPPORTED, "raft_corr: radius = %d, this build takes at most 1024", p.r);
  TS_REQUIRE((p.W >> (p.L - 1)) >= 1, TS_ERR_SHAPE, "raft_corr: W = %d is too narrow for %d levels (level %d would be empty)", p.W,
             p.L, p.L - 1);
  return TS_OK;
}

}  // namespace

extern "C" int ts_raft_corr_pyramid_fwd(const float* fmap1, const float* fmap2, float* pyramid, int B, int C, int H, int W,
                                        int num_levels, void* stream) {
  Raft p{{}, B, C, H, W, num_levels, 0};
  if (int rc = check(p, true, false)) return rc;
  TS_REQUIRE_PTR(fmap1); TS_REQUIRE_PTR(fmap2); TS_REQUIRE_PTR(pyramid);
  level_offsets(p);
  const int strips = (W + RT - 1) / RT;
  const unsigned blocks = grid_blocks(static_cast<unsigned long long>(B) * H * strips * strips);
  TS_REQUIRE(blocks != 0, TS_ERR_UNSUPPORTED, "raft_corr_pyramid_fwd: grid too large");
  hipLaunchKernelGGL(raft_pyramid_fwd_kernel, dim3(blocks), dim3(256), 0, ts::as_stream(stream), fmap1, fmap2, pyramid, p,
                     sqrtf(static_cast<float>(C)), strips);
  return ts::launched("raft_pyramid_fwd_kernel");
}

extern "C" int ts_raft_corr_lookup_fwd(const float* pyramid, const float* disp, float* out, int B, int H, int W, int num_levels,
                                       int radius, void* stream) {
  Raft p{{}, B, 0, H, W, num_levels, radius};
  if (int rc = check(p, false, true)) return rc;
  TS_REQUIRE_PTR(pyramid); TS_REQUIRE_PTR(disp); TS_REQUIRE_PTR(out);
  level_offsets(p);
  const unsigned long long total = static_cast<unsigned long long>(B) * num_levels * H * W;
  const unsigned blocks = grid_blocks((total + 255) / 256);
  TS_REQUIRE(blocks != 0, TS_ERR_UNSUPPORTED, "raft_corr_lookup_fwd: grid too large");
  hipLaunchKernelGGL(raft_lookup_fwd_kernel, dim3(blocks), dim3(256), 0, ts::as_stream(stream), pyramid, disp, out, p);
  return ts::launched("raft_lookup_fwd_kernel");
}

extern "C" int ts_raft_corr_lookup_bwd(const float* pyramid, const float* disp, const float* grad_out, float* grad_disp,
                                       float* grad_pyramid, int B, int H, int W, int num_levels, int radius, int fold, void* stream) {
  Raft p{{}, B, 0, H, W, num_levels, radius};
  if (int rc = check(p, false, true)) return rc;
  TS_REQUIRE_PTR(disp); TS_REQUIRE_PTR(grad_out);
  TS_REQUIRE(grad_disp != nullptr || grad_pyramid != nullptr, TS_ERR_NULL, "raft_corr_lookup_bwd: grad_disp and grad_pyramid are both NULL");
  if (grad_disp != nullptr) TS_REQUIRE_PTR(pyramid);
  level_offsets(p);
  // cells a level's taps can touch: the positions of tap 0 and tap 2r lie 2r W_i / (W - 1) <= 2r W / (W - 1) apart, their floors at
  // most one more, the right tap of the last one more, and one spare for the roundings of the position
  const int cw = static_cast<int>(2.0 * radius * W / (W - 1.0)) + 4;
  const size_t shm = 4 * static_cast<size_t>(num_levels) * (cw + 1) * sizeof(float);
  TS_REQUIRE(shm <= 64 * 1024, TS_ERR_UNSUPPORTED, "raft_corr_lookup_bwd: radius = %d needs %zu bytes of LDS", radius, shm);
  const unsigned long long npix = static_cast<unsigned long long>(B) * H * W;
  const unsigned blocks = grid_blocks((npix + 3) / 4);
  TS_REQUIRE(blocks != 0, TS_ERR_UNSUPPORTED, "raft_corr_lookup_bwd: grid too large");
  hipLaunchKernelGGL(raft_lookup_bwd_kernel, dim3(blocks), dim3(256), shm, ts::as_stream(stream), pyramid, disp, grad_out,
                     grad_disp, grad_pyramid, p, cw, fold != 0);
  return ts::launched("raft_lookup_bwd_kernel");
}

extern "C" int ts_raft_corr_pyramid_bwd(const float* grad_pyramid, const float* fmap1, const float* fmap2, float* grad_fmap1,
                                        float* grad_fmap2, int B, int C, int H, int W, int levels, void* stream) {
  Raft p{{}, B, C, H, W, levels, 0};
  if (int rc = check(p, true, false)) return rc;
  TS_REQUIRE_PTR(grad_pyramid);
  TS_REQUIRE(grad_fmap1 != nullptr || grad_fmap2 != nullptr, TS_ERR_NULL, "raft_corr_pyramid_bwd: grad_fmap1 and grad_fmap2 are both NULL");
  if (grad_fmap1 != nullptr) TS_REQUIRE_PTR(fmap2);
  if (grad_fmap2 != nullptr) TS_REQUIRE_PTR(fmap1);
  level_offsets(p);
  const int strips = (W + RT - 1) / RT, cgroups = (C + RT - 1) / RT;
  const unsigned blocks = grid_blocks(static_cast<unsigned long long>(B) * H * strips * cgroups);
  TS_REQUIRE(blocks != 0, TS_ERR_UNSUPPORTED, "raft_corr_pyramid_bwd: grid too large");
  const float sc = sqrtf(static_cast<float>(C));
  hipStream_t st = ts::as_stream(stream);
  if (grad_fmap1 != nullptr) {
    hipLaunchKernelGGL(raft_pyramid_bwd_kernel<false>, dim3(blocks), dim3(256), 0, st, grad_pyramid, fmap2, grad_fmap1, p, sc, strips, cgroups);
    if (int rc = ts::launched("raft_pyramid_bwd_kernel<fmap1>")) return rc;
  }
  if (grad_fmap2 != nullptr) {
    hipLaunchKernelGGL(raft_pyramid_bwd_kernel<true>, dim3(blocks), dim3(256), 0, st, grad_pyramid, fmap1, grad_fmap2, p, sc, strips, cgroups);
    if (int rc = ts::launched("raft_pyramid_bwd_kernel<fmap2>")) return rc;
  }
  return TS_OK;
}
