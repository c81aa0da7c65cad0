// What the two correlation pyramids share (raft_corr.hip: CorrBlock, rows of one image line; flow_corr.hip: FlowCorrBlock, rows of
// the whole image): the level offsets of the one pyramid buffer, 2^-i, and the staging / contraction of an fp32 MFMA tile.
#pragma once
#include "ts_common.hpp"

namespace corr {

typedef float v4f __attribute__((ext_vector_type(4)));

constexpr int RKC = 32;          // contraction elements per staged chunk
// LDS pitches.  A 4-byte LDS read or write is served per 32-lane half over banks (address / 4) mod 32; a fragment read has lane
// (j = lane & 15, kq = lane >> 4), so a half holds j = 0..15 and two values of kq.  Not measured: the bank arithmetic only.
//   a [k][columns] operand image wants a pitch == 16 mod 32: bank 16 kq + j, disjoint within a half
//   a [rows][k] operand image wants a pitch == 2 mod 32:     bank 2 j + kq, disjoint within a half
//   an output tile wants 4 * pitch == 16 mod 32:             a store of the accumulators hits bank 16 kq + j
constexpr int RPM = 34;          // pitch of a [64][k] operand image
constexpr int kMaxLevels = 7;    // levels a pyramid buffer can hold (64 >> 6 == 1: the deepest level a 64-wide tile still pools by itself)

// Float offset of level i in the pyramid buffer: level i is [rows][len_i] contiguous, stored after the levels before it.
struct Levels {
  size_t off[kMaxLevels];
};

template <class Len>
inline void level_offsets(Levels& lv, size_t rows, Len len) {
  size_t o = 0;
  for (int i = 0; i < kMaxLevels; ++i) {
    lv.off[i] = o;
    o += rows * static_cast<size_t>(len(i));
  }
}

__device__ __forceinline__ float pow2_neg(int i) { return __int_as_float((127 - i) << 23); }      // 2^-i, exact

// One staged chunk of a k-major pair of operand images (sA [k][PA], sB [k][PB]) into NT accumulators of a wave:
// acc[t] += A[:, acol .. acol+15]^T B[:, bcol + 16 t .. + 15], `ksteps` steps of 4 along k.  v_mfma_f32_16x16x4_f32: a lane gives
// A[k = kq][row j] and B[k = kq][column j], and holds rows 4 kq .. 4 kq + 3 of column j of the tile.
template <int PA, int PB, int NT>
__device__ __forceinline__ void mfma_chunk(v4f (&acc)[NT], const float* sA, int acol, const float* sB, int bcol, int ksteps, int j,
                                           int kq) {
#pragma unroll
  for (int q = 0; q < RKC / 4; ++q) {
    if (q < ksteps) {
      const float a = sA[(4 * q + kq) * PA + acol + j];
#pragma unroll
      for (int t = 0; t < NT; ++t)
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, sB[(4 * q + kq) * PB + bcol + 16 * t + j], acc[t], 0, 0, 0);
    }
  }
}

// The accumulators of a wave, divided by `div`, into an output tile in LDS (pitch PO): row row0 + 4 kq + r, column col0 + 16 t + j.
template <int PO, int NT>
__device__ __forceinline__ void store_tile(float* sO, const v4f (&acc)[NT], int row0, int col0, float div, int j, int kq) {
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) sO[(row0 + 4 * kq + r) * PO + col0 + 16 * t + j] = __fdiv_rn(acc[t][r], div);
}

// blocks of a 1-D grid, or 0 when they do not fit one
inline unsigned grid_blocks(unsigned long long n) { return n < 0x7fffffffull ? static_cast<unsigned>(n) : 0u; }

}  // namespace corr
