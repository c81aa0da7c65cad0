// Device-side pieces shared by the convolution kernels (conv3d.hip, conv_x6s.hip): activation codes, the launch
// descriptor, buffer-resource helper and the fp32 -> three-bf16 split of the "x6" kernels.
#pragma once
#include "act_fast.hpp"
#include "ts_common.hpp"

namespace {

enum Act { ACT_NONE = 0, ACT_SILU = 1, ACT_RELU = 2, ACT_TANH_OFFSET = 3, ACT_HEAD_PAIR = 4 };

// co: output channel (only ACT_HEAD_PAIR looks at it: channel 0 = the cost head, no activation; channel 1 =
// the offset head -- both prediction heads as one block-diagonal convolution)
__device__ __forceinline__ float apply_act(float v, int act, float p, int co = 0) {
  if (act == ACT_HEAD_PAIR) act = co == 0 ? ACT_NONE : ACT_TANH_OFFSET;
  switch (act) {
    case ACT_SILU: return silu_fast(v);
    case ACT_RELU: return fmaxf(v, 0.f);
    // PredictionHeads.regress_offset (module.py:384-390): tanh(x/100).clamp(-1,1) * delta
    case ACT_TANH_OFFSET: return fminf(fmaxf(tanhf(v / 100.f), -1.f), 1.f) * p;
    default: return v;
  }
}

typedef float v4f __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
enum { MODE_HW = 0, MODE_HWT = 1, MODE_D = 2 };
constexpr unsigned kOOB = 0x80000000u;   // buffer offset past every num_records we allow: the load returns 0

struct IG {
  int Cin, Cout, coutp;         // coutp: padded channel count of the weight / scale / shift arrays
  int D, H, W;                  // input: planes per channel, plane geometry
  int Do, Ho, Wo;               // output
  int stride, dil, pad, k, transposed;
  int act;
  float act_param;
  long long in_bstride, in_cstride, out_bstride, out_cstride;
  unsigned in_bytes, w_bytes;   // extent of one batch element of x / of the weight array (buffer range checks)
  unsigned out_bytes, part_bytes;   // ... of one batch element of y / of one (slice, batch) block of the partials
  int tiles_x, co_groups;
  int ksplit, kspan;            // split-K: this many slices of `kspan` input channels each (partials -> workspace)
  float* partial;               // [ksplit][B][Cout][Do*Ho*Wo] raw sums when ksplit > 1
  int B;
  const float* addend;          // [B][Cout][Ho*Wo] added to every depth plane's sum before scale/shift (or null);
  long long add_bstride;        // add_dstride != 0: one term per depth plane, [B][Cout][D][Ho*Wo] (ts_conv3d_hw_warp_fwd)
  long long add_cstride, add_dstride;
  int xcd;                      // XCD-banded workgroup order (ig_conv_kernel)
  // split input (the *_split_fwd entries): channels [0, csplit) are read from x, channels [csplit, Cin) from x2, which has its own
  // batch / channel strides and its own extent.  csplit is a multiple of every K-chunk size (32), so a chunk lies on one side of
  // the seam and the choice of base is ONE uniform select per chunk.  No second base: x2 == x with x's strides and csplit = INT_MAX.
  const float* x2;
  int csplit;
  long long in2_bstride, in2_cstride;
  unsigned in2_bytes;
};

// The base of one K chunk of a (possibly split) input: descriptor, channel stride in bytes and the channel the base starts at --
// all wave-uniform (chunk index and kernel arguments only), so they stay in scalar registers.
struct ChunkBase {
  __amdgpu_buffer_rsrc_t rsrc;
  unsigned cstride_b;
  int c_first;
};
__device__ __forceinline__ ChunkBase chunk_base(int c0, int csplit, __amdgpu_buffer_rsrc_t r1, __amdgpu_buffer_rsrc_t r2, unsigned cs1,
                                                unsigned cs2) {
  const bool second = c0 >= csplit;
  return ChunkBase{second ? r2 : r1, second ? cs2 : cs1, second ? csplit : 0};
}

__device__ __forceinline__ __amdgpu_buffer_rsrc_t ig_rsrc(const void* base, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, bytes, 0x00020000);
}

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned pack_bf16(float a, float b) {
  return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{a, b}, bf16x2));      // v_cvt_pk_bf16_f32 (RNE)
}
// (a, b) -> packed (hi, mid, lo) parts
__device__ __forceinline__ void split6(float a, float b, unsigned& hi, unsigned& mid, unsigned& lo) {
  hi = pack_bf16(a, b);
  a -= __uint_as_float(hi << 16); b -= __uint_as_float(hi & 0xffff0000u);
  mid = pack_bf16(a, b);
  a -= __uint_as_float(mid << 16); b -= __uint_as_float(mid & 0xffff0000u);
  lo = pack_bf16(a, b);
}

}  // namespace
