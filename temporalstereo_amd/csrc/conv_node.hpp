// What surrounds the two fp32-MFMA cores (conv_hw3.hpp, conv_pw1.hpp) in every 2-D node -- conv_gru.hip, feature_decoder.hip, mbconv.hip,
// fused_mbconv.hip -- and is the same in all of them: the shared constants, a strided plane operand with its host checks, the affine
// epilogue, and the host sequence of a node entry.
#pragma once
#include <initializer_list>
#include <type_traits>

#include "conv_common.hpp"

namespace node {

constexpr int kMaxAxis = 1 << 20;
constexpr int kGridCap = 4096;               // blocks of the grid-stride layout and element kernels

inline int pitch_for(int rows) { return rows <= 64 ? 64 : (rows + 127) / 128 * 128; }      // global pitch of a weight row: whole workgroups of any MT

// ------------------------------------------------------------------------------------------------------------------ operands
// A strided [B][C][plane] operand as a kernel reads or writes it.
template <class T>
struct Plane {
  T* p;
  long long bs, cs;
  __device__ __forceinline__ T* at(int b, long long pix) const { return p + b * bs + pix; }
};

// The same operand as a host check sees it.  C == 0: the operand is absent (an optional residual, a memory that is not there, a resize
// source of no channels) -- nothing of it is looked at, its pointer included.
enum Role { IN, RES, OUT };
struct Operand {
  const char* name;
  const float* p;
  int C;
  long long vol, bs, cs;
  Role role;
  Plane<const float> plane() const { return {p, bs, cs}; }
};
struct Pointer {
  const char* name;
  const void* p;
};

// every element the kernels touch lies inside what the strides describe (ts::strides_ok)
inline int check_strides(const char* who, int B, std::initializer_list<Operand> ops) {
  for (const Operand& o : ops)
    TS_REQUIRE(ts::strides_ok(B, o.C, o.vol, o.bs, o.cs), TS_ERR_SHAPE, "%s: %s strides %lld / %lld overlap", who, o.name, o.bs, o.cs);
  return TS_OK;
}

// Whether the bounding extents [p, p + (B - 1) bs + (C - 1) cs + vol) of two operands are apart.  The test is on extents, not elements:
// two interleaved channel slices of one wider buffer are refused although no element is shared.
inline bool disjoint(const Operand& a, const Operand& b, int B) {
  const float* ae = a.p + (B - 1) * a.bs + (a.C - 1) * a.cs + a.vol;
  const float* be = b.p + (B - 1) * b.bs + (b.C - 1) * b.cs + b.vol;
  return ae <= b.p || be <= a.p;
}

// The overlap rules of an output: it lies apart from every input (other workgroups read what a workgroup would overwrite), and a
// residual is either the output's own elements (the in-place residual: an element is read by the thread that writes it) or apart.
// The operands are looked at in the order they are listed.
inline int check_overlap(const char* who, int B, std::initializer_list<Operand> ops) {
  for (const Operand& y : ops) {
    if (y.role != OUT) continue;
    for (const Operand& o : ops) {
      if (o.role == OUT || o.C == 0) continue;
      if (o.role == IN)
        TS_REQUIRE(disjoint(o, y, B), TS_ERR_SHAPE, "%s: %s overlaps %s (read by other workgroups than the one that writes it)", who, y.name, o.name);
      else
        TS_REQUIRE((o.p == y.p && o.bs == y.bs && o.cs == y.cs) || disjoint(o, y, B), TS_ERR_SHAPE,
                   "%s: %s overlaps the %s without being its own elements", who, y.name, o.name);
    }
  }
  return TS_OK;
}

// ------------------------------------------------------------------------------------------------------------------ epilogue
// y = act(sum * scale + shift) + residual: scale / shift may be NULL (1 / 0), act is ACT_NONE | ACT_SILU, the residual may be absent
// (res.p NULL).  Runtime fields by default.  ACT / RES other than kRuntime are the compile-time answer of a use that knows it (ACT: the
// activation code; RES = 1: a residual is always there, 0: never): the projections and the expansion take them -- with runtime fields
// project_kernel<2> held 137 VGPRs against the parent's 135 (profiles/nodes_kernel_resources.txt) and the block's batch-8 eval row at
// 128 -> 512 was 1-3 us above the parent's (profiles/nodes_refactor_bench.txt).  The decoder and the 3x3 keep runtime fields.
// Observed, not understood: with Dec's and Conv3's Affine placed behind their scalar fields, decoder_conv_kernel<2> and
// conv3x3_kernel<2, 2> were allocated more registers and lost a resident wave; every problem type here keeps its Affine ahead of them.
// The writer holds copies of what it uses, never `this`: a store through y then cannot be taken to change a field.
constexpr int kRuntime = -1;
template <int ACT = kRuntime, int RES = kRuntime>
struct Affine {
  const float* scale;
  const float* shift;
  int act;
  Plane<const float> res;
  Plane<float> y;

  __device__ __forceinline__ auto writer(int b, long long pix) const {
    return [py = y.at(b, pix), pr = (RES == 1 || (RES != 0 && res.p)) ? res.at(b, pix) : nullptr, y_cs = y.cs, r_cs = res.cs, scale = scale, shift = shift,
            act = act](int row, float v) {
      if (scale) v *= scale[row];
      if (shift) v += shift[row];
      if (ACT == kRuntime ? act == ACT_SILU : ACT == ACT_SILU) v = silu_fast(v);
      if (RES == 1 || (RES != 0 && pr)) v += pr[row * r_cs];
      py[row * y_cs] = v;
    };
  }
};

// ------------------------------------------------------------------------------------------------------------------ launch
// MT blocks of 16 output rows per workgroup and the blocks of the 1-D grid (0: they do not fit one): what a core's launch_rule returns
struct Launch {
  int mt;
  unsigned blocks;
};

// a runtime MT as a compile-time one: dispatch_mt(mt, [&](auto MT) { hipLaunchKernelGGL(kern<MT()>, ...); })
template <class F>
inline void dispatch_mt(int mt, F&& f) {
  switch (mt) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    default: f(std::integral_constant<int, 8>{}); break;
  }
}

// A node entry after its own size checks (TS_ERR_SHAPE), in the order every entry keeps: strides, the entry's envelope, axes, launch
// rule and grid, required pointers, the alignment of w_l, the overlap rules; then the launch.  `envelope` returns a code; `rule` returns
// the core's Launch; `go(MT, grid)` launches the kernel.
template <class Envelope, class Rule, class Go>
int launch(const char* who, const char* kernel, int B, std::initializer_list<Operand> ops, std::initializer_list<Pointer> ptrs,
           const float* w_l, std::initializer_list<int> axes, Envelope&& envelope, Rule&& rule, Go&& go) {
  if (int rc = check_strides(who, B, ops)) return rc;
  if (int rc = envelope()) return rc;
  for (int a : axes) TS_REQUIRE(a < kMaxAxis, TS_ERR_UNSUPPORTED, "%s: an axis of 2^20 or more", who);
  const Launch l = rule();
  TS_REQUIRE(l.blocks != 0, TS_ERR_UNSUPPORTED, "%s: grid too large", who);
  for (const Operand& o : ops) TS_REQUIRE(o.C == 0 || o.p != nullptr, TS_ERR_NULL, "%s: %s is NULL", who, o.name);
  for (const Pointer& n : ptrs) TS_REQUIRE(n.p != nullptr, TS_ERR_NULL, "%s: %s is NULL", who, n.name);
  TS_REQUIRE(w_l != nullptr, TS_ERR_NULL, "%s: w_l is NULL", who);
  TS_REQUIRE(ts::aligned16(w_l), TS_ERR_ALIGN, "%s: w_l not 16-byte aligned", who);
  if (int rc = check_overlap(who, B, ops)) return rc;
  dispatch_mt(l.mt, [&](auto MT) { go(MT, dim3(l.blocks)); });
  return ts::launched(kernel);
}

}  // namespace node
