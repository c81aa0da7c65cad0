// Shared host-side helpers for libts_hip.so (gfx950 only; no CUDA compatibility layer).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <type_traits>

#include "../../include/ts_hip.h"

#define TS_ABI_VERSION 24   // 24: the overlap rules of ts_conv3x3_s_fwd / ts_fused_project_fwd hold for ts_mbconv_expand_fwd, ts_mbconv_project_fwd, ts_decoder_conv_fwd and ts_depthwise3x3_fwd as well (y apart from every input; a residual is y's own elements or apart from y: TS_ERR_SHAPE); 23: ts_conv3x3_s_weight_{bytes,layout} / ts_conv3x3_s_fwd / ts_fused_project_fwd (the encoder's large planes: the stem, ConvBnAct and the fused-MBConv blocks -- a 3x3 convolution of stride 1 or 2 with BatchNorm, SiLU and the residual in its epilogue, the stride-2 one in the phase form of the same core, and a 1x1 projection with BatchNorm and the residual); 22: ts_mbconv_weight_{bytes,layout} / ts_mbconv_expand_fwd / ts_mbconv_project_fwd / ts_depthwise3x3_fwd / ts_depthwise3x3_bwd_weight / ts_se_gate_fwd (MemoryInvertedResidual: the encoder's memory MBConv block as four launches -- a 1x1 convolution that reads [memory | input] in place, a depthwise 3x3 with the plane sums, the squeeze-excite gate, a 1x1 convolution that reads the gated map and adds the residual); 21: ts_decoder_conv_fwd / ts_decoder_weight_{bytes,layout} / ts_resize_bilinear_bwd (FeatureDecoder: a 3x3 convolution whose input is [resize(up) | skip] read in place, its weight layout, and the adjoint of the align-corners resize as a gather); 20: ts_conv_gru_* (ConvGRU: the gated recurrent cell as two launches, its gate-gradient kernels and weight layout); 19: ts_regress_convex_upsample_fwd / ts_topk_softargmax_half_fwd / ts_deconv2d_k4s2_unet_upsample_fwd (the regression tails of an inference pass as single launches); 18: ts_spp3d_pool_{fwd,bwd} / ts_spp3d_expand_{fwd,bwd} / ts_depth_sum3_fwd / ts_bn_small_train_bwd (SPP3D: pyramid pooling, the resize-and-concat, and the depth sum of a 3x3x3 convolution run as three (1,3,3) ones); 17:ts_flow_metrics_* / ts_flow_render_* / ts_flow_u16_decode_fwd (optical-flow metrics, colour maps and the KITTI 16-bit decode on the device); 16: ts_flow_corr_pyramid_{fwd,bwd} / ts_flow_corr_lookup_{fwd,bwd} (FlowCorrBlock: the 2-D all-pairs correlation pyramid and lookup); 15: ts_raft_corr_pyramid_{fwd,bwd} / ts_raft_corr_lookup_{fwd,bwd} (CorrBlock: the RAFT-Stereo correlation pyramid and lookup); 14: ts_inverse_warp_fwd / ts_inverse_warp_bwd (the 2-D inverse_warp: disparity, flow and depth mode); 13: ts_frames_prepare_fwd / ts_intrinsics_pyramid_fwd / ts_disp_u16_decode_fwd (input frames prepared on the device); 12: ts_disp_render_* (disparity / error colour maps and the 16-bit map on the device); 11: ts_disp_metrics_* (validation / test metrics on the device); 10: ts_inverse_warp_3d_fwd (the inverse_warp_3d seam); 9: ts_peer_status_async / set_timeout_ms / reset, layout + bf16 split of a framework-layout weight in one launch (ts_conv3d_hw_x6_weight_split_from), two-table weight layouts (ts_conv_weight_layout_many2); 8: ts_peer_* (SyncBatchNorm exchanges as kernels over peer-mapped memory); 7: ts_conv3d_hw_x6s_* (bf16-split stride-2 / transposed convolutions); 6: ts_block_cost_sampled_corr_fwd, ts_conv3d_hw_warp_fwd (first layer of a sampled level without the warped volume); 5: split-K workspace of ts_conv3d_hw_x6_fwd; 4: train_ops (candidates, offset head, deconv2d training forms, clip+RMSprop); 3: bwd_weight workspace, bn_stats counter, x6 / weight-layout / bn_train

namespace ts {

// thread-local message for ts_last_error_string()
char* err_buf();
int fail(int code, const char* fmt, ...);

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

inline size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// check the launch that was just issued; returns 0 or the positive hipError_t
inline int launched(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(static_cast<int>(e), "%s: %s", what, hipGetErrorString(e));
  return TS_OK;
}

// a runtime bool as a compile-time one: dispatch_bool(vec, [&](auto V) { hipLaunchKernelGGL(kern<V()>, ...); })
template <class F>
inline void dispatch_bool(bool b, F&& f) {
  if (b) f(std::true_type{});
  else f(std::false_type{});
}

// environment switches (callers read them once, into a `static const`): a number with a default; on unless the value starts with '0'
inline long long env_ll(const char* name, long long dflt) { const char* e = getenv(name); return e ? atoll(e) : dflt; }
inline bool env_not_zero(const char* name) { const char* e = getenv(name); return !(e && e[0] == '0'); }

// blocks of a 256-thread grid-stride grid over `items`, at most `cap`
inline unsigned blocks_for(long long items, long long cap) {
  long long n = (items + 255) / 256;
  if (n > cap) n = cap;
  return static_cast<unsigned>(n < 1 ? 1 : n);
}

// a strided [B][C][vol] operand: every element the kernels touch lies inside what the strides describe (C == 0: nothing is touched)
inline bool strides_ok(int B, int C, long long vol, long long bs, long long cs) {
  if (C == 0) return true;
  return cs >= vol && (B == 1 || bs >= cs * (C - 1) + vol);
}

constexpr int kWave = 64;       // CDNA4 wavefront
constexpr int kNumCU = 256;     // MI355X
constexpr int kNumXCD = 8;

}  // namespace ts

#define TS_REQUIRE_PTR(p)                                                     \
  do {                                                                        \
    if ((p) == nullptr) return ts::fail(TS_ERR_NULL, "%s is NULL", #p);       \
  } while (0)
#define TS_REQUIRE_ALIGNED(p)                                                          \
  do {                                                                                 \
    if (!ts::aligned16(p)) return ts::fail(TS_ERR_ALIGN, "%s not 16-byte aligned", #p); \
  } while (0)
#define TS_REQUIRE(cond, code, ...)                       \
  do {                                                    \
    if (!(cond)) return ts::fail((code), __VA_ARGS__);    \
  } while (0)
