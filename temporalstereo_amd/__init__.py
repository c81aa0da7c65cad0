"""temporalstereo_amd -- MI355X-native (gfx950) cost-volume stereo hot path.

Drop-in for the hot path of youmi-zym/TemporalStereo (cost-volume build, temporal cost warp,
3-D aggregation pyramid, disparity regression): hand-written HIP kernels in libts_hip.so behind
the C ABI of include/ts_hip.h, wrapped here as torch.autograd.Function ops and nn.Modules that
mirror the reference's interfaces.  See DESIGN.md / INTEGRATION.md.
"""
__version__ = "0.1.0"

from .functional import (cat_fms, dif_fms, inverse_warp_3d, correlation, correlation1d, block_cost, topk_softargmax, soft_argmin, argmin_select,  # noqa: F401
                         FunctionSoftsplat, project_to_3d, inverse_warp, mesh_grid, CorrBlock, raft_corr_pyramid, raft_corr_lookup,
                         raft_corr_level_views, FlowCorrBlock, flow_corr_pyramid, flow_corr_lookup, flow_corr_level_views,
                         spp3d_pool, spp3d_expand, spp3d_level_sizes, conv3d_k333, conv_gru, decoder_conv, depthwise_conv3x3,
                         conv3x3_bn_act, fused_mbconv_eval, fused_mbconv_supported)
from .registry import (AGGREGATION_REGISTRY, PREDICTION_REGISTRY, build_aggregation, build_prediction,  # noqa: F401
                       CfgView, register_into)
from .aggregation import (TEMPORALSTEREO, CoarseAggregation, FineAggregation, PreciseAggregation, SPP3D)  # noqa: F401
from .prediction import SOFTARGMIN, ARGMIN  # noqa: F401
from .recurrent import ConvGRU  # noqa: F401
from .backbone import (FeatureDecoder, MemoryInvertedResidual, block_forward, FusedInvertedResidual, ConvBnAct, StemConv,  # noqa: F401
                       InvertedResidual, TemporalStereoBackbone)
from . import temporal  # noqa: F401
from . import evaluation  # noqa: F401
from .evaluation import validation_metrics, flow_calc_error, do_flow_evaluation, flow_validation_metrics  # noqa: F401
from . import visualization  # noqa: F401
from .visualization import (render_frame, make_color_wheel, flow_max_rad, flow_color, flow_to_color, flow_err_to_color,  # noqa: F401
                            render_flow_frame)
from . import preprocess  # noqa: F401
from .preprocess import prepare_frames, prepare_batch, intrinsics_pyramid, disp_from_uint16, decode_kitti_flow  # noqa: F401
from . import augment  # noqa: F401
from .augment import (Augmentation, draw_augmentation, gamma_table, augment_frames, prepare_train_batch,  # noqa: F401
                      disp_window_from_uint16)
