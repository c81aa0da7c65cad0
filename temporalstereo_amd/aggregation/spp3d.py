"""SPP3D: 3-D spatial pyramid pooling (architecture/modeling/aggregation/utils/SPP3D.py:8-49), constructor and state-dict keys of the
reference: `pools.{i}.weight`, `pools.{i}.norm.*`, `fuse.0.weight`, `fuse.0.norm.*`, `fuse.1.weight`.

On fp32 GPU tensors the module is five kinds of launches: ts_spp3d_pool_fwd (every level, x read once per chain of nested boxes), the
1x1x1 convolutions of the (k,1,1) family with their BatchNorm / ReLU, ts_spp3d_expand_fwd (the trilinear resizes and the concatenation
in one pass), the 3x3x3 convolution as three (1,3,3) convolutions and a depth sum (functional family "hw3"), and the last 1x1x1
convolution.  CPU tensors, other norms or activations and more than 64 channels take the reference's op sequence in torch.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import functional as TF
from .. import layers
from ..layers import Conv3d


class SPP3D(nn.Module):
    """
    Args:
        in_planes:      (int), the channels of feature map
        strides:        (list, tuple), pooling stride (and box) of each pyramid level
        norm:           (str), the type of normalization layer
        activation:     (str, list, tuple), the type of activation layer and its coefficient is needed
        fuse_conv:      'hip' | 'framework': which kernels run the 3x3x3 convolution on the GPU path
    """

    def __init__(self, in_planes=64, strides=(2, 4, 8, 16), norm='BN3d', activation='ReLU', fuse_conv='hip'):
        super().__init__()
        if fuse_conv not in ('hip', 'framework'):
            raise ValueError("fuse_conv must be 'hip' or 'framework'")
        self.in_planes = in_planes
        self.strides = strides
        self.norm = norm
        self.activation = activation
        self.fuse_conv = fuse_conv

        self.pools = nn.ModuleList()
        for _ in self.strides:
            self.pools.append(Conv3d(in_planes, 16, 1, 1, 0, 1, bias=False, norm=(norm, 16), activation=activation))
        self.fuse = nn.Sequential(
            Conv3d(16 * len(strides) + in_planes, in_planes, 3, 1, 1, 1, bias=False, norm=(norm, in_planes), activation=activation),
            nn.Conv3d(in_planes, in_planes, 1, 1, 0, 1, bias=False),
        )

    def _reference_forward(self, x):
        """utils/SPP3D.py:38-49 op for op."""
        features = [x]
        B, C, D, H, W = x.shape
        for stride, pool in zip(self.strides, self.pools):
            stride = (min(D, stride), min(H, stride), min(W, stride))
            out = F.avg_pool3d(x, kernel_size=stride, stride=stride)
            out = pool(out)
            out = F.interpolate(out, size=(D, H, W), mode='trilinear', align_corners=True)
            features.append(out)
        return self.fuse(torch.cat(features, dim=1))

    def _on_kernels(self, x):
        if not (layers._hip_conv(x) and x.dim() == 5 and 1 <= len(self.strides) <= TF._SPP_MAX_LEVELS and self.in_planes <= 64):
            return False
        if x.shape[0] * (self.in_planes + 16 * len(self.strides)) > 65535 or max(x.shape[2:]) >= 1 << 20:
            return False
        return all(m._fusable() is not False and m.norm is not None for m in list(self.pools) + [self.fuse[0]])

    def forward(self, x):
        if not self._on_kernels(x):
            return self._reference_forward(x)
        B, C, D, H, W = x.shape
        strides = tuple(int(s) for s in self.strides)
        for pool, n in zip(self.pools, TF.spp3d_level_sizes((D, H, W), strides)):
            bn = pool._modules["norm"]
            if bn.training or bn._buffers.get("running_mean") is None:          # this BatchNorm takes batch statistics (a frozen one does not)
                if B * n[0] * n[1] * n[2] == 1:         # F.batch_norm's own refusal (torch.nn.functional._verify_batch_size)
                    raise ValueError("Expected more than 1 value per channel when training, got input size {}".format(
                        torch.Size((B, 16) + n)))
        *levels, xa = TF.spp3d_pool(x, strides, alias=True)
        # (the wrapper's own fused node, with the fp64 BatchNorm backward for levels of few cells: functional._ConvBNAct few_values)
        levels = [TF.conv_bn_act(l, pool._parameters["weight"], None, pool._modules["norm"], pool._fusable(), "d", (1, 1, 0, False),
                                 few_values=True) for pool, l in zip(self.pools, levels)]
        cat = TF.spp3d_expand(levels, xa, strides)
        f0 = self.fuse[0]
        if self.fuse_conv == 'hip':
            out = TF.conv_bn_act(cat, f0._parameters["weight"], None, f0._modules["norm"], f0._fusable(), "hw3", (1, 1, False))
        else:
            out = f0._finish(F.conv3d(cat, f0.weight, None, 1, 1, 1, 1))
        f1 = self.fuse[1]
        return TF.conv3d(out, f1.weight, None, (1, 1, 1), (0, 0, 0), (1, 1, 1))
