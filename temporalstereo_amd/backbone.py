"""FeatureDecoder: the three-level decoder of the reference's backbone (architecture/modeling/backbone/TemporalStereo.py:78-90,125-138)
with its four submodules, their construction and their state-dict keys (`conv32.*`, `deconv32_16.{0,1}.*`, `deconv16_8.{0,1}.*`,
`deconv8_4.{0,1}.*`): a reference checkpoint filtered to those four names loads with strict=True.

    x32 = conv32(x32)
    x16 = deconv32_16(cat([resize(x32), x16]))     x8 = deconv16_8(cat([resize(x16), x8]))     x4 = deconv8_4(cat([resize(x8), x4]))

Every convolution is 3x3, stride 1, padding 1, without bias; the first of each pair is followed by the norm and the activation; the
resizes are bilinear with align_corners=True to the skip's plane.  The encoder (timm's EfficientNetV2) is not part of this package: the
four maps it produces are the arguments of `forward`, and the three it returns are the [x4, x8, x16] the aggregator reads in place.

On fp32 GPU tensors with the 'hip' convolution backend, BatchNorm (or no norm) and SiLU (or no activation) and widths inside the
kernel's envelope, every layer is functional.decoder_conv: the resized map and the concatenation are never written
(csrc/feature_decoder.hip).  Everything else -- CPU tensors, other dtypes, set_conv_backend('torch'), GroupNorm / InstanceNorm, other
activations, wider layers -- takes `_reference_forward`, the reference's op sequence on the Conv2d wrappers.  So does a SyncBatchNorm
(norm='SyncBN', dist.sync_batchnorm, a converted backbone) in train mode on more than one rank: the kernel path computes per-rank
statistics, the wrappers' conv_bn_act exchanges them; in eval mode and on a single rank a SyncBatchNorm takes the kernels.  The module
takes one path for a given configuration whatever the plane size.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import layers

_NAMES = ("conv32", "deconv32_16", "deconv16_8", "deconv8_4")


class FeatureDecoder(nn.Module):
    def __init__(self, channels=(24, 48, 64, 160, 272), out_channels=(0, 64, 128, 256, 320), norm='BN', activation='SiLU'):
        super().__init__()
        channels, out_channels = tuple(channels), tuple(out_channels)
        if len(channels) != 5 or len(out_channels) != 5:
            raise ValueError("FeatureDecoder: channels and out_channels hold five widths each")
        self.channels, self.out_channels = channels, out_channels
        self.norm, self.activation = norm, activation
        Conv2d = layers.Conv2d

        def pair(cin, cout):
            return nn.Sequential(Conv2d(cin, cout, 3, 1, 1, bias=False, norm=(norm, cout), activation=activation),
                                 Conv2d(cout, cout, 3, 1, 1, bias=False, norm=None, activation=None))
        self.conv32 = Conv2d(channels[4], out_channels[4], 3, 1, 1, bias=False, norm=None, activation=None)
        self.deconv32_16 = pair(out_channels[4] + channels[3], out_channels[3])
        self.deconv16_8 = pair(out_channels[3] + channels[2], out_channels[2])
        self.deconv8_4 = pair(out_channels[2] + channels[1], out_channels[1])

    @classmethod
    def from_backbone(cls, module):
        """Adopts `conv32`, `deconv32_16`, `deconv16_8` and `deconv8_4` of an existing reference backbone: the decoder's wrappers hold
        the SAME Parameter and buffer objects (nothing is copied), so the backbone's optimizer, checkpoints and .to() keep working.
        In the reference: `self.decoder = FeatureDecoder.from_backbone(self)` and `return self.decoder(x4, x8, x16, x32), out_memories`
        in place of lines 125-138 of `_forward`."""
        for name in _NAMES:
            if not hasattr(module, name):
                raise ValueError("FeatureDecoder.from_backbone: the module has no '%s'" % name)
        w32, w16, w8, w4 = (module.conv32.weight.shape, module.deconv32_16[0].weight.shape, module.deconv16_8[0].weight.shape,
                            module.deconv8_4[0].weight.shape)
        out_channels = (0, w4[0], w8[0], w16[0], w32[0])
        channels = (0, w4[1] - w8[0], w8[1] - w16[0], w16[1] - w32[0], w32[1])
        self = cls.__new__(cls)
        nn.Module.__init__(self)
        self.channels, self.out_channels = channels, out_channels
        self.norm, self.activation = getattr(module, "norm", None), getattr(module, "activation", None)

        def adopt(conv):
            if not isinstance(conv, nn.Conv2d) or conv.kernel_size != (3, 3) or conv.stride != (1, 1) or conv.padding != (1, 1) or \
                    conv.dilation != (1, 1) or conv.groups != 1:
                raise ValueError("FeatureDecoder.from_backbone: a 3x3 convolution with stride 1 and padding 1 expected, got %r" % (conv,))
            if isinstance(conv, layers.Conv2d):
                return conv
            own = layers.Conv2d(conv.in_channels, conv.out_channels, 3, 1, 1, bias=conv.bias is not None, norm=None, activation=None)
            own._parameters["weight"] = conv.weight
            own._parameters["bias"] = conv.bias
            own.norm, own.activation = getattr(conv, "norm", None), getattr(conv, "activation", None)
            return own
        self.conv32 = adopt(module.conv32)
        for name in _NAMES[1:]:
            seq = getattr(module, name)
            if len(seq) != 2:
                raise ValueError("FeatureDecoder.from_backbone: '%s' must hold two convolutions" % name)
            setattr(self, name, nn.Sequential(adopt(seq[0]), adopt(seq[1])))
        self.train(module.training)
        return self

    @staticmethod
    def _check(x4, x8, x16, x32):
        maps = (("x4", x4), ("x8", x8), ("x16", x16), ("x32", x32))
        for name, t in maps:
            if t.dim() != 4:
                raise ValueError("FeatureDecoder: %s must be [B,C,H,W], got %s" % (name, tuple(t.shape)))
        for name, t in maps[1:]:
            if t.shape[0] != x4.shape[0]:
                raise ValueError("FeatureDecoder: %s has batch %d, x4 has %d" % (name, t.shape[0], x4.shape[0]))
        for (fine_n, fine), (coarse_n, coarse) in zip(maps[:-1], maps[1:]):
            if fine.shape[2] < coarse.shape[2] or fine.shape[3] < coarse.shape[3]:
                raise ValueError("FeatureDecoder: the plane of %s %s is smaller than that of %s %s"
                                 % (fine_n, tuple(fine.shape[2:]), coarse_n, tuple(coarse.shape[2:])))

    def _reference_forward(self, x4, x8, x16, x32):
        x32 = self.conv32(x32)
        up = F.interpolate(x32, size=x16.shape[-2:], mode='bilinear', align_corners=True)
        x16 = self.deconv32_16(torch.cat([up, x16], dim=1))
        up = F.interpolate(x16, size=x8.shape[-2:], mode='bilinear', align_corners=True)
        x8 = self.deconv16_8(torch.cat([up, x8], dim=1))
        up = F.interpolate(x8, size=x4.shape[-2:], mode='bilinear', align_corners=True)
        x4 = self.deconv8_4(torch.cat([up, x4], dim=1))
        return [x4, x8, x16]

    def _on_kernels(self, *maps):
        from . import functional as TF
        for t in maps:
            if not layers._hip_conv(t) or t.dim() != 4:
                return False
        for conv in [self.conv32] + [c for name in _NAMES[1:] for c in getattr(self, name)]:
            w = conv.weight
            if not (w.is_cuda and w.dtype == torch.float32 and TF.decoder_conv_supported(w.shape[1], w.shape[0])):
                return False
            if conv.norm is None:
                if conv.activation is not None:
                    return False
            elif conv._fusable() not in (None, "SiLU") or TF.bn_exchanges(conv.norm):
                return False            # (a train-mode SyncBatchNorm over several ranks: the exchange is conv_bn_act's)
        return True

    @staticmethod
    def _layer(conv, up, skip):
        from . import functional as TF
        act = conv._fusable() if conv.norm is not None else None
        return TF.decoder_conv(up, skip, conv.weight, conv.bias, conv.norm, act)

    def forward(self, x4, x8, x16, x32):
        self._check(x4, x8, x16, x32)
        if not self._on_kernels(x4, x8, x16, x32):
            return self._reference_forward(x4, x8, x16, x32)
        up = self._layer(self.conv32, None, x32)
        outs = []
        for name, skip in (("deconv32_16", x16), ("deconv16_8", x8), ("deconv8_4", x4)):
            seq = getattr(self, name)
            up = self._layer(seq[1], None, self._layer(seq[0], up, skip))
            outs.append(up)
        return outs[::-1]
