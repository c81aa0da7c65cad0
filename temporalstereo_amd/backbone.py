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

MemoryInvertedResidual: the inverted-residual block of the encoder's last stages with the per-frame feature memory spliced into its
input -- the reference's `_inverted_residual_forward` (architecture/modeling/backbone/TemporalStereo.py:183-218) -- and `block_forward`,
its `_block_forward` (:165-180).

    mc = int(C * memory_percent);  x = cat([memory if given else input[:, :mc], input[:, mc:]], 1)
    x = act1(bn1(conv_pw(x)));  x = act2(bn2(conv_dw(x)));  x = se(x);  x = bn3(conv_pwl(x))
    return input + x, input[:, :mc]

Routing, one path per configuration whatever the plane size: fp32 GPU tensors under the 'hip' backend, a recognised block inside the
kernels' envelope (functional.mbconv_supported), eval mode and nothing that needs a gradient -> functional.mbconv_eval, four launches
(csrc/mbconv.hip).  The same tensors in train mode or with a gradient needed -> `_train_forward`: the reference's op sequence with the
splice on temporal.exchange_feature_memory and the depthwise convolution on functional.depthwise_conv3x3; the 1x1 convolutions, the
BatchNorms and the squeeze-excite step stay framework ops there.  Everything else -- CPU tensors, other dtypes,
set_conv_backend('torch'), drop_path_rate > 0 in train mode, a block `from_block` did not recognise -- takes `_reference_forward`, the
reference's statements on the block's own submodules.
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


# ------------------------------------------------------------------------------------------------------- the encoder's memory MBConv block
def _make_divisible(v, divisor=8):
    """The EfficientNet family's channel rounding: the nearest multiple of `divisor`, at least `divisor`, never more than 10 % below v."""
    new = max(divisor, int(v + divisor / 2) // divisor * divisor)
    return new + divisor if new < 0.9 * v else new


def _drop_path(x, rate, training):
    """Stochastic depth per sample: in train mode a sample's branch is dropped with probability `rate`, the kept ones scaled by 1 / (1 - rate)."""
    if rate == 0.0 or not training:
        return x
    keep = 1.0 - rate
    mask = x.new_empty((x.shape[0],) + (1,) * (x.dim() - 1)).bernoulli_(keep)
    return x.div(keep) * mask


class SqueezeExcite(nn.Module):
    """x * gate(conv_expand(act1(conv_reduce(mean_hw(x))))), both convolutions 1x1 with bias."""

    def __init__(self, chs, se_chs):
        super().__init__()
        self.conv_reduce = nn.Conv2d(chs, se_chs, 1, bias=True)
        self.act1 = nn.SiLU(inplace=True)
        self.conv_expand = nn.Conv2d(se_chs, chs, 1, bias=True)
        self.gate = nn.Sigmoid()

    def forward(self, x):
        x_se = x.mean((2, 3), keepdim=True)
        x_se = self.conv_expand(self.act1(self.conv_reduce(x_se)))
        return x * self.gate(x_se)


_MBCONV_PARTS = ("conv_pw", "bn1", "act1", "conv_dw", "bn2", "act2", "se", "conv_pwl", "bn3")


class MemoryInvertedResidual(nn.Module):
    """The inverted-residual (MBConv) block with a residual -- stride 1, equal input and output width -- whose first
    mc = int(in_chs * memory_percent) input channels are replaced by the previous frame's (`memory`), and whose own first mc input
    channels are returned as the next frame's memory.

    Attributes and state-dict keys are those of the block the reference takes from its pinned timm 0.4.12 (`InvertedResidual` of
    efficientnetv2_rw_s): conv_pw.weight, bn1.*, conv_dw.weight, bn2.*, se.conv_reduce.{weight,bias}, se.conv_expand.{weight,bias},
    conv_pwl.weight, bn3.*; has_residual, drop_path_rate.  timm is not a dependency of this package and was not at hand when this was
    written: the list is taken as given from the reference's use of the block (backbone/TemporalStereo.py:199-216 names every
    attribute but the squeeze-excite step's own)."""

    def __init__(self, in_chs, exp_ratio=4.0, se_ratio=0.25, memory_percent=0.25, mid_chs=None, se_chs=None, drop_path_rate=0.0):
        super().__init__()
        mid_chs = int(mid_chs) if mid_chs else _make_divisible(in_chs * exp_ratio)
        se_chs = int(se_chs) if se_chs else _make_divisible(in_chs * se_ratio, 1)
        self.conv_pw = nn.Conv2d(in_chs, mid_chs, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(mid_chs)
        self.act1 = nn.SiLU(inplace=True)
        self.conv_dw = nn.Conv2d(mid_chs, mid_chs, 3, 1, 1, groups=mid_chs, bias=False)
        self.bn2 = nn.BatchNorm2d(mid_chs)
        self.act2 = nn.SiLU(inplace=True)
        self.se = SqueezeExcite(mid_chs, se_chs)
        self.conv_pwl = nn.Conv2d(mid_chs, in_chs, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(in_chs)
        self.has_residual = True
        self.drop_path_rate = float(drop_path_rate)
        self.memory_percent = float(memory_percent)
        self._recognised = True

    @classmethod
    def from_block(cls, block, memory_percent):
        """Adopts an existing inverted-residual block by its attributes: the SAME submodule objects (so the same Parameters and buffers;
        nothing is copied), `has_residual` required.  The kernels are taken only when the block is recognised (`_recognise`); any other
        block keeps running its own submodules in the reference's order.  In the reference:
        `MemoryInvertedResidual.from_block(b, self.memory_percent)` over the residual members of block1..block4."""
        for name in _MBCONV_PARTS:
            if not hasattr(block, name):
                raise ValueError("MemoryInvertedResidual.from_block: the block has no '%s'" % name)
        if not getattr(block, "has_residual", False):
            raise ValueError("MemoryInvertedResidual.from_block: a block with a residual (stride 1, equal widths) expected")
        self = cls.__new__(cls)
        nn.Module.__init__(self)
        for name in _MBCONV_PARTS:
            setattr(self, name, getattr(block, name))
        self.has_residual = True
        self.drop_path_rate = float(getattr(block, "drop_path_rate", 0.0))
        self.memory_percent = float(memory_percent)
        self._recognised = self._recognise()
        self.train(block.training)
        return self

    def _recognise(self):
        """True when the submodules are exactly what csrc/mbconv.hip computes."""
        def conv(m, cin, cout, k, groups, bias):
            return isinstance(m, nn.Conv2d) and not isinstance(m, nn.ConvTranspose2d) and m.in_channels == cin and m.out_channels == cout and \
                m.kernel_size == (k, k) and m.stride == (1, 1) and m.padding == (k // 2, k // 2) and m.dilation == (1, 1) and \
                m.groups == groups and (m.bias is not None) == bias and m.padding_mode == "zeros"

        def norm(m, c):
            return type(m) in (nn.BatchNorm2d, nn.SyncBatchNorm) and m.num_features == c and m.affine and m.track_running_stats

        pw, se = self.conv_pw, self.se
        if not isinstance(pw, nn.Conv2d):
            return False
        C, Cmid = pw.in_channels, pw.out_channels
        if not (conv(pw, C, Cmid, 1, 1, False) and conv(self.conv_dw, Cmid, Cmid, 3, Cmid, False) and conv(self.conv_pwl, Cmid, C, 1, 1, False)):
            return False
        if not (norm(self.bn1, Cmid) and norm(self.bn2, Cmid) and norm(self.bn3, C)):
            return False
        if not (isinstance(self.act1, nn.SiLU) and isinstance(self.act2, nn.SiLU)):
            return False
        if not all(hasattr(se, n) for n in ("conv_reduce", "act1", "conv_expand", "gate")) or not isinstance(se.conv_reduce, nn.Conv2d):
            return False
        Cr = se.conv_reduce.out_channels
        gate = se.gate
        return conv(se.conv_reduce, Cmid, Cr, 1, 1, True) and conv(se.conv_expand, Cr, Cmid, 1, 1, True) and isinstance(se.act1, nn.SiLU) and \
            (isinstance(gate, nn.Sigmoid) or getattr(gate, "__name__", None) == "sigmoid")

    def _route(self, input, memory):
        """'kernels' | 'train' | 'reference' (the module's docstring)."""
        from . import functional as TF
        if not self._recognised or input.dim() != 4 or not layers._hip_conv(input) or (memory is not None and not layers._hip_conv(memory)):
            return "reference"
        norms = (self.bn1, self.bn2, self.bn3)
        training = self.training or any(bn.training for bn in norms)
        if training and self.drop_path_rate > 0:
            return "reference"
        params = [p for p in self.parameters()]
        if any(not (p.is_cuda and p.dtype == torch.float32) for p in params) or any(TF.bn_exchanges(bn) for bn in norms):
            return "reference"
        if not TF.mbconv_supported(self.conv_pw.in_channels, self.conv_pw.out_channels, self.se.conv_reduce.out_channels):
            return "reference"
        if training or (torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in [input, memory] + params)):
            return "train"
        return "kernels"

    def _reference_forward(self, input, memory, mc):
        input1, input2 = input[:, :mc], input[:, mc:]
        x = torch.cat([input1 if memory is None else memory, input2], dim=1)
        x = self.act1(self.bn1(self.conv_pw(x)))
        x = self.act2(self.bn2(self.conv_dw(x)))
        x = self.se(x)
        x = self.bn3(self.conv_pwl(x))
        if self.drop_path_rate > 0:
            x = _drop_path(x, self.drop_path_rate, self.training)
        return input + x, input1

    def _train_forward(self, input, memory, memory_percent):
        from . import functional as TF
        from . import temporal
        x, new_memory = temporal.exchange_feature_memory(input, memory, memory_percent)
        x = self.act1(self.bn1(self.conv_pw(x)))
        x = self.act2(self.bn2(TF.depthwise_conv3x3(x, self.conv_dw.weight, self.conv_dw.bias)))
        x = self.se(x)
        x = self.bn3(self.conv_pwl(x))
        return input + x, new_memory

    def _kernel_forward(self, input, memory, mc, return_stages=False):
        from . import functional as TF
        se = self.se
        res = TF.mbconv_eval(input, memory, self.conv_pw.weight, TF._bn_eval_fold(self.bn1), self.conv_dw.weight, TF._bn_eval_fold(self.bn2),
                             se.conv_reduce.weight, se.conv_reduce.bias, se.conv_expand.weight, se.conv_expand.bias, self.conv_pwl.weight,
                             TF._bn_eval_fold(self.bn3), return_stages=return_stages)
        if return_stages:
            return res[0], input[:, :mc], dict(act1=res[1], act2=res[2], gate=res[3])
        return res, input[:, :mc]

    def _forward(self, input, memory, memory_percent):
        ic = input.shape[1]
        mc = int(ic * memory_percent)
        if memory is not None and memory.shape[1] != mc:
            raise AssertionError("input shape: {}; memory shape: {}!".format(input.shape, memory.shape))
        if memory is not None and (memory.dim() != input.dim() or memory.shape[0] != input.shape[0] or memory.shape[2:] != input.shape[2:]):
            # the reference's torch.cat refuses these; the kernels take batch and plane from the input alone
            raise RuntimeError("MemoryInvertedResidual: memory {} does not match the batch and plane of input {}".format(
                tuple(memory.shape), tuple(input.shape)))
        if mc == 0:
            memory = None                   # an empty memory: the block sees its own input
        route = self._route(input, memory)
        if route == "kernels":
            return self._kernel_forward(input, memory, mc)
        if route == "train":
            return self._train_forward(input, memory, memory_percent)
        return self._reference_forward(input, memory, mc)

    def forward(self, input, memory=None):
        """-> (output, new_memory): new_memory is the view input[:, :mc]."""
        return self._forward(input, memory, self.memory_percent)


def block_forward(block, input, memory_percent=0.0, memories=None, memory_idx=0):
    """The reference's `_block_forward` (backbone/TemporalStereo.py:165-180): the walk over a stage -- a sequential of sequentials.  Every
    MemoryInvertedResidual goes through the memory path with memories[memory_idx] (None on the first frame) and appends its new memory;
    every other member is called.  -> (x, out_memories, memory_idx)."""
    out_memories = []
    for sequential in block:
        for member in sequential:
            if isinstance(member, MemoryInvertedResidual) and member.has_residual:
                if memory_percent > 0:
                    m = memories[memory_idx] if memories is not None and len(memories) > 0 else None
                    input, m = member._forward(input, m, memory_percent)
                    out_memories.append(m)
                    memory_idx += 1
                else:
                    input = member._forward(input, None, 0.0)[0]
            else:
                input = member(input)
    return input, out_memories, memory_idx
