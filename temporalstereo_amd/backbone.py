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

StemConv, ConvBnAct, FusedInvertedResidual: the encoder's large planes -- the stem, the members of block0 and the fused-MBConv
(edge-residual) members of block1 / block2 (backbone/TemporalStereo.py:62-70,105-113) -- routed the same way: one launch (stem, ConvBnAct)
or two (a fused block) in eval mode without a gradient (csrc/fused_mbconv.hip), the stride-1 3x3 on functional.decoder_conv's node in
train mode, the block's own submodules otherwise.  InvertedResidual: the MBConv block without a residual, framework ops.
TemporalStereoBackbone: the reference's backbone module over all of these, with its forward(l_img, r_img, prev_info), its state-dict
keys, `from_backbone` adopting an existing one and a constructor from a table of widths.
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
    def from_backbone(cls, module, set_mode=True):
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
        if set_mode:
            self.train(module.training)
        else:                               # (the submodules keep the modes they have: TemporalStereoBackbone adopts at every call)
            self.training = module.training
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


def _conv(m, k, strides=(1,), cin=None, cout=None, groups=1, bias=False, zeros=True):
    """A k x k nn.Conv2d as the kernels compute it: a stride out of `strides`, padding k // 2, no dilation, `groups` groups, with or
    without a bias; cin / cout: the widths it must have (None: any); zeros: padding_mode must be 'zeros' (the fused block's 1x1, which
    pads nothing, never asked)."""
    return isinstance(m, nn.Conv2d) and not isinstance(m, nn.ConvTranspose2d) and m.kernel_size == (k, k) and \
        m.stride in [(s, s) for s in strides] and m.padding == (k // 2, k // 2) and m.dilation == (1, 1) and m.groups == groups and \
        (m.bias is not None) == bias and (not zeros or m.padding_mode == "zeros") and cin in (None, m.in_channels) and cout in (None, m.out_channels)


def _batchnorm(m, c, momentum=True):
    """A BatchNorm over c channels with affine parameters and running statistics; momentum: a momentum is required (momentum=None, the
    cumulative average, is outside functional.decoder_conv's node, which the large-plane blocks train on)."""
    return type(m) in (nn.BatchNorm2d, nn.SyncBatchNorm) and m.num_features == c and m.affine and m.track_running_stats and \
        (not momentum or m.momentum is not None)


def _route(block, norms, supported, *tensors):
    """'kernels' | 'train' | 'reference' for a block of the encoder (the blocks' docstrings): `tensors` are what the block would hand to
    the kernels (the input first; None: absent), `norms` its BatchNorms, `supported()` its envelope."""
    from . import functional as TF
    tensors = [t for t in tensors if t is not None]
    if not block._recognised or tensors[0].dim() != 4 or not all(layers._hip_conv(t) for t in tensors):
        return "reference"
    training = block.training or any(bn.training for bn in norms)
    if training and block.drop_path_rate > 0:
        return "reference"
    params = [p for p in block.parameters()]
    if any(not (p.is_cuda and p.dtype == torch.float32) for p in params) or any(TF.bn_exchanges(bn) for bn in norms):
        return "reference"
    if not supported():
        return "reference"
    if training or (torch.is_grad_enabled() and any(t.requires_grad for t in tensors + params)):
        return "train"
    return "kernels"


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
        pw, se = self.conv_pw, self.se
        if not isinstance(pw, nn.Conv2d):
            return False
        C, Cmid = pw.in_channels, pw.out_channels
        if not (_conv(pw, 1) and _conv(self.conv_dw, 3, cin=Cmid, cout=Cmid, groups=Cmid) and _conv(self.conv_pwl, 1, cin=Cmid, cout=C)):
            return False
        if not all(_batchnorm(bn, c, momentum=False) for bn, c in ((self.bn1, Cmid), (self.bn2, Cmid), (self.bn3, C))):
            return False
        if not (isinstance(self.act1, nn.SiLU) and isinstance(self.act2, nn.SiLU)):
            return False
        if not all(hasattr(se, n) for n in ("conv_reduce", "act1", "conv_expand", "gate")) or not isinstance(se.conv_reduce, nn.Conv2d):
            return False
        Cr = se.conv_reduce.out_channels
        gate = se.gate
        return _conv(se.conv_reduce, 1, cin=Cmid, bias=True) and _conv(se.conv_expand, 1, cin=Cr, cout=Cmid, bias=True) and isinstance(se.act1, nn.SiLU) and \
            (isinstance(gate, nn.Sigmoid) or getattr(gate, "__name__", None) == "sigmoid")

    def _route(self, input, memory):
        """'kernels' | 'train' | 'reference' (the module's docstring)."""
        from . import functional as TF
        return _route(self, (self.bn1, self.bn2, self.bn3),
                      lambda: TF.mbconv_supported(self.conv_pw.in_channels, self.conv_pw.out_channels, self.se.conv_reduce.out_channels), input, memory)

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


# ------------------------------------------------------------------------------------------------------- the encoder's large planes
def _conv3x3(m):
    """A plain 3x3 convolution csrc/fused_mbconv.hip computes: stride 1 or 2, padding 1, no bias."""
    return _conv(m, 3, strides=(1, 2))


class _LargePlaneBlock(nn.Module):
    """What StemConv, ConvBnAct and FusedInvertedResidual share: the routing decision and the 3x3 + BatchNorm + SiLU step of the three
    routes.  A subclass names its 3x3 convolution and its BatchNorms (`_conv3`, `_norms`) and its envelope (`_supported`)."""
    has_residual = False
    drop_path_rate = 0.0

    def _route(self, x):
        """'kernels' | 'train' | 'reference' (the module's docstring)."""
        return _route(self, self._norms(), self._supported, x)

    @staticmethod
    def _conv3_train(conv, bn, act, x):
        """silu(bn(conv3x3(x))) with a gradient or batch statistics: stride 1 on functional.decoder_conv's node, stride 2 framework ops."""
        from . import functional as TF
        if conv.stride == (1, 1):
            return TF.decoder_conv(None, x, conv.weight, None, bn, "SiLU")
        return act(bn(conv(x)))

    def forward(self, x):
        route = self._route(x)
        if route == "kernels":
            return self._kernel_forward(x)
        if route == "train":
            return self._train_forward(x)
        return self._reference_forward(x)


class StemConv(_LargePlaneBlock):
    """The encoder's stem, `act1(bn1(conv_stem(x)))`: a 3x3 convolution of stride 2 (or 1), padding 1, without bias, BatchNorm, SiLU --
    attributes and state-dict keys as the reference's backbone holds them (backbone/TemporalStereo.py:62-64, 105).  Eval mode without a
    gradient: ONE launch, the stride-2 form in the phase order (csrc/fused_mbconv.hip)."""

    def __init__(self, in_chs=3, out_chs=24, stride=2):
        super().__init__()
        self.conv_stem = nn.Conv2d(in_chs, out_chs, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(out_chs)
        self.act1 = nn.SiLU(inplace=True)
        self._recognised = True

    @classmethod
    def from_modules(cls, conv_stem, bn1, act1):
        """Adopts the three submodule objects themselves (the same Parameters and buffers; nothing is copied)."""
        self = cls.__new__(cls)
        nn.Module.__init__(self)
        self.conv_stem, self.bn1, self.act1 = conv_stem, bn1, act1
        self._recognised = self._recognise()
        self.training = bn1.training            # (the three keep the modes they have)
        return self

    def _recognise(self):
        c = self.conv_stem
        return _conv3x3(c) and _batchnorm(self.bn1, c.out_channels) and isinstance(self.act1, nn.SiLU)

    def _norms(self):
        return (self.bn1,)

    def _supported(self):
        from . import functional as TF
        c = self.conv_stem
        return TF.conv3x3_s_supported(c.in_channels, c.out_channels, c.stride[0])

    def _reference_forward(self, x):
        return self.act1(self.bn1(self.conv_stem(x)))

    def _train_forward(self, x):
        return self._conv3_train(self.conv_stem, self.bn1, self.act1, x)

    def _kernel_forward(self, x):
        from . import functional as TF
        return TF.conv3x3_bn_act(x, self.conv_stem.weight, TF._bn_eval_fold(self.bn1), self.conv_stem.stride[0], "SiLU")


class ConvBnAct(_LargePlaneBlock):
    """A member of the encoder's first stage: `act1(bn1(conv(x)))` plus the input where `has_residual` (stride 1, equal widths, `skip`).
    Attributes and state-dict keys follow timm 0.4.12's `ConvBnAct` as efficientnetv2_rw_s builds it -- conv.weight, bn1.*; act1,
    has_residual, drop_path_rate.  timm is not a dependency of this package and was not at hand when this was written: the list rests
    on the record (the reference's backbone takes `net.blocks[0]` as it is, backbone/TemporalStereo.py:68).  Eval mode without a gradient:
    ONE launch with the residual added after the activation (csrc/fused_mbconv.hip)."""

    def __init__(self, in_chs, out_chs, stride=1, skip=False, drop_path_rate=0.0):
        super().__init__()
        self.conv = nn.Conv2d(in_chs, out_chs, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(out_chs)
        self.act1 = nn.SiLU(inplace=True)
        self.has_residual = bool(skip) and stride == 1 and in_chs == out_chs
        self.drop_path_rate = float(drop_path_rate)
        self._recognised = True

    @classmethod
    def from_block(cls, block):
        """Adopts an existing block by its attributes: the SAME submodule objects.  A block `_recognise` does not accept keeps running its
        own submodules in the reference's order."""
        for name in ("conv", "bn1", "act1"):
            if not hasattr(block, name):
                raise ValueError("ConvBnAct.from_block: the block has no '%s'" % name)
        self = cls.__new__(cls)
        nn.Module.__init__(self)
        self.conv, self.bn1, self.act1 = block.conv, block.bn1, block.act1
        self.has_residual = bool(getattr(block, "has_residual", False))
        self.drop_path_rate = float(getattr(block, "drop_path_rate", 0.0))
        self._recognised = self._recognise()
        self.train(block.training)
        return self

    def _recognise(self):
        c = self.conv
        if not (_conv3x3(c) and _batchnorm(self.bn1, c.out_channels) and isinstance(self.act1, nn.SiLU)):
            return False
        return not self.has_residual or (c.stride == (1, 1) and c.in_channels == c.out_channels)

    def _norms(self):
        return (self.bn1,)

    def _supported(self):
        from . import functional as TF
        return TF.conv3x3_s_supported(self.conv.in_channels, self.conv.out_channels, self.conv.stride[0])

    def _reference_forward(self, x):
        shortcut = x
        x = self.conv(x)
        x = self.bn1(x)
        x = self.act1(x)
        if self.has_residual:
            if self.drop_path_rate > 0:
                x = _drop_path(x, self.drop_path_rate, self.training)
            x += shortcut
        return x

    def _train_forward(self, x):
        y = self._conv3_train(self.conv, self.bn1, self.act1, x)
        return y + x if self.has_residual else y

    def _kernel_forward(self, x):
        from . import functional as TF
        return TF.conv3x3_bn_act(x, self.conv.weight, TF._bn_eval_fold(self.bn1), self.conv.stride[0], "SiLU",
                                 residual=x if self.has_residual else None)


_FUSED_PARTS = ("conv_exp", "bn1", "act1", "conv_pwl", "bn2")


class FusedInvertedResidual(_LargePlaneBlock):
    """The fused-MBConv (edge-residual) block of the encoder's second and third stages:

        x = act1(bn1(conv_exp(input)));  x = se(x);  x = bn2(conv_pwl(x));  return x + input if has_residual else x

    conv_exp a 3x3 of stride 1 or 2 and padding 1, conv_pwl a 1x1, neither with a bias.  Attributes and state-dict keys follow timm
    0.4.12's `EdgeResidual` as efficientnetv2_rw_s builds it -- conv_exp.weight, bn1.*, conv_pwl.weight, bn2.*; act1, se (None or
    nn.Identity there: no squeeze-excite in these stages), has_residual, drop_path_rate.  timm is not a dependency of this package and
    was not at hand when this was written: the list rests on the record (the reference takes `net.blocks[1:3]` as they are,
    backbone/TemporalStereo.py:69-70; its `_block_forward` calls every member that is not an InvertedResidual).

    Routing, one path per configuration whatever the plane size: fp32 GPU tensors under the 'hip' backend, a recognised block inside
    the envelope (functional.fused_mbconv_supported), eval mode and nothing that needs a gradient -> functional.fused_mbconv_eval, TWO
    launches (csrc/fused_mbconv.hip).  The same in train mode or with a gradient needed -> `_train_forward`: the stride-1 expansion with
    its BatchNorm and SiLU on functional.decoder_conv's node; the 1x1, its BatchNorm, the residual and a stride-2 expansion stay
    framework ops.  Everything else -- CPU tensors, other dtypes, set_conv_backend('torch'), a train-mode SyncBatchNorm over several
    ranks, drop_path_rate > 0 in train mode, a block `from_block` did not recognise (a real squeeze-excite, a stride on conv_pwl,
    another activation or norm) -- takes `_reference_forward`, the statements above on the block's own submodules."""

    def __init__(self, in_chs, out_chs, exp_ratio=4.0, stride=1, mid_chs=None, noskip=False, drop_path_rate=0.0):
        super().__init__()
        mid_chs = int(mid_chs) if mid_chs else _make_divisible(in_chs * exp_ratio)
        self.conv_exp = nn.Conv2d(in_chs, mid_chs, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(mid_chs)
        self.act1 = nn.SiLU(inplace=True)
        self.se = nn.Identity()
        self.conv_pwl = nn.Conv2d(mid_chs, out_chs, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(out_chs)
        self.has_residual = in_chs == out_chs and stride == 1 and not noskip
        self.drop_path_rate = float(drop_path_rate)
        self._recognised = True

    @classmethod
    def from_block(cls, block):
        """Adopts an existing edge-residual block by its attributes: the SAME submodule objects (so the same Parameters and buffers;
        nothing is copied).  The kernels are taken only when the block is recognised (`_recognise`)."""
        for name in _FUSED_PARTS:
            if not hasattr(block, name):
                raise ValueError("FusedInvertedResidual.from_block: the block has no '%s'" % name)
        self = cls.__new__(cls)
        nn.Module.__init__(self)
        for name in _FUSED_PARTS:
            setattr(self, name, getattr(block, name))
        self.se = getattr(block, "se", None)
        self.has_residual = bool(getattr(block, "has_residual", False))
        self.drop_path_rate = float(getattr(block, "drop_path_rate", 0.0))
        self._recognised = self._recognise()
        self.train(block.training)
        return self

    def _recognise(self):
        """True when the submodules are exactly what csrc/fused_mbconv.hip computes."""
        e, p = self.conv_exp, self.conv_pwl
        if not _conv3x3(e) or not _conv(p, 1, cin=e.out_channels, zeros=False):
            return False
        if not (_batchnorm(self.bn1, e.out_channels) and _batchnorm(self.bn2, p.out_channels) and isinstance(self.act1, nn.SiLU)):
            return False
        if not (self.se is None or type(self.se) is nn.Identity):
            return False
        return not self.has_residual or (e.stride == (1, 1) and e.in_channels == p.out_channels)

    def _norms(self):
        return (self.bn1, self.bn2)

    def _supported(self):
        from . import functional as TF
        e = self.conv_exp
        return TF.fused_mbconv_supported(e.in_channels, e.out_channels, self.conv_pwl.out_channels, e.stride[0])

    def _reference_forward(self, x):
        shortcut = x
        x = self.conv_exp(x)
        x = self.bn1(x)
        x = self.act1(x)
        if self.se is not None:
            x = self.se(x)
        x = self.conv_pwl(x)
        x = self.bn2(x)
        if self.has_residual:
            if self.drop_path_rate > 0:
                x = _drop_path(x, self.drop_path_rate, self.training)
            x += shortcut
        return x

    def _train_forward(self, x):
        y = self._conv3_train(self.conv_exp, self.bn1, self.act1, x)
        y = self.bn2(self.conv_pwl(y))
        return y + x if self.has_residual else y

    def _kernel_forward(self, x, return_stages=False):
        from . import functional as TF
        res = TF.fused_mbconv_eval(x, self.conv_exp.weight, TF._bn_eval_fold(self.bn1), self.conv_exp.stride[0], self.conv_pwl.weight,
                                   TF._bn_eval_fold(self.bn2), x if self.has_residual else None, return_stages=return_stages)
        if return_stages:
            return res[0], dict(mid=res[1])
        return res


class InvertedResidual(nn.Module):
    """The MBConv block WITHOUT a residual -- the first member of a stage, which changes the stride or the width -- on framework ops in
    the reference's op order (the one `_inverted_residual_forward` spells out, minus the memory and the residual).  It exists so that a
    backbone can be constructed without timm; it has no kernel path (a stride-2 depthwise kernel is not part of this package)."""

    def __init__(self, in_chs, out_chs, stride=1, exp_ratio=4.0, se_ratio=0.25, mid_chs=None, se_chs=None):
        super().__init__()
        if in_chs == out_chs and stride == 1:
            raise ValueError("InvertedResidual: a block of stride 1 and equal widths has a residual: MemoryInvertedResidual")
        mid_chs = int(mid_chs) if mid_chs else _make_divisible(in_chs * exp_ratio)
        se_chs = int(se_chs) if se_chs else _make_divisible(in_chs * se_ratio, 1)
        self.conv_pw = nn.Conv2d(in_chs, mid_chs, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(mid_chs)
        self.act1 = nn.SiLU(inplace=True)
        self.conv_dw = nn.Conv2d(mid_chs, mid_chs, 3, stride, 1, groups=mid_chs, bias=False)
        self.bn2 = nn.BatchNorm2d(mid_chs)
        self.act2 = nn.SiLU(inplace=True)
        self.se = SqueezeExcite(mid_chs, se_chs)
        self.conv_pwl = nn.Conv2d(mid_chs, out_chs, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(out_chs)
        self.has_residual = False
        self.drop_path_rate = 0.0

    def forward(self, x):
        x = self.act1(self.bn1(self.conv_pw(x)))
        x = self.act2(self.bn2(self.conv_dw(x)))
        x = self.se(x)
        return self.bn3(self.conv_pwl(x))


# per stage: runs of (kind, output width, stride of the first member, expansion ratio, members); kinds: 'cn' ConvBnAct with skip,
# 'er' fused (edge-residual), 'ir' inverted residual with squeeze-excite.  efficientnetv2_rw_s as timm 0.4.12 defines it
# (cn_r2_k3_s1_e1_c24_skip / er_r4_k3_s2_e4_c48 / er_r4_k3_s2_e4_c64 / ir_r6_k3_s2_e4_c128_se0.25 / ir_r9_k3_s1_e6_c160_se0.25 /
# ir_r15_k3_s2_e6_c272_se0.25, stem 24), cut into five stages as the reference cuts it (backbone/TemporalStereo.py:66-72).
ARCHS = {
    "efficientnetv2_rw_s": dict(
        stem=24, se_ratio=0.25,
        stages=((("cn", 24, 1, 1.0, 2),),
                (("er", 48, 2, 4.0, 4),),
                (("er", 64, 2, 4.0, 4),),
                (("ir", 128, 2, 4.0, 6), ("ir", 160, 1, 6.0, 9)),
                (("ir", 272, 2, 6.0, 15),)),
        out_channels=(0, 64, 128, 256, 320)),
}
_STAGES = ("block0", "block1", "block2", "block3", "block4")


class TemporalStereoBackbone(nn.Module):
    """The reference's backbone `TEMPORALSTEREO` (architecture/modeling/backbone/TemporalStereo.py:19-162): the two eyes concatenated
    along the batch, the stem, five stages, the three-level decoder, and the per-frame feature memories of the residual MBConv blocks
    kept in `prev_info['memories']`.  `_forward` and `forward` are the reference's, statement for statement, with `block_forward` for
    its `_block_forward` and a FeatureDecoder for its decoder lines.  State-dict keys are the reference module's: conv_stem.weight,
    bn1.*, block0.0.0.conv.weight, ..., block1.0.0.conv_exp.weight, ..., block3.0.1.conv_pw.weight, ..., conv32.*, deconv32_16.*,
    deconv16_8.*, deconv8_4.*.

    arch: a name in ARCHS or a table of the same form (dict(stem, se_ratio, stages, out_channels)).  The layout is built from the table
    of widths: there are no pretrained weights and nothing is downloaded (the reference asks timm for `pretrained=True`; load a
    checkpoint of the reference's backbone with load_state_dict).  `from_backbone(module)` adopts an existing reference backbone.

    Who runs what: the stem is a StemConv, block0's members ConvBnAct, the members of block1 / block2 FusedInvertedResidual, the
    residual members of block3 / block4 MemoryInvertedResidual, the decoder a FeatureDecoder -- each with its own routing (kernels in
    eval mode without a gradient).  The non-residual first member of a run in block3 / block4 is an InvertedResidual on framework ops.
    The StemConv and the FeatureDecoder are made at every call from the submodules registered on this module AT THAT MOMENT (they
    hold no state of their own), so a replaced child -- nn.SyncBatchNorm.convert_sync_batchnorm(model), `net.bn1 = ...` -- is what runs.
    In eval mode under no_grad `forward` opens a `WeightLayouts` and a `BNFolds` context for the call when none is open; nothing is
    kept between calls (a caller that wants layouts and folds kept across frames opens the contexts itself and refreshes them)."""

    def __init__(self, arch="efficientnetv2_rw_s", in_planes=3, memory_percent=1 / 4, norm='BN', activation='SiLU'):
        super().__init__()
        table = ARCHS[arch] if isinstance(arch, str) else dict(arch)
        self.in_planes, self.memory_percent, self.norm, self.activation = in_planes, memory_percent, norm, activation
        self.conv_stem = nn.Conv2d(in_planes, table["stem"], 3, 2, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(table["stem"])
        self.act1 = nn.SiLU(inplace=True)
        width, channels = table["stem"], []
        if len(table["stages"]) != 5:
            raise ValueError("TemporalStereoBackbone: the table holds five stages")
        for name, runs in zip(_STAGES, table["stages"]):
            seqs = []
            for kind, out, stride, exp, members in runs:
                blocks = []
                for i in range(members):
                    s = stride if i == 0 else 1
                    if kind == "cn":
                        blocks.append(ConvBnAct(width, out, s, skip=True))
                    elif kind == "er":
                        blocks.append(FusedInvertedResidual(width, out, exp, s))
                    elif kind == "ir" and width == out and s == 1:
                        blocks.append(MemoryInvertedResidual(width, exp, table["se_ratio"], memory_percent))
                    elif kind == "ir":
                        blocks.append(InvertedResidual(width, out, s, exp, table["se_ratio"]))
                    else:
                        raise ValueError("TemporalStereoBackbone: unknown block kind %r" % (kind,))
                    width = out
                seqs.append(nn.Sequential(*blocks))
            setattr(self, name, nn.Sequential(*seqs))
            channels.append(width)
        decoder = FeatureDecoder(channels, table["out_channels"], norm, activation)
        for name in _NAMES:
            setattr(self, name, getattr(decoder, name))

    @classmethod
    def from_backbone(cls, module):
        """Adopts an existing reference backbone: the stem's three submodules, every member of block0 .. block4 (ConvBnAct,
        FusedInvertedResidual and MemoryInvertedResidual `from_block` by the members' attributes; a member none of them takes -- the
        non-residual MBConv blocks -- is kept as it is) and the decoder's four.  Parameters and buffers are the SAME objects, nothing is
        copied: the module's state dict, optimizer and .to() keep working.  `model.backbone = TemporalStereoBackbone.from_backbone(
        model.backbone)` replaces the per-submodule recipe."""
        for name in ("conv_stem", "bn1", "act1") + _STAGES + _NAMES:
            if not hasattr(module, name):
                raise ValueError("TemporalStereoBackbone.from_backbone: the module has no '%s'" % name)
        self = cls.__new__(cls)
        nn.Module.__init__(self)
        self.in_planes = getattr(module, "in_planes", module.conv_stem.in_channels)
        self.memory_percent = getattr(module, "memory_percent", 1 / 4)
        self.norm, self.activation = getattr(module, "norm", None), getattr(module, "activation", None)
        self.conv_stem, self.bn1, self.act1 = module.conv_stem, module.bn1, module.act1

        def adopt(m):
            if isinstance(m, (ConvBnAct, FusedInvertedResidual, MemoryInvertedResidual)):
                return m
            if all(hasattr(m, n) for n in _FUSED_PARTS):
                return FusedInvertedResidual.from_block(m)
            if all(hasattr(m, n) for n in _MBCONV_PARTS):
                return MemoryInvertedResidual.from_block(m, self.memory_percent) if getattr(m, "has_residual", False) else m
            if all(hasattr(m, n) for n in ("conv", "bn1", "act1")):
                return ConvBnAct.from_block(m)
            return m
        for name in _STAGES:
            setattr(self, name, nn.Sequential(*[nn.Sequential(*[adopt(m) for m in seq]) for seq in getattr(module, name)]))
        decoder = FeatureDecoder.from_backbone(module, set_mode=False)
        for name in _NAMES:                     # (a plain nn.Conv2d is wrapped once: the wrapper shares its Parameters and is what is registered)
            setattr(self, name, getattr(decoder, name))
        self.training = module.training         # (every adopted submodule keeps the mode it has)
        return self

    @property
    def _parts(self):
        """(StemConv, FeatureDecoder) over the submodules registered on this module NOW.  Both are views without parameters of their
        own, kept out of the module registry so that the state-dict keys stay conv_stem.*, bn1.*, conv32.*, deconv*; they are made per
        call so that a child replaced after construction (a SyncBatchNorm conversion, an assignment) is the one that runs."""
        stem = StemConv.from_modules(self.conv_stem, self.bn1, self.act1)
        stem.training = self.training
        return stem, FeatureDecoder.from_backbone(self, set_mode=False)

    def _forward(self, x, memories):
        stem, decoder = self._parts
        memory_idx = 0
        out_memories = []
        x = stem(x)
        x = self.block0(x)
        x, out, memory_idx = block_forward(self.block1, x, self.memory_percent, memories, memory_idx)
        x4 = x
        out_memories.extend(out)
        x, out, memory_idx = block_forward(self.block2, x, self.memory_percent, memories, memory_idx)
        x8 = x
        out_memories.extend(out)
        x, out, memory_idx = block_forward(self.block3, x, self.memory_percent, memories, memory_idx)
        x16 = x
        out_memories.extend(out)
        x, out, memory_idx = block_forward(self.block4, x, self.memory_percent, memories, memory_idx)
        x32 = x
        out_memories.extend(out)
        return decoder(x4, x8, x16, x32), out_memories

    def forward(self, *input):
        if len(input) != 3:
            raise ValueError('expected input length 3 (got {} length input)'.format(len(input)))
        from . import functional as TF
        l_img, r_img, prev_info = input
        mem = prev_info.get('memories', [])
        B, _, _, _ = l_img.shape

        lr_img = torch.cat([l_img, r_img], dim=0)

        if not self.training and not torch.is_grad_enabled() and TF._LAYOUTS is None and TF._FOLDS is None and layers._hip_conv(lr_img):
            with TF.WeightLayouts(), TF.BNFolds():
                lr_fms, mem = self._forward(lr_img, mem)
        else:
            lr_fms, mem = self._forward(lr_img, mem)

        l_fms = [fms[:B] for fms in lr_fms]
        r_fms = [fms[B:] for fms in lr_fms]

        if self.memory_percent > 0:
            prev_info['memories'] = mem
        else:
            prev_info['memories'] = []

        return l_fms, r_fms, prev_info
