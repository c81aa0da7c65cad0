"""ConvGRU: the gated recurrent cell of the reference's `layers` package (architecture/modeling/layers/conv_gru.py:4-28), with its
constructor, attributes, state-dict keys (`convz.*`, `convr.*`, `convq.*`) and `forward(last_hidden, x)`.

    z = sigmoid(convz([h, x]))     r = sigmoid(convr([h, x]))     q = tanh(convq([r * h, x]))     hidden = (1 - z) * h + z * q

The three convolutions are 3x3, padding 1, with bias, over the in_planes + hidden_planes channels of the concatenation.  On fp32 GPU
tensors with the 'hip' convolution backend and at most 64 planes on either side the step is functional.conv_gru: two launches after
one weight-layout launch, no concatenation, no gate plane read twice (csrc/conv_gru.hip).  Everything else -- CPU tensors, other
dtypes, set_conv_backend('torch'), wider cells -- takes `_reference_forward`, the same operations on the Conv2d wrappers.  The module
takes one path for a given configuration whatever the plane size, so its bits do not depend on the shape.
"""
import torch
import torch.nn as nn

from . import layers


class ConvGRU(nn.Module):
    def __init__(self, in_planes, hidden_planes):
        super().__init__()
        self.in_planes = in_planes
        self.hidden_planes = hidden_planes
        fused = in_planes + hidden_planes
        self.convz = layers.Conv2d(fused, hidden_planes, 3, padding=1)
        self.convr = layers.Conv2d(fused, hidden_planes, 3, padding=1)
        self.convq = layers.Conv2d(fused, hidden_planes, 3, padding=1)

    def _reference_forward(self, last_hidden, x):
        both = torch.cat((last_hidden, x), dim=1)
        z = torch.sigmoid(self.convz(both))
        r = torch.sigmoid(self.convr(both))
        q = torch.tanh(self.convq(torch.cat((r * last_hidden, x), dim=1)))
        return (1 - z) * last_hidden + z * q

    def _on_kernels(self, last_hidden, x):
        from . import functional as TF
        return (layers._hip_conv(last_hidden) and layers._hip_conv(x) and last_hidden.dim() == 4 and x.dim() == 4 and
                self.convz.weight.is_cuda and self.convz.weight.dtype == torch.float32 and
                TF.conv_gru_supported(self.hidden_planes, self.in_planes))

    def forward(self, last_hidden, x):
        if self._on_kernels(last_hidden, x):
            from . import functional as TF
            return TF.conv_gru(last_hidden, x, self.convz.weight, self.convz.bias, self.convr.weight, self.convr.bias,
                               self.convq.weight, self.convq.bias)
        return self._reference_forward(last_hidden, x)
