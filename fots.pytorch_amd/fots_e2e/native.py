"""fots_e2e.native -- the one operator of FOTSNet that runs on the package's own kernel: its depthwise 3x3 convolutions.

The 22 depthwise convolutions of the network (`_SeparableBlock.conv_sep1[0]`, `_SeparableBlock.conv2[0]`, `_smooth(...)[0]`
in upconv1 / upconv2; tools/models.py:70-102 of the reference) are the largest single item of the end-to-end chain's
kernel time in stock torch (profiles/half_e2e.md).  `use_native_depthwise(net)` switches them to `DepthwiseConv3x3`, which
calls `rroi_align._ext.rroi_align.depthwise3x3` wherever `native_ok` holds and `nn.Conv2d.forward`
otherwise.  Opt-in, like `net.to(torch.bfloat16)`: the caller switches the network, the pipeline takes no new argument.
Inference only: a call that needs a gradient takes the stock path, so training is untouched.
"""
import torch
import torch.nn as nn

_DTYPES = (torch.float32, torch.bfloat16, torch.float16)


def _static_ok(m) -> bool:
    """What of `native_ok` depends on the module alone: a depthwise 3x3, padding 1, stride 1 or 2, no bias."""
    return (m.kernel_size == (3, 3) and m.padding == (1, 1) and m.dilation == (1, 1) and m.stride in ((1, 1), (2, 2))
            and m.groups == m.in_channels == m.out_channels and m._parameters["bias"] is None and m.padding_mode == "zeros")


def native_ok(m, x) -> bool:
    """True where `m(x)` may run the native kernel: pure, no GPU needed to ask.  (Cheapest tests first, parameters read
    from `_parameters`: the network asks 22 times per pass.)"""
    w = m._parameters["weight"]
    return (isinstance(x, torch.Tensor) and x.is_cuda and x.dim() == 4 and x.dtype == w.dtype and x.dtype in _DTYPES
            and x.is_contiguous() and _static_ok(m) and x.size(1) == m.in_channels and w.device == x.device
            and 0 < x.numel() < (1 << 31)
            and not torch.is_autocast_enabled()   # (autocast changes the stock module's output dtype: left to it)
            and not (torch.is_grad_enabled() and (x.requires_grad or w.requires_grad)))


_EXT = []


def _ext():
    """The ctypes binding, loaded on first use: asking `native_ok` needs neither the library nor a GPU."""
    if not _EXT:
        from rroi_align._ext import rroi_align as ext
        _EXT.append(ext)
    return _EXT[0]


class DepthwiseConv3x3(nn.Conv2d):
    """An `nn.Conv2d` (same parameters, same `state_dict` keys) whose forward runs the native depthwise kernel where
    `native_ok(self, x)` holds."""

    def forward(self, x):
        if native_ok(self, x):
            return _ext()._depthwise3x3_run(x, self._parameters["weight"], self.stride[0])
        return super().forward(x)


def use_native_depthwise(net: nn.Module, enable: bool = True) -> int:
    """Switch every qualifying `nn.Conv2d` of `net` to `DepthwiseConv3x3` (enable=False: back).  Only the class of the
    module changes: no parameter is copied, no key of the state_dict moves.  Returns the number of modules switched
    (22 for `FOTSNet()`)."""
    src, dst = (nn.Conv2d, DepthwiseConv3x3) if enable else (DepthwiseConv3x3, nn.Conv2d)
    n = 0
    for m in net.modules():
        if type(m) is src and (not enable or _static_ok(m)):
            m.__class__ = dst
            n += 1
    return n
