"""fots_e2e.native_remainder -- the last stock operators of a 16-bit pass of FOTSNet on the package's own kernels.

With the eight switches of `fots_e2e.native` on and every kernel forced, one `forward` and one `forward_ocr` still run
three ATen operators that compute something: the recogniser's (2,3) convolution `conv10_s`, and the two
bilinear resizes in front of `upconv1` / `upconv2`.  Two more switches, with the same terms as the eight -- opt-in, only
classes change, inference only, each call asks a pure predicate and runs the stock expression where it fails:

`use_native_conv2x3(net)` switches `conv10_s` to `DenseConv2x3`, which calls
`rroi_align._ext.rroi_align.remainder.conv2x3` (an implicit GEMM on the matrix cores, one launch, a fixed
summation order) wherever `conv2x3_ok` holds, in bfloat16 / float16.  `conv10_s` was the one operator that made the fully
switched `forward_ocr` differ from call to call.

`use_native_upconv(net)` switches the two `_smooth` blocks to `UpSmooth`, whose `forward_resized(t, like)` runs the resize
and the depthwise half of the block as one call of `rroi_align._ext.rroi_align.remainder.up_depthwise3x3`
wherever `up_depthwise_ok` holds, in all three dtypes: the resized 256-channel map is never written.  The 1x1 half runs as
the module it is.

They live in a module of their own because the names of `fots_e2e.native` -- its `_*_slower` hooks above all -- are a
closed list that the network tests read."""
import torch
import torch.nn as nn

from . import _switching as _sw
from . import native as _nat
from .model import FOTSNet

_rem = _sw.lazy_module("rroi_align._ext.rroi_align.remainder")   # the binding of the two kernels, loaded on first use


# --------------------------------------------------------------------------- the (2,3) convolution, bf16 / fp16, DESIGN 5.19
def _conv2x3_static_ok(m) -> bool:
    """What of `conv2x3_ok` depends on the module alone: an exact (2,3), padding (0,1), stride 1, groups 1, no bias."""
    return _nat._conv_static_ok(m, (2, 3), (0, 1), ((1, 1),)) and m.groups == 1


def conv2x3_ok(m, x) -> bool:
    """True where `m(x)` may run the native matrix-core kernel: pure, no GPU needed to ask.  The clauses of
    `native.conv3x3_ok`: a 16-bit dtype equal to the weight's (float32 keeps the stock path), a contiguous CUDA 4-D input
    of at least two rows and fewer than 2^31 elements whose output stays below that too, a contiguous weight on x's
    device, no autocast, no gradient needed, and not one of the shape classes that measured slower (`_conv2x3_slower`)."""
    w = m._parameters["weight"]
    return (_nat._tensor_ok(x, _nat._CONV_DTYPES) and _conv2x3_static_ok(m) and _nat._conv_operands_ok(m, x)
            and w.is_contiguous() and x.size(2) >= 2 and x.size(0) * m.out_channels * (x.size(2) - 1) * x.size(3) < (1 << 31)
            and not _conv2x3_slower(m, x) and _nat._inference(x, w))


def _conv2x3_slower(m, x) -> bool:
    """The shape classes in which the native kernel's median was not below the stock one's (profiles/native_remainder.md,
    256 > 256 channels, (N, 256, 2, T), microseconds per call, native / stock, bf16 | fp16): more than 9,216 output columns
    N * (H - 1) * W.  Up to 192 workgroups the call takes 30 us at T = 32 and 43 - 45 us at T = 64 / 128 whatever the grid,
    against a stock chain of some 45 us: 8 crops of 32 columns 30.2 / 45.4 | 30.3 / 45.5, 24 crops of 64 45.0 / 45.3 |
    45.0 / 45.5 (the closest rows: 1 %), 24 crops of 128 (3,072 columns) 43.5 / 44.8 | 43.5 / 45.5, 192 crops of 32 (6,144)
    32.2 / 67.5 | 32.2 / 44.7.  Beyond that it grows with the grid where MIOpen's kernels do not: 192 crops of 64 (12,288
    columns) 119.2 / 82.1 | 118.9 / 54.0, of 128 188.1 / 112.7 | 188.3 / 70.3.  14 of 18 rows win, the 4 of 192 crops at
    T >= 64 do not; the line is drawn between the nearest measured rows, 6,144 and 12,288 columns."""
    return x.size(0) * (x.size(2) - 1) * x.size(3) > 9216


class DenseConv2x3(nn.Conv2d):
    """An `nn.Conv2d` (same parameters, same `state_dict` keys) whose forward runs the native matrix-core kernel where
    `conv2x3_ok(self, x)` holds."""

    def forward(self, x):
        if conv2x3_ok(self, x):
            return _rem().run_conv2x3(x, self._parameters["weight"])
        return super().forward(x)


def use_native_conv2x3(net: nn.Module, enable: bool = True) -> int:
    """Switch every qualifying `nn.Conv2d` of `net` -- by exact type: a (2,3) kernel, padding (0,1), stride 1, dilation 1,
    groups 1, no bias, zero padding -- to `DenseConv2x3` (enable=False: back).  Only the class of the module changes: no
    parameter is copied, no key of the state_dict moves; the other switches test exact types and other kernel sizes, so
    it composes with them in any order.  `FOTSNet.forward_ocr` calls `self.conv10_s(x)`, stock or native recogniser, and so
    picks the class up.  Whether a call runs the native kernel is decided per call by `conv2x3_ok` (float32 never does).
    Returns the number of modules switched (1 for `FOTSNet()`)."""
    return _sw.swap_classes(net, ((nn.Conv2d, DenseConv2x3),), enable, _conv2x3_static_ok)[0]


# --------------------------------------------------------------------------- resize + depthwise 3x3, DESIGN 5.20
def _smooth_pair(seq):
    """(depthwise 3x3, 1x1) of a Sequential whose modules are exactly a qualifying depthwise 3x3 convolution at stride 1 and
    a 1x1 convolution from its channels, whatever `use_native_depthwise` / `use_native_conv1x1` have made of their classes;
    None otherwise."""
    mods = list(seq._modules.values())
    if len(mods) != 2:
        return None
    dw, pw = mods
    if type(dw) not in (nn.Conv2d, _nat.DepthwiseConv3x3) or type(pw) not in (nn.Conv2d, _nat.PointwiseConv1x1):
        return None
    if not (_nat._static_ok(dw) and dw.stride == (1, 1)):
        return None
    if not (pw.kernel_size == (1, 1) and pw.stride == (1, 1) and pw.padding == (0, 0) and pw.dilation == (1, 1)
            and pw.groups == 1 and pw.in_channels == dw.out_channels):
        return None
    return dw, pw


def up_depthwise_ok(seq, t, like) -> bool:
    """True where the resize of `t` to `like`'s size and the depthwise convolution `seq[0]` behind it may run as ONE
    native call: pure, no GPU needed to ask.  `t` a contiguous 4-D CUDA tensor of one of the three dtypes and `like` a 4-D
    tensor; a first module that is a depthwise 3x3 (padding 1, no bias) at stride 1, whatever its class, with a weight of
    t's dtype on t's device and t's channels; fewer than 2^31 elements in and out; no autocast, no gradient needed; not a
    class of `_up_depthwise_slower`."""
    mods = seq._modules
    dw = next(iter(mods.values())) if mods else None
    # (the clauses of `native._tensor_ok` and `native._inference` written out: through the helpers this one measured slower)
    if not (isinstance(dw, nn.Conv2d) and isinstance(t, torch.Tensor) and isinstance(like, torch.Tensor) and t.is_cuda
            and t.dim() == 4 and like.dim() == 4 and t.dtype in _nat._DTYPES and t.is_contiguous()):
        return False
    w = dw._parameters["weight"]
    return (_nat._static_ok(dw) and dw.stride == (1, 1) and w.dtype == t.dtype and w.device == t.device
            and t.size(1) == dw.in_channels and 0 < t.numel() < (1 << 31)
            and 0 < t.size(0) * t.size(1) * like.size(2) * like.size(3) < (1 << 31)
            and not _up_depthwise_slower(seq, t, like)
            and not torch.is_autocast_enabled()
            and not (torch.is_grad_enabled() and (t.requires_grad or w.requires_grad)))


def _up_depthwise_slower(seq, t, like) -> bool:
    """The shape classes in which the fused call's median was not below that of the stock resize followed by the native
    depthwise kernel (profiles/native_remainder.md, 256 channels, microseconds per call, fused / unfused, fp32 | bf16 |
    fp16): none.  All 12 rows win: 44x80 > 88x160 on one image 14.7 / 94.1 | 14.8 / 64.9 | 14.8 / 58.6, on eight 78.9 / 773.8 |
    79.6 / 733.5 | 79.9 / 681.6; 88x160 > 176x320 on one image 43.4 / 106.6 | 39.3 / 111.8 | 39.4 / 105.0, on eight
    338.8 / 1136.7 | 305.2 / 1077.2 | 306.5 / 1027.7."""
    return False


class UpSmooth(nn.Sequential):
    """An `nn.Sequential` of (depthwise 3x3, 1x1) -- `upconv1` / `upconv2`; same modules, same `state_dict` keys -- that can
    take the map BEFORE its resize.  Called as a module it is the Sequential it was."""

    def forward_resized(self, t, like):
        """`self(up(t, like))`: the resize and the depthwise convolution as one native call where `up_depthwise_ok` holds,
        then the Sequential's second module as it is."""
        if up_depthwise_ok(self, t, like):
            dw, pw = self._modules.values()
            return pw(_rem().run_up_depthwise3x3(t, dw._parameters["weight"], (like.size(2), like.size(3))))
        return self(FOTSNet._up(t, like))


def use_native_upconv(net: nn.Module, enable: bool = True) -> int:
    """Switch every `nn.Sequential` of `net` -- by exact type -- whose modules are exactly a qualifying depthwise 3x3 at
    stride 1 and a 1x1 convolution to `UpSmooth` (enable=False: back).  Only the class changes: no parameter is copied, no
    key of the state_dict moves, and the classes of the two convolutions are left as they are, so it composes with the
    other switches in any order.  Without `use_native_merge` this switch has NO effect on what runs: only the native
    merge (`native._NativeMerge._merge`) hands the block the map before its resize; the stock `FOTSNet._merge` resizes
    first and calls the block as the Sequential it is.  Returns the number of blocks switched (2 for `FOTSNet()`)."""
    return _sw.swap_classes(net, ((nn.Sequential, UpSmooth),), enable, lambda m: _smooth_pair(m) is not None)[0]
