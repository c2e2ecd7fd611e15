"""fots_e2e.native -- the operators of FOTSNet that run on the package's own kernels: its depthwise 3x3 convolutions, its
InstanceNorms (with the activation behind them, the stem's mirror in front of them and the residual add of a block's tail),
its detection heads and attention gates, the gated merges of its feature merge, its dense 3x3 convolutions, its recogniser's
tail and its bias-free 1x1 convolutions with the shortcuts' BatchNorms.

The 22 depthwise convolutions of the network (`_SeparableBlock.conv_sep1[0]`, `_SeparableBlock.conv2[0]`, `_smooth(...)[0]`
in upconv1 / upconv2; tools/models.py:70-102 of the reference) are the largest single item of the end-to-end chain's
kernel time in stock torch (profiles/half_e2e.md).  `use_native_depthwise(net)` switches them to `DepthwiseConv3x3`, which
calls `rroi_align._ext.rroi_align.depthwise3x3` wherever `native_ok` holds and `nn.Conv2d.forward`
otherwise.  Opt-in, like `net.to(torch.bfloat16)`: the caller switches the network, the pipeline takes no new argument.
Inference only: a call that needs a gradient takes the stock path, so training is untouched.

The 52 `nn.InstanceNorm2d` of the network (49 run per pass) are the next item of that trace: MIOpen's spatial batch norm
in fp32, two ATen kernels and the casts around them in 16 bits, and a LeakyReLU / ReLU launch behind each.
`use_native_instancenorm(net)` switches them to `NativeInstanceNorm2d`, which calls
`rroi_align._ext.rroi_align.instance_norm` wherever `instancenorm_ok` holds, and lets a norm that is directly
followed by its activation inside an `nn.Sequential` apply that activation itself.  The same terms: opt-in, inference only.

The tail of `FOTSNet.forward` -- `_heads` twice per pass (three 1x1 convolutions that each read the 256-channel map, and
eleven elementwise launches on maps of 1 to 4 channels) and the convolution + sigmoid of `_gate` three times -- is one
launch per call after `use_native_heads(net)`: `rroi_align._ext.rroi_align.heads` / `gate` wherever `heads_ok`
holds, the stock methods otherwise.  The same terms once more.

The feature merge between them -- three times `up(a) + f * up(gate)`: a bilinear resize of the one-channel gate, a multiply
and an add over a 256-channel map, in the first merge also a resize of the coarser map -- is one launch per merge after
`use_native_merge(net)`: `rroi_align._ext.rroi_align.gated_merge` wherever `merge_ok` holds, the stock
expression otherwise.  The resize in front of `upconv1` / `upconv2` stays stock here: `fots_e2e.native_remainder` folds it into
the depthwise half of the block (`use_native_upconv`), and `_merge` hands such a block the map before its resize.

What `model.py` applies functionally around its norms -- the stem's `cat(x, -x)` and LeakyReLU in `_MirrorNorm` (twice per
pass, on the two largest tensors of the network), the ReLU behind `_PlainBlock.bn1`, and the shortcut add and activation
of all 17 residual blocks -- is folded into the norm's own launch after `use_native_blocks(net)`:
`rroi_align._ext.rroi_align.instance_norm_fused` wherever `fused_norm_ok` holds, the stock forward otherwise.

The 23 dense 3x3 convolutions -- stem, `layer0_1`, `layer1`, `layer2`, the recogniser's `conv5` - `conv9` -- are the last
large item on stock kernels.  In bfloat16 / float16 `use_native_conv3x3(net)` switches them to `DenseConv3x3`, which calls
`rroi_align._ext.rroi_align.conv3x3` (an implicit GEMM on the matrix cores, one launch, the ReLU of
`layer0_1` fused) wherever `conv3x3_ok` holds and `nn.Conv2d.forward` otherwise; float32 inputs always take the stock
path, and so does every shape class `_conv3x3_slower` lists.

The recogniser, `FOTSNet.forward_ocr`, runs once per pooled-width bucket, several times per image, and half of its launches
do no arithmetic worth one: nine functional LeakyReLUs, and a bias add and a log-softmax behind `conv11`.  After
`use_native_recogniser(net)` every activation is folded into the native call in front of it (`_conv3x3_run`,
`_instance_norm_run`) or behind it (`rroi_align._ext.rroi_align.act_maxpool2x1`: LeakyReLU + (2,1) max-pool), and the tail
-- `conv11`, its bias, the log-softmax -- is one launch, `rroi_align._ext.rroi_align.ocr_head`, each step
where its own predicate holds (`fused_norm_ok`, `conv3x3_ok`, `act_pool_ok`, `ocr_head_ok`) and the stock expression
otherwise.  `conv10_s` stays stock here (`fots_e2e.native_remainder.use_native_conv2x3` switches it).

The 29 bias-free 1x1 convolutions -- the pointwise halves of the separable blocks of `layer3` / `layer4`, the three
shortcuts `layerN.0.downsample[0]`, the laterals `feature1` - `feature4` and the pointwise halves of `upconv1` / `upconv2`
-- are the largest group of launches left on stock kernels.  In bfloat16 / float16 `use_native_conv1x1(net)` switches them
to `PointwiseConv1x1`, which calls `rroi_align._ext.rroi_align.conv1x1` (a GEMM per image on the matrix
cores, one launch) wherever `conv1x1_ok` holds and `nn.Conv2d.forward` otherwise, and the three shortcut pairs
(convolution, `nn.BatchNorm2d`) to `NativeShortcut`, which folds the eval-mode norm into that one launch wherever
`shortcut_ok` holds.  float32 inputs always take the stock path, and so does every shape class `_conv1x1_slower` lists.
The five 1x1 convolutions with a bias belong to the heads and the recogniser's head above.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _switching as _sw
from .model import FOTSNet, _MirrorNorm, _PlainBlock, _SeparableBlock

_DTYPES = (torch.float32, torch.bfloat16, torch.float16)
_CONV_DTYPES = (torch.bfloat16, torch.float16)   # the matrix-core convolutions': float32 keeps the stock kernels
_STRIDES = ((1, 1), (2, 2))

_ext = _sw.lazy_module("rroi_align._ext.rroi_align")   # the ctypes binding, loaded on first use


# --------------------------------------------------------------------------- the clauses every predicate shares
def _tensor_ok(x, dtypes=_DTYPES) -> bool:
    """A contiguous 4-D CUDA tensor of one of `dtypes` with 1 to 2^31 - 1 elements.  Every predicate asks this first: a CPU
    tensor is declined before a parameter is read or the library loaded."""
    return (isinstance(x, torch.Tensor) and x.is_cuda and x.dim() == 4 and x.dtype in dtypes and x.is_contiguous()
            and 0 < x.numel() < (1 << 31))


def _inference(*tensors) -> bool:
    """No autocast (it changes the stock module's output dtype: left to it), and no gradient needed by any of `tensors`
    (None: absent).  Every predicate asks this last."""
    return not torch.is_autocast_enabled() and not (torch.is_grad_enabled()
                                                    and any(t is not None and t.requires_grad for t in tensors))


def _conv_static_ok(m, kernel, padding, strides=_STRIDES) -> bool:
    """A convolution of exactly this kernel and padding, a stride of `strides`, no dilation, no bias, zero padding."""
    return (m.kernel_size == kernel and m.padding == padding and m.dilation == (1, 1) and m.stride in strides
            and m._parameters["bias"] is None and m.padding_mode == "zeros")


def _conv_operands_ok(m, x) -> bool:
    """x has the weight's dtype, device and input channels."""
    w = m._parameters["weight"]
    return x.dtype == w.dtype and w.device == x.device and x.size(1) == m.in_channels


def _conv_out_numel(m, x) -> int:
    """The elements of `m(x)` for a convolution whose padding keeps the size at stride 1."""
    s = m.stride[0]
    return x.size(0) * m.out_channels * ((x.size(2) - 1) // s + 1) * ((x.size(3) - 1) // s + 1)


def _matrix_conv_ok(m, x, static_ok) -> bool:
    """What the matrix-core convolutions ask of their operands: a 16-bit x, a module `static_ok` accepts, a contiguous
    weight of x's dtype on x's device, fewer than 2^31 elements out."""
    return (_tensor_ok(x, _CONV_DTYPES) and static_ok(m) and _conv_operands_ok(m, x)
            and m._parameters["weight"].is_contiguous() and _conv_out_numel(m, x) < (1 << 31))


# --------------------------------------------------------------------------- depthwise 3x3 convolution, DESIGN 5.10
def _static_ok(m) -> bool:
    """What of `native_ok` depends on the module alone: a depthwise 3x3, padding 1, stride 1 or 2, no bias."""
    return _conv_static_ok(m, (3, 3), (1, 1)) and m.groups == m.in_channels == m.out_channels


def native_ok(m, x) -> bool:
    """True where `m(x)` may run the native kernel: pure, no GPU needed to ask.  (Parameters are read from `_parameters`:
    the network asks 22 times per pass.)"""
    return (_tensor_ok(x) and _static_ok(m) and _conv_operands_ok(m, x)
            and _inference(x, m._parameters["weight"]))


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
    return _sw.swap_classes(net, ((nn.Conv2d, DepthwiseConv3x3),), enable, _static_ok)[0]


# --------------------------------------------------------------------------- InstanceNorm2d (+ activation), DESIGN 5.11
def instancenorm_ok(m, x) -> bool:
    """True where `m(x)` may run the native kernel: pure, no GPU needed to ask.  Instance statistics only (a module that
    tracks running statistics keeps the stock path, in training and in eval; so does a plane of one element, which the
    stock module refuses with a ValueError)."""
    return _inorm_ok(m, x, 1)


def _inorm_ok(m, x, widen) -> bool:
    """`instancenorm_ok` for a norm of `widen` times x's channels (2: the stem's mirror, which widens x on the way in)."""
    if not _tensor_ok(x):
        return False
    w = m._parameters.get("weight")
    b = None if w is None else m._parameters.get("bias")
    return (not m.track_running_stats and widen * x.size(1) == m.num_features
            and (widen == 1 or widen * x.numel() < (1 << 31))
            and x.size(2) * x.size(3) > 1 and not _inorm_slower(x)
            and (w is None or (w.dtype == x.dtype and w.device == x.device and b is not None))
            and _inference(x, w, b))


def _inorm_slower(x) -> bool:
    """The one shape class in which the native kernel measured slower than the stock one (profiles/native_instancenorm.md):
    float32, very many tiny planes -- 49,152 planes of 64 / 96 elements (the head's last norm on eight images' crops):
    77-85 us against MIOpen's 30-35; a workgroup per plane is mostly idle lanes there.  6,144 such planes win (12 against
    33 us) and so do 49,152 planes of 320 elements (93 against 157); the line between them is drawn by interpolation at
    16,384 planes and 128 elements.  The 16-bit types win at every measured shape (98 against 346 us in this one)."""
    return x.dtype == torch.float32 and x.size(2) * x.size(3) <= 128 and x.size(0) * x.size(1) > 16384


class NativeInstanceNorm2d(nn.InstanceNorm2d):
    """An `nn.InstanceNorm2d` (same parameters, same `state_dict` keys) whose forward runs the native kernel where
    `instancenorm_ok(self, x)` holds.  `fused_slope` (None: nothing absorbed) is the negative slope of an activation that
    `use_native_instancenorm` has folded into this module: it is applied on BOTH paths, so the pair computes the same
    function whichever path a call takes."""
    fused_slope = None

    def forward(self, x):
        slope = self.fused_slope
        if instancenorm_ok(self, x):
            p = self._parameters
            return _ext()._instance_norm_run(x, p.get("weight"), p.get("bias"), self.eps, 1.0 if slope is None else slope)
        y = super().forward(x)
        return y if slope is None else F.leaky_relu(y, slope)


class AbsorbedLeakyReLU(nn.LeakyReLU):
    """An `nn.LeakyReLU` whose work the `NativeInstanceNorm2d` in front of it does: returns its input."""

    def forward(self, x):
        return x


class AbsorbedReLU(nn.ReLU):
    """An `nn.ReLU` whose work the `NativeInstanceNorm2d` in front of it does: returns its input."""

    def forward(self, x):
        return x


_ABSORBED = {nn.LeakyReLU: AbsorbedLeakyReLU, nn.ReLU: AbsorbedReLU}


def use_native_instancenorm(net: nn.Module, enable: bool = True, fuse_activation: bool = True):
    """Switch every `nn.InstanceNorm2d` of `net` to `NativeInstanceNorm2d` (52 for `FOTSNet()`), and -- with
    `fuse_activation` -- let every switched norm that an `nn.Sequential` follows directly with an `nn.LeakyReLU` /
    `nn.ReLU` take over that activation's slope, the activation becoming a pass-through (20 pairs for `FOTSNet()`).  A pair
    is fused only where both modules occur once in `net`: a module that is also called from somewhere else keeps its
    meaning.  enable=False: every `NativeInstanceNorm2d` back, its slope removed and the activation behind it restored with
    it.  A norm that `native_train.use_trainable_instancenorm` has switched further is not this switch's to restore, so it
    keeps its slope and its pass-through activation, the call reports (0, 0) and the network computes what it did; undo
    the trainable switch first, and the same call restores everything.  Only classes change: no parameter is copied, no
    key of the state_dict moves.  Activations applied functionally (`F.leaky_relu` in a forward) stay what they are.
    How the switches compose and undo: `fots_e2e._switching`.  Returns (norms switched, activations switched)."""
    return _sw.swap_absorbing(net, nn.InstanceNorm2d, NativeInstanceNorm2d, _ABSORBED, enable, fuse_activation)


# --------------------------------------------------------------------------- detection heads and attention gate, DESIGN 5.12
_HEAD_CONVS = (("act", 1), ("rbox", 4), ("angle", 2))
_GATE_CONVS = (("conv_attenton", 1),)


def _pointwise_conv_ok(m, outputs, t) -> bool:
    """A plain 1x1, stride-1, ungrouped `nn.Conv2d` from t's channels to `outputs`, with t's dtype, on t's device, that
    needs no gradient."""
    if type(m) is not nn.Conv2d:
        return False
    w, b = m._parameters["weight"], m._parameters["bias"]
    return (m.kernel_size == (1, 1) and m.stride == (1, 1) and m.padding == (0, 0) and m.dilation == (1, 1)
            and m.groups == 1 and m.out_channels == outputs and m.in_channels == t.size(1) and m.padding_mode == "zeros"
            and w.dtype == t.dtype and w.device == t.device and (b is None or (b.dtype == t.dtype and b.device == t.device))
            and not (torch.is_grad_enabled() and (w.requires_grad or (b is not None and b.requires_grad))))


def heads_ok(net, t, gate: bool = False) -> bool:
    """True where `net._heads(t)` (gate=True: the convolution and sigmoid of `net._gate(t, like)`) may run the native
    kernel: pure, no GPU needed to ask.  No shape class is declined for speed: every measured one won
    (profiles/native_heads.md).
    (The clauses of `_tensor_ok` and `_inference` written out: through the helpers this predicate measured slower.)"""
    return (isinstance(t, torch.Tensor) and t.is_cuda and t.dim() == 4 and t.dtype in _DTYPES and t.is_contiguous()
            and 0 < t.numel() < (1 << 31)
            and not torch.is_autocast_enabled()
            and not (torch.is_grad_enabled() and t.requires_grad)
            and all(_pointwise_conv_ok(net._modules.get(name), k, t) for name, k in (_GATE_CONVS if gate else _HEAD_CONVS)))


def _wb(m):
    p = m._parameters
    return p["weight"], p["bias"]


class NativeHeadsFOTSNet(FOTSNet):
    """A `FOTSNet` (same modules, same `state_dict` keys) whose `_heads` and `_gate` run the native kernel where `heads_ok`
    holds."""

    def _heads(self, t):
        if heads_ok(self, t):
            return _ext()._heads_run(t, *_wb(self.act), *_wb(self.rbox), *_wb(self.angle), 128.0)
        return super()._heads(t)

    def _gate(self, t, like):
        if heads_ok(self, t, gate=True):
            return self._up(_ext()._gate_run(t, *_wb(self.conv_attenton)), like)
        return super()._gate(t, like)


def use_native_heads(net: nn.Module, enable: bool = True) -> bool:
    """Switch a network whose type is exactly `FOTSNet` to `NativeHeadsFOTSNet` (enable=False: back), and one that
    `use_native_merge` / `use_native_recogniser` have switched to the class that has the heads as well (`_NETS` below).
    Only the class of the network changes: no parameter is copied, no key of the state_dict moves.  A network of any
    other type is left alone.  Returns whether the class was switched."""
    return _sw.toggle_feature(net, _NETS, NativeHeadsFOTSNet, enable)


# --------------------------------------------------------------------------- the feature merge, DESIGN 5.14
def merge_ok(a, f, gate=None) -> bool:
    """True where `up(a) + f * up(gate)` (gate=None: `up(a) + f`) may run the native kernel: pure, no GPU needed to ask.
    CUDA tensors that are 4-D, contiguous, of one of the three dtypes, all of one dtype and device, `a` with f's batch
    size and channels, a one-channel gate with f's batch size, each of fewer than 2^31 elements, no autocast, no
    gradient needed."""
    ts = (f, a) if gate is None else (f, a, gate)
    if not _tensor_ok(f):
        return False
    like_f = (f.dtype,)
    return (all(_tensor_ok(t, like_f) and t.device == f.device for t in ts[1:])
            and a.shape[:2] == f.shape[:2] and (gate is None or (gate.size(0) == f.size(0) and gate.size(1) == 1))
            and not _merge_slower(a, f, gate) and _inference(*ts))


def _merge_slower(a, f, gate) -> bool:
    """The shape classes in which the native kernel measured slower than the stock chain (profiles/native_merge.md): none."""
    return False


class _NativeMerge:
    """Mixin in front of a `FOTSNet`: `_merge` runs each of the three merges, `up(a) + f * up(gate)`, as one native call
    where `merge_ok` holds, and as the stock expression where it does not.  The resize in front of `upconv1` / `upconv2`
    stays stock unless the block takes the unresized map itself (`_smoothed`).  A network in training mode takes the stock
    method."""

    def _low_gate(self, t):
        """The gate at its source's size, before the resize: the native gate where the network has it."""
        if isinstance(self, NativeHeadsFOTSNet) and heads_ok(self, t, gate=True):
            return _ext()._gate_run(t, *_wb(self.conv_attenton))
        return torch.sigmoid(self.conv_attenton(t))

    def _merge_one(self, a, f, t):
        """up(a) + f * up(gate of t), or up(a) + f for a network without attention; `a` of f's size is not resized."""
        g = self._low_gate(t) if self.attention else None
        if merge_ok(a, f, g):
            return _ext()._gated_merge_run(a, f, g)
        A = a if a.shape[2:] == f.shape[2:] else self._up(a, f)
        return A + f if g is None else A + f * self._up(g, f)

    def _smoothed(self, upconv, t, like):
        """upconv(up(t, like)); a block that can take the map before its resize (`native_remainder.UpSmooth`) is given it."""
        resized = getattr(upconv, "forward_resized", None)
        return upconv(self._up(t, like)) if resized is None else resized(t, like)

    def _merge(self, f1, f2, f3, f4):
        if self.training:
            return super()._merge(f1, f2, f3, f4)
        t = self._merge_one(f4, f3, f4)
        m2 = self._merge_one(self._smoothed(self.upconv1, t, f2), f2, t)
        m1 = self._merge_one(self._smoothed(self.upconv2, m2, f1), f1, m2)
        return m1, m2


class NativeMergeFOTSNet(_NativeMerge, FOTSNet):
    """A `FOTSNet` (same modules, same `state_dict` keys) whose three merges run the native kernel where `merge_ok` holds."""


class NativeHeadsMergeFOTSNet(_NativeMerge, NativeHeadsFOTSNet):
    """A `NativeHeadsFOTSNet` with the native merges: the gate kernel's output goes into the merge at its own size."""


def use_native_merge(net: nn.Module, enable: bool = True) -> bool:
    """Switch a network whose type is exactly `FOTSNet` to `NativeMergeFOTSNet` (enable=False: back), and one that
    `use_native_heads` / `use_native_recogniser` have switched to the class that has the merge as well (`_NETS` below).
    Only the class of the network changes: no parameter is copied, no key of the state_dict moves.  A network of any
    other type is left alone.  Returns whether the class was switched."""
    return _sw.toggle_feature(net, _NETS, _NativeMerge, enable)


# --------------------------------------------------------------------------- the stem's mirror and the blocks' tails, DESIGN 5.13
def fused_norm_ok(norm, t, residual=None, mirror: bool = False) -> bool:
    """True where `norm` on `t` may run `rroi_align._ext.rroi_align._instance_norm_fused_run` (with neither a residual
    nor the mirror: `_instance_norm_run` with a slope of the caller's): pure, no GPU needed to ask.  It is
    `instancenorm_ok(norm, t)` and
      residual   a contiguous tensor of t's shape, dtype and device that needs no gradient;
      mirror     an affine norm of twice t's channels, whose output stays below 2^31 elements;
      a norm to which `use_native_instancenorm` has given a `fused_slope` applies an activation of its own: declined."""
    if getattr(norm, "fused_slope", None) is not None:
        return False
    if mirror:
        return residual is None and norm._parameters.get("weight") is not None and _inorm_ok(norm, t, 2)
    if not _inorm_ok(norm, t, 1):
        return False
    return residual is None or (
        isinstance(residual, torch.Tensor) and residual.is_cuda and residual.shape == t.shape and residual.dtype == t.dtype
        and residual.device == t.device and residual.is_contiguous()
        and not (torch.is_grad_enabled() and residual.requires_grad))


def _block_input_ok(block, x) -> bool:
    """What can be asked before a block computes anything: where this fails, no predicate further down can hold, and the
    stock forward runs without anything having been computed twice.  (A block in training mode is left to the stock code
    whatever its input: the BatchNorm of a shortcut keeps running statistics.  Under grad mode the block's first
    parameter stands for all of them; under `torch.no_grad()`, where the pipeline runs, none is looked at.)"""
    return (not block.training and isinstance(x, torch.Tensor) and x.is_cuda and x.dim() == 4 and x.dtype in _DTYPES
            and x.numel() > 0 and not torch.is_autocast_enabled()
            and not (torch.is_grad_enabled() and (x.requires_grad or next(block.parameters()).requires_grad)))


def _affine(norm):
    p = norm._parameters
    return p.get("weight"), p.get("bias")


class NativeMirrorNorm(_MirrorNorm):
    """A `_MirrorNorm` (same module, same `state_dict` keys) whose negation, concatenation, norm and LeakyReLU are one
    native call where `fused_norm_ok(self.bn, x, mirror=True)` holds."""

    def forward(self, x):
        bn = self.bn
        if fused_norm_ok(bn, x, mirror=True):
            return _ext()._instance_norm_fused_run(x, *_affine(bn), bn.eps, 0.01, None, True)
        return super().forward(x)


class NativePlainBlock(_PlainBlock):
    """A `_PlainBlock` whose `bn1` + ReLU is one native call and whose `bn2` + shortcut + ReLU is another, where
    `fused_norm_ok` holds for both; the stock forward otherwise (what a late refusal had computed is computed again by
    it: the stock code is not restated here)."""

    def forward(self, x):
        if not _block_input_ok(self, x):
            return super().forward(x)
        bn1, bn2 = self.bn1, self.bn2
        t = self.conv1(x)
        if not fused_norm_ok(bn1, t):
            return super().forward(x)
        t = self.conv2(_ext()._instance_norm_run(t, *_affine(bn1), bn1.eps, 0.0))
        r = x if self.downsample is None else self.downsample(x)
        if not fused_norm_ok(bn2, t, residual=r):
            return super().forward(x)
        return _ext()._instance_norm_fused_run(t, *_affine(bn2), bn2.eps, float(self.slope), r, False)


class NativeSeparableBlock(_SeparableBlock):
    """A `_SeparableBlock` whose last norm, shortcut add and LeakyReLU are one native call where `fused_norm_ok` holds.
    The modules of `conv2` in front of that norm run as they are, so what `use_native_depthwise` and
    `use_native_instancenorm` made of them -- absorbed activations included -- keeps working."""

    def forward(self, x):
        if not _block_input_ok(self, x):
            return super().forward(x)
        t = self.conv_sep1(x)
        body = list(self.conv2._modules.values())
        for m in body[:-1]:
            t = m(t)
        last = body[-1]
        r = x if self.downsample is None else self.downsample(x)
        if not (isinstance(last, nn.InstanceNorm2d) and fused_norm_ok(last, t, residual=r)):
            return super().forward(x)
        return _ext()._instance_norm_fused_run(t, *_affine(last), last.eps, float(self.slope), r, False)


_BLOCKS = ((_MirrorNorm, NativeMirrorNorm), (_PlainBlock, NativePlainBlock), (_SeparableBlock, NativeSeparableBlock))


def use_native_blocks(net: nn.Module, enable: bool = True):
    """Switch every `_MirrorNorm`, `_PlainBlock` and `_SeparableBlock` of `net` -- by exact type -- to its native subclass
    (enable=False: back).  Only classes change: no parameter is copied, no key of the state_dict moves; the switches above
    compose with this one in any order.  Returns (mirror norms, plain blocks, separable blocks) switched: (2, 7, 10) for
    `FOTSNet()`."""
    return _sw.swap_classes(net, _BLOCKS, enable)


# --------------------------------------------------------------------------- dense 3x3 convolutions, bf16 / fp16, DESIGN 5.15

def _dense_static_ok(m) -> bool:
    """What of `conv3x3_ok` depends on the module alone: an exact 3x3, padding 1, stride 1 or 2, groups 1, no bias."""
    return _conv_static_ok(m, (3, 3), (1, 1)) and m.groups == 1


def conv3x3_ok(m, x) -> bool:
    """True where `m(x)` may run the native matrix-core kernel: pure, no GPU needed to ask.  A 16-bit dtype equal to the
    weight's (float32 keeps the stock Winograd kernels: DESIGN 5.15), a contiguous CUDA 4-D input of fewer than 2^31
    elements whose output stays below that too, no autocast, no gradient needed, and not one of the shape classes that
    measured slower (`_conv3x3_slower`)."""
    return _matrix_conv_ok(m, x, _dense_static_ok) and not _conv3x3_slower(m, x) and _inference(x, m._parameters["weight"])


def _conv3x3_slower(m, x) -> bool:
    """The shape classes in which the native kernel's median was not below the stock one's (profiles/native_conv3x3.md,
    microseconds per call, native / stock, bf16 | fp16).  With M = N * Cout * Ho * Wo * 9 * Cin multiply-adds:
      stride 1, M above 5.0e9 (bf16) / 2.5e9 (fp16): the kernel reaches 130-190 TFLOP/s where MIOpen's reach up to 470 --
        64>64 at 352x640 (M 8.3e9) 98/83 | 98/83; 256>256 on 24 crops (6.8e9) 106/81 | 106/52; every row of eight images
        or 192 crops, e.g. 128>128 at 88x160 x 8 (16.6e9) 172/98 | 172/100.  Below the line it wins: 64>64 at 176x320 and
        128>128 at 88x160 (2.1e9) 30/45 and 35/45 in both types, 64>128 on 24 crops (1.9e9) 24/59 | 23/45.  Between
        2.5e9 and 5.0e9 the types part -- 128>128 and 128>256 on 24 crops (3.7e9, 3.4e9): 56/83 and 45/75 in bf16, where
        the stock path has no Winograd kernel, 56/52 and 45.4/44.8 in fp16; the lines are drawn between the nearest
        measured rows on either side.
      stride 2, except Cout <= 32 with M <= 2.5e9: the input tile with its halo is four times the output tile, and the
        staging dominates -- 64>128 at 176x320 (1.0e9) 56/45 | 56/45, 64>64 at 352x640 (2.1e9) 59/54 | 59/50, 32>32 at
        704x1280 x 8 (16.6e9) 584/461 | 583/395; the stem's 32>32 at one image (2.1e9) wins 64/69 | 64.2/64.8.
    Fewer than 16 input channels (the stem's 3>16) win at every measured size, 27/62 at one image and 186/375 at eight."""
    if m.in_channels < 16:
        return False
    macs = _conv_out_numel(m, x) * 9 * m.in_channels
    if m.stride[0] == 2:
        return not (m.out_channels <= 32 and macs <= 2.5e9)
    return macs > (5.0e9 if x.dtype == torch.bfloat16 else 2.5e9)


class DenseConv3x3(nn.Conv2d):
    """An `nn.Conv2d` (same parameters, same `state_dict` keys) whose forward runs the native matrix-core kernel where
    `conv3x3_ok(self, x)` holds.  `fused_slope` (None: nothing absorbed) is the negative slope of an activation that
    `use_native_conv3x3` has folded into this module: it is applied on BOTH paths, so the pair computes the same function
    whichever path a call takes."""
    fused_slope = None

    def forward(self, x):
        slope = self.fused_slope
        if conv3x3_ok(self, x):
            return _ext()._conv3x3_run(x, self._parameters["weight"], self.stride[0], 1.0 if slope is None else slope)
        y = super().forward(x)
        if slope is None:
            return y
        return F.relu(y) if slope == 0.0 else F.leaky_relu(y, slope)


class ConvAppliedLeakyReLU(nn.LeakyReLU):
    """An `nn.LeakyReLU` whose work the `DenseConv3x3` in front of it does: returns its input.  (A class of this switch's
    own: `use_native_instancenorm(net, enable=False)` restores every `Absorbed*` and must not re-arm this one.)"""

    def forward(self, x):
        return x


class ConvAppliedReLU(nn.ReLU):
    """An `nn.ReLU` whose work the `DenseConv3x3` in front of it does: returns its input."""

    def forward(self, x):
        return x


_CONV_APPLIED = {nn.LeakyReLU: ConvAppliedLeakyReLU, nn.ReLU: ConvAppliedReLU}


def use_native_conv3x3(net: nn.Module, enable: bool = True, fuse_activation: bool = True):
    """Switch every qualifying `nn.Conv2d` of `net` -- by exact type: a dense 3x3, padding 1, stride 1 or 2, no bias -- to
    `DenseConv3x3` (23 for `FOTSNet()`: 18 in the trunk, conv5 - conv9), and -- with `fuse_activation` -- let every
    switched convolution that an `nn.Sequential` follows directly with an `nn.ReLU` / `nn.LeakyReLU` take over that
    activation's slope, the activation becoming a pass-through (the two pairs of `layer0_1` for `FOTSNet()`).  A pair is
    fused only where both modules occur once in `net`.  enable=False: every class back, every slope removed.  Only
    classes change: no parameter is copied, no key of the state_dict moves; the pass-through classes are this switch's
    own, so it and `use_native_instancenorm` leave each other's work alone in either order.  Whether a call runs the
    native kernel is decided per call by `conv3x3_ok` (float32 never does).  Returns (convolutions switched, activations
    absorbed)."""
    return _sw.swap_absorbing(net, nn.Conv2d, DenseConv3x3, _CONV_APPLIED, enable, fuse_activation, _dense_static_ok)


# --------------------------------------------------------------------------- the recogniser, DESIGN 5.16
_OCR_HEAD_MAX_CLASSES = 128   # RROI_OCR_HEAD_MAX_CLASSES of the header (the binding's OCR_HEAD_MAX_CLASSES)


def act_pool_ok(x, slope: float = 0.01) -> bool:
    """True where `F.max_pool2d(F.leaky_relu(x, slope), (2, 1), stride=(2, 1))` (slope 1.0: the pool alone) may run the
    native kernel: pure, no GPU needed to ask.  A contiguous CUDA 4-D tensor of one of the three dtypes with at least two
    rows and fewer than 2^31 elements, no autocast, no gradient needed, and not a class of `_act_pool_slower`."""
    return _tensor_ok(x) and x.size(2) >= 2 and not _act_pool_slower(x, slope) and _inference(x)


def _act_pool_slower(x, slope: float = 0.01) -> bool:
    """The shape classes in which the native kernel's median was not below the stock one's
    (profiles/native_recogniser.md, microseconds per call, native / stock; the three dtypes agree to about 1 us).
      With an activation to apply (slope != 1.0), against the stock pair: none -- all 54 rows win, 9.3 / 11.4 on 8 crops of
        32 columns up to 16.5 / 104.9 (bf16) and 27.4 / 134.7 (fp32) on 192 crops of 128.
      The pool alone (slope 1.0), against `F.max_pool2d` alone, where no launch is saved: below 3.0e6 elements -- both
        calls are then bound by what the host can issue, 8.8 - 9.4 for the call through ctypes against 5.5 - 8.1: every row
        of 8 crops (9.4 / 6.2), 24 crops of 32 columns (9.4 / 6.1) and of 64 (128 x 11 rows, 2.2e6 elements: 9.4 / 8.1;
        256 x 5 rows, 2.0e6: 9.3 / 6.9).  From 24 crops of 128 (3.9e6 and 4.3e6 elements) it wins, 9.5 / 11.4 and
        9.4 / 13.7, up to 16.5 / 81.8 on 192 crops of 128 (bf16); the line is drawn between the nearest measured rows,
        2.2e6 and 3.9e6 elements.  30 of 54 rows lose, 24 win."""
    return slope == 1.0 and x.numel() < 3.0e6


def ocr_head_ok(net, x) -> bool:
    """True where `F.log_softmax(net.conv11(x).squeeze(2), dim=1)` may run the native kernel: pure, no GPU needed to ask.
    A contiguous CUDA (N, C, 1, T) tensor of one of the three dtypes, `conv11` a plain 1x1 convolution from C channels
    with parameters of that dtype on that device and at most 128 classes, fewer than 2^31 elements in and out, no
    autocast, no gradient needed, and not a class of `_ocr_head_slower`."""
    if not (_tensor_ok(x) and x.size(2) == 1):
        return False
    m = net._modules.get("conv11")
    return (type(m) is nn.Conv2d and 1 <= m.out_channels <= _OCR_HEAD_MAX_CLASSES
            and _pointwise_conv_ok(m, m.out_channels, x) and m._parameters["weight"].is_contiguous()
            and x.size(0) * m.out_channels * x.size(3) < (1 << 31) and not _ocr_head_slower(m, x) and _inference(x))


def _ocr_head_slower(m, x) -> bool:
    """The shape classes in which the native kernel's median was not below that of the stock convolution + log-softmax
    (profiles/native_recogniser.md, 256 channels to 87 classes, microseconds per call, native / stock, fp32 | bf16 | fp16):
    more than 4,608 columns N * T.  A workgroup takes 16 columns and runs for 29 us whatever the grid, so up to 192
    workgroups the call takes 29 - 30 us -- 8 crops of 32 columns 28.9 / 42.7 | 29.5 / 41.7 | 29.8 / 41.6, 24 crops of 128
    (3,072 columns) 29.4 / 56.0 | 29.9 / 54.9 | 30.2 / 56.0 -- and beyond that it grows with the grid where the stock GEMM
    does not: 192 crops of 32 (6,144 columns) 43.0 / 43.0 | 44.6 / 41.7 | 44.1 / 41.7, of 128 117.7 / 68.6 | 122.9 / 60.4 |
    122.8 / 60.6.  All 18 rows of 8 and 24 crops win, all 9 of 192 crops do not; the line is drawn between the nearest
    measured rows, 3,072 and 6,144 columns."""
    return x.size(0) * x.size(3) > 4608


def _ocr_norm_act(norm, t):
    """act(norm(t)): one native call where `fused_norm_ok` holds."""
    if fused_norm_ok(norm, t):
        return _ext()._instance_norm_run(t, *_affine(norm), norm.eps, 0.01)
    return F.leaky_relu(norm(t), 0.01)


def _ocr_conv_act(conv, t, before_pool: bool):
    """act(conv(t)) -> (tensor, the slope the pool behind it still has to apply: 1.0 where the activation is done).  One
    native call where `use_native_conv3x3` has switched the module, it carries no slope of its own and `conv3x3_ok`
    holds; otherwise the module, and its activation either at once or -- in front of a pool -- left to the pool."""
    if isinstance(conv, DenseConv3x3) and conv.fused_slope is None and conv3x3_ok(conv, t):
        return _ext()._conv3x3_run(t, conv._parameters["weight"], conv.stride[0], 0.01), 1.0
    y = conv(t)
    return (y, 0.01) if before_pool else (F.leaky_relu(y, 0.01), 1.0)


def _ocr_pool(t, slope: float):
    """pool(act(t)), act of `slope` (1.0: already applied): one native call where `act_pool_ok` holds."""
    if act_pool_ok(t, slope):
        return _ext()._act_maxpool2x1_run(t, slope)
    if slope != 1.0:
        t = F.leaky_relu(t, slope)
    return F.max_pool2d(t, (2, 1), stride=(2, 1))


class _NativeRecogniser:
    """Mixin in front of a `FOTSNet`: `forward_ocr` with every activation folded into the call in front of it or behind it
    and the tail -- `conv11`, its bias, the log-softmax -- as one native call.  Each step asks its own predicate and runs
    the stock expression where that fails; nothing is computed twice.  `conv10_s` and the first convolution (whose input
    may be a non-contiguous crop view) stay on their modules.  A network in training mode takes the stock method."""

    def forward_ocr(self, x):
        if self.training:
            return super().forward_ocr(x)
        x = _ocr_norm_act(self.batch5, self.conv5(x))
        x, _ = _ocr_conv_act(self.conv6, x, False)
        x = _ocr_pool(*_ocr_conv_act(self.conv6, x, True))
        x = _ocr_norm_act(self.batch7, self.conv7(x))
        x, _ = _ocr_conv_act(self.conv8, x, False)
        x, _ = _ocr_conv_act(self.conv8, x, False)
        x, _ = _ocr_conv_act(self.conv9, x, False)
        x = _ocr_pool(*_ocr_conv_act(self.conv9, x, True))
        x = _ocr_norm_act(self.batch10_s, self.conv10_s(x))
        if ocr_head_ok(self, x):
            return _ext()._ocr_head_run(x, *_wb(self.conv11))
        return F.log_softmax(self.conv11(self.drop1(x)).squeeze(2), dim=1)


class NativeRecogniserFOTSNet(_NativeRecogniser, FOTSNet):
    """A `FOTSNet` (same modules, same `state_dict` keys) whose `forward_ocr` runs the native head and pools."""


class NativeHeadsRecogniserFOTSNet(_NativeRecogniser, NativeHeadsFOTSNet):
    """A `NativeHeadsFOTSNet` with the native recogniser."""


class NativeMergeRecogniserFOTSNet(_NativeRecogniser, NativeMergeFOTSNet):
    """A `NativeMergeFOTSNet` with the native recogniser."""


class NativeHeadsMergeRecogniserFOTSNet(_NativeRecogniser, NativeHeadsMergeFOTSNet):
    """A `NativeHeadsMergeFOTSNet` with the native recogniser."""


def use_native_recogniser(net: nn.Module, enable: bool = True) -> bool:
    """Switch a network whose type is exactly `FOTSNet`, `NativeHeadsFOTSNet`, `NativeMergeFOTSNet` or
    `NativeHeadsMergeFOTSNet` to the subclass of it with the native `forward_ocr` (enable=False: back to exactly that
    type).  Only the class of the network changes: no parameter is copied, no key of the state_dict moves.  A network of
    any other type is left alone.  Returns whether the class was switched."""
    return _sw.toggle_feature(net, _NETS, _NativeRecogniser, enable)


# The network classes by what they have: the heads from `NativeHeadsFOTSNet`, the merge from `_NativeMerge`, the recogniser
# from `_NativeRecogniser`.  Read off the classes above: a class added there is in the table, a combination left out is not.
# Each of the three switches toggles its own feature and nothing else, so they compose with each other, and with the
# module switches, in any order (`fots_e2e._switching` has the rules for all thirteen).
_FEATURES = (NativeHeadsFOTSNet, _NativeMerge, _NativeRecogniser)
_NETS = _sw.feature_table([c for c in list(globals().values()) if isinstance(c, type) and issubclass(c, FOTSNet)], _FEATURES)


# --------------------------------------------------------------------------- the 1x1 convolutions, DESIGN 5.17
def _pointwise_static_ok(m) -> bool:
    """What of `conv1x1_ok` depends on the module alone: an exact 1x1, no padding, stride 1 or 2, groups 1, no bias."""
    return _conv_static_ok(m, (1, 1), (0, 0)) and m.groups == 1


def conv1x1_ok(m, x) -> bool:
    """True where `m(x)` may run the native matrix-core kernel: pure, no GPU needed to ask.  A 16-bit dtype equal to the
    weight's (float32 keeps the stock path), a contiguous CUDA 4-D input of fewer than 2^31 elements whose output stays
    below that too, a contiguous weight on x's device, no autocast, no gradient needed, and not one of the shape classes
    that measured slower (`_conv1x1_slower`)."""
    return _matrix_conv_ok(m, x, _pointwise_static_ok) and not _conv1x1_slower(m, x) and _inference(x, m._parameters["weight"])


def _conv1x1_slower(m, x) -> bool:
    """The shape classes in which the native kernel's median was not below the stock one's (profiles/native_conv1x1.md,
    microseconds per call, native / stock, bf16 | fp16; a shortcut with its norm against `F.conv2d` + eval `BatchNorm2d`).
    With M = N * Cout * Ho * Wo * Cin multiply-adds: M above 5.5e9, at either stride -- the large maps of eight images,
    where the stock GEMM streams faster than this kernel's 2-byte stores: 64>256 at 176x320 x 8 (M 7.4e9) 86.7/74.2 |
    86.5/71.4, 256>256 at 88x160 x 8 (7.4e9) 50.4/49.8 | 51.5/51.2, 256>256 at 176x320 x 8 (29.5e9) 206/124 | 209/125.
    Below the line every measured row wins, 54 of 60: the nearest are 128>256 at 88x160 x 8 (3.7e9) 33.6/44.1 | 34.1/44.4
    and 256>256 at 176x320 x 1 (3.7e9) 28.5/45.4 | 29.0/45.5; every shape of one image does, 9.2-16.9 against 44.8-60.2
    (the stock path is a chain of launches there, bound by what the host can issue); the line is drawn between the nearest
    measured rows on either side, 3.7e9 and 7.4e9."""
    return _conv_out_numel(m, x) * m.in_channels > 5.5e9


class PointwiseConv1x1(nn.Conv2d):
    """An `nn.Conv2d` (same parameters, same `state_dict` keys) whose forward runs the native matrix-core kernel where
    `conv1x1_ok(self, x)` holds."""

    def forward(self, x):
        if conv1x1_ok(self, x):
            return _ext()._conv1x1_run(x, self._parameters["weight"], self.stride[0])
        return super().forward(x)


def _shortcut_pair(seq):
    """(convolution, norm) of a Sequential whose modules are exactly a qualifying 1x1 convolution and an `nn.BatchNorm2d`;
    None otherwise."""
    mods = list(seq._modules.values())
    if len(mods) != 2:
        return None
    conv, bn = mods
    if type(conv) not in (nn.Conv2d, PointwiseConv1x1) or type(bn) is not nn.BatchNorm2d or not _pointwise_static_ok(conv):
        return None
    return conv, bn


def shortcut_ok(seq, x) -> bool:
    """True where `seq(x)` -- a 1x1 convolution and the `nn.BatchNorm2d` behind it -- may run as ONE native call with the
    norm folded in: pure, no GPU needed to ask.  `conv1x1_ok` for the convolution, and a norm in eval mode that tracks
    running statistics and has both buffers, of the convolution's `out_channels`, its buffers and its parameters (both or
    neither) of x's dtype on x's device, none of which needs a gradient."""
    pair = _shortcut_pair(seq)
    if pair is None:
        return False
    conv, bn = pair
    if not conv1x1_ok(conv, x):
        return False
    mean, var = bn._buffers.get("running_mean"), bn._buffers.get("running_var")
    g, b = bn._parameters.get("weight"), bn._parameters.get("bias")
    if bn.training or not bn.track_running_stats or mean is None or var is None or bn.num_features != conv.out_channels:
        return False
    if (g is None) != (b is None):
        return False
    vectors = (mean, var) if g is None else (mean, var, g, b)
    return (all(v.dtype == x.dtype and v.device == x.device and v.is_contiguous() for v in vectors)
            and not (torch.is_grad_enabled() and g is not None and (g.requires_grad or b.requires_grad)))


class NativeShortcut(nn.Sequential):
    """An `nn.Sequential` of (1x1 convolution, `nn.BatchNorm2d`) -- the shortcut of a stage's first block; same modules,
    same `state_dict` keys -- that runs as one native call with the norm folded in where `shortcut_ok(self, x)` holds;
    otherwise the Sequential's own forward, which still runs a switched convolution natively and the stock norm."""

    def forward(self, x):
        if shortcut_ok(self, x):
            conv, bn = self._modules.values()
            return _ext()._conv1x1_run(x, conv._parameters["weight"], conv.stride[0], 1.0,
                                       (bn._parameters.get("weight"), bn._parameters.get("bias"),
                                        bn._buffers["running_mean"], bn._buffers["running_var"], bn.eps))
        return super().forward(x)


def use_native_conv1x1(net: nn.Module, enable: bool = True):
    """Switch every qualifying `nn.Conv2d` of `net` -- by exact type: a 1x1, no padding, stride 1 or 2, groups 1, no bias
    -- to `PointwiseConv1x1` (29 for `FOTSNet()`), and every `nn.Sequential` -- by exact type -- whose modules are exactly
    such a convolution and an `nn.BatchNorm2d` to `NativeShortcut` (3 for `FOTSNet()`).  enable=False: every class back.
    Only classes change: no parameter is copied, no key of the state_dict moves; the other switches test exact types, so
    they leave these classes alone and compose with this one in any order.  Whether a call runs the native kernel is
    decided per call by `conv1x1_ok` / `shortcut_ok` (float32 never does).  Returns (convolutions switched, shortcuts
    switched)."""
    return _sw.swap_classes(net, ((nn.Conv2d, PointwiseConv1x1), (nn.Sequential, NativeShortcut)), enable,
                            lambda m: _pointwise_static_ok(m) if type(m) is nn.Conv2d else _shortcut_pair(m) is not None)
