"""The network's TRAINING pass against a float64 twin, stage by stage: what test_training_twin.py (CPU) and
test_gpu_training_network.py (MI355X) share.  The counterpart of network_cases.py, whose stage table, `drive`, `rel` and
forward MUTATIONS it reuses.

  network, twin   fresh networks in `.train()` with `drop1.eval()` (the one dropout: its masks differ between dtypes and
                  devices, so no mask may take part in a comparison); BatchNorm runs on batch statistics.  `training=False`
                  gives the whole network in `.eval()` with gradients still needed: frozen-BatchNorm fine-tuning.
  train_step      one training step of ONE stage: the inputs are leaves that require a gradient, one cotangent per output
                  is drawn from a generator seeded by the stage's name and rounded to the dtype, `zero_grad(set_to_none)`
                  comes first (`conv_attenton` and the head convolutions are shared between calls and stages), then
                  `torch.autograd.backward`.  -> the outputs, the input gradients, the gradient of every parameter touched.
  figures         every tensor of a step against the twin's: (kind, name) -> (rel, elements), kind one of "out", "din",
                  "dparam".  A gradient that is None where the twin has one is an infinite error, not a skipped row.
  BACKWARD        ten ways in which the BACKWARD of the composition can be wrong while its forward is right bit for bit,
                  each a context manager on a stock network; TRAIN_MUTATIONS adds the twelve forward ones.

float32 is the asserting instrument for gradients.  On the CPU the stock float32 network is within H_MEASURED = 4.04e-5 of
the twin on every output, input gradient and parameter gradient, and the weakest mutation, at its most visible tensor, is
W_MEASURED off; FP32_CAP is their geometric mean, and test_training_twin.py asserts a decade of room on either side.  The
stock bfloat16 gradients are themselves 1e-2 to 0.3 off the twin, so in bfloat16 a gradient is held to the blunt ratio
rule `rel_native <= RATIO_CAP * max(rel_stock, 2^-8)` on tensors of at least RATIO_MIN_ELEMENTS elements."""
import contextlib
import copy
import math
import zlib
from typing import Dict, NamedTuple, Tuple

import torch
import torch.nn.functional as F

import network_cases as C

# Measured on the CPU by test_training_twin.py (profiles/native_training_network.md), float32, both inputs:
# the honest worst over all stages and tensors: the two-element angle.bias at _heads(m1), 2x64x96 -- a sum over 768 positions
# through the angle's normalisation, ill-conditioned where the pair is short, which moves with the order the CPU's
# convolutions sum in: 4.04e-5 on one thread, 1.42e-5 on 2 to 16, 7.6e-6 on 32.  The largest of them is taken.
H_MEASURED = 4.04e-5
W_MEASURED = 8.07e-3       # the weakest mutation's largest error over its stages: M3, ReLU for LeakyReLU(0.01) in layer4.1
FP32_CAP = math.sqrt(H_MEASURED * W_MEASURED)          # the geometric mean of the two
BF16_FLOOR = 2.0 ** -8     # one rounding to bfloat16, which a correctly rounded gradient may show
RATIO_MIN_ELEMENTS = 64    # smaller gradients (the one- to four-element biases of the heads and the gate) are asserted in
                           # float32 only: their stock bfloat16 error reached 0.29 on the CPU

# The hooks that decline a shape class for speed, by module: test_gpu_training_network.py forces all of them to False.
# network_cases.SLOWER_HOOKS is the list of fots_e2e.native; these are the lists of the three modules beside it.
BACKWARD_HOOKS = {"fots_e2e.native_train": ("_dw_backward_slower", "_inorm_backward_slower", "_merge_backward_slower"),
                  "fots_e2e.native_train_heads": ("_heads_backward_slower",),
                  "fots_e2e.native_remainder": ("_conv2x3_slower", "_up_depthwise_slower")}


def every_hook():
    """[(module, hook name)] of every `_*_slower` hook of the four switch modules; the lists above must be all of them."""
    import importlib
    from fots_e2e import native as nat
    found = [(nat, k) for k in C.slower_hooks()]
    for path, names in BACKWARD_HOOKS.items():
        mod = importlib.import_module(path)
        own = tuple(sorted(k for k, v in vars(mod).items()
                           if k.startswith("_") and k.endswith("_slower") and getattr(v, "__module__", None) == path))
        assert own == tuple(sorted(names)), (path, own)
        found += [(mod, k) for k in own]
    assert sum(k.endswith("_backward_slower") for _, k in found) == 4
    return found


# --------------------------------------------------------------------------- networks
def train_mode(net, training=True):
    net.train(training)
    net.drop1.eval()
    return net


def network(dtype=None, training=True):
    """A fresh network: train mode moves the running statistics, so none is shared between tests."""
    return train_mode(C.network(dtype), training)


def twin(net):
    """The float64 copy of the unswitched network on the CPU, every module in the mode `net` has it in."""
    from fots_e2e.model import FOTSNet
    assert type(net) is FOTSNet, "the twin is taken of the unswitched network"
    tw = copy.deepcopy(net).double().cpu()
    assert [m.training for m in tw.modules()] == [m.training for m in net.modules()] and not tw.drop1.training
    return tw


def glue_is_not_overridden():
    """`forward` and `forward_features` of every network class a switch can make are FOTSNet's own functions: what lies
    between the stages of the table (the dropouts, the order of the calls) is the same code in every configuration, and the
    table covers everything a trainable class replaces."""
    from fots_e2e import native as nat, native_train as T, native_train_heads as TH
    from fots_e2e.model import FOTSNet
    classes = {c for table in (nat._NETS, T._NETS, TH._NETS) for c in table.values()} | {FOTSNet}
    assert len(classes) >= 1 + 7 + 4 + 6
    for c in classes:
        assert issubclass(c, FOTSNet) and c.forward is FOTSNet.forward, c
        assert c.forward_features is FOTSNet.forward_features and c._up is FOTSNet._up, c
    return classes


# --------------------------------------------------------------------------- one training step of one stage
class Step(NamedTuple):
    outs: Tuple[torch.Tensor, ...]
    dins: Tuple[torch.Tensor, ...]                  # None where autograd gave the input no gradient
    dparams: Dict[str, torch.Tensor]                # name -> gradient, of every parameter the stage touched


def cotangents(stage, outs, dtype):
    """One cotangent per output, from a generator seeded by the stage's name, rounded to `dtype`, on the CPU."""
    g = torch.Generator().manual_seed(zlib.crc32(stage.name.encode()) & 0x7FFFFFFF)
    return tuple(torch.randn(o.shape, generator=g).to(dtype) for o in outs)


def train_step(net, call, ins, cots=None, stage=None):
    """`cots` None: drawn for `stage` in the outputs' dtype.  -> (Step, the cotangents on the CPU)."""
    leaves = [t.detach().clone().requires_grad_(True) for t in ins]
    net.zero_grad(set_to_none=True)
    outs = C.as_tuple(call(net, *leaves))
    if cots is None:
        cots = cotangents(stage, outs, outs[0].dtype)
    assert len(cots) == len(outs) and all(c.shape == o.shape for c, o in zip(cots, outs))
    torch.autograd.backward(outs, [c.to(device=o.device, dtype=o.dtype) for c, o in zip(cots, outs)])
    dparams = {k: p.grad for k, p in net.named_parameters() if p.grad is not None}
    step = Step(tuple(o.detach() for o in outs), tuple(t.grad for t in leaves), dparams)
    net.zero_grad(set_to_none=True)
    return step, cots


def twin_step(tw, stage, ins, cots):
    return train_step(tw, stage.on_twin, [t.detach().double().cpu() for t in ins], [c.double() for c in cots])[0]


# --------------------------------------------------------------------------- the reference at a kink
# A ReLU or LeakyReLU whose input lies within float32's own forward error of zero has no one derivative to compare with: the
# float64 twin takes one side, a correct float32 path may land on the other, and ONE such element costs sqrt(2 / n) of an
# n-element gradient -- 9e-3 at 24,576 elements, above any cap float32 can otherwise keep.  It is no rarity: of the 5.0e6
# activation inputs of one pass over both inputs, 4 lie within 1e-6 of their tensor's RMS of zero, 15 within 4e-6, 45
# within 1e-5 (CPU, twin), and on the MI355X the stock float32 copy and the switched network missed layer2.3 (2x64x96) by
# the same 5.710e-3 in the same tensors.  So the float32 reference of a stage is the twin with each such element on
# either side: `twin_references` yields them, `nearest_reference` takes the ONE whose worst figure over all tensors of the
# stage is smallest, and every tensor is then held to that one float64 step.  KINK_GUARD is four times the largest
# relative L2 error of a stock float32 output (6.6e-7 to 1e-6), the tail of an element's error; more than MAX_KINKS such
# elements in one stage is an error, not a wider search.  (The (2,1) max-pools of `forward_ocr` can tie in the same way and
# are not handled: their inputs are 0.3 e6 pairs per pass.)
KINK_GUARD = 4e-6
MAX_KINKS = 8


@contextlib.contextmanager
def _kinks(found, flip=frozenset()):
    """Under it, every F.relu / F.leaky_relu of a float64 tensor appends (call number, flat index) of its elements within
    KINK_GUARD of zero to `found`, and takes the OTHER side for those of them that are in `flip`."""
    calls = [0]

    def wrap(fn, slope_of):
        def act(x, *a, **k):
            if x.dtype != torch.float64:
                return fn(x, *a, **k)
            call, slope = calls[0], slope_of(*a, **k)
            calls[0] += 1
            v = x.detach()
            near = (v.abs() < KINK_GUARD * v.pow(2).mean().sqrt()).flatten().nonzero().flatten().tolist()
            found.extend((call, i) for i in near)
            mine = [i for c, i in flip if c == call]
            y = fn(x, *a, **k)
            if not mine:
                return y
            other = torch.zeros(x.numel(), dtype=torch.bool)
            other[mine] = True
            other = other.view_as(x)
            return torch.where(other, x * torch.where(v > 0, slope, 1.0), y)
        return act

    stock = F.relu, F.leaky_relu
    F.relu = wrap(stock[0], lambda inplace=False: 0.0)
    F.leaky_relu = wrap(stock[1], lambda negative_slope=0.01, inplace=False: float(negative_slope))
    try:
        yield
    finally:
        F.relu, F.leaky_relu = stock


def twin_references(tw, stage, ins, cots):
    """The twin's step, and -- where activation inputs lie within KINK_GUARD of zero -- the same step with every
    combination of them on the other side."""
    import itertools
    found = []
    with _kinks(found):
        yield twin_step(tw, stage, ins, cots)
    assert len(found) <= MAX_KINKS, (stage.name, len(found))
    for r in range(1, len(found) + 1):
        for flip in itertools.combinations(found, r):
            with _kinks([], frozenset(flip)):
                yield twin_step(tw, stage, ins, cots)


def nearest_reference(tw, stage, ins, cots, step):
    """-> (the reference of `twin_references` that `step` is nearest to by its worst figure, how many there were)."""
    refs = list(twin_references(tw, stage, ins, cots))
    return min(refs, key=lambda ref: worst(figures(stage, step, ref))), len(refs)


def figures(stage, step, ref):
    """Every tensor of `step` against the twin's `ref`: (kind, name) -> (rel, elements of the tensor)."""
    rows = {}
    for name, y, r in zip(stage.makes, step.outs, ref.outs):
        rows["out", name] = (C.rel(y, r), r.numel())
    for name, g, r in zip(stage.takes, step.dins, ref.dins):
        assert r is not None, (stage.name, name)
        rows["din", name] = (math.inf if g is None else C.rel(g, r), r.numel())
    for name, r in ref.dparams.items():
        g = step.dparams.get(name)
        rows["dparam", name] = (math.inf if g is None else C.rel(g, r), r.numel())
    assert set(step.dparams) <= set(ref.dparams), (stage.name, set(step.dparams) - set(ref.dparams))
    return rows


def worst(rows):
    return max(v[0] for v in rows.values())


# --------------------------------------------------------------------------- backward faults (CPU test only)
class _ScaledGrad(torch.autograd.Function):
    """x forward, `k * dy` backward."""

    @staticmethod
    def forward(ctx, x, k):
        ctx.k = k
        return x.view_as(x)

    @staticmethod
    def backward(ctx, dy):
        return dy * ctx.k, None


class _LeakyNoMask(torch.autograd.Function):
    """LeakyReLU(0.01) forward, `dy` backward: the activation's mask ignored."""

    @staticmethod
    def forward(ctx, x):
        return F.leaky_relu(x, 0.01)

    @staticmethod
    def backward(ctx, dy):
        return dy


class _MulNoGate(torch.autograd.Function):
    """f * g forward (g of one channel); backward df = dy for dy * g, dg right."""

    @staticmethod
    def forward(ctx, f, g):
        ctx.save_for_backward(f)
        return f * g

    @staticmethod
    def backward(ctx, dy):
        f, = ctx.saved_tensors
        return dy, (dy * f).sum(1, keepdim=True)


class _Times128NoScale(torch.autograd.Function):
    """x * 128 forward, `dy` backward."""

    @staticmethod
    def forward(ctx, x):
        return x * 128

    @staticmethod
    def backward(ctx, dy):
        return dy


class _DepthwiseMirroredTap(torch.autograd.Function):
    """The depthwise convolution forward; backward dx right, dw with the taps of its first row mirrored in kx."""

    @staticmethod
    def forward(ctx, x, w, stride):
        ctx.save_for_backward(x, w)
        ctx.stride = stride
        return F.conv2d(x, w, None, stride, 1, 1, w.size(0))

    @staticmethod
    def backward(ctx, dy):
        x, w = (t.detach().requires_grad_(True) for t in ctx.saved_tensors)
        with torch.enable_grad():
            y = F.conv2d(x, w, None, ctx.stride, 1, 1, w.size(0))
        dx, dw = torch.autograd.grad(y, (x, w), dy)
        dw = dw.clone()
        dw[:, :, 0] = dw[:, :, 0].flip(-1)
        return dx, dw, None


def merge(net, f1, f2, f3, f4, gate=None, up=None, mul=None):
    """`FOTSNet._merge` (with attention) restated with three knobs, each called with the place it stands at: the gate of
    merge 1, 2, 3; the resize "a1" (`a` of the first merge), "r2", "r3" (the stand-alone ones); the product of merge k."""
    gate = gate or (lambda k, t, like: net._gate(t, like))
    up = up or (lambda k, t, like: net._up(t, like))
    mul = mul or (lambda k, f, g: f * g)
    t = up("a1", f4, f3) + mul(1, f3, gate(1, f4, f3).expand_as(f3))
    gate2 = gate(2, t, f2)                 # (in FOTSNet._merge's order: autograd sums t's gradients in the order of the calls)
    m2 = net.upconv1(up("r2", t, f2)) + mul(2, f2, gate2)
    gate1 = gate(3, m2, f1)
    m1 = net.upconv2(up("r3", m2, f1)) + mul(3, f1, gate1)
    return m1, m2


def heads(net, t, scale=None, norm=None):
    """`FOTSNet._heads` restated with two knobs: the rbox scale and the length the angle pair is divided by."""
    scale = scale or (lambda d: d * 128)
    norm = norm or (lambda n: n)
    score = torch.sigmoid(net.act(t))
    dist = scale(torch.sigmoid(net.rbox(t)))
    ang = torch.sigmoid(net.angle(t)) * 2 - 1
    ang = ang / norm(torch.sqrt(ang[:, 0] * ang[:, 0] + ang[:, 1] * ang[:, 1]).unsqueeze(1))
    return score, dist, ang


def _merge_as(net, **knobs):
    return C._forward_of(net, lambda *f: merge(net, *f, **knobs), "_merge")


def _heads_as(net, **knobs):
    return C._forward_of(net, lambda t: heads(net, t, **knobs), "_heads")


@contextlib.contextmanager
def _both(a, b):
    with a, b:
        yield


def _b2(seq):
    """conv2[1] + conv2[2], an affine norm and the LeakyReLU absorbed into it: the right value, the right dx, and weight
    and bias gradients taken as if there were no activation (`z - z.detach()` is zero and carries their gradient)."""
    norm, act = seq[1], seq[2]
    stock = type(norm).forward

    def forward(x):
        y = F.leaky_relu(F.instance_norm(x, weight=norm.weight.detach(), bias=norm.bias.detach(), eps=norm.eps), 0.01)
        z = stock(norm, x.detach())
        return y + (z - z.detach())
    return _both(C._forward_of(norm, forward), C._forward_of(act, lambda x: x))


def _gate_of_last_call_only(net):
    def gate(k, t, like):
        if k == 3:
            return net._gate(t, like)
        w, b = net.conv_attenton.weight.detach(), net.conv_attenton.bias.detach()
        return net._up(torch.sigmoid(F.conv2d(t, w, b)), like)
    return gate


def _dw_as(conv):
    return C._forward_of(conv, lambda x: _DepthwiseMirroredTap.apply(x, conv.weight, conv.stride[0]))


_HEADS = ("_heads(m2)", "_heads(m1)")
# name -> (what is wrong in the backward, the stages it can show at, network -> context manager)
BACKWARD = {
    "B1": ("the mask of the LeakyReLU absorbed at layer3.1.conv_sep1 ignored backward", ("layer3.1.conv_sep1", "layer3.1"),
           lambda n: C._forward_of(n.layer3[1].conv_sep1[3], _LeakyNoMask.apply)),
    "B2": ("the same at layer4.1.conv2[1], for the norm's weight and bias gradients only", ("layer4.1.conv2", "layer4.1"),
           lambda n: _b2(n.layer4[1].conv2)),
    "B3": ("the gate detached in the second merge", ("_merge",),
           lambda n: _merge_as(n, gate=lambda k, t, like: n._gate(t, like).detach() if k == 2 else n._gate(t, like))),
    "B4": ("df returned as dy in the third merge", ("_merge",),
           lambda n: _merge_as(n, mul=lambda k, f, g: _MulNoGate.apply(f, g) if k == 3 else f * g)),
    "B5": ("da of the first merge zeroed", ("_merge",),
           lambda n: _merge_as(n, up=lambda k, t, like: _ScaledGrad.apply(n._up(t, like), 0.0 if k == "a1" else 1.0))),
    "B6": ("the gradient of the resize in front of upconv1 zeroed", ("_merge",),
           lambda n: _merge_as(n, up=lambda k, t, like: _ScaledGrad.apply(n._up(t, like), 0.0 if k == "r2" else 1.0))),
    "B7": ("conv_attenton's gradient taken from the last of its three calls only", ("_merge",),
           lambda n: _merge_as(n, gate=_gate_of_last_call_only(n))),
    "B8": ("the rbox scale of 128 omitted backward", _HEADS, lambda n: _heads_as(n, scale=_Times128NoScale.apply)),
    "B9": ("the gradient of the angle's normalisation omitted", _HEADS, lambda n: _heads_as(n, norm=lambda v: v.detach())),
    "B10": ("the weight gradient of layer3.2.conv2[0] with the taps of one row mirrored in kx", ("layer3.2.conv2", "layer3.2"),
            lambda n: _dw_as(n.layer3[2].conv2[0])),
}
BACKWARD_ONLY = tuple(BACKWARD)          # their forward is the stock one bit for bit: no forward test could see them


def _m7_train(bn):
    """BatchNorm applied twice is no fault on batch statistics (the second application finds mean `bias` and variance
    `weight^2` and gives the first one's output to 5e-6): in training the fault of that kind is the norm FOLDED, that is
    run on its running statistics, where it has to run on the batch's."""
    def forward(x):
        return F.batch_norm(x, bn.running_mean, bn.running_var, bn.weight, bn.bias, False, 0.0, bn.eps)
    return C._forward_of(bn, forward)


def _m8_train(bn):
    """network_cases._m8 on the statistics the mode calls for: the scale alone, `bias - mean * scale` dropped."""
    def forward(x):
        var = x.var((0, 2, 3), unbiased=False) if bn.training else bn.running_var
        return x * (bn.weight / torch.sqrt(var + bn.eps)).view(1, -1, 1, 1).to(x.dtype)
    return C._forward_of(bn, forward)


# The twelve forward mutations of network_cases (they change gradients too), M7 and M8 restated for batch statistics.
TRAIN_MUTATIONS = dict(C.MUTATIONS)
TRAIN_MUTATIONS["M7"] = ("the BatchNorm of layer3.0's shortcut run on its running statistics", ("layer3.0",),
                         lambda n: _m7_train(n.layer3[0].downsample[1]))
TRAIN_MUTATIONS["M8"] = (C.MUTATIONS["M8"][0], ("layer2.0",), lambda n: _m8_train(n.layer2[0].downsample[1]))
TRAIN_MUTATIONS.update(BACKWARD)
