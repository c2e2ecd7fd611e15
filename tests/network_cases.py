"""The whole network against a float64 twin, stage by stage: what test_network_twin.py (CPU) and
test_gpu_network.py (MI355X) share.

  twin(net)       a deep copy of the unswitched, already 16-bit network in float64 on the CPU: its weights are the rounded
                  ones the GPU sees, so what separates a 16-bit path from it is that path's own arithmetic and wiring.
  stages(net)     the stage table: layer0, layer0_1, the 17 residual blocks (and, of each separable block, its two
                  Sequentials), feature1..4, the merge, the heads twice, the recogniser.  A row names the tensors it takes
                  and the tensors it makes, so a test drives the table itself (`drive`) and decides what each stage is
                  fed: no hooks.
  rel, rel_neg    the two statistics, in float64: the relative L2 error, and the same over the elements whose reference is
                  negative -- where a slope of 0.01 taken for 0, 0.0001 or 1 is an error of at least 0.99.
  all_eight       the eight switches of fots_e2e.native in a given order, each asserting its own count.
  MUTATIONS       twelve ways in which the composition can be wrong while every kernel is right, each a context manager
                  on a stock network.  The CPU test shows that the caps the GPU test asserts catch them.

The two caps.  RATIO_CAP = 2: a native path and the stock path round to the same type at every module boundary, the
native kernels accumulate in fp32 or double and round less often, so rel(native) / rel(stock) is expected at or below 1; a
mis-wiring that the type can see at all measured between 2.3 and 18 on the CPU.  NEG_CAP = 0.25: the slopes in play are 0,
0.0001, 0.01 and 1, any confusion among them gives at least 0.99, and the honest worst on the CPU was 0.053 (bf16)."""
import contextlib
import copy
from typing import Callable, NamedTuple, Tuple

import torch
import torch.nn.functional as F

RATIO_CAP = 2.0
NEG_CAP = 0.25
MIN_NEGATIVE = 64          # rel_neg is defined only where the reference has this many negative elements

DTYPES = (torch.bfloat16, torch.float16)
IDS = ("bf16", "fp16")
SEED = 7
# The second image gives odd sizes at every level (40x56, 20x28, 10x14, 5x7, 3x4): stride 2 on odd maps, non-integer
# resize ratios in the merge; a batch of two and a batch of one.  The second crop set is one crop of eight columns.
IMAGES = {"2x64x96": (2, 3, 64, 96), "1x80x112": (1, 3, 80, 112)}
CROPS = {"4x11x40": (4, 64, 11, 40), "1x11x8": (1, 64, 11, 8)}
INPUTS = tuple(zip(IMAGES, CROPS))     # the (image, crop set) pairs the tests run


def draw(shape):
    return torch.randn(shape, generator=torch.Generator().manual_seed(SEED))


def network(dtype=None):
    from fots_e2e.model import FOTSNet
    from fots_e2e.weights import deterministic_init
    net = deterministic_init(FOTSNet()).eval()
    return net if dtype is None else net.to(dtype)


def twin(net):
    from fots_e2e.model import FOTSNet
    assert type(net) is FOTSNet, "the twin is taken of the unswitched network"
    return copy.deepcopy(net).double().cpu().eval()


# --------------------------------------------------------------------------- the two statistics
def rel(y, ref) -> float:
    y, ref = y.detach().double().cpu(), ref.detach().double().cpu()
    assert y.shape == ref.shape, (y.shape, ref.shape)
    return float((y - ref).norm() / ref.norm())


def rel_neg(y, ref) -> float:
    y, ref = y.detach().double().cpu(), ref.detach().double().cpu()
    assert y.shape == ref.shape, (y.shape, ref.shape)
    neg = ref < 0
    assert int(neg.sum()) >= MIN_NEGATIVE, f"only {int(neg.sum())} negative reference elements"
    return float((y - ref)[neg].norm() / ref[neg].norm())


# --------------------------------------------------------------------------- the stage table
class Stage(NamedTuple):
    name: str
    takes: Tuple[str, ...]        # names of the tensors it is called on
    makes: Tuple[str, ...]        # names of the tensors it returns
    on_net: Callable              # (network, *tensors) -> tensor or tuple of tensors
    on_twin: Callable             # the same on the float64 twin
    leaky: bool                   # its last operation is a LeakyReLU of slope 0.01


def _stage(name, takes, makes, call, leaky=False):
    return Stage(name, tuple(takes), tuple(makes), call, call, leaky)


def _sub(path):
    """(network, *tensors) -> the submodule at `path` of that network, called on the tensors."""
    return lambda net, *ts: net.get_submodule(path)(*ts)


def stages(net):
    """The table for `net`'s structure (the rows hold paths, not modules: they apply to every copy of the network and to
    its twin).  "image" and "crops" are the two tensors the table itself does not make."""
    from fots_e2e.model import _SeparableBlock
    rows = [_stage("layer0", ["image"], ["stem"], _sub("layer0"), leaky=True),
            _stage("layer0_1", ["stem"], ["focr"], _sub("layer0_1"))]
    x = "focr"                                                   # (drop1 is the identity in eval mode)
    for k in (1, 2, 3, 4):
        for i, block in enumerate(getattr(net, f"layer{k}")):
            path = f"layer{k}.{i}"
            separable = isinstance(block, _SeparableBlock)
            if separable:
                rows.append(_stage(path + ".conv_sep1", [x], [path + ".sep"], _sub(path + ".conv_sep1"), leaky=True))
                rows.append(_stage(path + ".conv2", [path + ".sep"], [path + ".body"], _sub(path + ".conv2")))
            rows.append(_stage(path, [x], [path + ".out"], _sub(path), leaky=separable))
            x = path + ".out"
        rows.append(_stage(f"feature{k}", [x], [f"f{k}"], _sub(f"feature{k}")))
    rows.append(_stage("_merge", ["f1", "f2", "f3", "f4"], ["m1", "m2"], lambda n, *f: n._merge(*f)))
    rows.append(_stage("_heads(m2)", ["m2"], ["s8", "r8", "a8"], lambda n, m: n._heads(m)))
    rows.append(_stage("_heads(m1)", ["m1"], ["s4", "r4", "a4"], lambda n, m: n._heads(m)))
    rows.append(_stage("forward_ocr", ["crops"], ["ocr"], lambda n, c: n.forward_ocr(c)))
    return rows


def as_tuple(out):
    return tuple(out) if isinstance(out, (tuple, list)) else (out,)


def drive(table, image, crops, step):
    """Run the table in order: `step(stage, inputs)` returns the tuple of tensors that are FED ON under the stage's
    `makes`; what else it computes and compares is its own affair.  Returns every named tensor."""
    env = {"image": image, "crops": crops}
    for st in table:
        outs = as_tuple(step(st, tuple(env[k] for k in st.takes)))
        assert len(outs) == len(st.makes), st.name
        env.update(zip(st.makes, outs))
    return env


def network_outputs(env):
    """What `net(image)` returns, out of the tensors `drive` made."""
    return [env["s4"], env["s8"]], [env["r4"], env["r8"]], [env["a4"], env["a8"]], [env["m1"], env["focr"]]


def flat(outputs):
    return [t for pair in outputs for t in pair]


# --------------------------------------------------------------------------- the switches
ORDER = ("depthwise", "instancenorm", "heads", "merge", "blocks", "conv3x3", "recogniser", "conv1x1")
FP32_ORDER = tuple(k for k in ORDER if k not in ("conv3x3", "conv1x1"))    # the two matrix-core switches are 16-bit only
COUNTS = {"depthwise": 22, "instancenorm": (52, 20), "heads": True, "merge": True, "blocks": (2, 7, 10),
          "conv3x3": (23, 2), "recogniser": True, "conv1x1": (29, 3)}
SLOWER_HOOKS = ("_inorm_slower", "_merge_slower", "_conv3x3_slower", "_act_pool_slower", "_ocr_head_slower",
                "_conv1x1_slower")


def all_eight(net, order=ORDER, enable=True):
    """The switches named in `order`, in that order; each reports its own full count whatever is already switched
    (test_all_eight_switches_compose_and_restore_exact_classes_in_every_order)."""
    from fots_e2e import native as nat
    assert sorted(order) == sorted(set(order)) and set(order) <= set(COUNTS)
    for name in order:
        got = getattr(nat, "use_native_" + name)(net, enable)
        assert got == COUNTS[name], (name, got)
    return net


def slower_hooks():
    """Every `_..._slower` hook fots_e2e.native has; the tuple above must be all of them."""
    from fots_e2e import native as nat
    found = tuple(sorted(k for k in vars(nat) if k.startswith("_") and k.endswith("_slower")))
    assert found == tuple(sorted(SLOWER_HOOKS)), found
    return found


# --------------------------------------------------------------------------- the mutation table (CPU test only)
@contextlib.contextmanager
def _forward_of(module, forward, attr="forward"):
    """`module.<attr>` replaced on the instance, put back on the way out."""
    assert attr not in module.__dict__
    module.__dict__[attr] = forward
    try:
        yield
    finally:
        del module.__dict__[attr]


def _twice(module):
    stock = type(module).forward
    return _forward_of(module, lambda x: stock(module, stock(module, x)))


def _finish_as(block, finish):
    return _forward_of(block, lambda out, x: finish(out, x if block.downsample is None else block.downsample(x)), "_finish")


def _m4(block):
    return _forward_of(block, lambda x: block._finish(block.bn2(block.conv2(block.bn1(block.conv1(x)))), x))


def _m8(bn):
    def forward(x):
        scale = bn.weight / torch.sqrt(bn.running_var + bn.eps)
        return (x * scale.view(1, -1, 1, 1)).to(x.dtype)          # the folded scale alone: beta - mean * scale dropped
    return _forward_of(bn, forward)


def _m9(mirror):
    return _forward_of(mirror, lambda x: F.leaky_relu(mirror.bn(torch.cat((x, x), 1)), 0.01))


def _m10(net):
    def merge(f1, f2, f3, f4):
        t = net._up(f4, f3) + f3 * net._gate(f4, f3).expand_as(f3)
        m2 = net.upconv1(net._up(t, f2)) + f2                     # the second merge without its gate
        return net.upconv2(net._up(m2, f1)) + f1 * net._gate(m2, f1), m2
    return _forward_of(net, merge, "_merge")


def recogniser(net, x, inner6=True, bias=True, pool_first=False):
    """`FOTSNet.forward_ocr` restated with three knobs: the activation between the two applications of conv6, the bias of
    conv11, and -- a rewrite that is the same function, LeakyReLU being monotone -- the pool in front of its activation."""
    act = lambda t: F.leaky_relu(t, 0.01)  # noqa: E731
    pool = lambda t: F.max_pool2d(t, (2, 1), stride=(2, 1))  # noqa: E731
    act_pool = (lambda t: act(pool(t))) if pool_first else (lambda t: pool(act(t)))
    x = act(net.batch5(net.conv5(x)))
    x = net.conv6(x)
    x = act_pool(net.conv6(act(x) if inner6 else x))
    x = act(net.batch7(net.conv7(x)))
    x = act(net.conv8(act(net.conv8(x))))
    x = act_pool(net.conv9(act(net.conv9(x))))
    x = act(net.batch10_s(net.conv10_s(x)))
    x = F.conv2d(net.drop1(x), net.conv11.weight, net.conv11.bias if bias else None).squeeze(2)
    return F.log_softmax(x, dim=1)


def _ocr_as(net, **knobs):
    return _forward_of(net, lambda x: recogniser(net, x, **knobs), "forward_ocr")


# name -> (what is mis-wired, the stages it can show at, network -> context manager)
MUTATIONS = {
    "M1": ("LeakyReLU twice at the end of layer3.1.conv_sep1", ("layer3.1.conv_sep1", "layer3.1"),
           lambda n: _twice(n.layer3[1].conv_sep1[3])),
    "M2": ("LeakyReLU twice at layer3.1.conv2[2]", ("layer3.1.conv2", "layer3.1"),
           lambda n: _twice(n.layer3[1].conv2[2])),
    "M3": ("ReLU for the leaky activation in layer4.1._finish", ("layer4.1",),
           lambda n: _finish_as(n.layer4[1], lambda out, r: F.relu(out + r))),
    "M4": ("the ReLU behind layer1.1.bn1 dropped", ("layer1.1",), lambda n: _m4(n.layer1[1])),
    "M5": ("the residual of layer2.1 added twice", ("layer2.1",),
           lambda n: _finish_as(n.layer2[1], lambda out, r: F.relu(out + r + r))),
    "M6": ("the residual of layer3.2 not added", ("layer3.2",),
           lambda n: _finish_as(n.layer3[2], lambda out, r: F.leaky_relu(out, 0.01))),
    "M7": ("the BatchNorm of layer3.0's shortcut applied twice", ("layer3.0",),
           lambda n: _twice(n.layer3[0].downsample[1])),
    "M8": ("the shift of the BatchNorm of layer2.0's shortcut dropped", ("layer2.0",),
           lambda n: _m8(n.layer2[0].downsample[1])),
    "M9": ("cat(x, x) for cat(x, -x) in layer0[1]", ("layer0",), lambda n: _m9(n.layer0[1])),
    "M10": ("the gate factor omitted in the second merge", ("_merge",), _m10),
    "M11": ("the activation between the two applications of conv6 dropped", ("forward_ocr",),
            lambda n: _ocr_as(n, inner6=False)),
    "M12": ("the bias of conv11 dropped before the log-softmax", ("forward_ocr",), lambda n: _ocr_as(n, bias=False)),
}
