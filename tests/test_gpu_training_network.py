"""GPU (MI355X): the switched network's TRAINING pass, stage by stage against its float64 twin (DESIGN 5.28,
training_cases.py).  Every backward kernel has a derived bound in its own test; what is bounded here is the composition: an
activation absorbed into a norm and applied again by a fall-back path, `fused_slope` honoured forward but not backward, the
gate's gradient reaching `conv_attenton` from one of its three calls only, `df` without its gate factor, `da` of the first
merge dropped, the 128 of the rbox head missing backward, a `need_*` flag that turns a gradient into None -- each passes
every per-kernel test, because each kernel is right on its own input.

Each stage is teacher-forced and takes one training step of its own (training_cases.train_step): the switched network,
the unswitched copy on the same GPU and the twin get the same inputs, as leaves that require a gradient, and the same
cotangents; the next stage is fed the switched network's own detached output.  Asserted per stage, against the twin:
    float32    rel <= FP32_CAP (5.7e-4) for every output, every input gradient and every parameter gradient; a gradient that
               is None where the twin has one is a failure.  Where an activation input of the twin lies within 4e-6 of zero
               the reference is the twin with that element on either side, one choice for the whole stage
               (training_cases.nearest_reference): float32 cannot tell the sides apart and one element costs 9e-3
    bfloat16   forward outputs: the RATIO_CAP and NEG_CAP rules of network_cases, now in training mode;
               input gradients, and parameter gradients of at least 64 elements:
               rel_native <= RATIO_CAP * max(rel_stock, 2^-8)
The bfloat16 gradient leg is blunt, and is meant to be: the stock bfloat16 gradients are themselves 1e-2 to 0.26 off the
twin on the CPU (the recogniser's worst), so it catches a fault that costs a large part of a tensor and no finer one; the
floor is one rounding to the type, which a correctly rounded result may show; the one- to four-element biases of the heads
and the gate, whose stock error reached 0.29, are asserted in float32 only.  Neither cap is taken from what the kernels
give: test_training_twin.py sets FP32_CAP from CPU measurements and shows which faults each leg catches.

The test is not vacuous: the Python-level backward runners of rroi_align.norm, conv, merge and heads are counted, and with
every kernel forced on each stage must make exactly the calls its structure predicts -- over one pass 46 norm backwards in
`forward` and the recogniser's 3 (the 49 of DESIGN 5.24), 22 depthwise, 3 merge and 3 resize, 2 heads, 3 gate.

With NETWORK_TWIN_RECORD set to a file name, every figure is appended to it as a JSON line
(profiles/native_training_network.md)."""
import collections
import json
import math
import os

import pytest
import torch

import network_cases as C
import training_cases as T

pytestmark = pytest.mark.gpu

KINDS = ("norm", "depthwise", "merge", "resize", "heads", "gate")
RUNNERS = (("norm", "rroi_align.norm", "run_instance_norm_backward"),
           ("depthwise", "rroi_align.conv", "run_depthwise3x3_backward"),
           ("merge", "rroi_align.merge", "run_gated_merge_backward"),
           ("resize", "rroi_align.merge", "run_resize_bilinear_backward"),
           ("heads", "rroi_align.heads", "run_heads_backward"),
           ("gate", "rroi_align.heads", "run_gate_backward"))


def record(**row):
    path = os.environ.get("NETWORK_TWIN_RECORD")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(row) + "\n")


def name_of(dtype):
    return {torch.bfloat16: "bf16", torch.float32: "fp32"}[dtype]


# ---------------------------------------------------------------- the configurations
def trainable_four(net, natives=True):
    """The four native / trainable pairs in their documented order: a trainable switch goes on after its native one, the
    trainable heads last (fots_e2e.native_train, native_train_heads).  natives=False: the native four are on already."""
    from fots_e2e import native as nat, native_train as tr
    from fots_e2e.native_train_heads import use_trainable_heads
    if natives:
        assert nat.use_native_instancenorm(net) == C.COUNTS["instancenorm"] and nat.use_native_depthwise(net) == 22
        assert nat.use_native_heads(net) and nat.use_native_merge(net)
    assert tr.use_trainable_instancenorm(net) == 52 and tr.use_trainable_depthwise(net) == 22
    assert tr.use_trainable_merge(net) and use_trainable_heads(net)
    return net


def everything(net, dtype):
    """What a user gets: every switch of fots_e2e.native that applies to the dtype, the two of native_remainder, then the
    four trainable ones."""
    from fots_e2e import native_remainder as rm
    C.all_eight(net, C.FP32_ORDER if dtype == torch.float32 else C.ORDER)
    assert rm.use_native_conv2x3(net) == 1 and rm.use_native_upconv(net) == 2
    return trainable_four(net, natives=False)


CONFIGS = {"everything": everything, "trainable-only": lambda net, dtype: trainable_four(net)}


def trio(dtype, config, training):
    """Fresh networks: (switched, unswitched copy on the same GPU, float64 twin on the CPU)."""
    native = T.train_mode(CONFIGS[config](T.network(dtype, training).cuda(), dtype), training)
    stock = T.network(dtype, training).cuda()
    T.glue_is_not_overridden()
    assert type(native).forward is type(stock).forward and type(native).forward_features is type(stock).forward_features
    return native, stock, T.twin(T.network(dtype, training))


def force_every_kernel(monkeypatch):
    for module, hook in T.every_hook():
        monkeypatch.setattr(module, hook, lambda *a, **k: False)


def count_backward_calls(monkeypatch):
    import importlib
    calls = collections.Counter()

    def counted(kind, run):
        def call(*a, **k):
            calls[kind] += 1
            return run(*a, **k)
        return call

    for kind, path, name in RUNNERS:
        module = importlib.import_module(path)
        monkeypatch.setattr(module, name, counted(kind, getattr(module, name)))
    return calls


def expected_calls(net, stage, training):
    """The native backward calls one training step of `stage` makes with every kernel forced on, from the structure of the
    model: every norm and depthwise convolution of a submodule is called once; `forward_ocr` applies batch5, batch7 and
    batch10_s; in training mode `_merge` runs three gated merges (one merge backward each), the two stand-alone resizes and
    the resize of the first merge's `a`, three gates, and the depthwise halves of upconv1 / upconv2.  In eval mode
    `_TrainableMerge` steps aside, and the merge's own resizes, products and gates are the stock expression."""
    from fots_e2e import native_train as tr
    want = dict.fromkeys(KINDS, 0)
    if stage.name == "_merge":
        want.update(depthwise=2)
        if training:
            want.update(merge=3, resize=3, gate=3 if net.attention else 0)
    elif stage.name.startswith("_heads"):
        want.update(heads=1)
    elif stage.name == "forward_ocr":
        want.update(norm=3)
    else:
        inside = list(net.get_submodule(stage.name).modules())
        want.update(norm=sum(isinstance(m, tr.TrainableInstanceNorm2d) for m in inside),
                    depthwise=sum(isinstance(m, tr.TrainableDepthwiseConv3x3) for m in inside))
    return want


def is_a_part(stage):
    """The two Sequentials of a separable block are stages of their own AND run inside their block's stage."""
    return stage.name.endswith((".conv_sep1", ".conv2"))


# ---------------------------------------------------------------- one pass over the table
def one_pass(dtype, config, mode, training, calls):
    native, stock, tw = trio(dtype, config, training)
    table = C.stages(stock)
    rows, broken, per_pass = [], [], []
    tag = dict(test="training", config=config, mode=mode, training=training, dtype=name_of(dtype))
    for which, (image_key, crops_key) in enumerate(C.INPUTS):
        total = collections.Counter()

        def step(st, xs):
            calls.clear()
            got, cots = T.train_step(native, st.on_net, xs, stage=st)
            made = {k: calls[k] for k in KINDS}
            calls.clear()
            base, _ = T.train_step(stock, st.on_net, xs, cots)
            assert not calls, (st.name, dict(calls))                 # the unswitched copy runs no native backward
            if dtype == torch.float32:                               # the twin, and its neighbours at a kink
                ref, candidates = T.nearest_reference(tw, st, xs, cots, got)
                if candidates > 1:
                    print(f"{st.name} {image_key}: {candidates} references at activation kinks")
            else:
                ref = T.twin_step(tw, st, xs, cots)
            assert all(t.dtype == dtype for t in got.outs) and all(g is None or g.dtype == dtype for g in got.dins), st.name
            if mode == "forced":
                want = expected_calls(native, st, training)
                if made != want:
                    broken.append((st.name, image_key, "calls", made, want))
            if not is_a_part(st):
                total.update(made)
            mine, theirs = T.figures(st, got, ref), T.figures(st, base, ref)
            assert mine.keys() == theirs.keys() and all(v[0] < math.inf for v in theirs.values()), st.name
            for (kind, tensor), (rel, numel) in mine.items():
                rel_stock = theirs[kind, tensor][0]
                neg = None
                if kind == "out" and st.leaky:
                    k = st.makes.index(tensor)
                    neg = C.rel_neg(got.outs[k], ref.outs[k])
                row = dict(tag, image=image_key, stage=st.name, kind=kind, tensor=tensor, elements=numel, rel_native=rel,
                           rel_stock=rel_stock, rel_neg=neg)
                rows.append(row)
                record(**row)
                where = (st.name, kind, tensor, image_key)
                if dtype == torch.float32:
                    if not rel <= T.FP32_CAP:
                        broken.append(where + ("rel", rel))
                elif kind == "out":
                    if not rel <= C.RATIO_CAP * rel_stock:
                        broken.append(where + ("ratio", rel / rel_stock if rel_stock else math.inf))
                    if neg is not None and not neg <= C.NEG_CAP:
                        broken.append(where + ("rel_neg", neg))
                elif kind == "din" or numel >= T.RATIO_MIN_ELEMENTS:
                    bound = C.RATIO_CAP * max(rel_stock, T.BF16_FLOOR)
                    if not rel <= bound:
                        broken.append(where + ("gradient ratio", rel, bound))
            return got.outs                                          # fed on: the switched network's own output

        C.drive(table, C.draw(C.IMAGES[image_key]).to(dtype).cuda(), C.draw(C.CROPS[crops_key]).to(dtype).cuda(), step)
        per_pass.append({k: total[k] for k in KINDS})
    torch.cuda.synchronize()
    for kind in ("out", "din", "dparam"):
        top = max((r for r in rows if r["kind"] == kind), key=lambda r: r["rel_native"])
        print("{dtype} {config} {mode} training={training}: worst {kind:6s} rel native {rel_native:.3e} stock {rel_stock:.3e}"
              "  {tensor} at {stage}, {image}".format(**top))
    for line in sorted(broken, key=str):
        print("BROKEN", line)
    record(**dict(tag, test="training-calls", calls=per_pass))
    print(f"{name_of(dtype)} {config} {mode}: native backward calls per pass {per_pass}")
    assert len(rows) == 2 * 357, len(rows)                           # the 714 figures test_training_twin.py measures
    return rows, broken, per_pass


def whole_pass(training):
    merges = dict(merge=3, resize=3, gate=3) if training else dict(merge=0, resize=0, gate=0)
    return dict(norm=46 + 3, depthwise=22, heads=2, **merges)


FORCED = [(torch.float32, "everything", True), (torch.bfloat16, "everything", True),
          (torch.float32, "trainable-only", True), (torch.float32, "everything", False)]
FORCED_IDS = ["fp32-everything", "bf16-everything", "fp32-trainable-only", "fp32-everything-eval"]


@pytest.mark.parametrize("dtype,config,training", FORCED, ids=FORCED_IDS)
def test_every_stage_trains_within_its_cap_with_every_kernel_forced_on(dtype, config, training, monkeypatch):
    """One pass over the table per input.  The last case is frozen-BatchNorm fine-tuning: the whole network in `.eval()`
    with gradients still needed, where `_TrainableMerge` steps aside and the norms, the depthwise convolutions and the
    heads do not."""
    force_every_kernel(monkeypatch)
    calls = count_backward_calls(monkeypatch)
    _, broken, per_pass = one_pass(dtype, config, "forced", training, calls)
    assert not broken, broken
    assert per_pass == [whole_pass(training)] * len(C.INPUTS), per_pass


@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16), ids=("fp32", "bf16"))
def test_every_stage_trains_within_its_cap_with_the_hooks_as_shipped(dtype, monkeypatch):
    """The production mixture of native and stock calls per shape class: a call that is declined must still apply, forward
    and backward, the activation it has absorbed.  The call counts are what the hooks make them; a pass that ran no native
    backward at all would be vacuous."""
    calls = count_backward_calls(monkeypatch)
    _, broken, per_pass = one_pass(dtype, "everything", "shipped", True, calls)
    assert not broken, broken
    assert all(0 < made[k] <= whole_pass(True)[k] for made in per_pass for k in KINDS), per_pass
