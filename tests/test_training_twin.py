"""CPU: the instrument of test_gpu_training_network.py, validated -- so that its cap is not taken on trust.

In the manner of test_network_twin.py: the stock CPU network in training mode stands in for "a training path with the wiring
right", a mutated copy of it (training_cases TRAIN_MUTATIONS) for "a path with one fault", and the float64 twin is the
reference of both.  Every stage is teacher-forced and takes one training step of its own (training_cases.train_step):
outputs, input gradients and the gradient of every parameter it touched are each compared with the twin's.

float32 asserts.  Measured here, both inputs, 47 stages each, 714 figures: every output within 6.6e-7 of the twin, every
input gradient within 2.5e-6, every parameter gradient within 4.04e-5 -- h: the two-element angle.bias at _heads(m1),
2x64x96, on one thread; 1.42e-5 on 2 to 16 threads and 7.6e-6 on 32, the next tensor, angle.weight, at 7e-6.  The weakest of the 22 mutations is M3, ReLU for LeakyReLU(0.01) at the end of layer4.1, at 8.07e-3 on its most
visible tensor -- w; every backward-only fault is at 0.48 or more.  FP32_CAP is their geometric mean, 5.7e-4, a factor of
14 from either: the decade on each side covers MIOpen's convolutions differing from the CPU's in accuracy.

bfloat16 is blunt.  The stock bfloat16 gradients are themselves 1e-2 to 0.26 off the twin (forward_ocr: the crops'
gradient 0.25, conv5.weight 0.26), so a fault of a few 1e-2 of a tensor -- which float32 sees two decades above its cap --
can drown in them.  The 22 mutations of the table are coarse enough for the ratio rule of the GPU test to flag all but
M2, which sits at the bound (BF16_WEAK); what a finer fault would cost is what the float32 leg is for."""
import functools
import math

import pytest
import torch

import network_cases as C
import training_cases as T

DTYPES = (torch.float32, torch.bfloat16)
IDS = ("fp32", "bf16")

# What the bfloat16 rule of the GPU test (forward outputs by RATIO_CAP / NEG_CAP, gradients of at least 64 elements by
# `rel <= RATIO_CAP * max(rel_honest, 2^-8)`) sees weakly: mutation -> the largest figure / bound over its stages and both
# inputs, as measured on the CPU; above 1 is flagged.  M2 sits at the bound itself, as it does in
# test_network_twin.BF16_WEAK: a run with other convolution kernels may land on either side.  The test asserts that it
# stays below BF16_CLEAR, that every other mutation stays above it (the weakest, M1 and M3, measured 3.96 and 4.00, both
# by `rel_neg` forward; the weakest backward-only one, B1, 13.1), and that the measured figure is still the one written here.
BF16_WEAK = {"M2": 1.11}
BF16_CLEAR = 2.0


@functools.lru_cache(maxsize=None)
def honest(dtype, which):
    """The stock network in training mode driven through the table on input pair `which`, one training step per stage:
    -> (network, {stage name: (stage, inputs, cotangents, the twin's step, the honest figures, the honest rel_neg)})."""
    image_key, crops_key = C.INPUTS[which]
    net = T.network(dtype)
    tw = T.twin(net)
    record = {}

    def step(st, ins):
        got, cots = T.train_step(net, st.on_net, ins, stage=st)
        ref = T.nearest_reference(tw, st, ins, cots, got)[0] if dtype == torch.float32 else T.twin_step(tw, st, ins, cots)
        assert all(y.dtype == dtype for y in got.outs) and all(g is not None and g.dtype == dtype for g in got.dins), st.name
        negs = [C.rel_neg(y, r) if st.leaky else None for y, r in zip(got.outs, ref.outs)]
        record[st.name] = (st, ins, cots, ref, T.figures(st, got, ref), negs)
        return got.outs

    C.drive(C.stages(net), C.draw(C.IMAGES[image_key]).to(dtype), C.draw(C.CROPS[crops_key]).to(dtype), step)
    return net, record


def test_the_glue_between_the_stages_is_fotsnets_own_in_every_switched_class():
    T.glue_is_not_overridden()


def test_every_slower_hook_is_on_the_closed_lists():
    hooks = T.every_hook()
    assert len(hooks) == len(C.SLOWER_HOOKS) + sum(len(v) for v in T.BACKWARD_HOOKS.values())


def test_the_restated_merge_and_heads_are_the_stock_ones_bit_for_bit():
    """The knobs of the backward mutations turn on `training_cases.merge` and `heads`: without a knob they must be
    `FOTSNet._merge` and `_heads`, in value and in every gradient."""
    net, record = honest(torch.float32, 1)
    for name, restated in (("_merge", lambda n, *f: T.merge(n, *f)), ("_heads(m1)", lambda n, t: T.heads(n, t))):
        st, ins, cots = record[name][:3]
        a, _ = T.train_step(net, st.on_net, ins, cots)
        b, _ = T.train_step(net, restated, ins, cots)
        assert all(torch.equal(x, y) for x, y in zip(a.outs + a.dins, b.outs + b.dins))
        assert a.dparams.keys() == b.dparams.keys() and all(torch.equal(a.dparams[k], b.dparams[k]) for k in a.dparams)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_the_honest_figures(dtype):
    """Every figure of the stock network is positive (the comparison is not of a thing with itself), no reference gradient
    has a zero norm, no gradient is None where the twin has one; in float32 every figure is a decade below FP32_CAP."""
    top = {"out": (0.0, None), "din": (0.0, None), "dparam": (0.0, None)}
    rows = 0
    for which, keys in enumerate(C.INPUTS):
        _, record = honest(dtype, which)
        assert len(record) == 47
        for name, (st, _, _, ref, figs, _) in record.items():
            assert all(float(r.double().norm()) > 0 for r in ref.outs + ref.dins + tuple(ref.dparams.values())), name
            assert ref.dparams, name                                      # every stage has parameters of its own
            for (kind, tensor), (rel, _) in figs.items():
                assert 0.0 < rel < math.inf, (name, kind, tensor, rel)
                top[kind] = max(top[kind], (rel, f"{tensor} at {name}, {keys[0]}"))
                rows += 1
                if dtype == torch.float32:
                    assert 10 * rel <= T.FP32_CAP, (name, kind, tensor, rel)
    for kind, (rel, where) in top.items():
        print(f"{dtype} honest worst {kind}: {rel:.2e} ({where})")
    print(f"{dtype}: {rows} figures")
    if dtype == torch.float32:
        assert max(v[0] for v in top.values()) <= T.FP32_CAP / 10


def measure(dtype, mutation):
    """The mutated network on the mutation's stages and both inputs -> (the largest rel over all tensors; the largest
    figure / bound under the bfloat16 rule of the GPU test, which flags above 1; whether any OUTPUT differs from the honest
    one's bits)."""
    _, stage_names, make = T.TRAIN_MUTATIONS[mutation]
    top, margin, forward_moved = 0.0, 0.0, False
    for which in range(len(C.INPUTS)):
        net, record = honest(dtype, which)
        for name in stage_names:
            st, ins, cots, ref, figs, _ = record[name]
            clean, _ = T.train_step(net, st.on_net, ins, cots)
            with make(net):
                got, _ = T.train_step(net, st.on_net, ins, cots)
            forward_moved |= not all(torch.equal(a, b) for a, b in zip(got.outs, clean.outs))
            mutated = T.figures(st, got, ref)
            top = max(top, T.worst(mutated))
            for key, (rel, numel) in mutated.items():
                if key[0] == "out":
                    k = st.makes.index(key[1])
                    margin = max(margin, rel / (C.RATIO_CAP * figs[key][0]),
                                 C.rel_neg(got.outs[k], ref.outs[k]) / C.NEG_CAP if st.leaky else 0.0)
                elif numel >= T.RATIO_MIN_ELEMENTS:
                    margin = max(margin, rel / (C.RATIO_CAP * max(figs[key][0], T.BF16_FLOOR)))
            # the context manager has put the network back: the honest step again, bit for bit
            again, _ = T.train_step(net, st.on_net, ins, cots)
            assert T.figures(st, again, ref) == T.figures(st, clean, ref) == figs, (mutation, name)
    return top, margin, forward_moved


@functools.lru_cache(maxsize=None)
def fp32_table():
    return {m: measure(torch.float32, m) for m in T.TRAIN_MUTATIONS}


def test_the_table_has_the_ten_backward_faults_and_the_twelve_forward_ones():
    assert len(T.BACKWARD) == 10 and len(T.TRAIN_MUTATIONS) == 22 and set(C.MUTATIONS) < set(T.TRAIN_MUTATIONS)
    names = {st.name for st in C.stages(C.network())}
    assert all(set(stages) <= names for _, stages, _ in T.TRAIN_MUTATIONS.values())


def test_a_backward_fault_leaves_every_forward_value_alone():
    """... so that no forward test, this suite's or test_gpu_network's, could see one."""
    table = fp32_table()
    assert [m for m in T.BACKWARD_ONLY if table[m][2]] == []
    assert all(table[m][2] for m in C.MUTATIONS)


def test_fp32_cap_is_the_geometric_mean_of_the_measured_figures_with_a_decade_on_either_side():
    h = 0.0
    for which in range(len(C.INPUTS)):
        _, record = honest(torch.float32, which)
        h = max([h] + [T.worst(figs) for _, _, _, _, figs, _ in record.values()])
    table = fp32_table()
    for m, (top, _, _) in sorted(table.items(), key=lambda kv: kv[1][0]):
        print(f"fp32 {m:4s} {top:.3e}  {T.TRAIN_MUTATIONS[m][0]}")
    weakest, (w, _, _) = min(table.items(), key=lambda kv: kv[1][0])
    print(f"h = {h:.3e}, w = {w:.3e} ({weakest}), geometric mean {math.sqrt(h * w):.3e}, FP32_CAP {T.FP32_CAP:.3e}")
    assert T.FP32_CAP == math.sqrt(T.H_MEASURED * T.W_MEASURED)
    assert 10 * h <= T.FP32_CAP <= w / 10, (h, T.FP32_CAP, w)
    # the constants are the figures measured, not remembered ones: w as this run gives it; h, which is a two-element
    # tensor's and moves with the number of threads the CPU's convolutions sum on (training_cases), at most the largest
    # measured and within the range seen
    assert T.H_MEASURED / 8 <= h <= 1.25 * T.H_MEASURED and abs(w - T.W_MEASURED) <= 0.25 * T.W_MEASURED, (h, w)


@pytest.mark.parametrize("mutation", list(T.TRAIN_MUTATIONS))
def test_fp32_sees_every_mutation(mutation):
    top, _, _ = fp32_table()[mutation]
    assert top > 10 * T.FP32_CAP, (mutation, top)


def test_bf16_sees_every_mutation_but_the_listed_ones():
    weak = {}
    for m in T.TRAIN_MUTATIONS:
        top, margin, _ = measure(torch.bfloat16, m)
        print(f"bf16 {m:4s} largest rel {top:.3e}  figure / bound {margin:8.2f}  {T.TRAIN_MUTATIONS[m][0]}")
        if margin < BF16_CLEAR:
            weak[m] = margin
    assert sorted(weak) == sorted(BF16_WEAK), weak                           # it stays on the list, nothing joins it
    for m, margin in weak.items():
        assert abs(margin - BF16_WEAK[m]) <= 0.25 * BF16_WEAK[m], (m, margin)
