"""CPU: the instrument of test_gpu_network.py, validated -- so that its two caps are not taken on trust.

The stock 16-bit CPU network stands in for "a 16-bit path with the wiring right", a mutated copy of it (network_cases
MUTATIONS) for "a path with one wiring fault", and the float64 twin is the reference of both.  Every stage is teacher-forced:
it is fed the honest 16-bit network's previous output, its twin the same tensor, so an error is that stage's own.  Every
16-bit operator the network needs exists on the CPU in this torch (convolutions, InstanceNorm, BatchNorm, bilinear resize,
max-pool, log-softmax in bfloat16 and float16), so nothing is emulated in fp32 here.

What bfloat16 cannot see.  A second LeakyReLU(0.01) changes a negative element by 0.99 of itself, but the negative elements
behind the first one carry 1e-4 of the tensor's energy, so on the whole tensor the fault is about 1e-2 -- the size of
bf16's own rounding (2^-9 per element, a few 1e-3 per stage).  BF16_WEAK lists the mutations whose ratio stays at or below
the cap in bf16 with the ratios measured here; fp16 sees all twelve by `rel` alone (the weakest, M3, at 5.5 times the
honest error), which is why the GPU test runs both types.

Measured here: the honest rel per stage is 2.4e-3 to 5.5e-3 in bf16 and 3e-4 to 6.5e-4 in fp16; the honest rel_neg is at
most 0.069 in bf16 (layer4.2, 2x64x96) and 0.0045 in fp16."""
import functools

import pytest
import torch

import network_cases as C

# What bf16 sees weakly or not at all BY `rel`: mutation -> the largest rel(mutated) / rel(honest) over its stages and both
# inputs, as measured on the CPU.  M1 and M2 sit at the cap itself (a run with other convolution kernels may land on either
# side of 2), M3 below it; M1 and M3 are caught by `rel_neg` all the same (0.990 and 1.000), M2 by nothing that can be
# relied on.  The test asserts that these stay below BF16_WEAK_BELOW, that every other mutation stays above it, and that
# the measured ratios are still the ones written here.
BF16_WEAK = {"M1": 2.46, "M2": 2.05, "M3": 1.20}
BF16_WEAK_BELOW = 3.0          # between the weakest clear detection (M12, 5.5) and the strongest weak one (M1, 2.46)


@functools.lru_cache(maxsize=None)
def honest(dtype, which):
    """The stock 16-bit network driven through the table on input pair `which`: per stage the inputs it was fed, the twin's
    outputs on them, and the honest rel / rel_neg of every output."""
    image_key, crops_key = C.INPUTS[which]
    net = C.network(dtype)
    tw = C.twin(net)
    record = {}

    def step(st, ins):
        with torch.no_grad():
            ys = C.as_tuple(st.on_net(net, *ins))
            refs = C.as_tuple(st.on_twin(tw, *(t.double() for t in ins)))
        assert all(y.dtype == dtype for y in ys), st.name
        record[st.name] = (st, ins, refs, [C.rel(y, r) for y, r in zip(ys, refs)],
                           [C.rel_neg(y, r) if st.leaky else None for y, r in zip(ys, refs)])
        return ys

    C.drive(C.stages(net), C.draw(C.IMAGES[image_key]).to(dtype), C.draw(C.CROPS[crops_key]).to(dtype), step)
    return net, record


def judge(record, name, ys):
    """The rule of the GPU test on one stage: -> (largest rel / honest rel over the outputs, largest rel_neg or None)."""
    st, _, refs, rels, _ = record[name]
    ratio = max(C.rel(y, r) / h for y, r, h in zip(ys, refs, rels))
    neg = max(C.rel_neg(y, r) for y, r in zip(ys, refs)) if st.leaky else None
    return ratio, neg


def flagged(ratio, neg):
    return ratio > C.RATIO_CAP or (neg is not None and neg > C.NEG_CAP)


def test_the_table_has_every_stage_the_network_has():
    net = C.network()
    table = C.stages(net)
    names = [st.name for st in table]
    assert len(names) == len(set(names))
    blocks = [n for n in names if n.startswith("layer") and n.count(".") == 1]
    assert len(blocks) == 17 and sum(n.endswith(".conv_sep1") for n in names) == sum(n.endswith(".conv2") for n in names) == 10
    assert len(names) == 2 + 17 + 20 + 4 + 1 + 2 + 1
    assert sorted(st.name for st in table if st.leaky) == sorted(
        ["layer0"] + [f"layer{k}.{i}{s}" for k, d in ((3, 6), (4, 4)) for i in range(d) for s in ("", ".conv_sep1")])
    made = [k for st in table for k in st.makes]
    assert len(made) == len(set(made)) and all(k in made + ["image", "crops"] for st in table for k in st.takes)
    assert C.slower_hooks() and sorted(C.COUNTS) == sorted(C.ORDER)


@pytest.mark.parametrize("dtype", C.DTYPES, ids=C.IDS)
def test_the_driven_stages_are_the_network_and_the_twin_has_its_rounded_weights(dtype):
    """The chain of stages, each fed the previous one's output, is `net(image)` and `net.forward_ocr(crops)` bit for bit;
    the twin's parameters are the 16-bit ones, widened."""
    net = C.network(dtype)
    tw = C.twin(net)
    assert all(q.dtype == torch.float64 and torch.equal(p.double(), q)
               for p, q in zip(net.state_dict().values(), tw.state_dict().values()) if p.is_floating_point())
    for image_key, crops_key in C.INPUTS:
        image, crops = C.draw(C.IMAGES[image_key]).to(dtype), C.draw(C.CROPS[crops_key]).to(dtype)
        with torch.no_grad():
            env = C.drive(C.stages(net), image, crops, lambda st, ins: st.on_net(net, *ins))
            want, ocr = net(image), net.forward_ocr(crops)
        assert all(torch.equal(a, b) for a, b in zip(C.flat(C.network_outputs(env)), C.flat(want)))
        assert torch.equal(env["ocr"], ocr) and tuple(ocr.shape) == (crops.size(0), 87, crops.size(3))


@pytest.mark.parametrize("dtype", C.DTYPES, ids=C.IDS)
def test_the_stock_16_bit_network_is_within_the_negative_branch_cap_on_every_leaky_stage(dtype):
    worst, worst_rel = (0.0, None), (0.0, None)
    for which, keys in enumerate(C.INPUTS):
        _, record = honest(dtype, which)
        for name, (st, _, _, rels, negs) in record.items():
            worst_rel = max(worst_rel, (max(rels), name))
            assert all(0.0 < r < 0.05 for r in rels), (name, rels)          # the honest error: small, and not zero
            if st.leaky:
                assert all(n <= C.NEG_CAP for n in negs), (name, keys, negs)
                worst = max(worst, (max(negs), f"{name} {keys[0]}"))
    print(f"{dtype}: worst honest rel_neg {worst[0]:.4f} at {worst[1]}; worst honest rel {worst_rel[0]:.2e} at {worst_rel[1]}")
    assert 0.0 < worst[0] <= C.NEG_CAP


def measure(dtype, mutation):
    """-> (largest ratio, largest rel_neg or None) of the mutated network over the mutation's stages and both inputs."""
    _, stage_names, make = C.MUTATIONS[mutation]
    ratio, neg = 0.0, None
    for which in range(len(C.INPUTS)):
        net, record = honest(dtype, which)
        with make(net), torch.no_grad():
            for name in stage_names:
                st, ins = record[name][:2]
                r, n = judge(record, name, C.as_tuple(st.on_net(net, *ins)))
                ratio = max(ratio, r)
                neg = n if neg is None else (neg if n is None else max(neg, n))
        # the context manager has put the network back: the honest path again, bit for bit
        st, ins, refs, rels, _ = record[stage_names[0]]
        with torch.no_grad():
            assert [C.rel(y, r) for y, r in zip(C.as_tuple(st.on_net(net, *ins)), refs)] == rels
    return ratio, neg


@pytest.mark.parametrize("mutation", list(C.MUTATIONS))
def test_fp16_sees_every_mutation(mutation):
    ratio, neg = measure(torch.float16, mutation)
    print(f"fp16 {mutation} ({C.MUTATIONS[mutation][0]}): rel ratio {ratio:.2f}, rel_neg {neg}")
    assert flagged(ratio, neg), (mutation, ratio, neg)
    assert ratio > C.RATIO_CAP, (mutation, ratio)                            # ... and each of them by `rel` alone


def test_bf16_sees_every_mutation_but_the_listed_ones():
    weak = {}
    for mutation in C.MUTATIONS:
        ratio, neg = measure(torch.bfloat16, mutation)
        print(f"bf16 {mutation} ({C.MUTATIONS[mutation][0]}): rel ratio {ratio:.2f}, rel_neg {neg}")
        if ratio < BF16_WEAK_BELOW:
            weak[mutation] = ratio
        else:
            assert flagged(ratio, neg) and ratio > C.RATIO_CAP, (mutation, ratio, neg)
        if mutation != "M2":                                                 # (M2 has no negative branch to show at)
            assert flagged(ratio, neg), (mutation, ratio, neg)
    assert sorted(weak) == sorted(BF16_WEAK), weak                           # they stay on the list, nothing joins it
    for mutation, ratio in weak.items():
        assert abs(ratio - BF16_WEAK[mutation]) <= 0.25 * BF16_WEAK[mutation], (mutation, ratio)


@pytest.mark.parametrize("dtype", C.DTYPES, ids=C.IDS)
def test_pooling_in_front_of_the_activation_is_not_flagged(dtype):
    """max-pool and LeakyReLU commute (both are monotone, and so is the rounding of 0.01 * x): a recogniser that pools
    first -- as the native act + pool kernel may -- is the same function and must stay within the caps."""
    for which in range(len(C.INPUTS)):
        net, record = honest(dtype, which)
        _, ins, refs, rels, _ = record["forward_ocr"]
        with torch.no_grad():
            restated = C.recogniser(net, *ins)
            rewritten = C.recogniser(net, *ins, pool_first=True)
            assert torch.equal(restated, net.forward_ocr(*ins))              # the restatement the mutations use is exact
        ratio, _ = judge(record, "forward_ocr", (rewritten,))
        print(f"{dtype} pool before act, input {which}: rel ratio {ratio:.3f}")
        assert not flagged(ratio, None) and ratio <= 1.0 + 1e-12
