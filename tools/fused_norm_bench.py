"""tools/fused_norm_bench.py -- the fused InstanceNorm epilogues against the stock chains they replace (measurement tool).

(a) per call    both `_MirrorNorm` shapes of the stem and a block tail at each of layer1 .. layer4's shapes at 1280 x 704, at
                N = 1 and N = 8, float32 and bfloat16.  The stock side is the exact stock chain on stock modules:
                `F.leaky_relu(bn(torch.cat((x, -x), 1)), 0.01)` for the mirror, `F.relu(bn(t) + r)` (layer1, layer2) /
                `F.leaky_relu(bn(t) + r, 0.01)` (layer3, layer4) for a tail; the native side is one
                `_instance_norm_fused_run`.  A third column, for information, is the chain as `use_native_instancenorm`
                leaves it: the native norm, then torch's add and activation.  Microseconds per call between device events (a
                round = as many back-to-back calls as fill `--window-ms`), the variants ALTERNATED inside one process, median
                and min-max over `--rounds` rounds.  For the stem's two shapes also the achieved bytes/s against
                (1 + 1 + 2) * N * C * H * W * sizeof(T): x read twice, 2C planes written.
(b) end to end  BASELINE configs[4] as tools/depthwise_bench.py runs it: infer_image, infer_batch (eight per pass),
                infer_stream in images/s, float32 and bfloat16, `dw+in+heads` against `dw+in+heads+blocks`, alternated
                per round.

Every comparison is against the stock path on the same tree in the same process.  Needs a GPU: there is no fallback.
    python tools/fused_norm_bench.py [--rounds 7] [--out profiles/native_fused_norm.json] [--skip-shapes | --skip-e2e]
`--profile VARIANT` `--profile-dtype D`: no figures -- the one-image leg alone, `--profile-passes` passes over the 11 images,
for `rocprofv3 --kernel-trace --stats -- python tools/fused_norm_bench.py --profile dw+in+heads+blocks` (a run of its own,
never with --pmc, after an unprofiled run of the same command); launches and kernel time per image are its stats divided by
passes x 11.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "fots.pytorch_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from depthwise_bench import DTYPES, IMAGES_PER_BATCH, _calls_for, _leg_fns, _spread, _time_calls  # noqa: E402

# (C of x, H, W): the stem's two mirror norms (16 -> 32, 32 -> 64 channels)
MIRRORS = ((16, 704, 1280), (32, 352, 640))
# (C, H, W, slope): a block tail in layer1 .. layer4
TAILS = ((64, 176, 320, 0.0), (128, 88, 160, 0.0), (256, 44, 80, 0.01), (512, 22, 40, 0.01))
VARIANTS = ("dw+in+heads", "dw+in+heads+blocks")
LEGS = ("infer_image", "infer_batch", "infer_stream")
EPS = 1e-5


def _norm(channels, device, dtype, g):
    bn = nn.InstanceNorm2d(channels, eps=EPS, momentum=0.1, affine=True)
    with torch.no_grad():
        bn.weight.copy_(torch.randn(channels, generator=g) * 0.5 + 1)
        bn.bias.copy_(torch.randn(channels, generator=g))
    return bn.to(device).to(dtype).eval()


def _cases(device, dtype, g):
    """-> (what, N, C, H, W, {variant: fn}, bytes of x)"""
    from rroi_align._ext import rroi_align as ext
    for N in (1, 8):
        for C, H, W in MIRRORS:
            x = torch.randn(N, C, H, W, device=device).to(dtype)
            bn = _norm(2 * C, device, dtype, g)
            w, b = bn.weight.detach(), bn.bias.detach()
            yield "mirror", N, C, H, W, {
                "native": lambda x=x, w=w, b=b: ext._instance_norm_fused_run(x, w, b, EPS, 0.01, None, True),
                "stock": lambda x=x, bn=bn: F.leaky_relu(bn(torch.cat((x, -x), 1)), 0.01),
                "in_chain": lambda x=x, w=w, b=b: ext._instance_norm_run(torch.cat((x, -x), 1), w, b, EPS, 0.01),
            }, x.numel() * x.element_size()
        for C, H, W, slope in TAILS:
            t = torch.randn(N, C, H, W, device=device).to(dtype)
            r = torch.randn(N, C, H, W, device=device).to(dtype)
            bn = _norm(C, device, dtype, g)
            w, b = bn.weight.detach(), bn.bias.detach()
            act = (lambda v: F.leaky_relu(v, slope)) if slope else F.relu
            yield "tail", N, C, H, W, {
                "native": lambda t=t, r=r, w=w, b=b, slope=slope: ext._instance_norm_fused_run(t, w, b, EPS, slope, r, False),
                "stock": lambda t=t, r=r, bn=bn, act=act: act(bn(t) + r),
                "in_chain": lambda t=t, r=r, w=w, b=b, act=act: act(ext._instance_norm_run(t, w, b, EPS, 1.0) + r),
            }, t.numel() * t.element_size()


def measure_shapes(device, rounds, window_ms):
    rows = []
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for name, dtype in DTYPES[:2]:
            for what, N, C, H, W, fns, nbytes in _cases(device, dtype, g):
                for fn in fns.values():                                     # warm-up: MIOpen picks here
                    for _ in range(3):
                        fn()
                torch.cuda.synchronize(device)
                n = {k: _calls_for(fn, window_ms) for k, fn in fns.items()}
                t = {k: [] for k in fns}
                for _ in range(rounds):
                    for k, fn in fns.items():
                        t[k].append(_time_calls(fn, n[k]))
                row = {"dtype": name, "what": what, "N": N, "C": C, "H": H, "W": W, "calls_per_round": n}
                for k in fns:
                    row[k + "_us"] = _spread(t[k])
                row["stock_over_native"] = round(row["stock_us"]["median"] / row["native_us"]["median"], 2)
                row["in_chain_over_native"] = round(row["in_chain_us"]["median"] / row["native_us"]["median"], 2)
                row["native_below_stock"] = row["native_us"]["median"] < row["stock_us"]["median"]
                if what == "mirror":
                    row["native_TBps"] = round(4 * nbytes / row["native_us"]["median"] * 1e-6, 3)
                rows.append(row)
                print("%-8s %-6s N=%d %3dx%3dx%4d  native %8.1f us (%.1f-%.1f)  stock %8.1f us (%.1f-%.1f)  x%.2f   5.11 chain %8.1f us  x%.2f%s" % (
                    name, what, N, C, H, W, row["native_us"]["median"], row["native_us"]["min"], row["native_us"]["max"],
                    row["stock_us"]["median"], row["stock_us"]["min"], row["stock_us"]["max"], row["stock_over_native"],
                    row["in_chain_us"]["median"], row["in_chain_over_native"],
                    "   %.2f TB/s" % row["native_TBps"] if what == "mirror" else ""), file=sys.stderr)
    return rows


def _switch(net, variant):
    from fots_e2e.native import use_native_blocks, use_native_depthwise, use_native_heads, use_native_instancenorm
    assert use_native_depthwise(net) == 22 and use_native_instancenorm(net) == (52, 20) and use_native_heads(net)
    if variant.endswith("blocks"):
        assert use_native_blocks(net) == (2, 7, 10)
    return net


def _e2e_setup(device, dtypes, stream_batches, variants):
    import bench_e2e as B
    from e2e_inputs import synthetic_detector_maps
    from fots_e2e.alphabet import ALPHABET
    from fots_e2e.hostcpus import cap_torch_threads
    from fots_e2e.model import FOTSNet
    from fots_e2e.weights import deterministic_init
    from rroi_align.decode import CTCLabelConverter
    host_threads = cap_torch_threads()
    conv = CTCLabelConverter(ALPHABET)
    ims, source = B.load_images()
    maps_np = [synthetic_detector_maps(704, 1280, B.BOXES_PER_IMAGE, seed=i) for i in range(len(ims))]
    order = [i % len(ims) for i in range(2 * IMAGES_PER_BATCH)]
    groups = [order[i:i + IMAGES_PER_BATCH] for i in range(0, len(order), IMAGES_PER_BATCH)]
    seq_groups = [k % len(groups) for k in range(stream_batches)]
    legs = {}
    for name, dtype in dtypes:
        maps = [tuple(torch.from_numpy(a).to(device).to(dtype) for a in m) for m in maps_np]
        stacked = [tuple(torch.stack([maps[i][j] for i in g]) for j in range(3)) for g in groups]   # outside every timer
        for variant in variants:
            net = _switch(deterministic_init(FOTSNet(len(ALPHABET) + 1)).eval().to(device).to(dtype), variant)
            legs[(name, variant)] = dict(net=net, maps=maps, stacked=stacked)
    torch.cuda.synchronize(device)
    return dict(conv=conv, ims=ims, source=source, groups=groups, seq_groups=seq_groups, legs=legs, host_threads=host_threads)


def measure_e2e(device, rounds, stream_batches):
    dtypes = DTYPES[:2]
    S = _e2e_setup(device, dtypes, stream_batches, VARIANTS)
    leg_image, leg_batch, leg_stream = _leg_fns(S, device)
    keys = [(name, v) for name, _ in dtypes for v in VARIANTS]
    raw = {k: {leg: [] for leg in LEGS} for k in keys}
    with torch.no_grad():
        for k in keys:                                   # warm-up: every shape of every dtype, the side stream included
            leg_image(S["legs"][k])
            leg_batch(S["legs"][k])
            leg_stream(S["legs"][k])
        for _round in range(rounds):
            for k in keys:                               # alternated: the variants within every round and dtype
                L = S["legs"][k]
                raw[k]["infer_image"].append(1.0 / float(np.median(leg_image(L))))
                raw[k]["infer_batch"].append(IMAGES_PER_BATCH / float(np.median(leg_batch(L))))
                raw[k]["infer_stream"].append(IMAGES_PER_BATCH * len(S["seq_groups"]) / leg_stream(L))
    out = {"images": S["source"], "images_per_batch": IMAGES_PER_BATCH, "stream_batches": len(S["seq_groups"]),
           "host_threads": S["host_threads"], "dtypes": {}}
    stock, native = VARIANTS
    for name, _ in dtypes:
        d = {v: {leg: {"images_per_s": _spread(raw[(name, v)][leg]), "per_round": [round(x, 2) for x in raw[(name, v)][leg]]}
                 for leg in LEGS} for v in VARIANTS}
        # the bar (DESIGN 5.10's): the native median is not below the stock leg's minimum of the same run
        d["blocks_over_without"] = {leg: round(d[native][leg]["images_per_s"]["median"] / d[stock][leg]["images_per_s"]["median"], 3) for leg in LEGS}
        d["blocks_not_below_without_min"] = {leg: d[native][leg]["images_per_s"]["median"] >= d[stock][leg]["images_per_s"]["min"] for leg in LEGS}
        out["dtypes"][name] = d
        for v in VARIANTS:
            print("%-9s %-19s" % (name, v) + "  ".join("%s %.1f (%.1f-%.1f)" % (
                leg, d[v][leg]["images_per_s"]["median"], d[v][leg]["images_per_s"]["min"], d[v][leg]["images_per_s"]["max"])
                for leg in LEGS) + " img/s", file=sys.stderr)
    return out


def profile(device, variant, dtype_name, passes):
    dtypes = [d for d in DTYPES if d[0] == dtype_name]
    S = _e2e_setup(device, dtypes, 2, (variant,))
    leg_image, _, _ = _leg_fns(S, device)
    with torch.no_grad():
        for _ in range(passes):
            leg_image(S["legs"][(dtype_name, variant)])
    return {"profiled": variant, "dtype": dtype_name, "passes": passes, "images": len(S["ims"])}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=50.0,
                    help="(a): a round times as many back-to-back calls as fill this window (at least 30)")
    ap.add_argument("--stream-batches", type=int, default=6)
    ap.add_argument("--skip-shapes", action="store_true")
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    ap.add_argument("--profile", choices=VARIANTS, default=None, help="untimed one-image passes of one variant, for rocprofv3")
    ap.add_argument("--profile-dtype", choices=[n for n, _ in DTYPES], default="float32")
    ap.add_argument("--profile-passes", type=int, default=3)
    args = ap.parse_args()
    if args.rounds < 3:
        ap.error("--rounds must be at least 3: the spread over the rounds is part of the result")
    if not torch.cuda.is_available():
        raise SystemExit("fused_norm_bench: no GPU -- this tool measures on the device and has no fallback")
    device = torch.device("cuda", 0)
    if args.profile:
        print(json.dumps(profile(device, args.profile, args.profile_dtype, args.profile_passes)))
        return
    out = {"rounds": args.rounds, "device": torch.cuda.get_device_name(device),
           "what": "fused InstanceNorm epilogues (mirror, residual tail) against the stock chains, alternated per round in one "
                   "process; median (min, max) over the rounds; (a) microseconds per call between device events, (b) images/s, "
                   "host clock around work that ends in a device synchronise"}
    if not args.skip_shapes:
        out["shapes"] = measure_shapes(device, args.rounds, args.window_ms)
        out["every_row_native_below_stock"] = all(r["native_below_stock"] for r in out["shapes"])
    if not args.skip_e2e:
        out["end_to_end"] = measure_e2e(device, args.rounds, args.stream_batches)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
