"""tools/recogniser_bench.py -- the native recogniser head and activation + (2,1) max-pool against the stock chain
(measurement tool).

(a) per call    the head, one `_ocr_head_run`, against `F.log_softmax(conv11(x).squeeze(2), dim=1)`; the pool, one
                `_act_maxpool2x1_run`, at slope 0.01 against the stock pair `F.max_pool2d(F.leaky_relu(x, 0.01), (2, 1),
                (2, 1))` and at slope 1.0 against the stock pool alone, on the two maps the recogniser pools (128 x 11 and
                256 x 5 rows); at 8, 24 and 192 crops, T = 32, 64, 128, float32, bfloat16 and float16.  Stock after
                unmeasured passes, so a solver search is outside the timing.  Microseconds per call between device events
                (a round = as many back-to-back calls as fill `--window-ms`), native and stock ALTERNATED inside one
                process, median and min-max over `--rounds` rounds.
(b) forward_ocr `FOTSNet.forward_ocr` on 24 crops of 11 x 64, the other six switches on in both arms, with and without
                `use_native_recogniser`: microseconds per call between device events, and host microseconds per call.
(c) end to end  BASELINE configs[4] as tools/conv3x3_bench.py runs it: infer_image, infer_batch (eight per pass),
                infer_stream in images/s, the other six switches on in both arms, alternated per round.

Every comparison is against the stock path on the same tree in the same process.  Needs a GPU: there is no fallback.
    python tools/recogniser_bench.py [--rounds 7] [--out profiles/native_recogniser.json] [--md FILE]
                                     [--skip-shapes | --skip-ocr | --skip-e2e] [--dtypes bfloat16,float16]
`--profile VARIANT` `--profile-dtype D` `--profile-what ocr|image`: no figures -- `--profile-passes` untimed passes of
`forward_ocr` on 24 crops (ocr) or of the one-image leg (image), for
`rocprofv3 --kernel-trace --stats -- python tools/recogniser_bench.py --profile ...` (a run of its own per variant, nothing
else traced); launches and kernel time per call / per image are its stats divided by the number of passes (x images).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "fots.pytorch_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from depthwise_bench import DTYPES, IMAGES_PER_BATCH, _calls_for, _leg_fns, _spread, _time_calls  # noqa: E402

CROPS, WIDTHS = (8, 24, 192), (32, 64, 128)
POOLS = (("pool1", 128, 11), ("pool2", 256, 5))          # (name, channels, rows) of the two maps forward_ocr pools
HEAD_C, HEAD_K = 256, 87
VARIANTS = ("dw+in+heads+blocks+merge+conv", "dw+in+heads+blocks+merge+conv+ocr")
LEGS = ("infer_image", "infer_batch", "infer_stream")
OCR_CROPS = (24, 64, 11, 64)


def _alternate(fns, rounds, window_ms, device):
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize(device)
    n = {k: _calls_for(fn, window_ms) for k, fn in fns.items()}
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():                                   # alternated
            t[k].append(_time_calls(fn, n[k]))
    return {k + "_us": _spread(v) for k, v in t.items()}, n


def measure_shapes(device, rounds, window_ms, dtypes):
    from rroi_align._ext import rroi_align as ext
    heads, pools = [], []
    torch.manual_seed(0)
    with torch.no_grad():
        for name, dtype in dtypes:
            conv11 = torch.nn.Conv2d(HEAD_C, HEAD_K, 1).to(device).to(dtype)
            w, b = conv11.weight.detach(), conv11.bias.detach()
            for N in CROPS:
                for T in WIDTHS:
                    x = torch.randn(N, HEAD_C, 1, T, device=device).to(dtype)
                    fns = {"native": lambda x=x: ext._ocr_head_run(x, w, b),
                           "stock": lambda x=x: F.log_softmax(conv11(x).squeeze(2), dim=1)}
                    row, n = _alternate(fns, rounds, window_ms, device)
                    p = ext.ocr_head_plan(N, HEAD_C, HEAD_K, T, dtype=dtype)
                    row.update(dtype=name, N=N, T=T, waves=p.waves, grid=p.grid_x, calls_per_round=n)
                    nat, stk = row["native_us"]["median"], row["stock_us"]["median"]
                    row["stock_over_native"] = round(stk / nat, 2)
                    row["native_below_stock"] = nat < stk
                    row["native_GFMAs"] = round(N * T * HEAD_C * HEAD_K / nat * 1e-3, 1)   # double FMAs per second, 1e9
                    heads.append(row)
                    print("%-8s head  N=%-3d T=%-3d grid %-4d native %7.1f us (%.1f-%.1f)  stock %7.1f us (%.1f-%.1f)  x%.2f" % (
                        name, N, T, p.grid_x, nat, row["native_us"]["min"], row["native_us"]["max"], stk,
                        row["stock_us"]["min"], row["stock_us"]["max"], row["stock_over_native"]), file=sys.stderr)
                    for what, C, H in POOLS:
                        x = torch.randn(N, C, H, T, device=device).to(dtype)
                        fns = {"native_act": lambda x=x: ext._act_maxpool2x1_run(x, 0.01),
                               "stock_pair": lambda x=x: F.max_pool2d(F.leaky_relu(x, 0.01), (2, 1), stride=(2, 1)),
                               "native_plain": lambda x=x: ext._act_maxpool2x1_run(x, 1.0),
                               "stock_pool": lambda x=x: F.max_pool2d(x, (2, 1), stride=(2, 1))}
                        row, n = _alternate(fns, rounds, window_ms, device)
                        row.update(dtype=name, what=what, N=N, C=C, H=H, T=T, calls_per_round=n)
                        moved = x.element_size() * N * C * T * (2 * (H // 2) + H // 2)
                        row["pair_over_native"] = round(row["stock_pair_us"]["median"] / row["native_act_us"]["median"], 2)
                        row["pool_over_native"] = round(row["stock_pool_us"]["median"] / row["native_plain_us"]["median"], 2)
                        row["native_below_pair"] = row["native_act_us"]["median"] < row["stock_pair_us"]["median"]
                        row["native_below_pool"] = row["native_plain_us"]["median"] < row["stock_pool_us"]["median"]
                        row["native_TBps"] = round(moved / row["native_act_us"]["median"] * 1e-6, 3)
                        pools.append(row)
                        print("%-8s %s N=%-3d T=%-3d native %6.1f / %6.1f us  stock pair %6.1f  pool %6.1f us  x%.2f x%.2f" % (
                            name, what, N, T, row["native_act_us"]["median"], row["native_plain_us"]["median"],
                            row["stock_pair_us"]["median"], row["stock_pool_us"]["median"], row["pair_over_native"],
                            row["pool_over_native"]), file=sys.stderr)
    return heads, pools


def _switch(net, variant):
    from fots_e2e.native import (use_native_blocks, use_native_conv3x3, use_native_depthwise, use_native_heads,
                                 use_native_instancenorm, use_native_merge, use_native_recogniser)
    assert use_native_depthwise(net) == 22 and use_native_instancenorm(net) == (52, 20) and use_native_heads(net)
    assert use_native_blocks(net) == (2, 7, 10) and use_native_merge(net) and use_native_conv3x3(net) == (23, 2)
    if variant.endswith("ocr"):
        assert use_native_recogniser(net)
    return net


def _network(device, dtype, variant):
    from fots_e2e.alphabet import ALPHABET
    from fots_e2e.model import FOTSNet
    from fots_e2e.weights import deterministic_init
    return _switch(deterministic_init(FOTSNet(len(ALPHABET) + 1)).eval().to(device).to(dtype), variant)


def _host_us(fn, iters, device):
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    t1 = time.perf_counter()                                        # the launches alone: the queue is drained afterwards
    torch.cuda.synchronize(device)
    return (t1 - t0) * 1e6 / iters


def measure_ocr(device, rounds, window_ms, dtypes):
    """(b): forward_ocr alone on 24 crops, switched against not switched."""
    out = []
    torch.manual_seed(0)
    with torch.no_grad():
        for name, dtype in dtypes:
            crops = torch.randn(*OCR_CROPS, device=device).to(dtype)
            nets = {v: _network(device, dtype, v) for v in VARIANTS}
            fns = {v: (lambda net=net: net.forward_ocr(crops)) for v, net in nets.items()}
            row, n = _alternate(fns, rounds, window_ms, device)
            host = {v: [] for v in VARIANTS}
            for _ in range(rounds):
                for v, fn in fns.items():
                    host[v].append(_host_us(fn, 50, device))
            without, with_ocr = VARIANTS
            r = {"dtype": name, "crops": list(OCR_CROPS), "device_us": {v: row[v + "_us"] for v in VARIANTS},
                 "host_us": {v: _spread(host[v]) for v in VARIANTS}, "calls_per_round": n}
            r["without_over_with"] = round(r["device_us"][without]["median"] / r["device_us"][with_ocr]["median"], 3)
            r["with_below_without_min"] = r["device_us"][with_ocr]["median"] < r["device_us"][without]["min"]
            out.append(r)
            print("%-8s forward_ocr  without %.1f us (%.1f-%.1f) host %.1f   with %.1f us (%.1f-%.1f) host %.1f   x%.3f" % (
                name, r["device_us"][without]["median"], r["device_us"][without]["min"], r["device_us"][without]["max"],
                r["host_us"][without]["median"], r["device_us"][with_ocr]["median"], r["device_us"][with_ocr]["min"],
                r["device_us"][with_ocr]["max"], r["host_us"][with_ocr]["median"], r["without_over_with"]), file=sys.stderr)
    return out


def _e2e_setup(device, dtypes, stream_batches, variants):
    import bench_e2e as B
    from e2e_inputs import synthetic_detector_maps
    from fots_e2e.alphabet import ALPHABET
    from fots_e2e.hostcpus import cap_torch_threads
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
            legs[(name, variant)] = dict(net=_network(device, dtype, variant), maps=maps, stacked=stacked)
    torch.cuda.synchronize(device)
    return dict(conv=conv, ims=ims, source=source, groups=groups, seq_groups=seq_groups, legs=legs, host_threads=host_threads)


def measure_e2e(device, rounds, stream_batches, dtypes):
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
    without, with_ocr = VARIANTS
    for name, _ in dtypes:
        d = {v: {leg: {"images_per_s": _spread(raw[(name, v)][leg]), "per_round": [round(x, 2) for x in raw[(name, v)][leg]]}
                 for leg in LEGS} for v in VARIANTS}
        # the bar (DESIGN 5.10's): the native median is not below the other arm's minimum of the same run
        d["ocr_over_without"] = {leg: round(d[with_ocr][leg]["images_per_s"]["median"] / d[without][leg]["images_per_s"]["median"], 3)
                                 for leg in LEGS}
        d["ocr_not_below_without_min"] = {leg: d[with_ocr][leg]["images_per_s"]["median"] >= d[without][leg]["images_per_s"]["min"]
                                          for leg in LEGS}
        # a gain outside the spread: the native arm's minimum above the other arm's maximum
        d["ocr_gain_outside_spread"] = {leg: d[with_ocr][leg]["images_per_s"]["min"] > d[without][leg]["images_per_s"]["max"]
                                        for leg in LEGS}
        out["dtypes"][name] = d
        for v in VARIANTS:
            print("%-9s %-36s" % (name, v) + "  ".join("%s %.1f (%.1f-%.1f)" % (
                leg, d[v][leg]["images_per_s"]["median"], d[v][leg]["images_per_s"]["min"], d[v][leg]["images_per_s"]["max"])
                for leg in LEGS) + " img/s", file=sys.stderr)
    return out


def profile(device, variant, dtype_name, passes, what):
    dtypes = [d for d in DTYPES if d[0] == dtype_name]
    if what == "ocr":
        net = _network(device, dtypes[0][1], variant)
        crops = torch.randn(*OCR_CROPS, device=device).to(dtypes[0][1])
        with torch.no_grad():
            for _ in range(passes):
                net.forward_ocr(crops)
        torch.cuda.synchronize(device)
        return {"profiled": variant, "what": what, "dtype": dtype_name, "passes": passes, "crops": list(OCR_CROPS)}
    S = _e2e_setup(device, dtypes, 2, (variant,))
    leg_image, _, _ = _leg_fns(S, device)
    with torch.no_grad():
        for _ in range(passes):
            leg_image(S["legs"][(dtype_name, variant)])
    return {"profiled": variant, "what": what, "dtype": dtype_name, "passes": passes, "images": len(S["ims"])}


def markdown(out):
    """The tables of profiles/native_recogniser.md, from the JSON."""
    md = ["<!-- tables written by tools/recogniser_bench.py --md; median (min-max) over %d rounds on %s -->" % (out["rounds"], out["device"]), ""]
    us = lambda r, k: "%.1f (%.1f-%.1f)" % (r[k]["median"], r[k]["min"], r[k]["max"])  # noqa: E731
    if "heads" in out:
        md += ["### Per call: the head against `log_softmax(conv11(x).squeeze(2))`, 256 channels, 87 classes", "",
               "| dtype | crops | T | grid | native us | stock us | stock / native | 1e9 double FMA/s |", "|---|---|---|---|---|---|---|---|"]
        for r in out["heads"]:
            md.append("| %s | %d | %d | %d | %s | %s | %.2f | %.1f |" % (r["dtype"], r["N"], r["T"], r["grid"], us(r, "native_us"),
                                                                        us(r, "stock_us"), r["stock_over_native"], r["native_GFMAs"]))
        md += ["", "### Per call: activation + pool against the stock pair (slope 0.01) and the stock pool alone (slope 1.0)", "",
               "| dtype | map | crops | T | native 0.01 us | stock pair us | pair / native | native 1.0 us | stock pool us | pool / native | native TB/s |",
               "|---|---|---|---|---|---|---|---|---|---|---|"]
        for r in out["pools"]:
            md.append("| %s | %dx%d | %d | %d | %s | %s | %.2f | %s | %s | %.2f | %.2f |" % (
                r["dtype"], r["C"], r["H"], r["N"], r["T"], us(r, "native_act_us"), us(r, "stock_pair_us"), r["pair_over_native"],
                us(r, "native_plain_us"), us(r, "stock_pool_us"), r["pool_over_native"], r["native_TBps"]))
        md.append("")
    if "forward_ocr" in out:
        md += ["### `forward_ocr` alone on 24 crops of 11 x 64, the other six switches on in both arms", "",
               "| dtype | without: device us | host us | with: device us | host us | without / with | with median < without min |",
               "|---|---|---|---|---|---|---|"]
        for r in out["forward_ocr"]:
            a, b = VARIANTS
            md.append("| %s | %s | %.1f | %s | %.1f | %.3f | %s |" % (
                r["dtype"], us(r["device_us"], a), r["host_us"][a]["median"], us(r["device_us"], b), r["host_us"][b]["median"],
                r["without_over_with"], "yes" if r["with_below_without_min"] else "no"))
        md.append("")
    if "end_to_end" in out:
        md += ["### End to end, images/s: the other six switches on in both arms", "",
               "| dtype | leg | without | with the recogniser | with / without | median >= the other's min | min > the other's max |",
               "|---|---|---|---|---|---|---|"]
        for name, d in out["end_to_end"]["dtypes"].items():
            for leg in LEGS:
                cell = lambda v: "%.1f (%.1f-%.1f)" % tuple(d[v][leg]["images_per_s"][k] for k in ("median", "min", "max"))  # noqa: E731
                md.append("| %s | %s | %s | %s | %.3f | %s | %s |" % (
                    name, leg, cell(VARIANTS[0]), cell(VARIANTS[1]), d["ocr_over_without"][leg],
                    "yes" if d["ocr_not_below_without_min"][leg] else "no", "yes" if d["ocr_gain_outside_spread"][leg] else "no"))
        md.append("")
    return "\n".join(md)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=20.0,
                    help="(a), (b): a round times as many back-to-back calls as fill this window (at least 30)")
    ap.add_argument("--stream-batches", type=int, default=6)
    ap.add_argument("--dtypes", default="float32,bfloat16,float16")
    ap.add_argument("--skip-shapes", action="store_true")
    ap.add_argument("--skip-ocr", action="store_true")
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    ap.add_argument("--md", default=None, help="write the tables as markdown here")
    ap.add_argument("--profile", choices=VARIANTS, default=None, help="untimed passes of one variant, for rocprofv3")
    ap.add_argument("--profile-dtype", choices=[n for n, _ in DTYPES], default="bfloat16")
    ap.add_argument("--profile-what", choices=("ocr", "image"), default="ocr")
    ap.add_argument("--profile-passes", type=int, default=3)
    args = ap.parse_args()
    if args.rounds < 3:
        ap.error("--rounds must be at least 3: the spread over the rounds is part of the result")
    if not torch.cuda.is_available():
        raise SystemExit("recogniser_bench: no GPU -- this tool measures on the device and has no fallback")
    device = torch.device("cuda", 0)
    if args.profile:
        print(json.dumps(profile(device, args.profile, args.profile_dtype, args.profile_passes, args.profile_what)))
        return
    dtypes = [d for d in DTYPES if d[0] in args.dtypes.split(",")]
    out = {"rounds": args.rounds, "device": torch.cuda.get_device_name(device),
           "what": "native recogniser head and activation + pool against the stock chain, alternated per round in one process; "
                   "median (min, max) over the rounds; (a), (b) microseconds per call between device events, (c) images/s, host "
                   "clock around work that ends in a device synchronise"}
    if not args.skip_shapes:
        out["heads"], out["pools"] = measure_shapes(device, args.rounds, args.window_ms, dtypes)
        out["every_head_row_native_below_stock"] = all(r["native_below_stock"] for r in out["heads"])
        out["every_pool_row_native_below_stock"] = all(r["native_below_pair"] and r["native_below_pool"] for r in out["pools"])
    if not args.skip_ocr:
        out["forward_ocr"] = measure_ocr(device, args.rounds, args.window_ms, dtypes)
    if not args.skip_e2e:
        out["end_to_end"] = measure_e2e(device, args.rounds, args.stream_batches, [d for d in dtypes if d[0] != "float32"])
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    if args.md:
        with open(args.md, "w") as f:
            f.write(markdown(out) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
