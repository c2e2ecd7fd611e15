"""tools/remainder_bench.py -- the native (2,3) convolution and the fused resize + depthwise 3x3 against what they replace
(measurement tool).  The method of tools/conv1x1_bench.py.

(a) conv2x3     `conv10_s` on 8, 24 and 192 crops at T = 32, 64 and 128 columns ((N, 256, 2, T) -> (N, 256, 1, T)), bfloat16
                and float16: one `run_conv2x3` against `F.conv2d(x, w, padding=(0, 1))` on the same tensors, after three
                unmeasured passes, so a solver search is outside the timing.
(b) resize+dw   256 x 44x80 -> 88x160 and 256 x 88x160 -> 176x320 at N = 1 and 8, three dtypes: one `run_up_depthwise3x3`
                against the path it replaces, stock `F.interpolate(bilinear, align_corners=True)` followed by the native
                `_depthwise3x3_run`.
                Microseconds per call between device events (a round = as many back-to-back calls as fill `--window-ms`),
                the arms ALTERNATED inside one process, median and min-max over `--rounds` rounds.
(c) end to end  BASELINE configs[4] as tools/depthwise_bench.py runs it: infer_image, infer_batch (eight per pass),
                infer_stream in images/s.  bfloat16 / float16: the eight switches of fots_e2e.native on in both arms,
                without and with the two of fots_e2e.native_remainder.  float32: the six switches that apply on in both
                arms, `use_native_upconv` alone as the new arm.  Alternated per round.

Every comparison is against the other path on the same tree in the same process.  Needs a GPU: there is no fallback.
    python tools/remainder_bench.py [--rounds 7] [--out profiles/native_remainder.json] [--md FILE]
                                    [--skip-shapes | --skip-e2e] [--e2e-dtypes bfloat16,float16,float32]
`--profile VARIANT` `--profile-dtype D`: no figures -- the one-image leg alone, `--profile-passes` passes over the images,
for `rocprofv3 --kernel-trace --stats -- python tools/remainder_bench.py --profile ...` (a run of its own per variant,
nothing else traced); launches per image are its stats divided by passes x images.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "fots.pytorch_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from depthwise_bench import DTYPES, IMAGES_PER_BATCH, _calls_for, _leg_fns, _spread, _time_calls  # noqa: E402

HALF = DTYPES[1:]                      # bfloat16, float16
CONV_ROWS = tuple((n, t) for n in (8, 24, 192) for t in (32, 64, 128))
UP_ROWS = tuple((n, s) for n in (1, 8) for s in ((256, 44, 80, 88, 160), (256, 88, 160, 176, 320)))
VARIANTS = ("without", "with the remainder")
LEGS = ("infer_image", "infer_batch", "infer_stream")


def _measure(fns, rounds, window_ms, device):
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize(device)
    n = {k: _calls_for(fn, window_ms) for k, fn in fns.items()}
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():                           # alternated
            t[k].append(_time_calls(fn, n[k]))
    return {k + "_us": _spread(t[k]) for k in fns}, n


def measure_conv2x3(device, rounds, window_ms):
    from rroi_align._ext.rroi_align import remainder as rem
    out = []
    torch.manual_seed(0)
    with torch.no_grad():
        for name, dtype in HALF:
            for N, T in CONV_ROWS:
                x = torch.randn(N, 256, 2, T, device=device).to(dtype)
                w = (torch.randn(256, 256, 2, 3, device=device) / (6 * 256) ** 0.5).to(dtype)
                fns = {"native": lambda x=x, w=w: rem.run_conv2x3(x, w),
                       "stock": lambda x=x, w=w: F.conv2d(x, w, padding=(0, 1))}
                row, n = _measure(fns, rounds, window_ms, device)
                p = rem.conv2x3_plan(N, 256, 256, 2, T, dtype=dtype)
                nat, stk = row["native_us"]["median"], row["stock_us"]["median"]
                row.update(dtype=name, N=N, T=T, items=p.items, grid=p.grid_x, calls_per_round=n,
                           stock_over_native=round(stk / nat, 2), native_below_stock=nat < stk,
                           native_TFLOPs=round(2.0 * 6 * 256 * N * 256 * T / nat * 1e-6, 2))
                out.append(row)
                print("%-8s conv2x3 N=%-3d T=%-3d grid %-4d native %7.1f us (%.1f-%.1f)  stock %7.1f us (%.1f-%.1f)  x%.2f" % (
                    name, N, T, p.grid_x, nat, row["native_us"]["min"], row["native_us"]["max"], stk, row["stock_us"]["min"],
                    row["stock_us"]["max"], row["stock_over_native"]), file=sys.stderr)
    return out


def measure_updw(device, rounds, window_ms):
    from rroi_align._ext import rroi_align as ext
    from rroi_align._ext.rroi_align import remainder as rem
    out = []
    torch.manual_seed(0)
    with torch.no_grad():
        for name, dtype in DTYPES:
            for N, (C, h, w_in, Ho, Wo) in UP_ROWS:
                a = torch.randn(N, C, h, w_in, device=device).to(dtype)
                w = torch.randn(C, 1, 3, 3, device=device).to(dtype)
                fns = {"native": lambda a=a, w=w, s=(Ho, Wo): rem.run_up_depthwise3x3(a, w, s),
                       "stock": lambda a=a, w=w, s=(Ho, Wo): ext._depthwise3x3_run(
                           F.interpolate(a, size=s, mode="bilinear", align_corners=True), w, 1)}
                row, n = _measure(fns, rounds, window_ms, device)
                nat, stk = row["native_us"]["median"], row["stock_us"]["median"]
                moved = a.element_size() * N * C * (h * w_in + Ho * Wo)
                row.update(dtype=name, N=N, C=C, source=[h, w_in], target=[Ho, Wo], calls_per_round=n,
                           stock_over_native=round(stk / nat, 2), native_below_stock=nat < stk,
                           native_TBps=round(moved / nat * 1e-6, 3))
                out.append(row)
                print("%-8s resize+dw N=%-2d %dx%d>%dx%d native %7.1f us (%.1f-%.1f)  resize, depthwise %7.1f us (%.1f-%.1f)  x%.2f" % (
                    name, N, h, w_in, Ho, Wo, nat, row["native_us"]["min"], row["native_us"]["max"], stk, row["stock_us"]["min"],
                    row["stock_us"]["max"], row["stock_over_native"]), file=sys.stderr)
    return out


def _switch(net, variant, dtype):
    from fots_e2e import native as nat
    from fots_e2e import native_remainder as rm
    assert nat.use_native_depthwise(net) == 22 and nat.use_native_instancenorm(net) == (52, 20) and nat.use_native_heads(net)
    assert nat.use_native_blocks(net) == (2, 7, 10) and nat.use_native_merge(net) and nat.use_native_recogniser(net)
    if dtype != torch.float32:
        assert nat.use_native_conv3x3(net) == (23, 2) and nat.use_native_conv1x1(net) == (29, 3)
    if variant == VARIANTS[1]:
        assert rm.use_native_upconv(net) == 2
        if dtype != torch.float32:
            assert rm.use_native_conv2x3(net) == 1
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
            net = _switch(deterministic_init(FOTSNet(len(ALPHABET) + 1)).eval().to(device).to(dtype), variant, dtype)
            legs[(name, variant)] = dict(net=net, maps=maps, stacked=stacked)
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
    without, with_new = VARIANTS
    for name, _ in dtypes:
        d = {v: {leg: {"images_per_s": _spread(raw[(name, v)][leg]), "per_round": [round(x, 2) for x in raw[(name, v)][leg]]}
                 for leg in LEGS} for v in VARIANTS}
        # the bar (DESIGN 5.10's): the native median is not below the other arm's minimum of the same run
        d["with_over_without"] = {leg: round(d[with_new][leg]["images_per_s"]["median"] / d[without][leg]["images_per_s"]["median"], 3)
                                  for leg in LEGS}
        d["with_not_below_without_min"] = {leg: d[with_new][leg]["images_per_s"]["median"] >= d[without][leg]["images_per_s"]["min"]
                                           for leg in LEGS}
        d["gain_outside_the_spread"] = {leg: d[with_new][leg]["images_per_s"]["min"] > d[without][leg]["images_per_s"]["max"]
                                        for leg in LEGS}
        out["dtypes"][name] = d
        for v in VARIANTS:
            print("%-9s %-20s" % (name, v) + "  ".join("%s %.1f (%.1f-%.1f)" % (
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


def markdown(out):
    """The tables of profiles/native_remainder.md, from the JSON."""
    md = ["<!-- tables written by tools/remainder_bench.py --md; median (min-max) over %d rounds on %s -->" % (out["rounds"], out["device"]), ""]
    us = lambda r, k: "%.1f (%.1f-%.1f)" % (r[k]["median"], r[k]["min"], r[k]["max"])  # noqa: E731
    if "conv2x3" in out:
        md += ["### conv2x3 per call: native against `F.conv2d`, (N, 256, 2, T) -> (N, 256, 1, T)", "",
               "| dtype | crops N | T | items | grid | native us | stock us | stock / native | native TFLOP/s |", "|---|---|---|---|---|---|---|---|---|"]
        for r in out["conv2x3"]:
            md.append("| %s | %d | %d | %d | %d | %s | %s | %.2f | %.2f |" % (
                r["dtype"], r["N"], r["T"], r["items"], r["grid"], us(r, "native_us"), us(r, "stock_us"), r["stock_over_native"],
                r["native_TFLOPs"]))
        md.append("")
    if "up_depthwise" in out:
        md += ["### resize + depthwise per call: one fused launch against `F.interpolate` then the native depthwise kernel", "",
               "| dtype | N | C | source | target | fused us | resize, depthwise us | unfused / fused | fused TB/s (source + result) |",
               "|---|---|---|---|---|---|---|---|---|"]
        for r in out["up_depthwise"]:
            md.append("| %s | %d | %d | %dx%d | %dx%d | %s | %s | %.2f | %.3f |" % (
                r["dtype"], r["N"], r["C"], r["source"][0], r["source"][1], r["target"][0], r["target"][1], us(r, "native_us"),
                us(r, "stock_us"), r["stock_over_native"], r["native_TBps"]))
        md.append("")
    if "end_to_end" in out:
        md += ["### End to end, images/s: the other switches on in both arms (float32: the six that apply, `use_native_upconv` alone as the new arm)", "",
               "| dtype | leg | without | with | with / without | median >= the other's min | gain outside the spread |",
               "|---|---|---|---|---|---|---|"]
        for name, d in out["end_to_end"]["dtypes"].items():
            for leg in LEGS:
                cell = lambda v: "%.1f (%.1f-%.1f)" % tuple(d[v][leg]["images_per_s"][k] for k in ("median", "min", "max"))  # noqa: E731
                md.append("| %s | %s | %s | %s | %.3f | %s | %s |" % (
                    name, leg, cell(VARIANTS[0]), cell(VARIANTS[1]), d["with_over_without"][leg],
                    "yes" if d["with_not_below_without_min"][leg] else "no", "yes" if d["gain_outside_the_spread"][leg] else "no"))
        md.append("")
    return "\n".join(md)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=50.0,
                    help="(a), (b): a round times as many back-to-back calls as fill this window (at least 30)")
    ap.add_argument("--stream-batches", type=int, default=6)
    ap.add_argument("--skip-shapes", action="store_true")
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--e2e-dtypes", default="bfloat16,float16,float32")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    ap.add_argument("--md", default=None, help="write the tables as markdown here")
    ap.add_argument("--profile", choices=VARIANTS, default=None, help="untimed one-image passes of one variant, for rocprofv3")
    ap.add_argument("--profile-dtype", choices=[n for n, _ in DTYPES], default="bfloat16")
    ap.add_argument("--profile-passes", type=int, default=3)
    args = ap.parse_args()
    if args.rounds < 3:
        ap.error("--rounds must be at least 3: the spread over the rounds is part of the result")
    if not torch.cuda.is_available():
        raise SystemExit("remainder_bench: no GPU -- this tool measures on the device and has no fallback")
    device = torch.device("cuda", 0)
    if args.profile:
        print(json.dumps(profile(device, args.profile, args.profile_dtype, args.profile_passes)))
        return
    out = {"rounds": args.rounds, "device": torch.cuda.get_device_name(device),
           "what": "native conv2x3 against F.conv2d and the fused resize + depthwise against F.interpolate + the native depthwise, "
                   "alternated per round in one process; median (min, max) over the rounds; (a), (b) microseconds per call "
                   "between device events, (c) images/s, host clock around work that ends in a device synchronise"}
    if not args.skip_shapes:
        out["conv2x3"] = measure_conv2x3(device, args.rounds, args.window_ms)
        out["up_depthwise"] = measure_updw(device, args.rounds, args.window_ms)
    if not args.skip_e2e:
        names = args.e2e_dtypes.split(",")
        out["end_to_end"] = measure_e2e(device, args.rounds, args.stream_batches, [d for d in DTYPES if d[0] in names])
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    if args.md:
        with open(args.md, "w") as f:
            f.write(markdown(out) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
