"""tools/conv1x1_bench.py -- the native 1x1 convolution (with the shortcut's BatchNorm folded in) against the stock one
(measurement tool).

(a) per call    every distinct bias-free 1x1 shape of a 704 x 1280 image at N = 1 and N = 8, bfloat16 and float16, and the
                three shortcuts once more with their norm.  Stock is `F.conv2d` on the same tensors -- for a shortcut with
                its norm `F.conv2d` followed by the eval-mode `nn.BatchNorm2d` -- after three unmeasured passes, so a
                solver search is outside the timing; native is one `_conv1x1_run`.  Microseconds per call between device
                events (a round = as many back-to-back calls as fill `--window-ms`), native and stock ALTERNATED inside one
                process, median and min-max over `--rounds` rounds.  TFLOP/s (2 * Cin * Cout * N * Ho * Wo) and bytes/s
                (x + w + y), beside `dst.copy_(src)` of the output's size timed in the same rounds.
(b) forms       `--forms`: 32 and 64 output channels per workgroup through the measurement build's entry point (`make -C
                fots.pytorch_amd/csrc conv1x1-forms`), same rows, the rule's choice marked.
(c) end to end  BASELINE configs[4] as tools/depthwise_bench.py runs it: infer_image, infer_batch (eight per pass),
                infer_stream in images/s, bfloat16 and float16, the other seven switches on in both arms, without and with
                `use_native_conv1x1`, alternated per round.

Every comparison is against the stock path on the same tree in the same process.  Needs a GPU: there is no fallback.
    python tools/conv1x1_bench.py [--rounds 7] [--out profiles/native_conv1x1.json] [--md FILE] [--forms]
                                  [--skip-shapes | --skip-e2e]
`--profile VARIANT` `--profile-dtype D`: no figures -- the one-image leg alone, `--profile-passes` passes over the images,
for `rocprofv3 --kernel-trace --stats -- python tools/conv1x1_bench.py --profile ...` (a run of its own per variant, nothing
else traced); launches and kernel time per image are its stats divided by passes x images.
"""
import argparse
import ctypes
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
# (name, Cin, Cout, H, W, stride, with the norm)
SHAPES = (("layer3 128>256", 128, 256, 44, 80, 1, False), ("layer3 / feature3", 256, 256, 44, 80, 1, False),
          ("layer4 256>512", 256, 512, 22, 40, 1, False), ("layer4 512>512", 512, 512, 22, 40, 1, False),
          ("feature1", 64, 256, 176, 320, 1, False), ("feature2", 128, 256, 88, 160, 1, False),
          ("feature4", 512, 256, 22, 40, 1, False), ("upconv1", 256, 256, 88, 160, 1, False),
          ("upconv2", 256, 256, 176, 320, 1, False),
          ("shortcut2", 64, 128, 176, 320, 2, False), ("shortcut3", 128, 256, 88, 160, 2, False),
          ("shortcut4", 256, 512, 44, 80, 2, False),
          ("shortcut2+BN", 64, 128, 176, 320, 2, True), ("shortcut3+BN", 128, 256, 88, 160, 2, True),
          ("shortcut4+BN", 256, 512, 44, 80, 2, True))
ROWS = tuple((s, n) for n in (1, 8) for s in SHAPES)
VARIANTS = ("seven switches", "seven switches+conv1x1")
LEGS = ("infer_image", "infer_batch", "infer_stream")
FORMS_LIB = os.path.join(ROOT, "tools", "_explore", "librroi_conv1x1_forms.so")


def _tensors(shape, N, device, dtype):
    _, ci, co, H, W, _, with_norm = shape
    x = torch.randn(N, ci, H, W, device=device).to(dtype)
    w = (torch.randn(co, ci, 1, 1, device=device) / ci ** 0.5).to(dtype)
    bn = None
    if with_norm:
        bn = torch.nn.BatchNorm2d(co).to(device)
        with torch.no_grad():
            bn.weight.normal_(1.0, 0.2), bn.bias.normal_(0.0, 0.2), bn.running_mean.normal_(0.0, 0.2), bn.running_var.uniform_(0.5, 1.5)
        bn = bn.to(dtype).eval()
    return x, w, bn


def _norm_of(bn):
    return None if bn is None else (bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var, bn.eps)


def measure_shapes(device, rounds, window_ms, rows=ROWS):
    from rroi_align._ext import rroi_align as ext
    out = []
    torch.manual_seed(0)
    with torch.no_grad():
        for name, dtype in HALF:
            for shape, N in rows:
                what, ci, co, H, W, s, with_norm = shape
                x, w, bn = _tensors(shape, N, device, dtype)
                norm = _norm_of(bn)
                stock = (lambda x=x, w=w, s=s, bn=bn: bn(F.conv2d(x, w, stride=s))) if with_norm else \
                    (lambda x=x, w=w, s=s: F.conv2d(x, w, stride=s))
                y = stock()
                dst = torch.empty_like(y)
                fns = {"native": lambda x=x, w=w, s=s, norm=norm: ext._conv1x1_run(x, w, s, 1.0, norm), "stock": stock,
                       "copy": lambda dst=dst, y=y: dst.copy_(y)}
                for fn in fns.values():
                    for _ in range(3):
                        fn()
                torch.cuda.synchronize(device)
                n = {k: _calls_for(fn, window_ms) for k, fn in fns.items()}
                t = {k: [] for k in fns}
                for _ in range(rounds):
                    for k, fn in fns.items():                           # alternated
                        t[k].append(_time_calls(fn, n[k]))
                p = ext.conv1x1_plan(N, ci, co, H, W, s, dtype=dtype)
                flop = 2.0 * ci * y.numel()
                moved = 2 * (x.numel() + w.numel() + y.numel())
                row = {"dtype": name, "what": what, "N": N, "cin": ci, "cout": co, "H": H, "W": W, "stride": s, "norm": with_norm,
                       "tile": [p.tile_m, p.tile_p], "grid": p.grid_x, "calls_per_round": n}
                for k in fns:
                    row[k + "_us"] = _spread(t[k])
                nat, stk = row["native_us"]["median"], row["stock_us"]["median"]
                row["stock_over_native"] = round(stk / nat, 2)
                row["native_below_stock"] = nat < stk
                row["native_TFLOPs"] = round(flop / nat * 1e-6, 1)
                row["native_TBps"] = round(moved / nat * 1e-6, 3)
                row["copy_TBps"] = round(4 * y.numel() / row["copy_us"]["median"] * 1e-6, 3)
                out.append(row)
                print("%-8s %-18s N=%-3d tile %dx%d native %8.1f us (%.1f-%.1f)  stock %8.1f us (%.1f-%.1f)  x%.2f  %.1f TF" % (
                    name, what, N, p.tile_m, p.tile_p, nat, row["native_us"]["min"], row["native_us"]["max"], stk,
                    row["stock_us"]["min"], row["stock_us"]["max"], row["stock_over_native"], row["native_TFLOPs"]),
                    file=sys.stderr)
    return out


def measure_forms(device, rounds, window_ms):
    """32 and 64 output channels per workgroup through the measurement build on the rows of (a) without a norm: median
    microseconds per call."""
    from rroi_align._ext import rroi_align as ext
    if not os.path.exists(FORMS_LIB):
        raise SystemExit("conv1x1_bench --forms: build the measurement library first: make -C fots.pytorch_amd/csrc conv1x1-forms")
    lib = ctypes.CDLL(FORMS_LIB)
    i, vp = ctypes.c_int, ctypes.c_void_p
    forced = lib.rroi_conv1x1_forward_forced_hip
    forced.restype = i
    forced.argtypes = [i, vp, vp, vp] + [i] * 6 + [ctypes.c_float] + [vp] * 4 + [ctypes.c_double, i, ctypes.POINTER(i), vp]
    out = []
    torch.manual_seed(0)
    with torch.no_grad():
        for name, dtype in HALF:
            for shape, N in ((s, n) for n in (1, 8) for s in SHAPES if not s[6]):
                what, ci, co, H, W, s, _ = shape
                x, w, _ = _tensors(shape, N, device, dtype)
                y = torch.empty((N, co, (H - 1) // s + 1, (W - 1) // s + 1), device=device, dtype=dtype)
                p = ext.conv1x1_plan(N, ci, co, H, W, s, dtype=dtype)
                code, stream = ext.dtype_code(dtype), torch.cuda.current_stream().cuda_stream
                table = {}
                for MT in (1, 2):
                    used = i(0)

                    def fn(MT=MT, used=used):
                        st = forced(code, x.data_ptr(), w.data_ptr(), y.data_ptr(), N, ci, co, H, W, s, 1.0, None, None, None,
                                    None, 0.0, MT, ctypes.byref(used), stream)
                        assert st == 1, st
                    fn()
                    torch.cuda.synchronize(device)
                    assert used.value == MT
                    n = _calls_for(fn, window_ms)
                    table[str(32 * MT)] = _spread([_time_calls(fn, n) for _ in range(rounds)])["median"]
                best = min(table, key=table.get)
                rule = str(p.tile_m)
                out.append({"dtype": name, "what": what, "N": N, "rule": rule, "rule_us": table[rule], "best": best,
                            "best_us": table[best], "us": table})
                print("%-8s %-18s N=%-3d rule %-3s %8.1f us   best %-3s %8.1f us" % (name, what, N, rule, table[rule], best,
                                                                                  table[best]), file=sys.stderr)
    return out


def _switch(net, variant):
    from fots_e2e.native import (use_native_blocks, use_native_conv1x1, use_native_conv3x3, use_native_depthwise,
                                 use_native_heads, use_native_instancenorm, use_native_merge, use_native_recogniser)
    assert use_native_depthwise(net) == 22 and use_native_instancenorm(net) == (52, 20) and use_native_heads(net)
    assert use_native_blocks(net) == (2, 7, 10) and use_native_merge(net) and use_native_conv3x3(net) == (23, 2)
    assert use_native_recogniser(net)
    if variant.endswith("conv1x1"):
        assert use_native_conv1x1(net) == (29, 3)
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
    S = _e2e_setup(device, HALF, stream_batches, VARIANTS)
    leg_image, leg_batch, leg_stream = _leg_fns(S, device)
    keys = [(name, v) for name, _ in HALF for v in VARIANTS]
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
    without, with_conv = VARIANTS
    for name, _ in HALF:
        d = {v: {leg: {"images_per_s": _spread(raw[(name, v)][leg]), "per_round": [round(x, 2) for x in raw[(name, v)][leg]]}
                 for leg in LEGS} for v in VARIANTS}
        # the bar (DESIGN 5.10's): the native median is not below the other arm's minimum of the same run
        d["conv1x1_over_without"] = {leg: round(d[with_conv][leg]["images_per_s"]["median"] / d[without][leg]["images_per_s"]["median"], 3)
                                     for leg in LEGS}
        d["conv1x1_not_below_without_min"] = {leg: d[with_conv][leg]["images_per_s"]["median"] >= d[without][leg]["images_per_s"]["min"]
                                              for leg in LEGS}
        d["gain_outside_the_spread"] = {leg: d[with_conv][leg]["images_per_s"]["min"] > d[without][leg]["images_per_s"]["max"]
                                        for leg in LEGS}
        out["dtypes"][name] = d
        for v in VARIANTS:
            print("%-9s %-24s" % (name, v) + "  ".join("%s %.1f (%.1f-%.1f)" % (
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
    """The tables of profiles/native_conv1x1.md, from the JSON."""
    md = ["<!-- tables written by tools/conv1x1_bench.py --md; median (min-max) over %d rounds on %s -->" % (out["rounds"], out["device"]), ""]
    if "shapes" in out:
        md += ["### Per call: native against `F.conv2d` (`+BN`: against `F.conv2d` and the eval `BatchNorm2d`)", "",
               "| dtype | conv | N | Cin>Cout | map | s | tile | grid | native us | stock us | stock / native | native TFLOP/s | native TB/s | `copy_` TB/s |",
               "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
        for r in out["shapes"]:
            us = lambda k: "%.1f (%.1f-%.1f)" % (r[k]["median"], r[k]["min"], r[k]["max"])  # noqa: E731
            md.append("| %s | %s | %d | %d>%d | %dx%d | %d | %dx%d | %d | %s | %s | %.2f | %.1f | %.2f | %.2f |" % (
                r["dtype"], r["what"], r["N"], r["cin"], r["cout"], r["H"], r["W"], r["stride"], r["tile"][0], r["tile"][1],
                r["grid"], us("native_us"), us("stock_us"), r["stock_over_native"], r["native_TFLOPs"], r["native_TBps"],
                r["copy_TBps"]))
        md.append("")
    if "forms" in out:
        md += ["### Forms: median us per call with 32 and 64 output channels per workgroup, the rule's choice in bold", "",
               "| dtype | conv | N | 32 | 64 |", "|---|---|---|---|---|"]
        for r in out["forms"]:
            cells = [("**%.1f**" if k == r["rule"] else "%.1f") % r["us"][k] for k in ("32", "64")]
            md.append("| %s | %s | %d | %s |" % (r["dtype"], r["what"], r["N"], " | ".join(cells)))
        md.append("")
    if "end_to_end" in out:
        md += ["### End to end, images/s: the other seven switches on in both arms", "",
               "| dtype | leg | without conv1x1 | with conv1x1 | with / without | median >= the other's min | gain outside the spread |",
               "|---|---|---|---|---|---|---|"]
        for name, d in out["end_to_end"]["dtypes"].items():
            for leg in LEGS:
                cell = lambda v: "%.1f (%.1f-%.1f)" % tuple(d[v][leg]["images_per_s"][k] for k in ("median", "min", "max"))  # noqa: E731
                md.append("| %s | %s | %s | %s | %.3f | %s | %s |" % (
                    name, leg, cell(VARIANTS[0]), cell(VARIANTS[1]), d["conv1x1_over_without"][leg],
                    "yes" if d["conv1x1_not_below_without_min"][leg] else "no",
                    "yes" if d["gain_outside_the_spread"][leg] else "no"))
        md.append("")
    return "\n".join(md)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=50.0,
                    help="(a): a round times as many back-to-back calls as fill this window (at least 30)")
    ap.add_argument("--stream-batches", type=int, default=6)
    ap.add_argument("--skip-shapes", action="store_true")
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--forms", action="store_true", help="(b): both channel tiles through the measurement build")
    ap.add_argument("--forms-rounds", type=int, default=3)
    ap.add_argument("--forms-window-ms", type=float, default=20.0)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    ap.add_argument("--md", default=None, help="write the tables as markdown here")
    ap.add_argument("--profile", choices=VARIANTS, default=None, help="untimed one-image passes of one variant, for rocprofv3")
    ap.add_argument("--profile-dtype", choices=[n for n, _ in HALF], default="bfloat16")
    ap.add_argument("--profile-passes", type=int, default=3)
    args = ap.parse_args()
    if args.rounds < 3:
        ap.error("--rounds must be at least 3: the spread over the rounds is part of the result")
    if not torch.cuda.is_available():
        raise SystemExit("conv1x1_bench: no GPU -- this tool measures on the device and has no fallback")
    device = torch.device("cuda", 0)
    if args.profile:
        print(json.dumps(profile(device, args.profile, args.profile_dtype, args.profile_passes)))
        return
    out = {"rounds": args.rounds, "device": torch.cuda.get_device_name(device),
           "what": "native 1x1 convolution against F.conv2d (+ eval BatchNorm2d), alternated per round in one process; median "
                   "(min, max) over the rounds; (a) microseconds per call between device events, (c) images/s, host clock "
                   "around work that ends in a device synchronise"}
    if not args.skip_shapes:
        out["shapes"] = measure_shapes(device, args.rounds, args.window_ms)
        out["every_row_native_below_stock"] = all(r["native_below_stock"] for r in out["shapes"])
    if args.forms:
        out["forms"] = measure_forms(device, args.forms_rounds, args.forms_window_ms)
    if not args.skip_e2e:
        out["end_to_end"] = measure_e2e(device, args.rounds, args.stream_batches)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    if args.md:
        with open(args.md, "w") as f:
            f.write(markdown(out) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
