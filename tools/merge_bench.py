"""tools/merge_bench.py -- the native gated merge against the stock chain it replaces (measurement tool).

(a) per call    the three merges of a 704 x 1280 image -- f (256, 44, 80) with a (256, 22, 40); f (256, 88, 160) and
                f (256, 176, 320) with `a` of f's size; the gate at half f's size -- at N = 1 and N = 8, float32 and bfloat16,
                gated, plus the ungated first merge.  The stock side is the exact stock chain of `FOTSNet._merge` on the
                same tensors: `up(a) + f * up(g).expand_as(f)` for the first merge, `a + f * up(g)` for the others,
                `up(a) + f` ungated; the native side is one `_gated_merge_run`.  Microseconds per call between device
                events (a round = as many back-to-back calls as fill `--window-ms`), native and stock ALTERNATED inside one
                process, median and min-max over `--rounds` rounds.  Bytes/s against (a's bytes + f's + y's), beside a plain
                `copy_` of a tensor of f's size (2 x f's bytes) timed in the same rounds.
(b) forms       `--forms`: every (V, K) through the measurement build's entry point (`make -C fots.pytorch_amd/csrc
                merge-forms`), same rows, the rule's choice marked.
(c) end to end  BASELINE configs[4] as tools/depthwise_bench.py runs it: infer_image, infer_batch (eight per pass),
                infer_stream in images/s, float32 and bfloat16, `dw+in+heads+blocks` against `dw+in+heads+blocks+merge`,
                alternated per round.

Every comparison is against the stock path on the same tree in the same process.  Needs a GPU: there is no fallback.
    python tools/merge_bench.py [--rounds 7] [--out profiles/native_merge.json] [--md profiles/native_merge.md]
                                [--forms] [--skip-shapes | --skip-e2e]
`--profile VARIANT` `--profile-dtype D`: no figures -- the one-image leg alone, `--profile-passes` passes over the 11 images,
for `rocprofv3 --kernel-trace --stats -- python tools/merge_bench.py --profile dw+in+heads+blocks+merge` (a run of its own,
never with --pmc, after an unprofiled run of the same command); launches and kernel time per image are its stats divided by
passes x 11.
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

C = 256
# (name, f's (H, W), a's (H, W), the gate's (H, W), gated)
MERGES = (("merge1", (44, 80), (22, 40), (22, 40), True), ("merge2", (88, 160), (88, 160), (44, 80), True),
          ("merge3", (176, 320), (176, 320), (88, 160), True), ("merge1-ungated", (44, 80), (22, 40), None, False))
VARIANTS = ("dw+in+heads+blocks", "dw+in+heads+blocks+merge")
LEGS = ("infer_image", "infer_batch", "infer_stream")
FORMS_LIB = os.path.join(ROOT, "tools", "_explore", "librroi_merge_forms.so")


def _up(t, like):
    return F.interpolate(t, size=like.shape[2:], mode="bilinear", align_corners=True)


def _tensors(N, merge, device, dtype):
    _, fs, as_, gs, gated = merge
    a = torch.randn(N, C, *as_, device=device).to(dtype)
    f = torch.randn(N, C, *fs, device=device).to(dtype)
    g = torch.rand(N, 1, *gs, device=device).to(dtype) if gated else None
    return a, f, g


def _stock_fn(name, a, f, g):
    if g is None:
        return lambda: _up(a, f) + f
    if a.shape[2:] != f.shape[2:]:
        return lambda: _up(a, f) + f * _up(g, f).expand_as(f)
    return lambda: a + f * _up(g, f)


def measure_shapes(device, rounds, window_ms):
    from rroi_align._ext import rroi_align as ext
    rows = []
    torch.manual_seed(0)
    with torch.no_grad():
        for name, dtype in DTYPES[:2]:
            for N in (1, 8):
                for merge in MERGES:
                    a, f, g = _tensors(N, merge, device, dtype)
                    dst = torch.empty_like(f)
                    fns = {"native": lambda a=a, f=f, g=g: ext._gated_merge_run(a, f, g), "stock": _stock_fn(merge[0], a, f, g),
                           "copy": lambda dst=dst, f=f: dst.copy_(f)}
                    for fn in fns.values():
                        for _ in range(3):
                            fn()
                    torch.cuda.synchronize(device)
                    n = {k: _calls_for(fn, window_ms) for k, fn in fns.items()}
                    t = {k: [] for k in fns}
                    for _ in range(rounds):
                        for k, fn in fns.items():                           # alternated
                            t[k].append(_time_calls(fn, n[k]))
                    p = ext.merge_plan(N, C, *merge[1], merge[2], merge[3], dtype=dtype)
                    fbytes = f.numel() * f.element_size()
                    moved = a.numel() * a.element_size() + 2 * fbytes
                    row = {"dtype": name, "what": merge[0], "N": N, "f": list(merge[1]), "a": list(merge[2]),
                           "gate": None if merge[3] is None else list(merge[3]), "V": p.vector_elems, "K": p.channel_groups,
                           "grid": p.grid_x, "calls_per_round": n}
                    for k in fns:
                        row[k + "_us"] = _spread(t[k])
                    row["stock_over_native"] = round(row["stock_us"]["median"] / row["native_us"]["median"], 2)
                    row["native_below_stock"] = row["native_us"]["median"] < row["stock_us"]["median"]
                    row["native_TBps"] = round(moved / row["native_us"]["median"] * 1e-6, 3)
                    row["copy_TBps"] = round(2 * fbytes / row["copy_us"]["median"] * 1e-6, 3)
                    row["native_over_copy_rate"] = round(row["native_TBps"] / row["copy_TBps"], 2)
                    rows.append(row)
                    print("%-8s %-14s N=%d V=%d K=%-2d native %8.1f us (%.1f-%.1f)  stock %8.1f us (%.1f-%.1f)  x%.2f   %.2f TB/s, copy %.2f TB/s" % (
                        name, merge[0], N, row["V"], row["K"], row["native_us"]["median"], row["native_us"]["min"],
                        row["native_us"]["max"], row["stock_us"]["median"], row["stock_us"]["min"], row["stock_us"]["max"],
                        row["stock_over_native"], row["native_TBps"], row["copy_TBps"]), file=sys.stderr)
    return rows


def measure_forms(device, rounds, window_ms):
    """Every (V, K) of the measurement build on the rows of (a), gated merges only: median microseconds per call."""
    from rroi_align._ext import rroi_align as ext
    if not os.path.exists(FORMS_LIB):
        raise SystemExit("merge_bench --forms: build the measurement library first: make -C fots.pytorch_amd/csrc merge-forms")
    lib = ctypes.CDLL(FORMS_LIB)
    i, vp = ctypes.c_int, ctypes.c_void_p
    forced = lib.rroi_merge_forward_forced_hip
    forced.restype = i
    forced.argtypes = [i, vp, i, i, vp, i, i, vp, vp, i, i, i, i, i, i, ctypes.POINTER(i), ctypes.POINTER(i), vp]
    rows = []
    torch.manual_seed(0)
    with torch.no_grad():
        for name, dtype in DTYPES[:2]:
            for N in (1, 8):
                for merge in MERGES[:3]:
                    a, f, g = _tensors(N, merge, device, dtype)
                    y = torch.empty_like(f)
                    p = ext.merge_plan(N, C, *merge[1], merge[2], merge[3], dtype=dtype)
                    code, stream = ext.dtype_code(dtype), torch.cuda.current_stream().cuda_stream
                    table = {}
                    for V in ((2, 4) if dtype == torch.float32 else (2, 4, 8)):
                        for K in (1, 2, 4, 8, 16, 32, 64):
                            vu, ku = i(0), i(0)

                            def fn(V=V, K=K):
                                st = forced(code, a.data_ptr(), a.size(2), a.size(3), g.data_ptr(), g.size(2), g.size(3),
                                            f.data_ptr(), y.data_ptr(), N, C, f.size(2), f.size(3), V, K, ctypes.byref(vu),
                                            ctypes.byref(ku), stream)
                                assert st == 1, st
                            fn()
                            torch.cuda.synchronize(device)
                            assert (vu.value, ku.value) == (V, K)
                            n = _calls_for(fn, window_ms)
                            table["V%d K%d" % (V, K)] = _spread([_time_calls(fn, n) for _ in range(rounds)])["median"]
                    best = min(table, key=table.get)
                    rule = "V%d K%d" % (p.vector_elems, p.channel_groups)
                    rows.append({"dtype": name, "what": merge[0], "N": N, "rule": rule, "rule_us": table[rule], "best": best,
                                 "best_us": table[best], "us": table})
                    print("%-8s %-7s N=%d rule %-7s %8.1f us   best %-7s %8.1f us" % (name, merge[0], N, rule, table[rule], best,
                                                                                   table[best]), file=sys.stderr)
    return rows


def _switch(net, variant):
    from fots_e2e.native import (use_native_blocks, use_native_depthwise, use_native_heads, use_native_instancenorm,
                                 use_native_merge)
    assert use_native_depthwise(net) == 22 and use_native_instancenorm(net) == (52, 20) and use_native_heads(net)
    assert use_native_blocks(net) == (2, 7, 10)
    if variant.endswith("merge"):
        assert use_native_merge(net)
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
        # the bar (DESIGN 5.10's): the native median is not below the other leg's minimum of the same run
        d["merge_over_without"] = {leg: round(d[native][leg]["images_per_s"]["median"] / d[stock][leg]["images_per_s"]["median"], 3) for leg in LEGS}
        d["merge_not_below_without_min"] = {leg: d[native][leg]["images_per_s"]["median"] >= d[stock][leg]["images_per_s"]["min"] for leg in LEGS}
        out["dtypes"][name] = d
        for v in VARIANTS:
            print("%-9s %-25s" % (name, v) + "  ".join("%s %.1f (%.1f-%.1f)" % (
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
    """The tables of profiles/native_merge.md, from the JSON."""
    md = ["<!-- tables written by tools/merge_bench.py --md; median (min-max) over %d rounds on %s -->" % (out["rounds"], out["device"]), ""]
    if "shapes" in out:
        md += ["### Per call: native against the stock chain, and bytes per second against a plain copy", "",
               "| dtype | merge | N | V | K | native us | stock us | stock / native | native TB/s | `copy_` TB/s | native / copy |",
               "|---|---|---|---|---|---|---|---|---|---|---|"]
        for r in out["shapes"]:
            us = lambda k: "%.1f (%.1f-%.1f)" % (r[k]["median"], r[k]["min"], r[k]["max"])  # noqa: E731
            md.append("| %s | %s | %d | %d | %d | %s | %s | %.2f | %.2f | %.2f | %.2f |" % (
                r["dtype"], r["what"], r["N"], r["V"], r["K"], us("native_us"), us("stock_us"), r["stock_over_native"],
                r["native_TBps"], r["copy_TBps"], r["native_over_copy_rate"]))
        md.append("")
    if "forms" in out:
        ks = (1, 2, 4, 8, 16, 32, 64)
        md += ["### Forms: median us per call of every (V, K), the rule's choice in bold", "",
               "| dtype | merge | N | V | " + " | ".join("K=%d" % k for k in ks) + " |", "|---|---|---|---|" + "---|" * len(ks)]
        for r in out["forms"]:
            for V in (2, 4, 8):
                if "V%d K1" % V not in r["us"]:
                    continue
                cells = []
                for k in ks:
                    key = "V%d K%d" % (V, k)
                    cells.append(("**%.1f**" if key == r["rule"] else "%.1f") % r["us"][key])
                md.append("| %s | %s | %d | %d | %s |" % (r["dtype"], r["what"], r["N"], V, " | ".join(cells)))
        md.append("")
    if "end_to_end" in out:
        md += ["### End to end, images/s: the other four switches on in both legs", "",
               "| dtype | leg | without merge | with merge | with / without | median >= the other's min |", "|---|---|---|---|---|---|"]
        for name, d in out["end_to_end"]["dtypes"].items():
            for leg in LEGS:
                cell = lambda v: "%.1f (%.1f-%.1f)" % tuple(d[v][leg]["images_per_s"][k] for k in ("median", "min", "max"))  # noqa: E731
                md.append("| %s | %s | %s | %s | %.3f | %s |" % (name, leg, cell(VARIANTS[0]), cell(VARIANTS[1]),
                                                                d["merge_over_without"][leg],
                                                                "yes" if d["merge_not_below_without_min"][leg] else "no"))
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
    ap.add_argument("--forms", action="store_true", help="(b): every (V, K) through the measurement build")
    ap.add_argument("--forms-rounds", type=int, default=3)
    ap.add_argument("--forms-window-ms", type=float, default=20.0)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    ap.add_argument("--md", default=None, help="write the tables as markdown here")
    ap.add_argument("--profile", choices=VARIANTS, default=None, help="untimed one-image passes of one variant, for rocprofv3")
    ap.add_argument("--profile-dtype", choices=[n for n, _ in DTYPES], default="float32")
    ap.add_argument("--profile-passes", type=int, default=3)
    args = ap.parse_args()
    if args.rounds < 3:
        ap.error("--rounds must be at least 3: the spread over the rounds is part of the result")
    if not torch.cuda.is_available():
        raise SystemExit("merge_bench: no GPU -- this tool measures on the device and has no fallback")
    device = torch.device("cuda", 0)
    if args.profile:
        print(json.dumps(profile(device, args.profile, args.profile_dtype, args.profile_passes)))
        return
    out = {"rounds": args.rounds, "device": torch.cuda.get_device_name(device),
           "what": "native gated merge against the stock chain, alternated per round in one process; median (min, max) over the "
                   "rounds; (a) microseconds per call between device events, (c) images/s, host clock around work that ends in "
                   "a device synchronise"}
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
