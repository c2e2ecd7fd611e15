"""tools/preprocess_bench.py -- native preprocessing against the stock front (measurement tool).

Stock and native ALTERNATE in one process over `--rounds` rounds (at least 7 by default); every figure is a median with
the minimum and maximum over the rounds next to it.

  per call     one image and eight images of 720 x 1280 > 704 x 1280, float32 / bfloat16 / float16:
                 device   microseconds between two device events, the bytes already on the device (the upload excluded):
                          stock = widen, permuted view, F.interpolate, / 128, - 1, the cast, torch.cat; native = one call
                 wall     host clock around the call as the pipeline makes it, upload included, ended by a synchronise:
                          stock = torch.cat([preprocess(im) ...]); native = preprocess_batch(ims); packed = images and
                          table packed into one host buffer for one upload (the form proposed first, not shipped)
                 launches NOT counted here: `--profile` runs `--passes` untimed passes of both arms' wall form (eight
                          images, bfloat16) for `rocprofv3 --kernel-trace --memory-copy-trace --stats -- python
                          tools/preprocess_bench.py --profile` (a run of its own); the native arm is the calls of
                          rroi_preprocess_kernel, the stock arm every other kernel, each divided by the passes
                 copy     a plain device copy of the call's bytes (read + written) in the same run: what those bytes cost
  pipeline     infer_image (one image per pass), infer_batch (eight per pass), infer_stream (two batches in flight) with
               every other native switch that applies on in BOTH arms, bfloat16 and float32; the arms differ by
               `native_preprocess` alone and share one network object.

Needs a GPU: there is no fallback.   python tools/preprocess_bench.py [--rounds 7] [--out X.json] [--md X.md]
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

from depthwise_bench import DTYPES, IMAGES_PER_BATCH, _calls_for, _spread, _time_calls  # noqa: E402
from remainder_bench import VARIANTS, _e2e_setup  # noqa: E402

ARMS = ("stock", "native")
LEGS = ("infer_image", "infer_batch", "infer_stream")
SOURCE, TARGET = (720, 1280), (704, 1280)


def _wall(fn, iters, device):
    """microseconds per call by the host clock, every call ended by a synchronise (as the pipeline's user sees it)"""
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
        torch.cuda.synchronize(device)
    return (time.perf_counter() - t0) * 1e6 / iters


def _stock_device(tensors, dtype):
    out = []
    for t in tensors:                                         # (H0, W0, 3) uint8, on the device already
        t = t.to(torch.float32).permute(2, 0, 1).unsqueeze(0)
        t = F.interpolate(t, size=TARGET, mode="bilinear", align_corners=False)
        t = t / 128 - 1
        out.append(t if dtype == torch.float32 else t.to(dtype))
    return out[0] if len(out) == 1 else torch.cat(out, 0)


def _packed_batch(ims, device, dtype):
    """The form that was proposed first and is measured here against what ships: images and table packed into ONE host
    buffer, the table in front, one upload, one launch."""
    from rroi_align._ext.rroi_align import preprocess as pp
    n = len(ims)
    head = 16 * n
    buf = np.empty(head + sum(im.size for im in ims), np.uint8)
    table = buf[:head].view(np.int32).reshape(n, 4)
    at = 0
    for k, im in enumerate(ims):
        table[k] = (at, im.shape[0], im.shape[1], 0)
        buf[head + at:head + at + im.size] = im.reshape(-1)
        at += im.size
    dev = torch.from_numpy(buf).to(device)
    return pp.run_preprocess_images(dev[head:], dev[:head].view(torch.int32).view(n, 4), TARGET, dtype)


def measure_calls(device, rounds, window_ms):
    from fots_e2e.pipeline import preprocess, preprocess_batch
    from rroi_align._ext.rroi_align import preprocess as pp
    rng = np.random.default_rng(0)
    ims_all = [rng.integers(0, 256, SOURCE + (3,), dtype=np.uint8) for _ in range(IMAGES_PER_BATCH)]
    rows = []
    with torch.no_grad():
        for N in (1, IMAGES_PER_BATCH):
            ims = ims_all[:N]
            on_dev = [torch.from_numpy(im).to(device) for im in ims]
            table = torch.tensor([[k * ims[0].size, SOURCE[0], SOURCE[1], 0] for k in range(N)], dtype=torch.int32).to(device)
            src = torch.cat([t.reshape(-1) for t in on_dev])
            for name, dtype in DTYPES:
                dev_fns = {"stock": lambda d=dtype, t=on_dev: _stock_device(t, d),
                           "native": lambda d=dtype, s=src, tb=table: pp.run_preprocess_images(s, tb, TARGET, d)}
                wall_fns = {"stock": (lambda d=dtype, x=ims: preprocess(x[0], device, d)) if N == 1 else
                            (lambda d=dtype, x=ims: torch.cat([preprocess(im, device, d) for im in x], 0)),
                            "native": lambda d=dtype, x=ims: preprocess_batch(x, device, d),
                            "packed": lambda d=dtype, x=ims: _packed_batch(x, device, d)}
                same = torch.equal(dev_fns["native"](), wall_fns["native"]()) and torch.equal(dev_fns["native"](), wall_fns["packed"]())
                for fns in (dev_fns, wall_fns):
                    for fn in fns.values():
                        for _ in range(3):
                            fn()
                torch.cuda.synchronize(device)
                n_dev = {k: _calls_for(fn, window_ms) for k, fn in dev_fns.items()}
                n_wall = {k: max(10, min(200, n_dev[k if k in n_dev else "native"] // 4)) for k in wall_fns}
                y = dev_fns["native"]()
                in_bytes, out_bytes = N * ims[0].size, y.numel() * y.element_size()
                half = torch.empty((in_bytes + out_bytes) // 2, dtype=torch.uint8, device=device)
                half2 = torch.empty_like(half)
                copy = lambda a=half, b=half2: b.copy_(a)                                   # noqa: E731
                n_copy = _calls_for(copy, window_ms)
                t = {"device": {k: [] for k in ARMS}, "wall": {k: [] for k in wall_fns}, "copy": []}
                for _ in range(rounds):
                    for k in ARMS:                              # alternated
                        t["device"][k].append(_time_calls(dev_fns[k], n_dev[k]))
                    t["copy"].append(_time_calls(copy, n_copy))
                    for k in wall_fns:
                        t["wall"][k].append(_wall(wall_fns[k], n_wall[k], device))
                p = pp.preprocess_plan(N, TARGET[0], TARGET[1], dtype)
                row = {"dtype": name, "N": N, "source": list(SOURCE), "target": list(TARGET),
                       "plan": {"grid": p.grid_x, "rows_per_thread": p.rows_per_thread, "columns_per_thread": p.columns_per_thread,
                                "wide_store": p.wide_store},
                       "calls_per_round": {"device": n_dev, "wall": n_wall},
                       "bytes": {"read": in_bytes, "written": out_bytes},
                       "device_us": {k: _spread(t["device"][k]) for k in ARMS},
                       "wall_us": {k: _spread(t["wall"][k]) for k in wall_fns},
                       "copy_of_the_same_bytes_us": _spread(t["copy"]),
                       "native_bits_equal_between_forms": bool(same)}
                for what in ("device_us", "wall_us"):
                    row[what]["stock_over_native"] = round(row[what]["stock"]["median"] / row[what]["native"]["median"], 2)
                    row[what]["native_below_stock"] = row[what]["native"]["median"] < row[what]["stock"]["median"]
                    row[what]["gain_outside_the_spread"] = row[what]["native"]["max"] < row[what]["stock"]["min"]
                row["native_over_copy"] = round(row["device_us"]["native"]["median"] / row["copy_of_the_same_bytes_us"]["median"], 2)
                row["native_TBps"] = round((in_bytes + out_bytes) / row["device_us"]["native"]["median"] * 1e-6, 3)
                row["copy_TBps"] = round((in_bytes + out_bytes) / row["copy_of_the_same_bytes_us"]["median"] * 1e-6, 3)
                rows.append(row)
                print("%-8s N=%d device native %8.1f us (%.1f-%.1f) stock %8.1f us (%.1f-%.1f) x%.1f | wall native %8.1f stock %8.1f x%.1f | copy %.1f us" % (
                    name, N, row["device_us"]["native"]["median"], row["device_us"]["native"]["min"], row["device_us"]["native"]["max"],
                    row["device_us"]["stock"]["median"], row["device_us"]["stock"]["min"], row["device_us"]["stock"]["max"],
                    row["device_us"]["stock_over_native"], row["wall_us"]["native"]["median"], row["wall_us"]["stock"]["median"],
                    row["wall_us"]["stock_over_native"], row["copy_of_the_same_bytes_us"]["median"]), file=sys.stderr)
    return rows


def measure_pipeline(device, rounds, stream_batches):
    from fots_e2e.pipeline import infer_batch, infer_image, infer_stream
    dtypes = (DTYPES[1], DTYPES[0])                          # bfloat16, float32
    S = _e2e_setup(device, dtypes, stream_batches, VARIANTS[1:])      # every other switch that applies, once per dtype
    conv, ims, groups, seq_groups = S["conv"], S["ims"], S["groups"], S["seq_groups"]

    def leg_image(L, native):
        per = []
        for i, im in enumerate(ims):
            t0 = time.perf_counter()
            infer_image(L["net"], conv, im, detector=lambda _x, m=L["maps"][i]: m, native_preprocess=native)
            torch.cuda.synchronize(device)
            per.append(time.perf_counter() - t0)
        return per

    def leg_batch(L, native):
        per = []
        for g, st in zip(groups, L["stacked"]):
            t0 = time.perf_counter()
            infer_batch(L["net"], conv, [ims[i] for i in g], detector=lambda _x, st=st: st, native_preprocess=native)
            torch.cuda.synchronize(device)
            per.append(time.perf_counter() - t0)
        return per

    def leg_stream(L, native):
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        for _r in infer_stream(L["net"], conv, ([ims[i] for i in groups[k]] for k in seq_groups),
                               detector=lambda k, _x: L["stacked"][seq_groups[k]], native_preprocess=native):
            pass
        torch.cuda.synchronize(device)
        return time.perf_counter() - t0

    keys = [(name, arm) for name, _ in dtypes for arm in ARMS]
    raw = {k: {leg: [] for leg in LEGS} for k in keys}
    with torch.no_grad():
        for name, arm in keys:                               # warm-up: every shape of every dtype, the side stream included
            L = S["legs"][(name, VARIANTS[1])]
            leg_image(L, arm == "native"), leg_batch(L, arm == "native"), leg_stream(L, arm == "native")
        for _round in range(rounds):
            for name, arm in keys:                           # alternated: the arms within every round and dtype
                L, nat = S["legs"][(name, VARIANTS[1])], arm == "native"
                raw[(name, arm)]["infer_image"].append(1.0 / float(np.median(leg_image(L, nat))))
                raw[(name, arm)]["infer_batch"].append(IMAGES_PER_BATCH / float(np.median(leg_batch(L, nat))))
                raw[(name, arm)]["infer_stream"].append(IMAGES_PER_BATCH * len(seq_groups) / leg_stream(L, nat))
    out = {"images": S["source"], "images_per_batch": IMAGES_PER_BATCH, "stream_batches": len(seq_groups),
           "host_threads": S["host_threads"], "dtypes": {}}
    for name, _ in dtypes:
        d = {arm: {leg: {"images_per_s": _spread(raw[(name, arm)][leg]), "per_round": [round(x, 2) for x in raw[(name, arm)][leg]]}
                   for leg in LEGS} for arm in ARMS}
        ips = lambda arm, leg, what: d[arm][leg]["images_per_s"][what]                      # noqa: E731
        d["native_over_stock"] = {leg: round(ips("native", leg, "median") / ips("stock", leg, "median"), 3) for leg in LEGS}
        d["native_not_below_stock_min"] = {leg: ips("native", leg, "median") >= ips("stock", leg, "min") for leg in LEGS}
        d["gain_outside_the_spread"] = {leg: ips("native", leg, "min") > ips("stock", leg, "max") for leg in LEGS}
        out["dtypes"][name] = d
        for arm in ARMS:
            print("%-9s %-7s" % (name, arm) + "  ".join("%s %.1f (%.1f-%.1f)" % (
                leg, ips(arm, leg, "median"), ips(arm, leg, "min"), ips(arm, leg, "max")) for leg in LEGS) + " img/s", file=sys.stderr)
    return out


def markdown(out):
    md = ["# Native preprocessing against the stock front", "",
          "`python tools/preprocess_bench.py --rounds %d` on %s; stock and native alternated in one process, median (min - max) "
          "over the rounds.  The JSON beside this file holds every round." % (out["rounds"], out["device"]), "",
          "## Per call, 720 x 1280 > 704 x 1280, microseconds", "",
          "| dtype | N | device: native | device: stock | x | wall: native | wall: stock | x | wall: packed | copy of the same bytes | native / copy |",
          "|---|---|---|---|---|---|---|---|---|---|---|"]
    f = lambda s: "%.1f (%.1f - %.1f)" % (s["median"], s["min"], s["max"])                  # noqa: E731
    for r in out["per_call"]:
        md.append("| %s | %d | %s | %s | %.1f | %s | %s | %.1f | %s | %s | %.2f |" % (
            r["dtype"], r["N"], f(r["device_us"]["native"]), f(r["device_us"]["stock"]), r["device_us"]["stock_over_native"],
            f(r["wall_us"]["native"]), f(r["wall_us"]["stock"]), r["wall_us"]["stock_over_native"],
            f(r["wall_us"]["packed"]), f(r["copy_of_the_same_bytes_us"]), r["native_over_copy"]))
    md += ["", "## Pipeline, images/s: every other switch that applies on in both arms", "",
           "| dtype | leg | stock | native | native / stock | not below the stock minimum | gain outside the spread |", "|---|---|---|---|---|---|---|"]
    for name, d in out["pipeline"]["dtypes"].items():
        for leg in LEGS:
            md.append("| %s | %s | %s | %s | %.3f | %s | %s |" % (
                name, leg, f(d["stock"][leg]["images_per_s"]), f(d["native"][leg]["images_per_s"]), d["native_over_stock"][leg],
                d["native_not_below_stock_min"][leg], d["gain_outside_the_spread"][leg]))
    return "\n".join(md) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=60.0)
    ap.add_argument("--stream-batches", type=int, default=6)
    ap.add_argument("--skip-pipeline", action="store_true")
    ap.add_argument("--profile", action="store_true", help="untimed passes of both arms, for rocprofv3")
    ap.add_argument("--passes", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    ap.add_argument("--md", default=None, help="write the tables here")
    args = ap.parse_args()
    if args.rounds < 3:
        ap.error("--rounds must be at least 3: the spread over the rounds is part of the result")
    if not torch.cuda.is_available():
        raise SystemExit("preprocess_bench: no GPU -- this tool measures on the device and has no fallback")
    device = torch.device("cuda", 0)
    out = {"rounds": args.rounds, "window_ms": args.window_ms, "device": torch.cuda.get_device_name(device)}

    def write():
        if args.out:
            with open(args.out, "w") as fh:
                fh.write(json.dumps(out, indent=1) + "\n")
        if args.md and "pipeline" in out:
            with open(args.md, "w") as fh:
                fh.write(markdown(out))

    if args.profile:
        from fots_e2e.pipeline import preprocess, preprocess_batch
        rng = np.random.default_rng(0)
        ims = [rng.integers(0, 256, SOURCE + (3,), dtype=np.uint8) for _ in range(IMAGES_PER_BATCH)]
        with torch.no_grad():
            for _ in range(args.passes):
                torch.cat([preprocess(im, device, torch.bfloat16) for im in ims], 0)
                preprocess_batch(ims, device, torch.bfloat16)
            torch.cuda.synchronize(device)
        print(json.dumps({"profiled": "stock and native, eight images, bfloat16", "passes": args.passes}))
        return
    out["per_call"] = measure_calls(device, args.rounds, args.window_ms)
    write()
    out["pipeline"] = {"dtypes": {}} if args.skip_pipeline else measure_pipeline(device, args.rounds, args.stream_batches)
    write()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
