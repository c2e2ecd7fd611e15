"""tools/depthwise_bench.py -- the native depthwise 3x3 convolution against the stock one (measurement tool).

(a) per shape   the six distinct depthwise shapes of FOTSNet at 1280 x 704, N = 1 and N = 8, float32 / bfloat16 / float16:
                microseconds per call between device events (a round = as many back-to-back calls as fill `--window-ms`),
                `rroi_align._ext.rroi_align.depthwise3x3` and `F.conv2d` ALTERNATED inside one process (`--rounds` rounds;
                within a round native, then stock, per shape), median and min-max over the rounds.  For the two largest
                shapes also the achieved bytes/s against (N * C * (H * W + Ho * Wo)) * sizeof(T) + 36 * C bytes.
(b) end to end  BASELINE configs[4] as tools/e2e_half_bench.py runs it (the images, boxes and detector maps of
                tests/e2e_inputs.py; maps uploaded and stacked outside the timers): infer_image, infer_batch (eight per
                pass), infer_stream in images/s, the stock network and `use_native_depthwise(net)` alternated per round,
                float32 and bfloat16.

Every comparison is against the stock path on the same tree in the same process.  Needs a GPU: there is no fallback.
    python tools/depthwise_bench.py [--rounds 5] [--out profiles/native_depthwise.json] [--skip-shapes | --skip-e2e]
`--profile VARIANT` (stock | native) `--profile-dtype D`: no figures -- the one-image leg alone, `--profile-passes` passes
over the 11 images, for `rocprofv3 --kernel-trace --stats -- python tools/depthwise_bench.py --profile native` (a run of its
own); the depthwise kernels' launches and summed time per image are its stats divided by passes x 11.  There is no
separate warm-up in that mode: the first pass's one-off kernels (MIOpen's first use of a shape) are in the stats' totals.
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
for _p in (ROOT, os.path.join(ROOT, "fots.pytorch_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

DTYPES = (("float32", torch.float32), ("bfloat16", torch.bfloat16), ("float16", torch.float16))
# (C, H, W, stride): _smooth of upconv2 / upconv1, layer3's first block, layer3, layer4's first block, layer4
SHAPES = ((256, 176, 320, 1), (256, 88, 160, 1), (128, 88, 160, 2), (256, 44, 80, 1), (256, 44, 80, 2), (512, 22, 40, 1))
IMAGES_PER_BATCH = 8


def _spread(values, scale=1.0, digits=2):
    a = np.asarray(values, np.float64) * scale
    return {"median": round(float(np.median(a)), digits), "min": round(float(a.min()), digits), "max": round(float(a.max()), digits)}


def model_bytes(N, C, H, W, stride, itemsize):
    ho, wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    return N * C * (H * W + ho * wo) * itemsize + 36 * C


def _time_calls(fn, iters):
    """microseconds per call: `iters` calls between two device events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def _calls_for(fn, window_ms, floor=30, cap=50000):
    """How many calls fill a window of `window_ms`: a 10 us call needs thousands, a 1 ms call a few hundred."""
    per = _time_calls(fn, floor)
    return int(min(cap, max(floor, window_ms * 1e3 / max(per, 1e-3))))


def measure_shapes(device, rounds, window_ms):
    from rroi_align._ext import rroi_align as ext
    rows = []
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for name, dtype in DTYPES:
            for N in (1, 8):
                for C, H, W, s in SHAPES:
                    x = torch.randn(N, C, H, W, generator=g).to(device).to(dtype)
                    w = torch.randn(C, 1, 3, 3, generator=g).to(device).to(dtype)
                    native = lambda: ext.depthwise3x3(x, w, s)                                  # noqa: E731
                    stock = lambda: F.conv2d(x, w, None, s, 1, 1, C)                            # noqa: E731
                    for fn in (native, stock):                                                  # warm-up: MIOpen picks here
                        for _ in range(3):
                            fn()
                    torch.cuda.synchronize(device)
                    n_native, n_stock = _calls_for(native, window_ms), _calls_for(stock, window_ms)
                    t = {"native": [], "stock": []}
                    for _ in range(rounds):
                        t["native"].append(_time_calls(native, n_native))
                        t["stock"].append(_time_calls(stock, n_stock))
                    row = {"dtype": name, "N": N, "C": C, "H": H, "W": W, "stride": s,
                           "calls_per_round": {"native": n_native, "stock": n_stock},
                           "native_us": _spread(t["native"]), "stock_us": _spread(t["stock"])}
                    row["stock_over_native"] = round(row["stock_us"]["median"] / row["native_us"]["median"], 2)
                    row["native_not_slower"] = row["native_us"]["median"] <= row["stock_us"]["median"]
                    if (C, H, W, s) in SHAPES[:2]:
                        nbytes = model_bytes(N, C, H, W, s, x.element_size())
                        row["model_bytes"] = nbytes
                        row["native_TBps"] = round(nbytes / row["native_us"]["median"] * 1e-6, 3)
                        row["stock_TBps"] = round(nbytes / row["stock_us"]["median"] * 1e-6, 3)
                    rows.append(row)
                    print("%-8s N=%d %3dx%3dx%3d s%d  native %8.1f us (%.1f-%.1f)  stock %8.1f us (%.1f-%.1f)  x%.2f" % (
                        name, N, C, H, W, s, row["native_us"]["median"], row["native_us"]["min"], row["native_us"]["max"],
                        row["stock_us"]["median"], row["stock_us"]["min"], row["stock_us"]["max"], row["stock_over_native"]),
                        file=sys.stderr)
    return rows


def _e2e_setup(device, dtypes, stream_batches):
    import bench_e2e as B
    from e2e_inputs import synthetic_detector_maps
    from fots_e2e.alphabet import ALPHABET
    from fots_e2e.hostcpus import cap_torch_threads
    from fots_e2e.model import FOTSNet
    from fots_e2e.native import use_native_depthwise
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
        for variant in ("stock", "native"):
            net = deterministic_init(FOTSNet(len(ALPHABET) + 1)).eval().to(device).to(dtype)
            if variant == "native":
                assert use_native_depthwise(net) == 22
            legs[(name, variant)] = dict(net=net, maps=maps, stacked=stacked)
    torch.cuda.synchronize(device)
    return dict(conv=conv, ims=ims, source=source, groups=groups, seq_groups=seq_groups, legs=legs, host_threads=host_threads)


def _leg_fns(S, device):
    from fots_e2e.pipeline import infer_batch, infer_image, infer_stream
    conv, ims, groups, seq_groups = S["conv"], S["ims"], S["groups"], S["seq_groups"]

    def leg_image(L):
        per = []
        for i, im in enumerate(ims):
            t0 = time.perf_counter()
            infer_image(L["net"], conv, im, detector=lambda _x, m=L["maps"][i]: m)
            torch.cuda.synchronize(device)
            per.append(time.perf_counter() - t0)
        return per

    def leg_batch(L):
        per = []
        for g, st in zip(groups, L["stacked"]):
            t0 = time.perf_counter()
            infer_batch(L["net"], conv, [ims[i] for i in g], detector=lambda _x, st=st: st)
            torch.cuda.synchronize(device)
            per.append(time.perf_counter() - t0)
        return per

    def leg_stream(L):
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        for _r in infer_stream(L["net"], conv, ([ims[i] for i in groups[k]] for k in seq_groups),
                               detector=lambda k, _x: L["stacked"][seq_groups[k]]):
            pass
        torch.cuda.synchronize(device)
        return time.perf_counter() - t0
    return leg_image, leg_batch, leg_stream


def measure_e2e(device, rounds, stream_batches):
    dtypes = DTYPES[:2]
    S = _e2e_setup(device, dtypes, stream_batches)
    leg_image, leg_batch, leg_stream = _leg_fns(S, device)
    keys = [(name, v) for name, _ in dtypes for v in ("stock", "native")]
    raw = {k: {"infer_image": [], "infer_batch": [], "infer_stream": []} for k in keys}
    with torch.no_grad():
        for k in keys:                                   # warm-up: every shape of every dtype, the side stream included
            leg_image(S["legs"][k])
            leg_batch(S["legs"][k])
            leg_stream(S["legs"][k])
        for _round in range(rounds):
            for k in keys:                               # alternated: stock, native within every round and dtype
                L = S["legs"][k]
                raw[k]["infer_image"].append(1.0 / float(np.median(leg_image(L))))
                raw[k]["infer_batch"].append(IMAGES_PER_BATCH / float(np.median(leg_batch(L))))
                raw[k]["infer_stream"].append(IMAGES_PER_BATCH * len(S["seq_groups"]) / leg_stream(L))
    out = {"images": S["source"], "images_per_batch": IMAGES_PER_BATCH, "stream_batches": len(S["seq_groups"]),
           "host_threads": S["host_threads"], "dtypes": {}}
    for name, _ in dtypes:
        d = {}
        for v in ("stock", "native"):
            d[v] = {leg: {"images_per_s": _spread(raw[(name, v)][leg]), "per_round": [round(x, 2) for x in raw[(name, v)][leg]]}
                    for leg in ("infer_image", "infer_batch", "infer_stream")}
        d["native_over_stock"] = {leg: round(d["native"][leg]["images_per_s"]["median"] / d["stock"][leg]["images_per_s"]["median"], 3)
                                  for leg in ("infer_image", "infer_batch", "infer_stream")}
        # the bar: the eight-per-pass legs with native are not below the stock legs' minimum over the rounds
        d["native_not_below_stock_min"] = {leg: d["native"][leg]["images_per_s"]["median"] >= d["stock"][leg]["images_per_s"]["min"]
                                           for leg in ("infer_batch", "infer_stream")}
        out["dtypes"][name] = d
        print("%-9s" % name + "  ".join("%s stock %.1f (%.1f-%.1f) native %.1f (%.1f-%.1f) img/s" % (
            leg, d["stock"][leg]["images_per_s"]["median"], d["stock"][leg]["images_per_s"]["min"], d["stock"][leg]["images_per_s"]["max"],
            d["native"][leg]["images_per_s"]["median"], d["native"][leg]["images_per_s"]["min"], d["native"][leg]["images_per_s"]["max"])
            for leg in ("infer_image", "infer_batch", "infer_stream")), file=sys.stderr)
    return out


def profile(device, variant, dtype_name, passes):
    dtypes = [d for d in DTYPES if d[0] == dtype_name]
    S = _e2e_setup(device, dtypes, 2)
    leg_image, _, _ = _leg_fns(S, device)
    with torch.no_grad():
        for _ in range(passes):
            leg_image(S["legs"][(dtype_name, variant)])
    return {"profiled": variant, "dtype": dtype_name, "passes": passes, "images": len(S["ims"])}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=200.0,
                    help="(a): a round times as many back-to-back calls as fill this window (at least 30)")
    ap.add_argument("--stream-batches", type=int, default=6)
    ap.add_argument("--skip-shapes", action="store_true")
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    ap.add_argument("--profile", choices=["stock", "native"], default=None, help="untimed one-image passes of one variant, for rocprofv3")
    ap.add_argument("--profile-dtype", choices=[n for n, _ in DTYPES], default="float32")
    ap.add_argument("--profile-passes", type=int, default=3)
    args = ap.parse_args()
    if args.rounds < 3:
        ap.error("--rounds must be at least 3: the spread over the rounds is part of the result")
    if not torch.cuda.is_available():
        raise SystemExit("depthwise_bench: no GPU -- this tool measures on the device and has no fallback")
    device = torch.device("cuda", 0)
    if args.profile:
        print(json.dumps(profile(device, args.profile, args.profile_dtype, args.profile_passes)))
        return
    out = {"rounds": args.rounds, "device": torch.cuda.get_device_name(device),
           "what": "native depthwise 3x3 against the stock convolution, alternated per round in one process; median (min, max) "
                   "over the rounds; (a) microseconds per call between device events, (b) images/s, host clock around work "
                   "that ends in a device synchronise"}
    if not args.skip_shapes:
        out["shapes"] = measure_shapes(device, args.rounds, args.window_ms)
        out["every_row_native_not_slower"] = all(r["native_not_slower"] for r in out["shapes"])
    if not args.skip_e2e:
        out["end_to_end"] = measure_e2e(device, args.rounds, args.stream_batches)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
