"""tools/instancenorm_bench.py -- the native InstanceNorm2d (+ activation) against the stock one (measurement tool).

(a) per call    every distinct (C, H, W) the network's norms see at 1280 x 704 at N = 1 and N = 8, and the recognition head's
                three norms on 11 x 64 / 11 x 96 crops at R = 24 and R = 192; float32 / bfloat16 / float16; the norm alone
                (`instance_norm` against `F.instance_norm`) and with the activation (`instance_norm(..., 0.01)` against
                `F.leaky_relu(F.instance_norm(...), 0.01)`).  Microseconds per call between device events (a round = as many
                back-to-back calls as fill `--window-ms`), native and stock ALTERNATED inside one process, median and min-max
                over `--rounds` rounds.  For the two stem shapes also the achieved bytes/s against 3 * N * C * H * W *
                sizeof(T) (two reads, one write) beside the same run's `y.copy_(x)` against 2 * N * C * H * W * sizeof(T).
(b) end to end  BASELINE configs[4] as tools/depthwise_bench.py runs it: infer_image, infer_batch (eight per pass),
                infer_stream in images/s, float32 and bfloat16, four variants alternated per round: stock, native
                (`use_native_instancenorm`), and both again with `use_native_depthwise` on in both legs.
(c) --forms     the form rule's measurement: the plane form and the split form FORCED (`make -C fots.pytorch_amd/csrc
                inorm-forms` builds the two measurement libraries into tools/_explore/) over plane counts x plane sizes
                through the raw C ABI, alternated per round.

Every comparison is against the stock path on the same tree in the same process.  Needs a GPU: there is no fallback.
    python tools/instancenorm_bench.py [--rounds 7] [--out profiles/native_instancenorm.json] [--skip-shapes | --skip-e2e]
`--profile VARIANT` (stock | native | dw | dw+native) `--profile-dtype D`: no figures -- the one-image leg alone,
`--profile-passes` passes over the 11 images, for `rocprofv3 --kernel-trace --stats -- python tools/instancenorm_bench.py
--profile native` (a run of its own, never with --pmc); launches and kernel time per image are its stats divided by
passes x 11.  There is no separate warm-up in that mode: the first pass's one-off kernels are in the stats' totals.
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

# (C, H, W): the stem's two mirror norms, layer1 .. layer4
TRUNK = ((32, 704, 1280), (64, 352, 640), (64, 176, 320), (128, 88, 160), (256, 44, 80), (512, 22, 40))
STEM = TRUNK[:2]
# the head's batch5, batch7, batch10_s on crops of width w (two (2, 1) pools, then a (2, 3) convolution without row padding)
HEAD = tuple((c, h, w) for w in (64, 96) for c, h in ((128, 11), (256, 5), (256, 1)))
VARIANTS = ("stock", "native", "dw", "dw+native")
SLOPE = 0.01


def _row_print(row, key):
    print("%-8s N=%-3d %3dx%3dx%4d %-9s native %8.1f us (%.1f-%.1f)  stock %8.1f us (%.1f-%.1f)  x%.2f" % (
        row["dtype"], row["N"], row["C"], row["H"], row["W"], key, row["native_us"]["median"], row["native_us"]["min"],
        row["native_us"]["max"], row["stock_us"]["median"], row["stock_us"]["min"], row["stock_us"]["max"],
        row["stock_over_native"]), file=sys.stderr)


def measure_shapes(device, rounds, window_ms):
    from rroi_align._ext import rroi_align as ext
    rows = []
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(0)
    cases = [(N, s) for N in (1, 8) for s in TRUNK] + [(R, s) for R in (24, 192) for s in HEAD]
    with torch.no_grad():
        for name, dtype in DTYPES:
            for N, (C, H, W) in cases:
                x = torch.randn(N, C, H, W, device=device).to(dtype)
                w = (torch.randn(C, generator=g) * 0.5 + 1).to(device).to(dtype)
                b = torch.randn(C, generator=g).to(device).to(dtype)
                pairs = {
                    "norm": (lambda: ext.instance_norm(x, w, b, 1e-5, 1.0),
                             lambda: F.instance_norm(x, weight=w, bias=b, use_input_stats=True, eps=1e-5)),
                    "norm+act": (lambda: ext.instance_norm(x, w, b, 1e-5, SLOPE),
                                 lambda: F.leaky_relu(F.instance_norm(x, weight=w, bias=b, use_input_stats=True, eps=1e-5), SLOPE)),
                }
                plan = ext.instance_norm_plan(N, C, H, W, dtype=dtype)
                for key, (native, stock) in pairs.items():
                    for fn in (native, stock):                                  # warm-up: MIOpen picks here
                        for _ in range(3):
                            fn()
                    torch.cuda.synchronize(device)
                    n_native, n_stock = _calls_for(native, window_ms), _calls_for(stock, window_ms)
                    t = {"native": [], "stock": []}
                    for _ in range(rounds):
                        t["native"].append(_time_calls(native, n_native))
                        t["stock"].append(_time_calls(stock, n_stock))
                    row = {"dtype": name, "N": N, "C": C, "H": H, "W": W, "what": key, "form": "split" if plan.form == 2 else "plane",
                           "segments": plan.segments, "calls_per_round": {"native": n_native, "stock": n_stock},
                           "native_us": _spread(t["native"]), "stock_us": _spread(t["stock"])}
                    row["stock_over_native"] = round(row["stock_us"]["median"] / row["native_us"]["median"], 2)
                    row["native_below_stock"] = row["native_us"]["median"] < row["stock_us"]["median"]
                    if (C, H, W) in STEM and key == "norm":
                        y = torch.empty_like(x)
                        copy = lambda: y.copy_(x)                               # noqa: E731
                        n_copy = _calls_for(copy, window_ms)
                        tc = [_time_calls(copy, n_copy) for _ in range(rounds)]
                        nbytes = x.numel() * x.element_size()
                        row["copy_us"] = _spread(tc)
                        row["native_TBps"] = round(3 * nbytes / row["native_us"]["median"] * 1e-6, 3)
                        row["stock_TBps"] = round(3 * nbytes / row["stock_us"]["median"] * 1e-6, 3)
                        row["copy_TBps"] = round(2 * nbytes / row["copy_us"]["median"] * 1e-6, 3)
                    rows.append(row)
                    _row_print(row, key)
    return rows


def _raw(lib_path):
    lib = ctypes.CDLL(lib_path)
    i, vp, sz = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    lib.rroi_instancenorm_forward_hip.restype = i
    lib.rroi_instancenorm_forward_hip.argtypes = [i, vp, vp, vp, vp, i, i, i, i, ctypes.c_double, ctypes.c_float, vp, sz, vp]
    lib.rroi_instancenorm_workspace_bytes.restype = sz
    lib.rroi_instancenorm_workspace_bytes.argtypes = [i] * 4
    return lib


def measure_forms(device, rounds, window_ms):
    """plane form against split form, forced, through the raw ABI (outputs and workspace allocated once, outside the timers)"""
    from rroi_align._ext import rroi_align as ext
    libs = {k: _raw(os.path.join(ROOT, "tools", "_explore", "librroi_inorm_%s.so" % k)) for k in ("plane", "split")}
    rows = []
    torch.manual_seed(0)
    sizes = ((44, 80), (88, 160), (128, 192), (128, 256), (176, 240), (176, 320), (352, 640), (704, 1280))
    with torch.no_grad():
        for name, dtype in (DTYPES[0], DTYPES[1]):
            for planes in (16, 32, 64, 128, 256, 512):
                for H, W in sizes:
                    if planes * H * W > (1 << 27):
                        continue
                    x = torch.randn(1, planes, H, W, device=device).to(dtype)
                    w, b, y = torch.ones(planes, device=device, dtype=dtype), torch.zeros(planes, device=device, dtype=dtype), torch.empty_like(x)
                    stream = torch.cuda.current_stream().cuda_stream
                    fns = {}
                    for k, lib in libs.items():
                        need = lib.rroi_instancenorm_workspace_bytes(1, planes, H, W)
                        ws = torch.empty(max(need, 1), dtype=torch.uint8, device=device)
                        fns[k] = (lambda lib=lib, ws=ws, need=need: lib.rroi_instancenorm_forward_hip(
                            ext.dtype_code(dtype), x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), 1, planes, H, W, 1e-5, SLOPE,
                            ws.data_ptr() if need else None, need, stream))
                        assert fns[k]() == 1
                    torch.cuda.synchronize(device)
                    n = {k: _calls_for(fns[k], window_ms) for k in fns}
                    t = {k: [] for k in fns}
                    for _ in range(rounds):
                        for k in fns:
                            t[k].append(_time_calls(fns[k], n[k]))
                    row = {"dtype": name, "planes": planes, "plane_elems": H * W, "plane_us": _spread(t["plane"]), "split_us": _spread(t["split"])}
                    row["plane_over_split"] = round(row["plane_us"]["median"] / row["split_us"]["median"], 2)
                    rows.append(row)
                    print("%-8s planes %4d x %7d  plane %8.1f us  split %8.1f us  x%.2f" % (
                        name, planes, H * W, row["plane_us"]["median"], row["split_us"]["median"], row["plane_over_split"]), file=sys.stderr)
    return rows


def _e2e_setup(device, dtypes, stream_batches, variants):
    import bench_e2e as B
    from e2e_inputs import synthetic_detector_maps
    from fots_e2e.alphabet import ALPHABET
    from fots_e2e.hostcpus import cap_torch_threads
    from fots_e2e.model import FOTSNet
    from fots_e2e.native import use_native_depthwise, use_native_instancenorm
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
            net = deterministic_init(FOTSNet(len(ALPHABET) + 1)).eval().to(device).to(dtype)
            if variant.startswith("dw"):
                assert use_native_depthwise(net) == 22
            if variant.endswith("native"):
                assert use_native_instancenorm(net) == (52, 20)
            legs[(name, variant)] = dict(net=net, maps=maps, stacked=stacked)
    torch.cuda.synchronize(device)
    return dict(conv=conv, ims=ims, source=source, groups=groups, seq_groups=seq_groups, legs=legs, host_threads=host_threads)


LEGS = ("infer_image", "infer_batch", "infer_stream")


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
            for k in keys:                               # alternated: the four variants within every round and dtype
                L = S["legs"][k]
                raw[k]["infer_image"].append(1.0 / float(np.median(leg_image(L))))
                raw[k]["infer_batch"].append(IMAGES_PER_BATCH / float(np.median(leg_batch(L))))
                raw[k]["infer_stream"].append(IMAGES_PER_BATCH * len(S["seq_groups"]) / leg_stream(L))
    out = {"images": S["source"], "images_per_batch": IMAGES_PER_BATCH, "stream_batches": len(S["seq_groups"]),
           "host_threads": S["host_threads"], "dtypes": {}}
    for name, _ in dtypes:
        d = {v: {leg: {"images_per_s": _spread(raw[(name, v)][leg]), "per_round": [round(x, 2) for x in raw[(name, v)][leg]]}
                 for leg in LEGS} for v in VARIANTS}
        # the bar (DESIGN 5.10's): the native median is not below the stock leg's minimum of the same run
        d["native_over_stock"] = {leg: round(d["native"][leg]["images_per_s"]["median"] / d["stock"][leg]["images_per_s"]["median"], 3) for leg in LEGS}
        d["dw+native_over_dw"] = {leg: round(d["dw+native"][leg]["images_per_s"]["median"] / d["dw"][leg]["images_per_s"]["median"], 3) for leg in LEGS}
        d["native_not_below_stock_min"] = {leg: d["native"][leg]["images_per_s"]["median"] >= d["stock"][leg]["images_per_s"]["min"] for leg in LEGS}
        d["dw+native_not_below_dw_min"] = {leg: d["dw+native"][leg]["images_per_s"]["median"] >= d["dw"][leg]["images_per_s"]["min"] for leg in LEGS}
        out["dtypes"][name] = d
        for v in VARIANTS:
            print("%-9s %-10s" % (name, v) + "  ".join("%s %.1f (%.1f-%.1f)" % (
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
                    help="(a), (c): a round times as many back-to-back calls as fill this window (at least 30)")
    ap.add_argument("--stream-batches", type=int, default=6)
    ap.add_argument("--skip-shapes", action="store_true")
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--forms", action="store_true", help="(c) only: plane form against split form, forced (needs `make inorm-forms`)")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    ap.add_argument("--profile", choices=VARIANTS, default=None, help="untimed one-image passes of one variant, for rocprofv3")
    ap.add_argument("--profile-dtype", choices=[n for n, _ in DTYPES], default="float32")
    ap.add_argument("--profile-passes", type=int, default=3)
    args = ap.parse_args()
    if args.rounds < 3:
        ap.error("--rounds must be at least 3: the spread over the rounds is part of the result")
    if not torch.cuda.is_available():
        raise SystemExit("instancenorm_bench: no GPU -- this tool measures on the device and has no fallback")
    device = torch.device("cuda", 0)
    if args.profile:
        print(json.dumps(profile(device, args.profile, args.profile_dtype, args.profile_passes)))
        return
    out = {"rounds": args.rounds, "device": torch.cuda.get_device_name(device),
           "what": "native InstanceNorm2d (+ activation) against the stock one, alternated per round in one process; median (min, "
                   "max) over the rounds; (a), (c) microseconds per call between device events, (b) images/s, host clock around "
                   "work that ends in a device synchronise"}
    if args.forms:
        out["forms"] = measure_forms(device, args.rounds, args.window_ms)
    else:
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
