"""tools/heads_bench.py -- the native detection heads and attention gate against the stock chain (measurement tool).

(a) per call    `FOTSNet._heads` on the 256 x 176 x 320 quarter map and the 256 x 88 x 160 1/8 map, and the convolution +
                sigmoid of `FOTSNet._gate` on its three maps (256 x 22 x 40, 44 x 80, 88 x 160), at N = 1 and N = 8, float32 /
                bfloat16 / float16: `rroi_align._ext.rroi_align._heads_run` / `_gate_run` against the stock methods with the
                same parameters.  Microseconds per call between device events (a round = as many back-to-back calls as fill
                `--window-ms`), native and stock ALTERNATED inside one process, median and min-max over `--rounds` rounds,
                and the native call's bytes/s against N * (C + outputs) * H * W * sizeof(T).
(b) end to end  BASELINE configs[4] as tools/depthwise_bench.py runs it: infer_image, infer_batch (eight per pass),
                infer_stream in images/s, float32 and bfloat16, four variants alternated per round: stock, heads
                (`use_native_heads`), and both again with `use_native_depthwise` and `use_native_instancenorm` on in both legs.
(c) --forms     the plan rule's measurement: the heads with (V, S) FORCED over {4, 2, 1} x {1, 2, 4, 8, 16} through the extra
                entry point of the measurement library (`make -C fots.pytorch_amd/csrc heads-forms` builds it into
                tools/_explore/), every form alternated per round, beside the form the rule picks.

Every comparison is against the stock path on the same tree in the same process.  Needs a GPU: there is no fallback.
    python tools/heads_bench.py [--rounds 7] [--out profiles/native_heads.json] [--skip-shapes | --skip-e2e]
`--profile VARIANT` (stock | heads | dw+in | dw+in+heads) `--profile-dtype D`: no figures -- the one-image leg alone,
`--profile-passes` passes over the 11 images, for `rocprofv3 --kernel-trace --stats -- python tools/heads_bench.py
--profile heads` (a run of its own, never with --pmc, after an unprofiled run of the same command: the stock convolutions'
first use of a shape searches its solvers); launches and kernel time per image are its stats divided by passes x 11.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "fots.pytorch_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from depthwise_bench import DTYPES, IMAGES_PER_BATCH, _calls_for, _leg_fns, _spread, _time_calls  # noqa: E402

C = 256
HEADS_MAPS = ((176, 320), (88, 160))
GATE_MAPS = ((22, 40), (44, 80), (88, 160))
VARIANTS = ("stock", "heads", "dw+in", "dw+in+heads")
LEGS = ("infer_image", "infer_batch", "infer_stream")


def _net(device, dtype):
    from fots_e2e.model import FOTSNet
    from fots_e2e.weights import deterministic_init
    return deterministic_init(FOTSNet()).eval().to(device).to(dtype)


def measure_shapes(device, rounds, window_ms):
    from fots_e2e.model import FOTSNet
    from fots_e2e.native import _wb
    from rroi_align._ext import rroi_align as ext
    rows = []
    torch.manual_seed(0)
    with torch.no_grad():
        for name, dtype in DTYPES:
            net = _net(device, dtype)
            hp = _wb(net.act) + _wb(net.rbox) + _wb(net.angle)
            gp = _wb(net.conv_attenton)
            cases = [("heads", N, hw) for N in (1, 8) for hw in HEADS_MAPS] + [("gate", N, hw) for N in (1, 8) for hw in GATE_MAPS]
            for what, N, (H, W) in cases:
                x = torch.randn(N, C, H, W, device=device).to(dtype)
                if what == "heads":
                    native, stock, outputs = (lambda: ext._heads_run(x, *hp, 128.0)), (lambda: FOTSNet._heads(net, x)), 7
                else:
                    native = lambda: ext._gate_run(x, *gp)                       # noqa: E731
                    stock, outputs = (lambda: torch.sigmoid(net.conv_attenton(x))), 1
                for fn in (native, stock):                                      # warm-up: the stock convolution is picked here
                    for _ in range(3):
                        fn()
                torch.cuda.synchronize(device)
                n_native, n_stock = _calls_for(native, window_ms), _calls_for(stock, window_ms)
                t = {"native": [], "stock": []}
                for _ in range(rounds):
                    t["native"].append(_time_calls(native, n_native))
                    t["stock"].append(_time_calls(stock, n_stock))
                plan = ext.heads_plan(N, C, H, W, outputs=outputs, dtype=dtype)
                row = {"dtype": name, "what": what, "N": N, "C": C, "H": H, "W": W, "V": plan.vector_elems, "S": plan.channel_splits,
                       "calls_per_round": {"native": n_native, "stock": n_stock},
                       "native_us": _spread(t["native"]), "stock_us": _spread(t["stock"])}
                row["stock_over_native"] = round(row["stock_us"]["median"] / row["native_us"]["median"], 2)
                row["native_below_stock"] = row["native_us"]["median"] < row["stock_us"]["median"]
                row["native_TBps"] = round(N * (C + outputs) * H * W * x.element_size() / row["native_us"]["median"] * 1e-6, 3)
                rows.append(row)
                print("%-8s %-5s N=%d %3dx%3d V=%d S=%-2d native %7.1f us (%.1f-%.1f)  stock %7.1f us (%.1f-%.1f)  x%.2f  %.2f TB/s" % (
                    name, what, N, H, W, row["V"], row["S"], row["native_us"]["median"], row["native_us"]["min"],
                    row["native_us"]["max"], row["stock_us"]["median"], row["stock_us"]["min"], row["stock_us"]["max"],
                    row["stock_over_native"], row["native_TBps"]), file=sys.stderr)
    return rows


def measure_forms(device, rounds, window_ms):
    """every (V, S) forced through the measurement library's entry point (outputs allocated once, outside the timers)"""
    from fots_e2e.native import _wb
    from rroi_align._ext import rroi_align as ext
    lib = ctypes.CDLL(os.path.join(ROOT, "tools", "_explore", "librroi_heads_forms.so"))
    i, vp = ctypes.c_int, ctypes.c_void_p
    f = lib.rroi_heads_forward_forced_hip
    f.restype = i
    f.argtypes = [i] + [vp] * 10 + [i] * 4 + [ctypes.c_double, i, i, ctypes.POINTER(i), ctypes.POINTER(i), vp]
    rows = []
    torch.manual_seed(0)
    with torch.no_grad():
        for name, dtype in DTYPES[:2]:
            net = _net(device, dtype)
            hp = [p.contiguous() for p in _wb(net.act) + _wb(net.rbox) + _wb(net.angle)]
            for N in (1, 2, 4, 8):
                for H, W in HEADS_MAPS:
                    x = torch.randn(N, C, H, W, device=device).to(dtype)
                    outs = [torch.empty(N, k, H, W, device=device, dtype=dtype) for k in (1, 4, 2)]
                    stream = torch.cuda.current_stream().cuda_stream
                    rule = ext.heads_plan(N, C, H, W, dtype=dtype)
                    fns = {}
                    for V in (4, 2, 1):
                        for S in (1, 2, 4, 8, 16):
                            v, s = i(), i()
                            fn = (lambda V=V, S=S, v=v, s=s: f(ext.dtype_code(dtype), x.data_ptr(), *(p.data_ptr() for p in hp),
                                                               *(o.data_ptr() for o in outs), N, C, H, W, 128.0, V, S,
                                                               ctypes.byref(v), ctypes.byref(s), stream))
                            assert fn() == 1
                            if (v.value, s.value) == (V, S):                    # the caps left it alone
                                fns[(V, S)] = fn
                    torch.cuda.synchronize(device)
                    n = {k: _calls_for(fn, window_ms) for k, fn in fns.items()}
                    t = {k: [] for k in fns}
                    for _ in range(rounds):
                        for k, fn in fns.items():
                            t[k].append(_time_calls(fn, n[k]))
                    med = {k: _spread(v) for k, v in t.items()}
                    best = min(med, key=lambda k: med[k]["median"])
                    picked = (rule.vector_elems, rule.channel_splits)
                    row = {"dtype": name, "N": N, "H": H, "W": W, "rule": list(picked), "best": list(best),
                           "rule_us": med[picked], "best_us": med[best],
                           "rule_over_best": round(med[picked]["median"] / med[best]["median"], 3),
                           "forms_us": {"V%d_S%d" % k: v["median"] for k, v in sorted(med.items())}}
                    rows.append(row)
                    print("%-8s N=%d %3dx%3d rule V%d S%-2d %7.1f us  best V%d S%-2d %7.1f us  x%.3f   %s" % (
                        name, N, H, W, *picked, med[picked]["median"], *best, med[best]["median"], row["rule_over_best"],
                        " ".join("%s:%.1f" % kv for kv in row["forms_us"].items())), file=sys.stderr)
    return rows


def _switch(net, variant):
    from fots_e2e.native import use_native_depthwise, use_native_heads, use_native_instancenorm
    if variant.startswith("dw+in"):
        assert use_native_depthwise(net) == 22 and use_native_instancenorm(net) == (52, 20)
    if variant.endswith("heads"):
        assert use_native_heads(net)
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
        for native, stock in (("heads", "stock"), ("dw+in+heads", "dw+in")):
            d["%s_over_%s" % (native, stock)] = {leg: round(d[native][leg]["images_per_s"]["median"] / d[stock][leg]["images_per_s"]["median"], 3) for leg in LEGS}
            d["%s_not_below_%s_min" % (native, stock)] = {leg: d[native][leg]["images_per_s"]["median"] >= d[stock][leg]["images_per_s"]["min"] for leg in LEGS}
        out["dtypes"][name] = d
        for v in VARIANTS:
            print("%-9s %-12s" % (name, v) + "  ".join("%s %.1f (%.1f-%.1f)" % (
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
    ap.add_argument("--forms", action="store_true", help="(c) only: every (V, S) forced (needs `make heads-forms`)")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    ap.add_argument("--profile", choices=VARIANTS, default=None, help="untimed one-image passes of one variant, for rocprofv3")
    ap.add_argument("--profile-dtype", choices=[n for n, _ in DTYPES], default="float32")
    ap.add_argument("--profile-passes", type=int, default=3)
    args = ap.parse_args()
    if args.rounds < 3:
        ap.error("--rounds must be at least 3: the spread over the rounds is part of the result")
    if not torch.cuda.is_available():
        raise SystemExit("heads_bench: no GPU -- this tool measures on the device and has no fallback")
    device = torch.device("cuda", 0)
    if args.profile:
        print(json.dumps(profile(device, args.profile, args.profile_dtype, args.profile_passes)))
        return
    out = {"rounds": args.rounds, "device": torch.cuda.get_device_name(device),
           "what": "native detection heads and attention gate against the stock chain, alternated per round in one process; median "
                   "(min, max) over the rounds; (a), (c) microseconds per call between device events, (b) images/s, host clock "
                   "around work that ends in a device synchronise"}
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
