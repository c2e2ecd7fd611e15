"""tools/depthwise_backward_bench.py -- depthwise 3x3 convolution forward + backward: the native autograd function
against autograd of the stock convolution (measurement tool).

(a) per call    the six shapes of the network's depthwise convolutions (tools/depthwise_bench.py: SHAPES) at one and
                eight images, float32 / bfloat16 / float16.  One call = forward + backward with gradients for x and the
                weight:
                  stock   `nn.Conv2d(C, C, 3, stride, 1, groups=C, bias=False)(x).backward(dy)`, cudnn.deterministic off
                  native  `rroi_align.conv.depthwise3x3(x, w, stride).backward(dy)`
                and a forward-only column (the same two without a gradient), so that the backward's share is visible.
                Microseconds per call between device events (a round = as many back-to-back calls as fill `--window-ms`),
                the two ALTERNATED inside one process, median and min-max over `--rounds` rounds; the host clock around the
                same rounds (calls, then a synchronise) beside it.  The bar is DESIGN 5.10's: a row is kept where the
                native median is not above the stock leg's minimum of the same run.
(b) --kernels   the dx launch and the two dweight launches alone, through the lean binding call, on the two large planes
                (176 x 320 and 88 x 160 with 256 channels, one and eight images), against `dst.copy_(src)` of x's size in
                the same run: bytes the algorithm needs (dx: dy in, dx out; dweight: dy and x in) over the time between
                device events.
(c) --step      one recognition-free training step of FOTSNet (forward, a scalar loss, backward) with
                `use_native_depthwise` alone (its convolutions take the stock path: a gradient is needed) and with
                `use_trainable_depthwise` too, float32 and bfloat16, on `--batch N` images of `--image H W`.  One
                measurement, not a claim.

Needs a GPU: there is no fallback.
    python tools/depthwise_backward_bench.py [--rounds 7] [--out profiles/native_depthwise_backward.json] [--kernels | --step]
(`--out` adds to a file that is already there: the three modes are three runs; `--tag` names a run's keys, e.g. run2.)
"""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "fots.pytorch_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from depthwise_bench import DTYPES, SHAPES, _calls_for, _spread, _time_calls  # noqa: E402


def _host_time_calls(fn, iters, device):
    """microseconds per call on the host clock: `iters` calls and a synchronise"""
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize(device)
    return (time.perf_counter() - t0) * 1e6 / iters


def _alternate(fns, rounds, window_ms, device, floor=30):
    """{name: fn} -> {name: {"us": spread between device events, "host_us": spread on the host clock, "calls": n}}, the
    legs alternated per round"""
    for fn in fns.values():                                   # warm-up: MIOpen picks here
        for _ in range(3):
            fn()
    torch.cuda.synchronize(device)
    n = {k: _calls_for(fn, window_ms, floor=floor) for k, fn in fns.items()}
    dev, host = {k: [] for k in fns}, {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            dev[k].append(_time_calls(fn, n[k]))
        for k, fn in fns.items():
            host[k].append(_host_time_calls(fn, n[k], device))
    return {k: {"us": _spread(dev[k]), "host_us": _spread(host[k]), "calls": n[k]} for k in fns}


def measure_shapes(device, rounds, window_ms):
    from rroi_align import conv
    from rroi_align._ext import rroi_align as ext
    rows = []
    g = torch.Generator().manual_seed(0)
    torch.backends.cudnn.deterministic = False
    for name, dtype in DTYPES:
        for N in (1, 8):
            for C, H, W, s in SHAPES:
                ho, wo = (H - 1) // s + 1, (W - 1) // s + 1
                x = torch.randn(N, C, H, W, generator=g).to(device).to(dtype).requires_grad_(True)
                dy = torch.randn(N, C, ho, wo, generator=g).to(device).to(dtype)
                m = nn.Conv2d(C, C, 3, s, 1, groups=C, bias=False).to(device).to(dtype)
                w = m.weight

                def step(forward):
                    def run():
                        x.grad = w.grad = None                 # (nothing accumulates: no add kernel in either leg)
                        forward().backward(dy)
                    return run

                def plain(forward):
                    def run():
                        with torch.no_grad():
                            forward()
                    return run
                t = _alternate({"native": step(lambda: conv.depthwise3x3(x, w, s)), "stock": step(lambda: m(x)),
                                "native_fwd": plain(lambda: conv.depthwise3x3(x, w, s)), "stock_fwd": plain(lambda: m(x))},
                               rounds, window_ms, device)
                plan = ext.depthwise3x3_backward_plan(N, C, H, W, s, dtype=dtype)
                row = {"dtype": name, "N": N, "C": C, "H": H, "W": W, "stride": s, "band": plan.dw_band, "segments": plan.segments,
                       "calls_per_round": {k: v["calls"] for k, v in t.items()}}
                for k, v in t.items():
                    row[k + "_us"], row[k + "_host_us"] = v["us"], v["host_us"]
                row["stock_over_native"] = round(row["stock_us"]["median"] / row["native_us"]["median"], 2)
                row["kept"] = row["native_us"]["median"] <= row["stock_us"]["min"]       # the bar
                rows.append(row)
                print("%-8s N=%d %3dx%3dx%3d s%d  fwd+bwd native %8.1f us (%.1f-%.1f, host %.1f)  stock %8.1f us (%.1f-%.1f, host %.1f)"
                      "  x%.2f %s | fwd native %.1f stock %.1f" % (
                          name, N, C, H, W, s, row["native_us"]["median"], row["native_us"]["min"], row["native_us"]["max"],
                          row["native_host_us"]["median"], row["stock_us"]["median"], row["stock_us"]["min"], row["stock_us"]["max"],
                          row["stock_host_us"]["median"], row["stock_over_native"], "" if row["kept"] else "LOSES",
                          row["native_fwd_us"]["median"], row["stock_fwd_us"]["median"]), file=sys.stderr)
                del x, dy, m
    return rows


def measure_kernels(device, rounds, window_ms):
    from rroi_align._ext import rroi_align as ext
    rows = []
    g = torch.Generator().manual_seed(0)
    for name, dtype in DTYPES:
        for N in (1, 8):
            for C, H, W, s in SHAPES[:2]:
                x = torch.randn(N, C, H, W, generator=g).to(device).to(dtype)
                dy = torch.randn(N, C, H, W, generator=g).to(device).to(dtype)
                w = torch.randn(C, 1, 3, 3, generator=g).to(device).to(dtype)
                dst = torch.empty_like(x)
                t = _alternate({"dx": lambda: ext.run_depthwise3x3_backward(dy, x, w, s, True, False),
                                "dweight": lambda: ext.run_depthwise3x3_backward(dy, x, w, s, False, True),
                                "copy": lambda: dst.copy_(x)}, rounds, window_ms, device)
                nbytes = 2 * x.numel() * x.element_size()           # the same for all three: two tensors of x's size
                row = {"dtype": name, "N": N, "C": C, "H": H, "W": W, "stride": s, "bytes": nbytes}
                for k, v in t.items():
                    row[k + "_us"] = v["us"]
                    row[k + "_GBps"] = round(nbytes / v["us"]["median"] / 1e3, 1)
                rows.append(row)
                print("%-8s N=%d %3dx%3dx%3d  dx %7.1f us %7.1f GB/s  dweight %7.1f us %7.1f GB/s  copy %7.1f us %7.1f GB/s" % (
                    name, N, C, H, W, row["dx_us"]["median"], row["dx_GBps"], row["dweight_us"]["median"], row["dweight_GBps"],
                    row["copy_us"]["median"], row["copy_GBps"]), file=sys.stderr)
                del x, dy, dst
    return rows


def measure_step(device, rounds, window_ms, image_hw, batch):
    """forward, a scalar loss and backward of the detection branch, with and without the switch"""
    from fots_e2e.model import FOTSNet
    from fots_e2e.native import use_native_depthwise
    from fots_e2e.native_train import use_trainable_depthwise
    from fots_e2e.weights import deterministic_init
    out = {"image": list(image_hw), "batch": batch}
    for name, dtype in DTYPES[:2]:
        image = torch.randn(batch, 3, *image_hw, generator=torch.Generator().manual_seed(7)).to(device).to(dtype)
        fns = {}
        for variant in ("stock_backward", "native_backward"):
            net = deterministic_init(FOTSNet()).to(device).to(dtype).train()
            assert use_native_depthwise(net) == 22
            if variant == "native_backward":
                assert use_trainable_depthwise(net) == 22
            params = list(net.parameters())

            def step(net=net, params=params):
                outs = [t for group in net(image) for t in group]
                sum(t.float().sum() for t in outs).backward()
                for p in params:
                    p.grad = None
            fns[variant] = step
        t = _alternate(fns, rounds, window_ms, device, floor=5)
        d = {k: v["us"] for k, v in t.items()}
        d.update({k + "_host": v["host_us"] for k, v in t.items()})
        d["stock_over_native"] = round(d["stock_backward"]["median"] / d["native_backward"]["median"], 3)
        out[name] = d
        print("%-8s recognition-free step on %d x %dx%d: stock backward %.1f us (%.1f-%.1f)  native backward %.1f us (%.1f-%.1f)  x%.3f" % (
            name, batch, image_hw[0], image_hw[1], d["stock_backward"]["median"], d["stock_backward"]["min"], d["stock_backward"]["max"],
            d["native_backward"]["median"], d["native_backward"]["min"], d["native_backward"]["max"], d["stock_over_native"]),
            file=sys.stderr)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=30.0, help="a round times as many back-to-back calls as fill this window")
    ap.add_argument("--kernels", action="store_true", help="(b) only: the dx and dweight launches against a plain copy")
    ap.add_argument("--step", action="store_true", help="(c) only: a recognition-free training step, switch on and off")
    ap.add_argument("--image", type=int, nargs=2, default=(64, 96), metavar=("H", "W"), help="the image of --step")
    ap.add_argument("--batch", type=int, default=1, help="images per step of --step")
    ap.add_argument("--tag", default="", help="suffix of this run's keys in the JSON (a second run of the same mode)")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    if args.rounds < 3:
        ap.error("--rounds must be at least 3: the spread over the rounds is part of the result")
    if not torch.cuda.is_available():
        raise SystemExit("depthwise_backward_bench: no GPU -- this tool measures on the device and has no fallback")
    device = torch.device("cuda", 0)
    out = {"rounds": args.rounds, "device": torch.cuda.get_device_name(device),
           "what": "depthwise 3x3 convolution forward + backward, native autograd function against autograd of the stock "
                   "module, alternated per round in one process; microseconds per call between device events and on the "
                   "host clock, median (min, max) over the rounds"}
    if args.kernels:
        out["kernels" + args.tag] = measure_kernels(device, args.rounds, args.window_ms)
    elif args.step:
        key = "train_step_%dx%d%s%s" % (args.image[0], args.image[1], "_n%d" % args.batch if args.batch > 1 else "", args.tag)
        out[key] = measure_step(device, args.rounds, args.window_ms, args.image, args.batch)
    else:
        rows = measure_shapes(device, args.rounds, args.window_ms)
        out["shapes" + args.tag] = rows
        out["rows_kept" + args.tag] = sum(r["kept"] for r in rows)
        out["rows_lost" + args.tag] = [(r["dtype"], r["N"], r["C"], r["H"], r["W"], r["stride"]) for r in rows if not r["kept"]]
    if args.out:
        if os.path.exists(args.out):                      # the modes and the second run are runs of their own: one file collects them
            out = dict(json.load(open(args.out)), **out)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
