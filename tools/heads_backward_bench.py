"""tools/heads_backward_bench.py -- detection heads and attention gate forward + backward: the native autograd functions
against autograd of the stock expressions (measurement tool).

(a) per call    the heads on the 1/4 and 1/8 maps of a 704 x 1280 image (256 x 176 x 320, 256 x 88 x 160) and the gate on its
                three maps (256 x 22 x 40, 44 x 80, 88 x 160), at one and eight images, float32 / bfloat16 / float16.  One call
                = forward + backward with gradients for x, the weights and the biases:
                  stock   `FOTSNet._heads`'s expression (gate: `torch.sigmoid(conv(x))`), `torch.autograd.backward`
                  native  `rroi_align.heads.detection_heads` / `attention_gate`, likewise
                Microseconds per call between device events (a round = as many back-to-back calls as fill `--window-ms`),
                the two ALTERNATED inside one process, median and min-max over `--rounds` rounds; the host clock around the
                same rounds beside it; the device launches of one call of each leg, counted by the profiler.  The bar is
                DESIGN 5.10's: a row is kept where the native median is not above the stock leg's minimum of the same run.
(b) --kernels   the backward alone through the lean binding call (dx + dw + db, two launches) and the training forward, on the
                heads' two maps and the gate's largest, against `dst.copy_(x)` in the same run: the bytes of x twice (x in, dx
                out; the copy moves the same) over the time between device events.
(c) --step      one recognition-free training step of FOTSNet (forward, a scalar loss, backward) with the other three
                trainable switches on in both arms and `use_trainable_heads` in one, float32 and bfloat16, on `--batch N`
                images of `--image H W`.  One measurement, not a claim.

Needs a GPU: there is no fallback.
    python tools/heads_backward_bench.py [--rounds 7] [--out profiles/native_heads_backward.json] [--kernels | --step]
(`--out` adds to a file that is already there: the modes are runs of their own; `--tag` names a run's keys, e.g. run2.)
"""
import argparse
import json
import os
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "fots.pytorch_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from depthwise_backward_bench import _alternate  # noqa: E402
from depthwise_bench import DTYPES  # noqa: E402

HEADS_MAPS = ((256, 176, 320), (256, 88, 160))
GATE_MAPS = ((256, 22, 40), (256, 44, 80), (256, 88, 160))


def _launches(fn, device):
    """Device kernels of one call of `fn`, by the profiler; None where this torch has no profiler to import."""
    try:
        from torch.profiler import ProfilerActivity, profile
    except ImportError:
        return None
    fn()
    torch.cuda.synchronize(device)
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize(device)
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "Memcpy" not in e.name
               and "Memset" not in e.name)


def _stock_heads(act, rbox, angle):
    def forward(t):
        score = torch.sigmoid(act(t))
        dist = torch.sigmoid(rbox(t)) * 128
        ang = torch.sigmoid(angle(t)) * 2 - 1
        ang = ang / torch.sqrt(ang[:, 0] * ang[:, 0] + ang[:, 1] * ang[:, 1]).unsqueeze(1)
        return score, dist, ang
    return forward


def measure_shapes(device, rounds, window_ms):
    from rroi_align import heads as fn
    from rroi_align._ext import rroi_align as ext
    rows = []
    g = torch.Generator().manual_seed(0)
    torch.backends.cudnn.deterministic = False
    for name, dtype in DTYPES:
        for N in (1, 8):
            for op, maps in (("heads", HEADS_MAPS), ("gate", GATE_MAPS)):
                for C, H, W in maps:
                    x = torch.randn(N, C, H, W, generator=g).to(device).to(dtype).requires_grad_(True)
                    convs = [nn.Conv2d(C, k, 1).to(device).to(dtype) for k in ((1, 4, 2) if op == "heads" else (1,))]
                    params = [p for m in convs for p in (m.weight, m.bias)]
                    dys = [torch.randn(N, m.out_channels, H, W, generator=g).to(device).to(dtype) for m in convs]
                    if op == "heads":
                        stock, native = _stock_heads(*convs), (lambda t: fn.detection_heads(t, *params))
                    else:
                        stock, native = (lambda t: torch.sigmoid(convs[0](t))), (lambda t: fn.attention_gate(t, *params))

                    def step(forward):
                        def run():
                            x.grad = None                          # (nothing accumulates: no add kernel in either leg)
                            for p in params:
                                p.grad = None
                            outs = forward(x)
                            torch.autograd.backward(outs if isinstance(outs, tuple) else (outs,), dys)
                        return run
                    legs = {"native": step(native), "stock": step(stock)}
                    t = _alternate(legs, rounds, window_ms, device)
                    plan = ext.heads_backward_plan(N, C, H, W, outputs=7 if op == "heads" else 1, dtype=dtype)
                    row = {"op": op, "dtype": name, "N": N, "C": C, "H": H, "W": W, "rows": plan.partial_rows,
                           "tiles_per_workgroup": plan.tiles_per_workgroup, "vector_elems": plan.vector_elems,
                           "launches": {k: _launches(f, device) for k, f in legs.items()},
                           "calls_per_round": {k: v["calls"] for k, v in t.items()}}
                    for k, v in t.items():
                        row[k + "_us"], row[k + "_host_us"] = v["us"], v["host_us"]
                    row["stock_over_native"] = round(row["stock_us"]["median"] / row["native_us"]["median"], 2)
                    row["kept"] = row["native_us"]["median"] <= row["stock_us"]["min"]       # the bar
                    rows.append(row)
                    print("%-5s %-8s N=%d %3dx%3dx%3d  fwd+bwd native %8.1f us (%.1f-%.1f, host %.1f, %s launches)  stock %8.1f us "
                          "(%.1f-%.1f, host %.1f, %s launches)  x%.2f %s" % (
                              op, name, N, C, H, W, row["native_us"]["median"], row["native_us"]["min"], row["native_us"]["max"],
                              row["native_host_us"]["median"], row["launches"]["native"], row["stock_us"]["median"],
                              row["stock_us"]["min"], row["stock_us"]["max"], row["stock_host_us"]["median"],
                              row["launches"]["stock"], row["stock_over_native"], "" if row["kept"] else "LOSES"), file=sys.stderr)
                    del x, dys, convs
    return rows


def measure_kernels(device, rounds, window_ms):
    from rroi_align._ext import rroi_align as ext
    rows = []
    g = torch.Generator().manual_seed(0)
    for name, dtype in DTYPES:
        for N in (1, 8):
            for op, (C, H, W) in (("heads", HEADS_MAPS[0]), ("heads", HEADS_MAPS[1]), ("gate", GATE_MAPS[2])):
                k = (1, 4, 2) if op == "heads" else (1,)
                x = torch.randn(N, C, H, W, generator=g).to(device).to(dtype)
                ws = [(torch.randn(n, C, generator=g) / 16).to(device).to(dtype) for n in k]
                bs = [torch.randn(n, generator=g).to(device).to(dtype) for n in k]
                dys = [torch.randn(N, n, H, W, generator=g).to(device).to(dtype) for n in k]
                dst = torch.empty_like(x)
                if op == "heads":
                    wb = [t for pair in zip(ws, bs) for t in pair]
                    z = ext.run_heads_train(x, *wb, 128.0)[3]
                    legs = {"backward": lambda: ext.run_heads_backward(*dys, x, z, *ws, 128.0, True, True, True),
                            "dx_only": lambda: ext.run_heads_backward(*dys, x, z, *ws, 128.0, True, False, False),
                            "forward_train": lambda: ext.run_heads_train(x, *wb, 128.0)}
                else:
                    z = ext.run_gate_train(x, ws[0], bs[0])[1]
                    legs = {"backward": lambda: ext.run_gate_backward(dys[0], x, z, ws[0], True, True, True),
                            "dx_only": lambda: ext.run_gate_backward(dys[0], x, z, ws[0], True, False, False),
                            "forward_train": lambda: ext.run_gate_train(x, ws[0], bs[0])}
                legs["copy"] = lambda: dst.copy_(x)
                t = _alternate(legs, rounds, window_ms, device)
                nbytes = 2 * x.numel() * x.element_size()
                row = {"op": op, "dtype": name, "N": N, "C": C, "H": H, "W": W, "bytes": nbytes}
                for key, v in t.items():
                    row[key + "_us"] = v["us"]
                    row[key + "_GBps"] = round((nbytes if key != "forward_train" else nbytes // 2) / v["us"]["median"] / 1e3, 1)
                rows.append(row)
                print("%-5s %-8s N=%d %3dx%3dx%3d  backward %7.1f us %7.1f GB/s  dx only %7.1f us %7.1f GB/s  train forward %7.1f us"
                      "  copy %7.1f us %7.1f GB/s" % (op, name, N, C, H, W, row["backward_us"]["median"], row["backward_GBps"],
                                                      row["dx_only_us"]["median"], row["dx_only_GBps"],
                                                      row["forward_train_us"]["median"], row["copy_us"]["median"],
                                                      row["copy_GBps"]), file=sys.stderr)
                del x, dys, dst, z
    return rows


def measure_step(device, rounds, window_ms, image_hw, batch):
    """forward, a scalar loss and backward of the detection branch, the other three trainable switches on in both arms"""
    from fots_e2e import native as nat
    from fots_e2e import native_train as T
    from fots_e2e.model import FOTSNet
    from fots_e2e.native_train_heads import use_trainable_heads
    from fots_e2e.weights import deterministic_init
    out = {"image": list(image_hw), "batch": batch}
    for name, dtype in DTYPES[:2]:
        image = torch.randn(batch, 3, *image_hw, generator=torch.Generator().manual_seed(7)).to(device).to(dtype)
        fns = {}
        for variant in ("stock_heads_backward", "native_heads_backward"):
            net = deterministic_init(FOTSNet()).to(device).to(dtype).train()
            nat.use_native_instancenorm(net)
            assert T.use_trainable_instancenorm(net) > 0
            assert nat.use_native_depthwise(net) == 22 and T.use_trainable_depthwise(net) == 22
            assert nat.use_native_heads(net) and nat.use_native_merge(net) and T.use_trainable_merge(net)
            if variant == "native_heads_backward":
                assert use_trainable_heads(net)
            params = list(net.parameters())

            def step(net=net, params=params):
                outs = [t for group in net(image)[:3] for t in group]
                sum(t.float().sum() for t in outs).backward()
                for p in params:
                    p.grad = None
            fns[variant] = step
        t = _alternate(fns, rounds, window_ms, device, floor=5)
        d = {k: v["us"] for k, v in t.items()}
        d.update({k + "_host": v["host_us"] for k, v in t.items()})
        d["stock_over_native"] = round(d["stock_heads_backward"]["median"] / d["native_heads_backward"]["median"], 3)
        out[name] = d
        print("%-8s recognition-free step on %d x %dx%d: stock heads backward %.1f us (%.1f-%.1f)  native %.1f us (%.1f-%.1f)  x%.3f" % (
            name, batch, image_hw[0], image_hw[1], d["stock_heads_backward"]["median"], d["stock_heads_backward"]["min"],
            d["stock_heads_backward"]["max"], d["native_heads_backward"]["median"], d["native_heads_backward"]["min"],
            d["native_heads_backward"]["max"], d["stock_over_native"]), file=sys.stderr)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=30.0, help="a round times as many back-to-back calls as fill this window")
    ap.add_argument("--kernels", action="store_true", help="(b) only: the backward and the training forward against a plain copy")
    ap.add_argument("--step", action="store_true", help="(c) only: a recognition-free training step, switch on and off")
    ap.add_argument("--image", type=int, nargs=2, default=(704, 1280), metavar=("H", "W"), help="the image of --step")
    ap.add_argument("--batch", type=int, default=1, help="images per step of --step")
    ap.add_argument("--tag", default="", help="suffix of this run's keys in the JSON (a second run of the same mode)")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    if args.rounds < 3:
        ap.error("--rounds must be at least 3: the spread over the rounds is part of the result")
    if not torch.cuda.is_available():
        raise SystemExit("heads_backward_bench: no GPU -- this tool measures on the device and has no fallback")
    device = torch.device("cuda", 0)
    out = {"rounds": args.rounds, "device": torch.cuda.get_device_name(device),
           "what": "detection heads and attention gate forward + backward, native autograd functions against autograd of the "
                   "stock expressions, alternated per round in one process; microseconds per call between device events and "
                   "on the host clock, median (min, max) over the rounds"}
    if args.kernels:
        out["kernels" + args.tag] = measure_kernels(device, args.rounds, args.window_ms)
    elif args.step:
        key = "train_step_%dx%d%s%s" % (args.image[0], args.image[1], "_n%d" % args.batch if args.batch > 1 else "", args.tag)
        out[key] = measure_step(device, args.rounds, args.window_ms, args.image, args.batch)
    else:
        rows = measure_shapes(device, args.rounds, args.window_ms)
        out["shapes" + args.tag] = rows
        out["rows_kept" + args.tag] = sum(r["kept"] for r in rows)
        out["rows_lost" + args.tag] = [(r["op"], r["dtype"], r["N"], r["C"], r["H"], r["W"]) for r in rows if not r["kept"]]
    if args.out:
        if os.path.exists(args.out):                      # the modes and the second run are runs of their own: one file collects them
            out = dict(json.load(open(args.out)), **out)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
