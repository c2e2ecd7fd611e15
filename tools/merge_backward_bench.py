"""tools/merge_backward_bench.py -- the gated merge and the bilinear resize, forward + backward: the native autograd
functions against autograd of the stock expression (measurement tool).

(a) per call    the network's three merges and its two stand-alone resizes at a 704 x 1280 image, one and eight images,
                float32 / bfloat16 / float16: 30 rows.  One call = forward + backward with gradients for every input:
                  stock   `(up(a) + f * up(gate)).backward(dy)` / `up(x).backward(dy)`,
                          up = F.interpolate(..., mode="bilinear", align_corners=True), a source of f's size as it is
                  native  `rroi_align.merge.gated_merge(a, f, gate).backward(dy)` / `bilinear_resize(x, size).backward(dy)`
                Microseconds per call between device events (a round = as many back-to-back calls as fill `--window-ms`),
                the two ALTERNATED inside one process, median and min-max over `--rounds` rounds; the host clock around the
                same rounds beside it.  The bar is DESIGN 5.10's: a row is kept where the native median is not above the
                stock leg's minimum of the same run.
(b) --kernels   the merge backward through the lean binding call on the two large merges -- the whole call (dy and f in, df
                out, the sums and the dgate launch) against `dst.copy_(src)` of one and a half maps (the same three
                map-sized streams), and df alone (dy in, df out) against a copy of one map -- in the same run.
                (The first launch alone is not isolated here: a call that wants dgate always runs the blocks' sum and
                the gather behind it.  `--profile` is for that.)
    --profile   untimed calls of the whole merge backward on the third merge at eight images, three dtypes, for a
                `rocprofv3 --kernel-trace --stats -- python tools/merge_backward_bench.py --profile` run of its own: the
                trace has each launch's duration (the element type is in the kernel's template arguments).
(c) --step      one recognition-free training step of FOTSNet (forward, a scalar loss, backward) with `use_native_merge`
                alone (training takes the stock merge) and with `use_trainable_merge` too, float32 and bfloat16, on
                `--batch N` images of `--image H W`.  One measurement, not a claim.

Needs a GPU: there is no fallback.
    python tools/merge_backward_bench.py [--rounds 7] [--out profiles/native_merge_backward.json] [--kernels | --step]
(`--out` adds to a file that is already there: the three modes are three runs; `--tag` names a run's keys, e.g. run2.)
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "fots.pytorch_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from depthwise_backward_bench import _alternate  # noqa: E402
from depthwise_bench import DTYPES  # noqa: E402

C = 256
# (name, f's / the output's size, a's / the source's size, the gate's size or None: a stand-alone resize)
ROWS = (("merge1", (44, 80), (22, 40), (22, 40)), ("merge2", (88, 160), (88, 160), (44, 80)),
        ("merge3", (176, 320), (176, 320), (88, 160)), ("resize1", (88, 160), (44, 80), None),
        ("resize2", (176, 320), (88, 160), None))


def _up(t, size):
    return t if tuple(t.shape[2:]) == tuple(size) else F.interpolate(t, size=size, mode="bilinear", align_corners=True)


def measure_shapes(device, rounds, window_ms):
    from rroi_align import merge
    rows = []
    g = torch.Generator().manual_seed(0)
    for name, dtype in DTYPES:
        for N in (1, 8):
            for what, size, a_size, g_size in ROWS:
                leaf = lambda *s: torch.randn(*s, generator=g).to(device).to(dtype).requires_grad_(True)  # noqa: E731
                a = leaf(N, C, *a_size)
                dy = torch.randn(N, C, *size, generator=g).to(device).to(dtype)
                if g_size is None:
                    leaves = (a,)
                    native, stock = (lambda: merge.bilinear_resize(a, size)), (lambda: _up(a, size))
                else:
                    f = leaf(N, C, *size)
                    gate = torch.rand(N, 1, *g_size, generator=g).to(device).to(dtype).requires_grad_(True)
                    leaves = (a, f, gate)
                    native = lambda: merge.gated_merge(a, f, gate)          # noqa: E731
                    stock = lambda: _up(a, size) + f * _up(gate, size)      # noqa: E731

                def step(forward, leaves=leaves, dy=dy):
                    def run():
                        for t in leaves:                      # (nothing accumulates: no add kernel in either leg)
                            t.grad = None
                        forward().backward(dy)
                    return run
                t = _alternate({"native": step(native), "stock": step(stock)}, rounds, window_ms, device, floor=10)
                row = {"what": what, "dtype": name, "N": N, "C": C, "size": list(size), "a_size": list(a_size),
                       "gate_size": None if g_size is None else list(g_size), "calls_per_round": {k: v["calls"] for k, v in t.items()}}
                for k, v in t.items():
                    row[k + "_us"], row[k + "_host_us"] = v["us"], v["host_us"]
                row["stock_over_native"] = round(row["stock_us"]["median"] / row["native_us"]["median"], 2)
                row["kept"] = row["native_us"]["median"] <= row["stock_us"]["min"]       # the bar
                rows.append(row)
                print("%-8s N=%d %-7s %3dx%3d  fwd+bwd native %8.1f us (%.1f-%.1f, host %.1f)  stock %8.1f us (%.1f-%.1f, host %.1f)"
                      "  x%.2f %s" % (name, N, what, size[0], size[1], row["native_us"]["median"], row["native_us"]["min"],
                                      row["native_us"]["max"], row["native_host_us"]["median"], row["stock_us"]["median"],
                                      row["stock_us"]["min"], row["stock_us"]["max"], row["stock_host_us"]["median"],
                                      row["stock_over_native"], "" if row["kept"] else "LOSES"), file=sys.stderr)
                del a, dy, leaves, native, stock
    return rows


def measure_kernels(device, rounds, window_ms):
    from rroi_align._ext import rroi_align as ext
    rows = []
    g = torch.Generator().manual_seed(0)
    for name, dtype in DTYPES:
        for N in (1, 8):
            for what, size, _, g_size in ROWS[1:3]:
                dy = torch.randn(N, C, *size, generator=g).to(device).to(dtype)
                f = torch.randn(N, C, *size, generator=g).to(device).to(dtype)
                gate = torch.rand(N, 1, *g_size, generator=g).to(device).to(dtype)
                src3 = torch.randn(3 * dy.numel() // 2, generator=g).to(device).to(dtype)      # 1.5 maps in, 1.5 out
                dst3, dst2 = torch.empty_like(src3), torch.empty_like(dy)
                t = _alternate({"backward": lambda: ext.run_gated_merge_backward(dy, f, gate, True, True),
                                "copy3": lambda: dst3.copy_(src3),
                                "df": lambda: ext.run_gated_merge_backward(dy, f, gate, True, False),
                                "copy2": lambda: dst2.copy_(dy)}, rounds, window_ms, device)
                map_bytes = dy.numel() * dy.element_size()
                row = {"what": what, "dtype": name, "N": N, "C": C, "size": list(size), "map_bytes": map_bytes}
                for k, v in t.items():
                    row[k + "_us"] = v["us"]
                    row[k + "_GBps"] = round((3 if k in ("backward", "copy3") else 2) * map_bytes / v["us"]["median"] / 1e3, 1)
                row["backward_over_copy"] = round(row["backward_GBps"] / row["copy3_GBps"], 3)
                row["df_over_copy"] = round(row["df_GBps"] / row["copy2_GBps"], 3)
                rows.append(row)
                print("%-8s N=%d %-6s  backward %7.1f us %7.1f GB/s  copy of 1.5 maps %7.1f us %7.1f GB/s  (%.2f)   df alone %7.1f us"
                      "  copy of a map %7.1f us  (%.2f)" % (
                          name, N, what, row["backward_us"]["median"], row["backward_GBps"], row["copy3_us"]["median"], row["copy3_GBps"],
                          row["backward_over_copy"], row["df_us"]["median"], row["copy2_us"]["median"], row["df_over_copy"]),
                      file=sys.stderr)
                del dy, f, gate, src3, dst3, dst2
    return rows


def measure_step(device, rounds, window_ms, image_hw, batch):
    """forward, a scalar loss and backward of the detection branch, with and without the switch"""
    from fots_e2e.model import FOTSNet
    from fots_e2e.native import use_native_merge
    from fots_e2e.native_train import use_trainable_merge
    from fots_e2e.weights import deterministic_init
    out = {"image": list(image_hw), "batch": batch}
    for name, dtype in DTYPES[:2]:
        image = torch.randn(batch, 3, *image_hw, generator=torch.Generator().manual_seed(7)).to(device).to(dtype)
        fns = {}
        for variant in ("stock_backward", "native_backward"):
            net = deterministic_init(FOTSNet()).to(device).to(dtype).train()
            assert use_native_merge(net)
            if variant == "native_backward":
                assert use_trainable_merge(net)
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
        print("%-8s recognition-free step on %d x %dx%d: stock merge %.1f us (%.1f-%.1f)  native merge %.1f us (%.1f-%.1f)  x%.3f" % (
            name, batch, image_hw[0], image_hw[1], d["stock_backward"]["median"], d["stock_backward"]["min"], d["stock_backward"]["max"],
            d["native_backward"]["median"], d["native_backward"]["min"], d["native_backward"]["max"], d["stock_over_native"]),
            file=sys.stderr)
        del fns, net
        torch.cuda.empty_cache()
    return out


def run_profile(device, calls):
    """`calls` untimed whole backward calls per dtype on the third merge at eight images, for a kernel trace"""
    from rroi_align._ext import rroi_align as ext
    g = torch.Generator().manual_seed(0)
    _, size, _, g_size = ROWS[2]
    for name, dtype in DTYPES:
        dy = torch.randn(8, C, *size, generator=g).to(device).to(dtype)
        f = torch.randn(8, C, *size, generator=g).to(device).to(dtype)
        gate = torch.rand(8, 1, *g_size, generator=g).to(device).to(dtype)
        for _ in range(calls):
            ext.run_gated_merge_backward(dy, f, gate, True, True)
        torch.cuda.synchronize(device)
        del dy, f, gate
    return {"calls_per_dtype": calls, "shape": [8, C, *size], "gate": list(g_size)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=30.0, help="a round times as many back-to-back calls as fill this window")
    ap.add_argument("--kernels", action="store_true", help="(b) only: the merge backward against plain copies")
    ap.add_argument("--step", action="store_true", help="(c) only: a recognition-free training step, switch on and off")
    ap.add_argument("--profile", action="store_true", help="untimed whole backward calls, for a rocprofv3 kernel trace")
    ap.add_argument("--profile-calls", type=int, default=60)
    ap.add_argument("--image", type=int, nargs=2, default=(704, 1280), metavar=("H", "W"), help="the image of --step")
    ap.add_argument("--batch", type=int, default=8, help="images per step of --step")
    ap.add_argument("--tag", default="", help="suffix of this run's keys in the JSON (a second run of the same mode)")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    if args.rounds < 3:
        ap.error("--rounds must be at least 3: the spread over the rounds is part of the result")
    if not torch.cuda.is_available():
        raise SystemExit("merge_backward_bench: no GPU -- this tool measures on the device and has no fallback")
    device = torch.device("cuda", 0)
    out = {"rounds": args.rounds, "device": torch.cuda.get_device_name(device),
           "what": "gated merge / bilinear resize forward + backward, native autograd functions against autograd of the stock "
                   "expression, alternated per round in one process; microseconds per call between device events and on the "
                   "host clock, median (min, max) over the rounds"}
    if args.profile:
        out["profile"] = run_profile(device, args.profile_calls)
    elif args.kernels:
        out["kernels" + args.tag] = measure_kernels(device, args.rounds, args.window_ms)
    elif args.step:
        key = "train_step_%dx%d_n%d%s" % (args.image[0], args.image[1], args.batch, args.tag)
        out[key] = measure_step(device, args.rounds, args.window_ms, args.image, args.batch)
    else:
        rows = measure_shapes(device, args.rounds, args.window_ms)
        out["shapes" + args.tag] = rows
        out["rows_kept" + args.tag] = sum(r["kept"] for r in rows)
        out["rows_lost" + args.tag] = [(r["what"], r["dtype"], r["N"]) for r in rows if not r["kept"]]
    if args.out:
        if os.path.exists(args.out):                      # the modes and the second run are runs of their own: one file collects them
            out = dict(json.load(open(args.out)), **out)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
