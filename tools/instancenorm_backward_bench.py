"""tools/instancenorm_backward_bench.py -- InstanceNorm2d (+ activation) forward + backward: the native autograd function
against autograd of the stock pair (measurement tool).

(a) per call    the twelve shapes of tools/instancenorm_bench.py at both batch sizes -- the trunk's six at N = 1 and N = 8,
                the recognition head's six at R = 24 and R = 192 -- float32 / bfloat16 / float16, the norm alone and with
                the activation.  One call = forward + backward with gradients for x, weight and bias:
                  stock   `F.leaky_relu(F.instance_norm(x, w, b, use_input_stats=True), 0.01).backward(dy)`, as the
                          16-bit types run it today
                  native  `rroi_align.norm.instance_norm(x, w, b, eps, 0.01).backward(dy)`
                Microseconds per call between device events (a round = as many back-to-back calls as fill `--window-ms`),
                the two ALTERNATED inside one process, median and min-max over `--rounds` rounds.  The bar is DESIGN
                5.10's: a row is kept where the native median is not above the stock leg's minimum of the same run.
(b) --step      the recognition branch of one training step (bench_legs.train_step's shape: 32 crops of 11 x 96 from a
                64-channel map, forward_ocr -> CTC loss -> backward), float32 and bfloat16, with `use_native_instancenorm`
                alone (its norms take the stock path: a gradient is needed) and with `use_trainable_instancenorm` too.
                Report only.
(c) --forms     the backward's form rule: the plane form and the split form FORCED (`make -C fots.pytorch_amd/csrc
                inorm-bwd-forms` builds the two measurement libraries into tools/_explore/) over plane counts x plane sizes
                through the raw C ABI, dx and parameter gradients, alternated per round.

Needs a GPU: there is no fallback.
    python tools/instancenorm_backward_bench.py [--rounds 7] [--out profiles/native_instancenorm_backward.json] [--step | --forms]
(`--out` adds to a file that is already there: the three modes are three runs.)
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

from depthwise_bench import DTYPES, _calls_for, _spread, _time_calls  # noqa: E402
from instancenorm_bench import HEAD, SLOPE, TRUNK  # noqa: E402

EPS = 1e-5


def measure_shapes(device, rounds, window_ms):
    from rroi_align import norm
    from rroi_align._ext import rroi_align as ext
    rows = []
    g = torch.Generator().manual_seed(0)
    cases = [(N, s) for N in (1, 8) for s in TRUNK] + [(R, s) for R in (24, 192) for s in HEAD]
    for name, dtype in DTYPES:
        for N, (C, H, W) in cases:
            x = torch.randn(N, C, H, W, device=device).to(dtype).requires_grad_(True)
            dy = torch.randn(N, C, H, W, device=device).to(dtype)
            w = (torch.randn(C, generator=g) * 0.5 + 1).to(device).to(dtype).requires_grad_(True)
            b = torch.randn(C, generator=g).to(device).to(dtype).requires_grad_(True)

            def step(forward):
                def run():
                    x.grad = w.grad = b.grad = None          # (nothing accumulates: no add kernel in either leg)
                    forward().backward(dy)
                return run
            pairs = {
                "norm": (step(lambda: norm.instance_norm(x, w, b, EPS, 1.0)),
                         step(lambda: F.instance_norm(x, weight=w, bias=b, use_input_stats=True, eps=EPS))),
                "norm+act": (step(lambda: norm.instance_norm(x, w, b, EPS, SLOPE)),
                             step(lambda: F.leaky_relu(F.instance_norm(x, weight=w, bias=b, use_input_stats=True, eps=EPS), SLOPE))),
            }
            plan = ext.instance_norm_backward_plan(N, C, H, W, dtype=dtype)
            for key, (native, stock) in pairs.items():
                for fn in (native, stock):                                      # warm-up: MIOpen picks here
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
                row["kept"] = row["native_us"]["median"] <= row["stock_us"]["min"]       # the bar
                rows.append(row)
                print("%-8s N=%-3d %3dx%3dx%4d %-9s native %8.1f us (%.1f-%.1f)  stock %8.1f us (%.1f-%.1f)  x%.2f %s" % (
                    name, N, C, H, W, key, row["native_us"]["median"], row["native_us"]["min"], row["native_us"]["max"],
                    row["stock_us"]["median"], row["stock_us"]["min"], row["stock_us"]["max"], row["stock_over_native"],
                    "" if row["kept"] else "LOSES"), file=sys.stderr)
            del x, dy
    return rows


def measure_step(device, rounds, window_ms):
    """bench_legs.train_step's recognition branch on crops that are already there, with and without the switch"""
    from fots_e2e.model import FOTSNet
    from fots_e2e.native import use_native_instancenorm
    from fots_e2e.native_train import use_trainable_instancenorm
    from fots_e2e.weights import deterministic_init
    C, R, PH, PW, nclass = 64, 32, 11, 96, 87
    rng = np.random.default_rng(77)
    lens = [int(v) for v in rng.integers(3, 10, R)]
    targets = torch.from_numpy(rng.integers(1, nclass, sum(lens)).astype(np.int64)).to(device)
    out = {}
    for name, dtype in DTYPES[:2]:
        crops = torch.from_numpy(rng.standard_normal((R, C, PH, PW), dtype=np.float32)).to(device).to(dtype)
        fns = {}
        for variant in ("stock_backward", "native_backward"):
            net = deterministic_init(FOTSNet(nclass)).to(device).to(dtype).train()
            assert use_native_instancenorm(net) == (52, 20)
            if variant == "native_backward":
                assert use_trainable_instancenorm(net) == 52
            params = list(net.parameters())

            def step(net=net, params=params):
                x = crops.clone().requires_grad_(True)
                preds = net.forward_ocr(x)
                T = preds.size(2)
                loss = F.ctc_loss(preds.float().permute(2, 0, 1), targets, [T] * R, lens, blank=0, reduction="sum") / R
                loss.backward()
                for p in params:
                    p.grad = None
            fns[variant] = step
        for fn in fns.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize(device)
        n = {k: _calls_for(fn, window_ms, floor=10) for k, fn in fns.items()}
        t = {k: [] for k in fns}
        for _ in range(rounds):
            for k, fn in fns.items():
                t[k].append(_time_calls(fn, n[k]))
        d = {k: _spread(v) for k, v in t.items()}
        d["stock_over_native"] = round(d["stock_backward"]["median"] / d["native_backward"]["median"], 3)
        out[name] = d
        print("%-8s recognition branch of a step, R = 32: stock backward %.1f us (%.1f-%.1f)  native backward %.1f us (%.1f-%.1f)  x%.3f" % (
            name, d["stock_backward"]["median"], d["stock_backward"]["min"], d["stock_backward"]["max"], d["native_backward"]["median"],
            d["native_backward"]["min"], d["native_backward"]["max"], d["stock_over_native"]), file=sys.stderr)
    return out


def _raw(lib_path):
    lib = ctypes.CDLL(lib_path)
    i, vp, sz = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    lib.rroi_instancenorm_forward_train_hip.restype = i
    lib.rroi_instancenorm_forward_train_hip.argtypes = [i] + [vp] * 5 + [i] * 4 + [ctypes.c_double, ctypes.c_float, vp, sz, vp]
    lib.rroi_instancenorm_backward_hip.restype = i
    lib.rroi_instancenorm_backward_hip.argtypes = [i] + [vp] * 8 + [i] * 4 + [ctypes.c_double, ctypes.c_float, vp, sz, vp]
    for name in ("rroi_instancenorm_workspace_bytes", "rroi_instancenorm_backward_workspace_bytes"):
        getattr(lib, name).restype = sz
        getattr(lib, name).argtypes = [i] * 4
    return lib


def measure_forms(device, rounds, window_ms):
    """plane form against split form of the backward, forced, through the raw ABI (everything allocated outside the timers)"""
    from rroi_align._ext import rroi_align as ext
    libs = {k: _raw(os.path.join(ROOT, "tools", "_explore", "librroi_inorm_bwd_%s.so" % k)) for k in ("plane", "split")}
    rows = []
    torch.manual_seed(0)
    sizes = ((44, 80), (88, 160), (128, 192), (128, 256), (176, 240), (176, 320), (352, 640), (704, 1280))
    for name, dtype in (DTYPES[0], DTYPES[1]):
        for planes in (16, 32, 64, 128, 256, 512):
            for H, W in sizes:
                if planes * H * W > (1 << 27):
                    continue
                x = torch.randn(1, planes, H, W, device=device).to(dtype)
                dy = torch.randn(1, planes, H, W, device=device).to(dtype)
                w, b = torch.ones(planes, device=device, dtype=dtype), torch.zeros(planes, device=device, dtype=dtype)
                y, dx, dw, db = torch.empty_like(x), torch.empty_like(x), torch.empty_like(w), torch.empty_like(w)
                stats = torch.empty(planes, 2, dtype=torch.float64, device=device)
                stream = torch.cuda.current_stream().cuda_stream
                code = ext.dtype_code(dtype)
                need = ext.instance_norm_workspace_bytes(1, planes, H, W)
                ws0 = torch.empty(max(need, 1), dtype=torch.uint8, device=device)
                assert ext._lib.rroi_instancenorm_forward_train_hip(code, x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(),
                                                                    stats.data_ptr(), 1, planes, H, W, EPS, SLOPE,
                                                                    ws0.data_ptr() if need else None, need, stream) == 1
                fns = {}
                for k, lib in libs.items():
                    nb = lib.rroi_instancenorm_backward_workspace_bytes(1, planes, H, W)
                    ws = torch.empty(nb, dtype=torch.uint8, device=device)
                    fns[k] = (lambda lib=lib, ws=ws, nb=nb: lib.rroi_instancenorm_backward_hip(
                        code, dy.data_ptr(), x.data_ptr(), stats.data_ptr(), w.data_ptr(), b.data_ptr(), dx.data_ptr(), dw.data_ptr(),
                        db.data_ptr(), 1, planes, H, W, EPS, SLOPE, ws.data_ptr(), nb, stream))
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


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=30.0,
                    help="a round times as many back-to-back calls as fill this window (at least 30; 10 for --step)")
    ap.add_argument("--step", action="store_true", help="(b) only: the recognition branch of a training step")
    ap.add_argument("--forms", action="store_true", help="(c) only: plane form against split form, forced (needs `make inorm-bwd-forms`)")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    if args.rounds < 3:
        ap.error("--rounds must be at least 3: the spread over the rounds is part of the result")
    if not torch.cuda.is_available():
        raise SystemExit("instancenorm_backward_bench: no GPU -- this tool measures on the device and has no fallback")
    device = torch.device("cuda", 0)
    out = {"rounds": args.rounds, "device": torch.cuda.get_device_name(device),
           "what": "InstanceNorm2d (+ activation) forward + backward, native autograd function against autograd of the stock "
                   "pair, alternated per round in one process; microseconds per call between device events, median (min, max) "
                   "over the rounds"}
    if args.forms:
        out["forms"] = measure_forms(device, args.rounds, args.window_ms)
    elif args.step:
        out["train_step_recognition"] = measure_step(device, args.rounds, args.window_ms)
    else:
        out["shapes"] = measure_shapes(device, args.rounds, args.window_ms)
        out["rows_kept"] = sum(r["kept"] for r in out["shapes"])
        out["rows_lost"] = [(r["dtype"], r["N"], r["C"], r["H"], r["W"], r["what"]) for r in out["shapes"] if not r["kept"]]
    if args.out:
        if os.path.exists(args.out):                      # the three modes are three runs: one file collects them
            out = dict(json.load(open(args.out)), **out)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
