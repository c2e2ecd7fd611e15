"""tools/detection_loss_bench.py -- the native detection loss against the stock restatement (measurement tool).

Stock and native ALTERNATE in one process over `--rounds` rounds (7 by default); every figure is a median with the minimum
and maximum over the rounds next to it, microseconds per call.  What is timed is LOSS PLUS GRADIENT: the total, and
`torch.autograd.grad` of it with respect to the six predictions.  Two clocks: between two device events, and the host's
(`perf_counter` around the same calls with a synchronisation at the end) -- the stock path waits for the device at every
boolean index and at both `if`s, which only the host clock shows in full.

  shapes   the reference's training shape (N = 2, 128 x 128 at 1/4 and 64 x 64 at 1/8: batch 2 at 512 px), N = 8 and N = 16 at
           the same size, and N = 8 at 176 x 320 and 88 x 160 (1280 x 704 images), each in float32 and bfloat16; ground truth
           with a few boxes per image, as tests/detection_loss_cases.py builds it
  stock    fots_e2e.train.detection_loss(native=False); for bfloat16 behind the widening copies it needs (`.float()`, their
           backward included: its MSE of a bfloat16 prediction against a float32 target fails in backward)
  native   fots_e2e.train.detection_loss(native=True)
  ratios   the worst bound ratios of tests/detection_loss_cases.py's cases per dtype, measured in the same run
  --profile stock|native   runs `--profile-calls` untimed calls at the training shape in `--profile-dtype` and nothing else,
           for a `rocprofv3 --kernel-trace` run of its own: two call counts per arm, the difference of the kernel counts
           over the difference of the calls is the launches per call

Needs a GPU: there is no fallback.   python tools/detection_loss_bench.py [--rounds 7] [--out X.json] [--md X.md]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "fots.pytorch_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from depthwise_bench import _calls_for, _spread, _time_calls  # noqa: E402

SHAPES = (("train", 2, 128, 128, 64, 64), ("n8", 8, 128, 128, 64, 64), ("n16", 16, 128, 128, 64, 64), ("n8_1280x704", 8, 176, 320, 88, 160))
DTYPES = (("float32", torch.float32), ("bfloat16", torch.bfloat16))


def _host_time_calls(fn, iters, device):
    """microseconds per call by the host clock: `iters` calls and the synchronisation that ends them"""
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize(device)
    return (time.perf_counter() - t0) * 1e6 / iters


def arms(shape, dtype, device):
    """The two arms on one set of tensors: callables that return the six gradients."""
    import detection_loss_cases as DC
    from fots_e2e.train import detection_loss
    tag, N, H, W, H8, W8 = shape
    case = DC._case(tag, N, H, W, H8, W8, seed=100 + N + H)
    lists = [[torch.from_numpy(p[k]).to(device).to(dtype).requires_grad_(True) for p in case["preds"]] for k in range(3)]
    gt = [torch.from_numpy(v).to(device) for v in case["gt"]]
    flat = [lists[k][s] for s in range(2) for k in range(3)]

    def run(native):
        # the stock path has no 16-bit form (its MSE of a bfloat16 prediction against a float32 target fails in backward):
        # its arm widens the predictions first, and the copies and their backward are part of what it costs
        ls = lists if native or dtype == torch.float32 else [[t.float() for t in v] for v in lists]
        total = detection_loss(ls[0], gt[0], gt[1], ls[1], gt[2], ls[2], gt[3], native=native)
        return torch.autograd.grad(total, flat)
    return {"stock": lambda: run(False), "native": lambda: run(True)}


def measure(device, rounds, window_ms):
    rows = []
    for shape in SHAPES:
        for name, dtype in DTYPES:
            fns = arms(shape, dtype, device)
            for fn in fns.values():
                for _ in range(3):
                    fn()
            torch.cuda.synchronize(device)
            diff = max(float((a.double() - b.double()).abs().max()) for a, b in zip(fns["stock"](), fns["native"]()))
            calls = {k: min(2000, _calls_for(fn, window_ms)) for k, fn in fns.items()}
            dev, host = {k: [] for k in fns}, {k: [] for k in fns}
            for _ in range(rounds):
                for k, fn in fns.items():                                # alternated
                    dev[k].append(_time_calls(fn, calls[k]))
                    host[k].append(_host_time_calls(fn, calls[k], device))
            row = {"shape": shape[0], "N": shape[1], "quarter": list(shape[2:4]), "eighth": list(shape[4:6]), "dtype": name,
                   "calls": calls, "max_abs_gradient_difference_stock_native": diff}
            for k in fns:
                row[k + "_device_us"], row[k + "_host_us"] = _spread(dev[k]), _spread(host[k])
            for clock in ("device", "host"):
                s, n = row["stock_%s_us" % clock], row["native_%s_us" % clock]
                row["native_over_stock_" + clock] = round(n["median"] / s["median"], 3)
                row["outside_the_spread_" + clock] = bool(n["max"] < s["min"] or n["min"] > s["max"])
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def bound_ratios(device):
    """The worst |got - ref| / tolerance over the test cases, per dtype (tests/detection_loss_cases.py states the tolerance)."""
    import detection_loss_cases as DC
    from rroi_align.detection import detection_loss
    out = {}
    for dtype in DC.DTYPES:
        worst = {"terms": (0.0, None), "grad": (0.0, None)}
        for case in DC.CASES:
            ref = DC.materialise(case, dtype)[1]
            lists, gt = DC.tensors(case, dtype, device)
            terms = detection_loss(lists[0], gt[0], gt[1], lists[1], gt[2], lists[2], gt[3], multi_scale=case["multi"], return_terms=True)
            flat = [lists[k][s] for s in range(1 + case["multi"]) for k in range(3)]
            grads = torch.autograd.grad(terms, flat, torch.tensor(case["g"], dtype=torch.float32, device=device))
            for key, r in (("terms", DC.terms_ratio(terms, ref)), ("grad", DC.grads_ratio(grads, ref, dtype))):
                if r >= worst[key][0]:
                    worst[key] = (r, case["name"])
        out[str(dtype).replace("torch.", "")] = {k: {"ratio": round(v[0], 4), "case": v[1]} for k, v in worst.items()}
    return out


def to_markdown(result):
    f = lambda s: "%.1f (%.1f .. %.1f)" % (s["median"], s["min"], s["max"])            # noqa: E731
    lines = []
    for clock in ("device", "host"):
        lines += ["", "Loss + gradient, us per call, %s clock:" % clock, "",
                  "| shape | dtype | stock (min .. max) | native (min .. max) | native / stock | outside the spread |", "|---|---|---|---|---|---|"]
        for r in result["timings"]:
            lines.append("| %s N=%d %dx%d + %dx%d | %s | %s | %s | %.3f | %s |" % (
                r["shape"], r["N"], *r["quarter"], *r["eighth"], r["dtype"], f(r["stock_%s_us" % clock]), f(r["native_%s_us" % clock]),
                r["native_over_stock_" + clock], "yes" if r["outside_the_spread_" + clock] else "no"))
    lines += ["", "| dtype | worst terms ratio (case) | worst gradient ratio (case) |", "|---|---|---|"]
    for d, w in result["bound_ratios"].items():
        lines.append("| %s | %.4f (%s) | %.4f (%s) |" % (d, w["terms"]["ratio"], w["terms"]["case"], w["grad"]["ratio"], w["grad"]["case"]))
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=40.0)
    ap.add_argument("--out")
    ap.add_argument("--md")
    ap.add_argument("--profile", choices=("stock", "native"))
    ap.add_argument("--profile-dtype", default="float32", choices=[n for n, _ in DTYPES])
    ap.add_argument("--profile-calls", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/detection_loss_bench.py needs a GPU")
    device = torch.device("cuda", 0)
    if args.profile:
        fn = arms(SHAPES[0], dict(DTYPES)[args.profile_dtype], device)[args.profile]
        for _ in range(args.profile_calls):
            fn()
        torch.cuda.synchronize(device)
        return
    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "bound_ratios": bound_ratios(device),
              "timings": measure(device, args.rounds, args.window_ms)}
    print(json.dumps(result["bound_ratios"]))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    if args.md:
        with open(args.md, "w") as f:
            f.write(to_markdown(result))


if __name__ == "__main__":
    main()
