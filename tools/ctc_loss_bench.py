"""tools/ctc_loss_bench.py -- the native CTC loss against torch's own (measurement tool).

Stock and native ALTERNATE in one process over `--rounds` rounds (7 by default); every figure is a median with the minimum
and maximum over the rounds next to it, microseconds per call between two device events.  What is timed is LOSS PLUS
GRADIENT: the loss of every sequence summed, and `torch.autograd.grad` of that sum with respect to the log-probabilities.

  shapes   the training shape (N = 32, K = 87, T = 96, L in 3..9) and N = 512, T = 128, each in float32 and bfloat16, the
           log-probabilities in the recogniser's (N, K, T) layout viewed as (T, N, K) -- what `forward_ocr(x).permute(2, 0, 1)`
           hands over -- and flat int64 targets with host lists of lengths, as bench_legs.train_step calls the loss
  stock    F.ctc_loss(reduction="sum"); for bfloat16 behind the widening copy it needs (`.float()`, its backward included)
  native   rroi_align.ctc.ctc_loss(reduction="sum")
  kernel   the native launch alone (run_ctc_loss on prepared tensors): what the surface's argument handling costs on top
  ratios   the worst bound ratios of tests/ctc_loss_cases.py's cases per dtype, measured in the same run

Needs a GPU: there is no fallback.   python tools/ctc_loss_bench.py [--rounds 7] [--out X.json] [--md X.md]
"""
import argparse
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

from depthwise_bench import _calls_for, _spread, _time_calls  # noqa: E402

SHAPES = (("train", 32, 87, 96), ("large", 512, 87, 128))
DTYPES = (("float32", torch.float32), ("bfloat16", torch.bfloat16))


def measure(device, rounds, window_ms):
    from rroi_align.ctc import _prepare, ctc_loss
    from rroi_align._ext.rroi_align.ctc_loss import run_ctc_loss
    rows = []
    for tag, N, K, T in SHAPES:
        rng = np.random.default_rng(77)
        lens = [int(v) for v in rng.integers(3, 10, N)]
        targets = torch.from_numpy(rng.integers(1, K, sum(lens)).astype(np.int64)).to(device)
        logits = torch.from_numpy(rng.standard_normal((N, K, T)).astype(np.float32)).to(device)
        for name, dtype in DTYPES:
            base = logits.log_softmax(1).to(dtype)                       # (N, K, T), as the head returns it
            leaf = base.clone().requires_grad_(True)

            def stock(leaf=leaf):
                lp = leaf.permute(2, 0, 1)
                loss = F.ctc_loss(lp if dtype == torch.float32 else lp.float(), targets, [T] * N, lens, blank=0, reduction="sum")
                return torch.autograd.grad(loss, leaf)[0]

            def native(leaf=leaf):
                loss = ctc_loss(leaf.permute(2, 0, 1), targets, [T] * N, lens, blank=0, reduction="sum")
                return torch.autograd.grad(loss, leaf)[0]
            prepared = _prepare(base.permute(2, 0, 1), targets, [T] * N, lens)
            kernel = lambda p=prepared: run_ctc_loss(*p, 0, False, True)                    # noqa: E731
            fns = {"stock": stock, "native": native, "kernel": kernel}
            for fn in fns.values():
                for _ in range(3):
                    fn()
            torch.cuda.synchronize(device)
            diff = float((stock().double() - native().double()).abs().max())
            calls = {k: min(2000, _calls_for(fn, window_ms)) for k, fn in fns.items()}
            t = {k: [] for k in fns}
            for _ in range(rounds):
                for k, fn in fns.items():                                # alternated
                    t[k].append(_time_calls(fn, calls[k]))
            row = {"shape": tag, "N": N, "K": K, "T": T, "dtype": name, "calls": calls,
                   "max_abs_gradient_difference_stock_native": diff}
            row.update({k + "_us": _spread(v) for k, v in t.items()})
            row["native_over_stock"] = round(row["native_us"]["median"] / row["stock_us"]["median"], 3)
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def bound_ratios(device):
    """The worst |got - ref| / tolerance over the test cases, per dtype (tests/ctc_loss_cases.py states the tolerance)."""
    import ctc_loss_cases as CC
    from rroi_align.ctc import ctc_loss
    out = {}
    for dtype in CC.DTYPES:
        worst = {"nll": (0.0, None), "grad": (0.0, None)}
        for case in CC.CASES:
            lp, (rn, rg, M) = CC.materialise(case, dtype)
            x = lp.to(device).requires_grad_(True)
            nll = ctc_loss(x, torch.from_numpy(case["targets"]).to(device), case["in_len"], case["tgt_len"], blank=case["blank"],
                           reduction="none")
            g, = torch.autograd.grad(nll, x, torch.ones_like(nll))
            for key, r in (("nll", CC.nll_ratio(nll, rn, case["T"], M)), ("grad", CC.grad_ratio(g, rg, dtype, case["T"], M))):
                if r >= worst[key][0]:
                    worst[key] = (r, case["name"])
        out[str(dtype).replace("torch.", "")] = {k: {"ratio": round(v[0], 4), "case": v[1]} for k, v in worst.items()}
    return out


def to_markdown(result):
    lines = ["| shape | dtype | stock us (min .. max) | native us (min .. max) | native / stock | launch alone us |", "|---|---|---|---|---|---|"]
    for r in result["timings"]:
        f = lambda s: "%.1f (%.1f .. %.1f)" % (s["median"], s["min"], s["max"])            # noqa: E731
        lines.append("| %s N=%d K=%d T=%d | %s | %s | %s | %.2f | %s |" % (r["shape"], r["N"], r["K"], r["T"], r["dtype"], f(r["stock_us"]),
                                                                         f(r["native_us"]), r["native_over_stock"], f(r["kernel_us"])))
    lines += ["", "| dtype | worst nll ratio (case) | worst gradient ratio (case) |", "|---|---|---|"]
    for d, w in result["bound_ratios"].items():
        lines.append("| %s | %.4f (%s) | %.4f (%s) |" % (d, w["nll"]["ratio"], w["nll"]["case"], w["grad"]["ratio"], w["grad"]["case"]))
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=40.0)
    ap.add_argument("--out")
    ap.add_argument("--md")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/ctc_loss_bench.py needs a GPU")
    device = torch.device("cuda", 0)
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
