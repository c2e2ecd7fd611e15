"""The deterministic backward on the MI355X (profiles/deterministic_backward.md): AUTO against ORDERED
(backward(deterministic=True)) at the same shapes, alternated round by round in one process and timed with HIP events
after warm-up -- us per call, the median over rounds of the per-call mean of back-to-back calls (>= 200 calls per shape
and plan).  Also counts, at configs[2], how many gradient elements of 20 AUTO calls on the same inputs differ from the
first call's (a measurement of AUTO's run-to-run spread, not a test).

    python tools/deterministic_bench.py [--rounds 10] [--calls 20] [--json out.json]
    python tools/deterministic_bench.py --profile [cfg2 | ref512 | ref512_cl]
        # 200 ORDERED then 200 AUTO calls of one shape, for a rocprofv3 --kernel-trace run: configs[2] (NCHW), or the
        # reference's C = 64, two 120 x 160 maps, 11 x 96, R = 512 with an NCHW / a channels-last top_diff
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "fots.pytorch_amd"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import plan_cases as PC  # noqa: E402
import workloads as Wk  # noqa: E402
from rroi_align._ext import rroi_align as ext  # noqa: E402


def timed(fns, rounds, calls, warm=20):
    """fns: name -> callable.  Alternates them round by round; us per call, median over the rounds."""
    for f in fns.values():
        for _ in range(warm):
            f()
    torch.cuda.synchronize()
    per = {n: [] for n in fns}
    for _ in range(rounds):
        for n, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                f()
            b.record()
            b.synchronize()
            per[n].append(a.elapsed_time(b) * 1e3 / calls)
    return {n: round(statistics.median(v), 2) for n, v in per.items()}


def leg(name, f, r, ph, pw, scale, rounds, calls, cl_td=False, dtype=torch.float32):
    R = torch.from_numpy(r).cuda()
    g = torch.from_numpy(np.random.default_rng(3).standard_normal((len(r), f.shape[1], ph, pw)).astype(np.float32))
    g = g.cuda().to(dtype)
    if cl_td:
        g = g.contiguous(memory_format=torch.channels_last)
    fns = {"auto": lambda: ext.backward(g, R, f.shape, scale),
           "ordered": lambda: ext.backward(g, R, f.shape, scale, deterministic=True)}
    t = timed(fns, rounds, calls)
    td = int(cl_td and ph * pw > 1)
    plans = {k: ext.backward_plan(*f.shape, len(r), ph, pw, top_diff_layout=td, dtype=dtype, deterministic=k == "ordered")
             for k in fns}
    return {"leg": name, "us": t, "ratio": round(t["ordered"] / t["auto"], 2),
            "plan": {k: (p.family, p.dest, p.gy) for k, p in plans.items()}}


def auto_spread(calls=20):
    """configs[2], NCHW: elements of each of `calls` AUTO gradients that differ from the first call's, and the largest
    difference (relative to the largest gradient element)."""
    f, r = Wk.bench_inputs()
    R = torch.from_numpy(r).cuda()
    g = torch.from_numpy(np.random.default_rng(3).standard_normal((512, 256, 8, 64)).astype(np.float32)).cuda()
    first = ext.backward(g, R, f.shape, 0.25)
    counts, worst = [], 0.0
    for _ in range(calls - 1):
        x = ext.backward(g, R, f.shape, 0.25)
        counts.append(int((x != first).sum()))
        worst = max(worst, float((x - first).abs().max()))
    det = [int((ext.backward(g, R, f.shape, 0.25, deterministic=True) != ext.backward(
        g, R, f.shape, 0.25, deterministic=True)).sum()) for _ in range(3)]
    return {"calls": calls, "elements": first.numel(), "differ_per_call": counts,
            "calls_that_differ": sum(c > 0 for c in counts), "max_abs_diff": worst,
            "max_abs_grad": float(first.abs().max()), "ordered_differ": det,
            "plan": ext.backward_plan(1, 256, 160, 160, 512, 8, 64).family}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--json", default=None)
    ap.add_argument("--profile", nargs="?", const="cfg2", choices=("cfg2", "ref512", "ref512_cl"), default=None)
    args = ap.parse_args()
    if args.profile:
        if args.profile == "cfg2":
            f, r = Wk.bench_inputs()
            ph, pw = 8, 64
        else:
            f, r = Wk.bench_inputs(R=512, C=64, H=120, W=160, img=640, seed=4, batch=2)
            ph, pw = 11, 96
        R = torch.from_numpy(r).cuda()
        g = torch.from_numpy(np.random.default_rng(3).standard_normal((len(r), f.shape[1], ph, pw)).astype(np.float32))
        g = g.cuda()
        if args.profile == "ref512_cl":
            g = g.contiguous(memory_format=torch.channels_last)
        for det in (True, False):
            for _ in range(200):
                ext.backward(g, R, f.shape, 0.25, deterministic=det)
            torch.cuda.synchronize()
        print(f"profile {args.profile}: 200 ORDERED then 200 AUTO backward calls")
        return
    rc = (args.rounds, args.calls)
    out = []
    f, r = Wk.bench_inputs()
    out.append(leg("configs[2] NCHW top_diff / gradient", f, r, 8, 64, 0.25, *rc))
    out.append(leg("configs[2] channels-last top_diff", f, r, 8, 64, 0.25, *rc, cl_td=True))
    out.append(leg("configs[2] bfloat16", f, r, 8, 64, 0.25, *rc, dtype=torch.bfloat16))
    for R in (32, 512):
        fr, rr = Wk.bench_inputs(R=R, C=64, H=120, W=160, img=640, seed=4, batch=2)
        out.append(leg(f"C=64 2x120x160 11x96 R={R} NCHW", fr, rr, 11, 96, 0.25, *rc))
        if R == 512:
            out.append(leg(f"C=64 2x120x160 11x96 R={R} channels-last top_diff", fr, rr, 11, 96, 0.25, *rc, cl_td=True))
    fo, ro = PC.inputs(PC.Case("overlap", "bwd", 2, 36, 64, 64, 1500, 16, 9, gen="overlap"), seed=3)
    out.append(leg("overlap generator R=1500 (2x36x64x64, 16x9)", fo, ro, 16, 9, PC.SCALE, *rc))
    spread = auto_spread()
    for o in out:
        t = o["us"]
        print(f"{o['leg']:48s} AUTO {t['auto']:8.2f} us  ORDERED {t['ordered']:8.2f} us  ({o['ratio']:.2f}x)  plan {o['plan']}")
    print("AUTO spread at configs[2]:", spread)
    res = {"gpu": torch.cuda.get_device_name(), "legs": out, "auto_spread": spread}
    print(json.dumps(res))
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
