"""Half-precision I/O on the MI355X (profiles/half_precision.md): the fp32 call, the native bfloat16 /
float16 call and the workaround `op(F.float()).to(dtype)` at the same shapes, alternated in one process and timed with
HIP events after warm-up (median over rounds of the per-call mean).

    python tools/half_bench.py [--rounds 5] [--calls 50] [--json out.json]
    python tools/half_bench.py --profile        # the configs[1] forward (bf16, then fp32), for a rocprofv3 --kernel-trace run

Shapes: configs[1] forward, configs[2] backward (NCHW both ends), the reference's own shapes (C = 64, two 120 x 160
maps, 11 x 96, R = 32 and 512), 11 x 83 (the SHIFT kernels' half-sector stores), and the one-launch range of fp32 AUTO
(f_fused_* of tests/plan_cases.py and around them) where a 16-bit call runs K2p or the two-launch path."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "fots.pytorch_amd"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import workloads as Wk  # noqa: E402
from rroi_align._ext import rroi_align as ext  # noqa: E402

DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


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


def forward_leg(name, f, r, ph, pw, rounds, calls, paths=None):
    F32, R = torch.from_numpy(f).cuda(), torch.from_numpy(r).cuda()
    fns = {"fp32": lambda: ext.forward(F32, R, ph, pw, 0.25)}
    for d in ("bf16", "fp16"):
        Fh = F32.to(DT[d])
        fns[d] = (lambda Fh=Fh: ext.forward(Fh, R, ph, pw, 0.25))
        fns[d + "_workaround"] = (lambda Fh=Fh, d=d: ext.forward(Fh.float(), R, ph, pw, 0.25).to(DT[d]))
    for label, (d, p) in (paths or {}).items():
        Fx = F32.to(DT[d])
        fns[label] = (lambda Fx=Fx, p=p: ext.forward(Fx, R, ph, pw, 0.25, path=p))
    t = timed(fns, rounds, calls)
    plans = {d: ext.forward_plan(*f.shape[:2], *f.shape[2:], len(r), ph, pw, dtype=DT[d]) for d in DT}
    return {"leg": name, "us": t, "plan": {d: (p.family, p.kernel, p.groups) for d, p in plans.items()},
            "crop_bytes": {d: len(r) * f.shape[1] * ph * pw * DT[d].itemsize for d in DT}}


def backward_leg(name, f, r, ph, pw, rounds, calls):
    R = torch.from_numpy(r).cuda()
    g32 = torch.from_numpy(np.random.default_rng(3).standard_normal((len(r), f.shape[1], ph, pw)).astype(np.float32)).cuda()
    fns = {"fp32": lambda: ext.backward(g32, R, f.shape, 0.25)}
    for d in ("bf16", "fp16"):
        gh = g32.to(DT[d])
        fns[d] = (lambda gh=gh: ext.backward(gh, R, f.shape, 0.25))
        fns[d + "_workaround"] = (lambda gh=gh, d=d: ext.backward(gh.float(), R, f.shape, 0.25).to(DT[d]))
    t = timed(fns, rounds, calls)
    plans = {d: ext.backward_plan(*f.shape[:2], *f.shape[2:], len(r), ph, pw, dtype=DT[d]) for d in DT}
    return {"leg": name, "us": t, "plan": {d: (p.family, p.dest, p.nk) for d, p in plans.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--json", default=None)
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    if args.profile:   # what a rocprofv3 --kernel-trace --stats run of the configs[1] forward sees: 300 bf16 calls,
        # then 300 fp32 calls for comparison (the kernels' names carry the element type)
        f, r = Wk.bench_inputs()
        R = torch.from_numpy(r).cuda()
        for dt in (torch.bfloat16, torch.float32):
            F = torch.from_numpy(f).cuda().to(dt)
            for _ in range(300):
                ext.forward(F, R, 8, 64, 0.25)
            torch.cuda.synchronize()
        print("profile: 300 bf16 then 300 fp32 configs[1] forward calls")
        return
    out = []
    f, r = Wk.bench_inputs()
    out.append(forward_leg("configs[1] forward", f, r, 8, 64, args.rounds, args.calls))
    out.append(backward_leg("configs[2] backward", f, r, 8, 64, args.rounds, max(10, args.calls // 5)))
    for R in (32, 512):
        fr, rr = Wk.bench_inputs(R=R, C=64, H=120, W=160, img=640, seed=4, batch=2)
        out.append(forward_leg(f"C=64 2x120x160 11x96 R={R}", fr, rr, 11, 96, args.rounds, args.calls))
        out.append(backward_leg(f"C=64 2x120x160 11x96 R={R} backward", fr, rr, 11, 96, args.rounds, args.calls))
    fr, rr = Wk.bench_inputs(R=512, C=64, H=120, W=160, img=640, seed=4, batch=2)
    out.append(forward_leg("C=64 2x120x160 11x83 R=512", fr, rr, 11, 83, args.rounds, args.calls))
    # the one-launch range of fp32 AUTO: K2p (PATH_DIRECT) against the two-launch path (PATH_TILED) in bf16
    alt = {"bf16_k2p": ("bf16", ext.PATH_DIRECT), "bf16_two_launch": ("bf16", ext.PATH_TILED)}
    for R in (12, 16, 20, 24, 28):
        fr, rr = Wk.bench_inputs(R=R, C=256, H=160, W=160, img=640, seed=6)
        out.append(forward_leg(f"fused range C=256 160x160 8x64 R={R}", fr, rr, 8, 64, args.rounds, args.calls, alt))
    for R in (24, 32, 40, 48, 56):
        fr, rr = Wk.bench_inputs(R=R, C=128, H=160, W=160, img=640, seed=6)
        out.append(forward_leg(f"fused range C=128 160x160 11x50 R={R}", fr, rr, 11, 50, args.rounds, args.calls, alt))
    for o in out:
        t = o["us"]
        line = f"{o['leg']:45s} fp32 {t['fp32']:8.2f}  bf16 {t['bf16']:8.2f} ({t['bf16'] / t['fp32']:.2f}x)  " \
               f"fp16 {t['fp16']:8.2f} ({t['fp16'] / t['fp32']:.2f}x)  workaround bf16 {t['bf16_workaround']:8.2f} fp16 " \
               f"{t['fp16_workaround']:8.2f}"
        if "bf16_k2p" in t:
            line += f"  | bf16 K2p {t['bf16_k2p']:.2f} two-launch {t['bf16_two_launch']:.2f}"
        print(line, "plan", o["plan"])
    print(json.dumps({"gpu": torch.cuda.get_device_name(), "legs": out}))
    if args.json:
        with open(args.json, "w") as fh:
            json.dump({"gpu": torch.cuda.get_device_name(), "legs": out}, fh, indent=1)


if __name__ == "__main__":
    main()
