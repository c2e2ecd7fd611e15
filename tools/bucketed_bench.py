#!/usr/bin/env python
"""tools/bucketed_bench.py -- the bucketed RoIRotate against what the dense op makes a caller do.

Needs a GPU (fails without one).  Writes profiles/bucketed.md and profiles/bucketed.json.

Contenders, forward and backward separately, per shape and dtype:
  (a) the bucketed call (forward_bucketed / backward_bucketed): one launch chain, nothing wider than a crop is written;
  (b) the dense route: forward at W_max + index_select + slice + .contiguous() per bucket; backward = the bucket
      gradients scattered into a dense zero tensor + the dense backward;
  (c) one dense call per bucket (backward: the per-bucket gradients summed).
Timed: us per call between device events, every shape warmed first, >= 200 calls per window, the contenders alternated
in one process for >= 5 rounds; median and spread (min .. max of the rounds) reported.  The bar is (b) OF THE SAME RUN:
with more than one bucket (a)'s median must not exceed (b)'s; with one bucket it must lie within the spread of (b)'s own
rounds.  A shape that misses stays in the table, marked.  Algorithmic bytes of (a) and (b) come from the shapes.
Where (a) runs the two-launch plan the ragged gather's own time comes from `rocprofv3 --kernel-trace --stats` over a
child process that runs that shape alone (--only).  images/s of the pipeline with bucketed=True against the default is
reported as a fact, with no bar (bench_e2e.py's inputs, the two alternated)."""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "fots.pytorch_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from rroi_align._ext import rroi_align as ext  # noqa: E402
import workloads as Wk  # noqa: E402
from e2e_inputs import synthetic_boxes  # noqa: E402

CALLS, ROUNDS = 200, 5
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


def round_up(v, q):
    return int(-(-int(v) // q) * q)


def natural_widths(r, ph, quantum):
    """floor(roi_pooled_width) + 1 columns hold every live bin; rounded up to `quantum`."""
    rpw = np.float32(ph) * r[:, 4] / r[:, 3]
    return [max(quantum, round_up(np.floor(v) + 1, quantum)) for v in rpw]


def training(R, long_tail, seed):
    f, r = Wk.bench_inputs(R=R, C=64, H=120, W=160, img=640, seed=seed, batch=2)
    rng = np.random.default_rng(seed + 1000)
    ratio = rng.uniform(1.5, 9.0, R)
    if long_tail:
        ratio[::16] = 25.0                    # one word in sixteen is a long text line
    r[:, 3] = rng.uniform(14, 48, R)
    r[:, 4] = r[:, 3] * ratio
    return f, r, 11, natural_widths(r, 11, 32)


def e2e(nimg):
    from rroi_align.batched import rois_from_quads
    boxes = np.concatenate([synthetic_boxes(24, 704, 1280, seed=100 + i) for i in range(nimg)])
    bidx = np.repeat(np.arange(nimg, dtype=np.float32), 24)
    rois, gw = rois_from_quads(torch.from_numpy(boxes[:, :8].copy()).cuda(), torch.from_numpy(bidx).cuda(), False, 11)
    f = np.random.default_rng(nimg).standard_normal((nimg, 64, 176, 320), dtype=np.float32)
    return f, rois.cpu().numpy(), 11, gw.cpu().tolist()


def cfg1():
    f, r = Wk.bench_inputs()
    return f, r, 8, natural_widths(r, 8, 16)


SHAPES = {
    "e2e 1 image (24 words)": lambda: e2e(1),
    "e2e 8 images (192 words)": lambda: e2e(8),
    "training R=32": lambda: training(32, False, 11),
    "training R=512": lambda: training(512, False, 12),
    "training R=32 long tail": lambda: training(32, True, 13),
    "training R=512 long tail": lambda: training(512, True, 14),
    "configs[1] PH=8 natural": cfg1,
}


class Problem(object):
    def __init__(self, name, dtype):
        f, r, ph, widths = SHAPES[name]()
        self.name, self.ph, self.widths, self.scale = name, ph, [int(w) for w in widths], 0.25
        self.F = torch.from_numpy(f).cuda().to(dtype)
        self.R = torch.from_numpy(np.ascontiguousarray(r)).cuda()
        self.shape = tuple(f.shape)
        self.layout = ext.bucket_layout(self.widths)
        self.wmax = max(self.widths)
        self.idx = [torch.tensor(i, dtype=torch.int64).cuda() for _, i in self.layout]
        self.rois_b = [self.R.index_select(0, i).contiguous() for i in self.idx]
        C = f.shape[1]
        g = torch.Generator(device="cuda").manual_seed(1)
        self.grads = [torch.randn((len(i), C, ph, w), device="cuda", generator=g).to(dtype) for w, i in self.layout]
        self.dense_g = torch.empty((len(self.widths), C, ph, self.wmax), device="cuda", dtype=dtype)

    # ---- forward
    def fwd_a(self):
        return ext.forward_bucketed(self.F, self.R, self.ph, self.widths, self.scale)

    def fwd_b(self):
        dense = ext.forward(self.F, self.R, self.ph, self.wmax, self.scale)
        return [dense.index_select(0, i)[:, :, :, :w].contiguous() for (w, _), i in zip(self.layout, self.idx)]

    def fwd_c(self):
        return [ext.forward(self.F, rb, self.ph, w, self.scale) for (w, _), rb in zip(self.layout, self.rois_b)]

    # ---- backward
    def bwd_a(self):
        return ext.backward_bucketed(self.grads, self.R, self.shape, self.ph, self.widths, self.scale)

    def bwd_b(self):
        d = self.dense_g.zero_()
        for (w, _), i, g in zip(self.layout, self.idx, self.grads):
            d[:, :, :, :w].index_copy_(0, i, g)
        return ext.backward(d, self.R, self.shape, self.scale)

    def bwd_c(self):
        out = None
        for g, rb in zip(self.grads, self.rois_b):
            gi = ext.backward(g, rb, self.shape, self.scale)
            out = gi if out is None else out.add_(gi)
        return out

    def bytes(self):
        es = self.F.element_size()
        B, C, H, W = self.shape
        per_col = C * self.ph * es
        crops, dense = per_col * sum(self.widths), per_col * self.wmax * len(self.widths)
        fmap = B * C * H * W * es
        return {"fwd_a": fmap + crops, "fwd_b": fmap + dense + 2 * crops,           # (b): dense written, buckets read + written
                "bwd_a": crops + fmap, "bwd_b": dense + crops + dense + dense + fmap}  # (b): zero fill, scatter r + w, dense read


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def contest(fns, calls=CALLS, rounds=ROUNDS):
    for fn in fns.values():            # warm: kernels loaded, scratch and tables allocated
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in fns}
    for _ in range(rounds):            # alternated: a drift of the clocks hits every contender alike
        for k, fn in fns.items():
            samples[k].append(window(fn, calls))
    return {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in samples.items()}


def kernel_stats_rocprof(name, dname, what="fwd_a", calls=50):
    """rocprofv3 --kernel-trace --stats over a child process that runs ONE contender of one shape alone ->
    {kernel name: us per call}, None where it could not be measured."""
    exe = shutil.which("rocprofv3")
    if not exe:
        return None
    d = tempfile.mkdtemp(prefix="bucketed_prof_")
    try:
        cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "p", "--",
               sys.executable, os.path.abspath(__file__), "--only", name, "--what", what, "--dtype", dname, "--calls", str(calls)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
        out = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                out[row["Name"]] = out.get(row["Name"], 0.0) + float(row["TotalDurationNs"]) / 1e3 / (calls + 3)   # (+ the warm-up calls)
        return out or None
    except Exception as e:   # the figure is then "not measured"
        print("rocprofv3:", e, file=sys.stderr)
    finally:
        shutil.rmtree(d, ignore_errors=True)
    return None


def gather_time_rocprof(name, dname):
    """us per call of the ragged gather kernel in (a)'s forward."""
    st = kernel_stats_rocprof(name, dname, "fwd_a") or {}
    hit = [v for k, v in st.items() if "rroi_fwd_split_kernel" in k]
    return sum(hit) if hit else None


def e2e_images_per_s(rounds=ROUNDS):
    from bench_e2e import BOXES_PER_IMAGE, load_images
    from fots_e2e.alphabet import ALPHABET
    from fots_e2e.hostcpus import cap_torch_threads
    from fots_e2e.model import FOTSNet
    from fots_e2e.pipeline import batched, preprocess, resize_rule
    from fots_e2e.weights import deterministic_init
    from rroi_align.decode import CTCLabelConverter
    cap_torch_threads()
    dev = torch.device("cuda", 0)
    net = deterministic_init(FOTSNet(len(ALPHABET) + 1)).eval().to(dev)
    conv = CTCLabelConverter(ALPHABET)
    ims, _ = load_images()
    boxes = [synthetic_boxes(BOXES_PER_IMAGE, *resize_rule(im.shape[0], im.shape[1]), seed=100 + i) for i, im in enumerate(ims)]

    def one_pass(bucketed):
        ts = []
        for im, bx in zip(ims, boxes):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, _, _, feats = net(preprocess(im, dev))
            batched(net, conv, feats, bx, bucketed=bucketed)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return ts
    out = {False: [], True: []}
    with torch.no_grad():
        for flag in (False, True):
            one_pass(flag)
        for _ in range(rounds):
            for flag in (False, True):
                out[flag].append(1.0 / statistics.median(one_pass(flag)))
    return {("bucketed" if k else "default"): {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", help="run ONE contender (--what) of this shape alone, --calls times (the child of a rocprofv3 run)")
    ap.add_argument("--what", default="fwd_a", choices=["fwd_a", "fwd_b", "fwd_c", "bwd_a", "bwd_b", "bwd_c"])
    ap.add_argument("--dtype", default="fp32")
    ap.add_argument("--calls", type=int, default=CALLS)
    ap.add_argument("--rounds", type=int, default=ROUNDS)
    ap.add_argument("--no-rocprof", action="store_true")
    ap.add_argument("--no-e2e", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bucketed"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bucketed_bench.py needs a GPU")
    if args.only:
        p = Problem(args.only, DTYPES[args.dtype])
        for _ in range(args.calls + 3):
            getattr(p, args.what)()
        torch.cuda.synchronize()
        return
    if args.calls < 200 or args.rounds < 5:
        sys.exit("at least 200 calls per window and five rounds")
    rows = []
    for name in SHAPES:
        for dname, dtype in DTYPES.items():
            p = Problem(name, dtype)
            B, C, H, W = p.shape
            fplan = ext.forward_bucketed_plan(B, C, H, W, p.ph, p.widths, dtype=dtype)
            bplan = ext.backward_bucketed_plan(B, C, H, W, p.ph, p.widths, dtype=dtype)
            two = fplan.family == ext.PLAN_FWD_TWO_LAUNCH
            row = {"shape": name, "dtype": dname, "R": len(p.widths), "buckets": [(w, len(i)) for w, i in p.layout],
                   "fwd_plan": "two-launch ragged gather" if two else "ragged patch kernel",
                   "bwd_plan": {ext.PLAN_BWD_LISTS: "LISTS", ext.PLAN_BWD_BUCKETS: "BUCKETS"}[bplan.family],
                   "bytes": p.bytes(),
                   "fwd": contest({"a": p.fwd_a, "b": p.fwd_b, "c": p.fwd_c}, args.calls, args.rounds),
                   "bwd": contest({"a": p.bwd_a, "b": p.bwd_b, "c": p.bwd_c}, args.calls, args.rounds)}
            row["gather_us_rocprofv3"] = gather_time_rocprof(name, dname) if two and not args.no_rocprof else None
            for d in ("fwd", "bwd"):
                a, b = row[d]["a"], row[d]["b"]
                row[d]["meets_bar"] = bool(a["median"] <= b["median"] if len(p.layout) > 1 else a["median"] <= b["max"])
                if not row[d]["meets_bar"] and not args.no_rocprof:   # a miss keeps its reading: the kernels' own time
                    row[d]["kernel_us"] = {c: (lambda st: None if st is None else {"kernels": len(st), "busy_us": sum(st.values())})(
                        kernel_stats_rocprof(name, dname, d + "_" + c)) for c in ("a", "b")}
            rows.append(row)
            print(json.dumps({k: row[k] for k in ("shape", "dtype", "fwd_plan", "bwd_plan", "fwd", "bwd", "gather_us_rocprofv3")}),
                  flush=True)
            del p
            torch.cuda.empty_cache()
    result = {"device": torch.cuda.get_device_name(0), "version": ext.version(), "calls_per_window": args.calls,
              "rounds": args.rounds, "rows": rows, "e2e_images_per_s": None if args.no_e2e else e2e_images_per_s(args.rounds)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(result, open(args.out + ".json", "w"), indent=1)
    open(args.out + ".md", "w").write(markdown(result))
    print("wrote", args.out + ".md")


def markdown(res):
    def cell(s):
        return "%.1f (%.1f .. %.1f)" % (s["median"], s["min"], s["max"])
    out = ["# Bucketed RoIRotate against the dense route", "",
           "%s, %s.  us per call between device events, %d calls per window, %d alternated rounds: median (min .. max)."
           % (res["device"], res["version"], res["calls_per_window"], res["rounds"]),
           "(a) bucketed call, (b) dense at W_max + index_select + slice + contiguous per bucket (backward: scatter into a dense",
           "zero tensor + dense backward), (c) one dense call per bucket.  The bar is (b) of the same run; `MISS` marks a shape",
           "where (a)'s median exceeds it.  MB: algorithmic bytes from the shapes.", ""]
    for d, title in (("fwd", "Forward"), ("bwd", "Backward")):
        out += ["## " + title, "",
                "| shape | dtype | R | buckets (width x count) | plan | (a) | (b) | (c) | MB (a) | MB (b) | bar |",
                "|---|---|---|---|---|---|---|---|---|---|---|"]
        for r in res["rows"]:
            out.append("| %s | %s | %d | %s | %s | %s | %s | %s | %.1f | %.1f | %s |" % (
                r["shape"], r["dtype"], r["R"], " ".join("%dx%d" % b for b in r["buckets"]), r[d + "_plan"],
                cell(r[d]["a"]), cell(r[d]["b"]), cell(r[d]["c"]), r["bytes"][d + "_a"] / 1e6, r["bytes"][d + "_b"] / 1e6,
                "met" if r[d]["meets_bar"] else "MISS"))
        out.append("")
    out += ["## Rows that miss the bar: what rocprofv3 says (GPU-busy us per call = the sum of the kernels' own durations)", ""]
    missed = False
    for r in res["rows"]:
        for d in ("fwd", "bwd"):
            if not r[d]["meets_bar"]:
                missed = True
                ku = r[d].get("kernel_us") or {}
                txt = ", ".join("(%s) %s" % (c, "%d kernels, %.1f us" % (ku[c]["kernels"], ku[c]["busy_us"]) if ku.get(c) else "not measured")
                                for c in ("a", "b"))
                out.append("- %s, %s, %s (plan %s): %s" % (r["shape"], r["dtype"], d, r[d + "_plan"], txt))
    if not missed:
        out.append("- none")
    out += ["", "## The ragged gather alone (rocprofv3 --kernel-trace --stats, a run of its own)", ""]
    for r in res["rows"]:
        if r["fwd_plan"].startswith("two"):
            g = r["gather_us_rocprofv3"]
            out.append("- %s, %s: %s" % (r["shape"], r["dtype"], "%.1f us per call" % g if g else "not measured"))
    e = res["e2e_images_per_s"]
    out += ["", "## Pipeline, images/s (bench_e2e.py's images and boxes; a fact, no bar)", ""]
    if e:
        out.append("- default: %s; bucketed=True: %s" % (cell(e["default"]), cell(e["bucketed"])))
    else:
        out.append("- not measured")
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    main()
