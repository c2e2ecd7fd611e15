"""tools/e2e_half_trace.py -- per-kernel time of the passes that `tools/e2e_half_bench.py --profile DTYPE` runs between its
two marker launches (rroi_sincos_probe_kernel), from rocprofv3's kernel trace (csv).  Host only.

    rocprofv3 --kernel-trace --output-format csv -d DIR -o NAME -- python tools/e2e_half_bench.py --profile bfloat16 --profile-legs image
    python tools/e2e_half_trace.py DIR/.../NAME_kernel_trace.csv [more traces ...] [--top 12] [--images 22]

Prints, per trace, the kernels grouped by a short name: launches, total and share of the device time between the markers,
microseconds per image (`--images`: images in the measured passes; 2 passes x 11 for the image leg)."""
import argparse
import collections
import csv
import re

MARKER = "rroi_sincos_probe_kernel"


def short(name):
    name = re.sub(r"\[clone[^\]]*\]", "", name).strip()
    name = re.sub(r"^void\s+", "", name)
    name = re.sub(r"\(anonymous namespace\)::", "", name)
    name = re.sub(r"<.*", "", name)          # template arguments
    name = re.sub(r"\(.*", "", name)         # parameter list
    return name.split("::")[-1][:72] if "::" in name and not name.startswith("miopen") else name[:72]


def summarise(path, top, images):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    marks = [i for i, r in enumerate(rows) if MARKER in r["Kernel_Name"]]
    if len(marks) < 2:
        raise SystemExit("%s: fewer than two marker launches" % path)
    part = rows[marks[0] + 1:marks[-1]]
    agg = collections.defaultdict(lambda: [0, 0])
    for r in part:
        a = agg[short(r["Kernel_Name"])]
        a[0] += 1
        a[1] += int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
    total = sum(v[1] for v in agg.values())
    print("%s: %d launches, %.3f ms of kernels between the markers = %.1f us per image" % (path, len(part), total / 1e6, total / 1e3 / images))
    for name, (n, ns) in sorted(agg.items(), key=lambda kv: -kv[1][1])[:top]:
        print("  %8.1f us/image %5.1f %% %6d launches  %s" % (ns / 1e3 / images, 100.0 * ns / total, n, name))
    return agg, total


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("traces", nargs="+")
    ap.add_argument("--top", type=int, default=12)
    ap.add_argument("--images", type=int, default=22)
    args = ap.parse_args()
    for p in args.traces:
        summarise(p, args.top, args.images)


if __name__ == "__main__":
    main()
