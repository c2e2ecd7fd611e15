"""profiles/native_network.json and .md from the record of one GPU run of tests/test_gpu_network.py and from the CPU
mutation table of tests/test_network_twin.py (computed here: CPU only).

    NETWORK_TWIN_RECORD=record.jsonl python -m pytest -m gpu tests/test_gpu_network.py      (on the MI355X)
    python tools/network_twin_report.py record.jsonl                                        (anywhere)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "fots.pytorch_amd"), os.path.join(ROOT, "tests")]


def mutation_table():
    import network_cases as C
    import test_network_twin as T
    rows = []
    for name, (what, stage_names, _) in C.MUTATIONS.items():
        row = {"mutation": name, "what": what, "stages": list(stage_names)}
        for tag, dtype in zip(C.IDS, C.DTYPES):
            ratio, neg = T.measure(dtype, name)
            row[tag] = {"ratio": ratio, "rel_neg": neg, "flagged": T.flagged(ratio, neg)}
        rows.append(row)
    honest = {}
    for tag, dtype in zip(C.IDS, C.DTYPES):
        rels, negs = [], []
        for which in range(len(C.INPUTS)):
            for st, _, _, r, n in T.honest(dtype, which)[1].values():
                rels += r
                negs += [v for v in n if v is not None]
        honest[tag] = {"rel_min": min(rels), "rel_max": max(rels), "rel_neg_max": max(negs)}
    return rows, honest


def fmt(v, spec=".2e"):
    return "-" if v is None else format(v, spec)


def main(path):
    rows = [json.loads(line) for line in open(path)]
    teacher = [r for r in rows if r["test"] == "teacher"]
    free = [r for r in rows if r["test"] == "free"]
    ledger = [r for r in rows if r["test"] == "ledger"]
    mutations, honest = mutation_table()
    out = {"teacher_forced": teacher, "free_running": free, "ledger": ledger, "cpu_mutations": mutations, "cpu_honest": honest,
           "caps": {"ratio": 2.0, "rel_neg": 0.25}}
    with open(os.path.join(ROOT, "profiles", "native_network.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")

    images = sorted({r["image"] for r in teacher}, reverse=True)
    md = ["# The fully switched network against its float64 twin, stage by stage (DESIGN 5.18)", "",
          "One MI355X, one run of `tests/test_gpu_network.py` with `NETWORK_TWIN_RECORD` set; tables by",
          "`tools/network_twin_report.py`.  Raw data: `native_network.json`.  `rel` is the relative L2 error against the twin,",
          "`rel_neg` the same over the elements whose reference is negative; every stage is fed the switched network's previous",
          "16-bit output (teacher-forced).  Asserted in the 16-bit types: ratio <= 2, rel_neg <= 0.25.", "",
          "## Summary", "", "| type | mode | rows | worst ratio (stage, image) | worst rel_neg (stage, image) | worst stock rel_neg |",
          "|---|---|---|---|---|---|"]
    for dtype in ("bf16", "fp16", "fp32"):
        for mode in ("forced", "shipped"):
            sel = [r for r in teacher if r["dtype"] == dtype and r["mode"] == mode]
            if not sel:
                continue
            a = max(sel, key=lambda r: r["ratio"])
            neg = [r for r in sel if r["rel_neg"] is not None]
            b = max(neg, key=lambda r: r["rel_neg"])
            c = max(neg, key=lambda r: r["rel_neg_stock"])
            md.append(f"| {dtype} | {mode} | {len(sel)} | {a['ratio']:.3f} ({a['stage']}, {a['image']}) | "
                      f"{b['rel_neg']:.2e} ({b['stage']}, {b['image']}) | {c['rel_neg_stock']:.2e} |")
    md += ["", "fp32 runs the six switches that apply to it and is recorded only: nothing is asserted of it."]
    for dtype in ("bf16", "fp16", "fp32"):
        for mode in ("forced", "shipped"):
            sel = [r for r in teacher if r["dtype"] == dtype and r["mode"] == mode]
            if not sel:
                continue
            md += ["", f"## Teacher-forced stages, {dtype}, hooks {mode}", "",
                   "| stage | output | " + " | ".join(f"{im}: rel native | rel stock | ratio | rel_neg" for im in images) + " |",
                   "|---|---|" + "---|---|---|---|" * len(images)]
            keys = []
            for r in sel:
                if (r["stage"], r["output"]) not in keys:
                    keys.append((r["stage"], r["output"]))
            for stage, output in keys:
                cells = []
                for im in images:
                    r = next(r for r in sel if (r["stage"], r["output"], r["image"]) == (stage, output, im))
                    cells.append(f"{r['rel_native']:.2e} | {r['rel_stock']:.2e} | {r['ratio']:.3f} | {fmt(r['rel_neg'])}")
                md.append(f"| {stage} | {output} | " + " | ".join(cells) + " |")
    md += ["", "## Free-running: the whole `net(x)` / `forward_ocr` against the whole twin (recorded, no cap)", "",
           "| type | image | output | rel native | rel stock |", "|---|---|---|---|---|"]
    for r in free:
        md.append(f"| {r['dtype']} | {r['image']} | {r['output']} | {r['rel_native']:.2e} | {r['rel_stock']:.2e} |")
    md += ["", "## The ledger of one `forward` + one `forward_ocr`, every kernel forced", ""]
    for r in ledger:
        md.append(f"- {r['dtype']}: native calls {json.dumps(r['native'], sort_keys=True)}; stock operators {json.dumps(r['stock'])}")
    md += ["", "## Repeatability (a diagnostic run: every stage four times on the same input, all of `net(x)` four times)", "",
           "- Switched network: every stage and all eight outputs of `net(x)` gave the same bits every time, in both types,",
           "  on both inputs, forced and shipped -- but `forward_ocr`, through the stock `conv10_s`: on 4 x 256 x 5 x 40 in fp16",
           "  17,815 - 19,897 of 40,960 outputs of that convolution changed between calls (bf16: 1 - 3), on one crop of 8",
           "  columns none.",
           "- Unswitched network: in fp16 128 - 185,279 elements of every output of `net(x)` but `focr` changed between calls",
           "  (the 1x1 convolutions of `feature2`, `layer3`, `layer4`), in bf16 up to 117,632 of `merged`.",
           "- With `torch.backends.cudnn.deterministic = True` nothing changed anywhere, stock or switched."]
    md += ["", "## CPU: what the two caps catch (tests/test_network_twin.py)", "",
           "The stock 16-bit CPU network against the twin: " + "; ".join(
               f"{k} rel per stage {v['rel_min']:.1e} to {v['rel_max']:.1e}, worst rel_neg {v['rel_neg_max']:.3f}"
               for k, v in honest.items()) + ".",
           "Ratio: the largest rel(mutated) / rel(honest) over the mutation's stages and both inputs.", "",
           "| | mutation | bf16 ratio | bf16 rel_neg | bf16 caught | fp16 ratio | fp16 rel_neg | fp16 caught |", "|---|---|---|---|---|---|---|---|"]
    for m in mutations:
        md.append(f"| {m['mutation']} | {m['what']} | " + " | ".join(
            f"{m[t]['ratio']:.2f} | {fmt(m[t]['rel_neg'], '.3f')} | {'yes' if m[t]['flagged'] else 'NO'}" for t in ("bf16", "fp16")) + " |")
    with open(os.path.join(ROOT, "profiles", "native_network.md"), "w") as f:
        f.write("\n".join(md) + "\n")


if __name__ == "__main__":
    main(sys.argv[1])
