"""tools/e2e_half_bench.py -- BASELINE configs[4] with the network in float32, bfloat16 and float16 (measurement tool).

What a 16-bit network gains on the end-to-end chain is a question about MIOpen's 16-bit convolutions and InstanceNorm
on this network as much as about this package, so it is MEASURED, not assumed: the three dtypes run over the same
images, boxes and detector maps as `bench_e2e.measure`, ALTERNATED inside one process and one call (`--rounds`
rounds; within a round fp32, bfloat16, float16 one after the other), and the spread over the rounds is printed next
to every median.  Legs, per dtype:

  infer_image    one image per pass, host clock around the call + a device synchronise, median over the 11 images
  infer_batch    eight images per pass (two different batches), median per batch
  infer_stream   the same batches with two in flight, wall clock over the sequence
  split          NOT part of the figures above (a synchronise between the halves costs time): preprocess + network +
                 decode launches | read-backs, merges, RoIRotate, head, CTC, strings -- per image and per batch of eight

The detector maps (the synthetic trained-detector maps of tests/e2e_inputs.py, in the network's dtype) are uploaded
and stacked per batch OUTSIDE the timers for every leg; every shape of every dtype is warmed up before the first
timed round (MIOpen picks its kernels per shape and dtype on first use).

Not timed: `text_agreement` -- the share of the 11 images' words (24 seeded boxes each, the same boxes for every dtype)
whose text in a 16-bit network equals the fp32 network's.  The weights are RANDOM (`deterministic_init`): the head's
arg-max sits on near-ties everywhere, so this share says nothing about the accuracy of a trained model in 16 bits; it
is recorded so that a later run with trained weights has something to be compared with.

Needs a GPU: there is no fallback.   python tools/e2e_half_bench.py [--rounds 3] [--out profiles/half_e2e.json]
`--profile DTYPE`: no figures -- after the warm-up, two untimed passes of the three legs in that dtype alone, for
`rocprofv3 --kernel-trace --stats -- python tools/e2e_half_bench.py --profile bfloat16` (a run of its own;
`--profile-legs image` restricts it to one leg).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "fots.pytorch_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

DTYPES = (("float32", torch.float32), ("bfloat16", torch.bfloat16), ("float16", torch.float16))
IMAGES_PER_BATCH = 8


def _spread(values, scale=1.0, digits=2):
    a = np.asarray(values, np.float64) * scale
    return {"median": round(float(np.median(a)), digits), "min": round(float(a.min()), digits),
            "max": round(float(a.max()), digits)}


def measure(device, rounds=3, stream_batches=6, channels_last=False, profile=None, profile_legs="image,batch,stream"):
    import bench_e2e as B
    from e2e_inputs import synthetic_boxes, synthetic_detector_maps
    from fots_e2e.alphabet import ALPHABET
    from fots_e2e.hostcpus import cap_torch_threads
    from fots_e2e.model import FOTSNet
    from fots_e2e.pipeline import (_batch_back, _batch_front, batched, infer_batch, infer_image, infer_stream, preprocess,
                                   resize_rule, target_widths_host)
    from fots_e2e.weights import deterministic_init
    from rroi_align.decode import CTCLabelConverter
    from rroi_align.nms import get_boxes
    host_threads = cap_torch_threads()
    conv = CTCLabelConverter(ALPHABET)
    ims, source = B.load_images()
    boxes = [synthetic_boxes(B.BOXES_PER_IMAGE, *resize_rule(im.shape[0], im.shape[1]), seed=100 + i) for i, im in enumerate(ims)]
    maps_np = [synthetic_detector_maps(704, 1280, B.BOXES_PER_IMAGE, seed=i) for i in range(len(ims))]
    order = [i % len(ims) for i in range(2 * IMAGES_PER_BATCH)]
    groups = [order[i:i + IMAGES_PER_BATCH] for i in range(0, len(order), IMAGES_PER_BATCH)]
    seq_groups = [k % len(groups) for k in range(stream_batches)]

    legs = {}
    for name, dtype in DTYPES:
        if profile not in (None, name):
            continue
        net = deterministic_init(FOTSNet(len(ALPHABET) + 1)).eval().to(device).to(dtype)
        if channels_last:
            net = net.to(memory_format=torch.channels_last)
        maps = [tuple(torch.from_numpy(a).to(device).to(dtype) for a in m) for m in maps_np]
        stacked = [tuple(torch.stack([maps[i][j] for i in g]) for j in range(3)) for g in groups]   # outside every timer
        legs[name] = dict(net=net, maps=maps, stacked=stacked, dtype=dtype)
    torch.cuda.synchronize(device)

    def leg_image(L):
        per = []
        for i, im in enumerate(ims):
            t0 = time.perf_counter()
            infer_image(L["net"], conv, im, detector=lambda _x, m=L["maps"][i]: m)
            torch.cuda.synchronize(device)
            per.append(time.perf_counter() - t0)
        return per

    def leg_batch(L):
        per = []
        for g, st in zip(groups, L["stacked"]):
            t0 = time.perf_counter()
            infer_batch(L["net"], conv, [ims[i] for i in g], detector=lambda _x, st=st: st)
            torch.cuda.synchronize(device)
            per.append(time.perf_counter() - t0)
        return per

    def leg_stream(L):
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        for _r in infer_stream(L["net"], conv, ([ims[i] for i in groups[k]] for k in seq_groups),
                               detector=lambda k, _x: L["stacked"][seq_groups[k]]):
            pass
        torch.cuda.synchronize(device)
        return time.perf_counter() - t0

    def split_image(L):
        front, back = [], []
        for i, im in enumerate(ims):
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            im_data = preprocess(im, device, L["dtype"])
            _, _, _, feats = L["net"](im_data)
            torch.cuda.synchronize(device)
            t1 = time.perf_counter()
            b = get_boxes(*L["maps"][i], 0.5)
            batched(L["net"], conv, feats, b, gw_host=target_widths_host(b))
            torch.cuda.synchronize(device)
            front.append(t1 - t0)
            back.append(time.perf_counter() - t1)
        return front, back

    def split_batch(L):
        front, back = [], []
        for g, st in zip(groups, L["stacked"]):
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            f = _batch_front(L["net"], [ims[i] for i in g], lambda _x, st=st: st, 0.5)
            torch.cuda.synchronize(device)
            t1 = time.perf_counter()
            _batch_back(L["net"], conv, f)
            torch.cuda.synchronize(device)
            front.append(t1 - t0)
            back.append(time.perf_counter() - t1)
        return front, back

    raw = {name: {"infer_image": [], "infer_batch": [], "infer_stream": [], "split_image": [], "split_batch": []} for name, _ in DTYPES}
    texts = {}
    with torch.no_grad():
        if profile is not None:
            L = legs[profile]
            fns = [{"image": leg_image, "batch": leg_batch, "stream": leg_stream}[x] for x in profile_legs.split(",")]
            from rroi_align._ext import rroi_align as ext
            mark = torch.zeros(4, device=device)
            for _pass in range(3):                   # the first pass is the warm-up (MIOpen tries kernels there) ...
                for fn in fns:
                    fn(L)
                if _pass != 1:                       # ... so the two measured passes sit between two MARKER launches:
                    ext.sincos_probe(mark)           # rroi_sincos_probe_kernel, which nothing in the pipeline launches
                    torch.cuda.synchronize(device)   # (tools/e2e_half_trace.py reads the trace between them)
            return {"profiled": profile, "legs": profile_legs, "passes": 3, "images": len(ims)}
        for name, _ in DTYPES:                       # warm-up: every shape of every dtype, the side stream included
            L = legs[name]
            leg_image(L)
            leg_batch(L)
            leg_stream(L)
            texts[name] = []
            for i, im in enumerate(ims):             # (also the text comparison: the same seeded boxes for every dtype)
                _, _, _, feats = L["net"](preprocess(im, device, L["dtype"]))
                texts[name] += batched(L["net"], conv, feats, boxes[i])
        for _round in range(rounds):
            for name, _ in DTYPES:                   # alternated: fp32, bfloat16, float16 within every round
                L = legs[name]
                per = leg_image(L)
                raw[name]["infer_image"].append(1.0 / float(np.median(per)))
                per = leg_batch(L)
                raw[name]["infer_batch"].append(IMAGES_PER_BATCH / float(np.median(per)))
                raw[name]["infer_stream"].append(IMAGES_PER_BATCH * len(seq_groups) / leg_stream(L))
                f, b = split_image(L)
                raw[name]["split_image"].append((float(np.median(f)), float(np.median(b))))
                f, b = split_batch(L)
                raw[name]["split_batch"].append((float(np.median(f)) / IMAGES_PER_BATCH, float(np.median(b)) / IMAGES_PER_BATCH))

    out = {"rounds": rounds, "images": source, "images_per_batch": IMAGES_PER_BATCH, "stream_batches": len(seq_groups),
           "host_threads": host_threads, "channels_last": bool(channels_last), "device": torch.cuda.get_device_name(device),
           "dtypes": {}}
    for name, _ in DTYPES:
        r = raw[name]
        d = {leg: {"images_per_s": _spread(r[leg]), "per_round": [round(v, 2) for v in r[leg]]}
             for leg in ("infer_image", "infer_batch", "infer_stream")}
        for leg in ("split_image", "split_batch"):
            a = np.asarray(r[leg])
            d[leg] = {"network_ms_per_image": _spread(a[:, 0], 1e3, 3), "recognition_ms_per_image": _spread(a[:, 1], 1e3, 3)}
        out["dtypes"][name] = d
    base = out["dtypes"]["float32"]
    out["ratio_to_float32"] = {
        name: {leg: round(out["dtypes"][name][leg]["images_per_s"]["median"] / base[leg]["images_per_s"]["median"], 3)
               for leg in ("infer_image", "infer_batch", "infer_stream")} for name, _ in DTYPES[1:]}
    nwords = len(texts["float32"])
    out["text_agreement"] = {
        "words": nwords,
        "same_text_as_float32": {name: round(sum(a == b for a, b in zip(texts[name], texts["float32"])) / max(1, nwords), 4)
                                 for name, _ in DTYPES[1:]},
        "note": "random weights: the share says nothing about the accuracy of a trained model in 16 bits"}
    out["what"] = ("configs[4] end to end with the network in three dtypes, alternated per round in one process: preprocess "
                   "+ FOTSNet + rroi_align.nms on injected synthetic detector maps (in the network's dtype, uploaded and stacked "
                   "outside the timers) + RoIRotate + CRNN head + greedy CTC + strings; host clock around work that ends in a "
                   "device synchronise; median (min, max) over the rounds")
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--stream-batches", type=int, default=6)
    ap.add_argument("--channels-last", action="store_true")
    ap.add_argument("--profile-legs", default="image,batch,stream", help="with --profile: which legs (image,batch,stream)")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    ap.add_argument("--profile", choices=[n for n, _ in DTYPES], default=None, help="untimed passes of one dtype, for rocprofv3")
    args = ap.parse_args()
    if args.rounds < 3:
        ap.error("--rounds must be at least 3: the spread over the rounds is part of the result")
    if not torch.cuda.is_available():
        raise SystemExit("e2e_half_bench: no GPU -- this tool measures on the device and has no fallback")
    out = measure(torch.device("cuda", 0), args.rounds, args.stream_batches, args.channels_last, args.profile, args.profile_legs)
    if args.profile:
        print(json.dumps(out))
        return
    for name, _ in DTYPES:
        d = out["dtypes"][name]
        print("%-9s" % name + "  ".join("%s %7.1f img/s (%.1f-%.1f)" % (leg, d[leg]["images_per_s"]["median"],
                                                                        d[leg]["images_per_s"]["min"], d[leg]["images_per_s"]["max"])
                                        for leg in ("infer_image", "infer_batch", "infer_stream")), file=sys.stderr)
    line = json.dumps(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
