"""detection post-processing.

CPU: the restatement (oracle/nms_oracle.py) and the product's host merge (`rroi_nms_merge_host`,
a host-only entry point of the library) against `tests/golden/nms_cases.npz` -- boxes computed by
the reference's OWN nms/ sources (make_nms_golden.py) on seeded detector maps, the 11 example-image
sized ones included.  GPU: the device decode bit for bit on the quads, and `get_boxes` end to end."""
import os
import zlib

import numpy as np
import pytest

from nms_cases import CASES, NUM_HARD, hard_case, hard_maps, quad_class, synth_maps
from oracle import nms_oracle as NO

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nms_cases.npz")


def _inputs(case, z):
    name, (h, w), words, seed, noise = case
    segm, geo, ang = synth_maps(h, w, words, seed, noise)
    assert zlib.crc32(segm.tobytes() + geo.tobytes() + ang.tobytes()) == int(z[name + "_crc"]), "generator drifted"
    return name, segm, geo, ang


def _records(polys):
    from rroi_align.nms import CANDIDATE
    rec = np.zeros(len(polys), CANDIDATE)
    for i, p in enumerate(polys):
        rec[i]["quad"] = np.asarray(p["poly"], np.int64).reshape(8)
        rec[i]["score"], rec[i]["rdist"], rec[i]["x"], rec[i]["y"] = p["score"], p["rdist"], p["x"], p["y"]
    return rec


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_oracle_and_host_merge_equal_the_references_own_nms(case):
    """Both reproduce every box the reference's build returns -- coordinates and scores bit for bit
    (the polygon intersection differs from Clipper's only below fp32 resolution of the areas)."""
    from rroi_align.nms import merge
    z = np.load(GOLD)
    name, segm, geo, ang = _inputs(case, z)
    want = z[name + "_boxes"]
    if segm.size <= 96 * 64:                       # the pure-Python restatement: small maps only
        assert np.array_equal(NO.get_boxes(segm, geo, ang, 0.5), want)
    polys = NO.decode(segm, geo, ang.swapaxes(0, 1).swapaxes(1, 2), 0.5)
    assert len(polys) == int(z[name + "_pixels"])
    got = merge(_records(polys), segm.shape[1], segm.shape[0])
    assert got.shape == want.shape and np.array_equal(got, want)


def _reference_adaptor():
    """The reference's own nms extension, built by `make -C oracle ref` (oracle/_ref travels as a binary)."""
    import importlib
    import sys
    d = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "nms_ref")
    if not os.path.exists(os.path.join(d, "adaptor.so")):
        if os.path.isdir("/root/reference"):
            pytest.fail("oracle/_ref/nms_ref/adaptor.so is not built although /root/reference is here: `make -C oracle ref`")
        pytest.skip("oracle/_ref/nms_ref not built")
    if d not in sys.path:
        sys.path.insert(0, d)
    return importlib.import_module("adaptor")


def test_host_merge_equals_reference_build_on_random_maps():
    """Beyond the frozen cases: 60 more seeded detector maps (different sizes, word counts, noise
    levels, thresholds), the product's host merge against the reference's own build run on the spot."""
    from rroi_align.nms import merge
    adaptor = _reference_adaptor()
    rng = np.random.default_rng(123)
    for trial in range(60):
        h, w = int(rng.integers(24, 96)), int(rng.integers(40, 160))
        segm, geo, ang = synth_maps(h, w, int(rng.integers(1, 9)), 1000 + trial, float(rng.uniform(0, 0.4)))
        thr = float(rng.choice([0.5, 0.65, 0.8]))
        a_hw2 = np.ascontiguousarray(ang.swapaxes(0, 1).swapaxes(1, 2))
        want = np.array(adaptor.do_nms(segm, geo, a_hw2, np.full((h, w), -1, np.int32), 0.4, 0.2, thr), dtype="float32").reshape(-1, 9)
        if len(want):
            want[:, :8] /= 10000
        got = merge(_records(NO.decode(segm, geo, a_hw2, thr)), w, h)
        assert got.shape == want.shape and np.array_equal(got, want), (trial, h, w, thr)


def test_hard_cases_non_convex_and_self_intersecting_quads():
    """the reference intersects / unions arbitrary paths with Clipper (pftEvenOdd,
    nms.h:24-36), and merged quads -- per-coordinate weighted means with different weights for X and Y,
    nms.h:87-96 -- need not stay convex or simple.  32 frozen maps built to get there (heavy noise, words
    on top of each other at other angles, thresholds 0.3 ... 0.9; the reference's own build returned 7
    concave and 19 self-intersecting boxes for them): the product's host merge reproduces every box bit for
    bit, and so does the restatement on the small ones.  Round 2's Sutherland-Hodgman clipper failed 21 %
    of such maps (tools/fuzz_nms.py: 63 of 300)."""
    from rroi_align.nms import merge
    z = np.load(GOLD)
    shapes = [0, 0, 0]
    for i in range(NUM_HARD):
        segm, geo, ang, thr, iou1, iou2 = hard_case(i)
        assert zlib.crc32(segm.tobytes() + geo.tobytes() + ang.tobytes()) == int(z["hard%d_crc" % i]), "generator drifted"
        want = z["hard%d_boxes" % i]
        a_hw2 = ang.swapaxes(0, 1).swapaxes(1, 2)
        polys = NO.decode(segm, geo, a_hw2, thr)
        got = merge(_records(polys), segm.shape[1], segm.shape[0], iou1, iou2)
        assert got.shape == want.shape and np.array_equal(got, want), i
        if len(polys) <= 400:                       # the pure-Python restatement: small candidate lists only
            ref = NO.merge_iou(polys, segm.shape[1], segm.shape[0], iou1, iou2)
            mine = np.array([[c for v in p["poly"] for c in v] + [p["score"]] for p in ref], np.float32).reshape(-1, 9)
            mine[:, :8] /= 10000                    # in fp32, as nms/__init__.py:27 does
            assert np.array_equal(mine, want), i
        for b in want:
            shapes[quad_class(b[:8])] += 1
    assert shapes[1] >= 5 and shapes[2] >= 10, shapes   # the hard cases were reached


def test_host_merge_equals_reference_build_on_hard_random_maps():
    """The same live: 250 more hard maps against the reference's own build run on the spot."""
    from rroi_align.nms import merge
    adaptor = _reference_adaptor()
    rng = np.random.default_rng(2024)
    odd = 0
    for trial in range(250):
        h, w = int(rng.integers(16, 72)), int(rng.integers(24, 120))
        noise = float(rng.choice([0.0, 0.2, 0.5, 1.0, 2.0]))
        thr = float(rng.choice([0.3, 0.5, 0.7, 0.9]))
        iou1, iou2 = float(rng.choice([0.1, 0.3, 0.4, 0.6])), float(rng.choice([0.05, 0.2, 0.5]))
        segm, geo, ang = hard_maps(h, w, int(rng.integers(1, 10)), rng, noise, float(rng.choice([0.0, 0.5, 0.9])))
        a_hw2 = np.ascontiguousarray(ang.swapaxes(0, 1).swapaxes(1, 2))
        want = np.array(adaptor.do_nms(segm, geo, a_hw2, np.full((h, w), -1, np.int32), iou1, iou2, thr), dtype="float32").reshape(-1, 9)
        if len(want):
            want[:, :8] /= 10000
        got = merge(_records(NO.decode(segm, geo, a_hw2, thr)), w, h, iou1, iou2)
        assert got.shape == want.shape and np.array_equal(got, want), (trial, h, w, noise, thr, iou1, iou2)
        odd += sum(quad_class(b[:8]) > 0 for b in want)
    assert odd >= 50, odd


def test_merge_statement_quirks():
    """nms.h:198/:201 append an unmerged polygon twice; standard_nms then folds the twins."""
    from rroi_align.nms import merge
    seg, geo, ang = synth_maps(32, 48, 1, 3)
    polys = NO.decode(seg, geo, ang.swapaxes(0, 1).swapaxes(1, 2), 0.5)
    far = dict(polys[0], poly=[[v[0] + 3000000, v[1] + 3000000] for v in polys[0]["poly"]], x=40, y=30)
    boxes = merge(_records([polys[0], far]), 48, 32)
    ref = NO.merge_iou([polys[0], far], 48, 32, 0.4, 0.2)
    assert len(boxes) == len(ref) == 2
    # the second polygon was appended twice and merged with its twin: score doubled
    assert sorted(boxes[:, 8]) == sorted(float(p["score"]) for p in ref)
    assert np.isclose(boxes[:, 8].max(), 2 * float(far["score"]))
    with pytest.raises(ValueError):
        merge(_records([dict(polys[0], x=99)]), 48, 32)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES[::2], ids=[c[0] for c in CASES[::2]])
def test_device_decode_and_get_boxes(case):
    import torch
    from rroi_align import nms as N
    z = np.load(GOLD)
    name, segm, geo, ang = _inputs(case, z)
    dev = torch.device("cuda", 0)
    S, G, A = torch.from_numpy(segm).to(dev), torch.from_numpy(geo.transpose(2, 0, 1).copy()).to(dev), torch.from_numpy(ang).to(dev)
    rec, cnt = N.decode(S, G, A, 0.5)
    n = int(cnt.item())
    got = rec[:n].cpu().numpy().view(N.CANDIDATE).reshape(-1)
    want = _records(NO.decode(segm, geo, ang.swapaxes(0, 1).swapaxes(1, 2), 0.5))
    assert n == len(want) == int(z[name + "_pixels"])
    # raster order; quads, scores and the raw RBOX distances bit for bit (the record carries r[0..3], round 4)
    for f in ("quad", "score", "rdist", "x", "y"):
        assert np.array_equal(got[f], want[f]), f
    # ... so the host merge, which forms expf(-r / 9) with the C library as adaptor.cpp:97-100 does, returns the
    # boxes of the reference's own build bit for bit (rounds 2-3: exp in double on the device, 2e-3 px)
    boxes = N.get_boxes(S, G, A, 0.5)
    ref = z[name + "_boxes"]
    assert boxes.shape == ref.shape and np.array_equal(boxes, ref)
    # the reference's call-site layout (numpy, rbox as (h, w, 4)) gives the same boxes
    assert np.array_equal(N.get_boxes(segm, geo, ang, 0.5), boxes)


@pytest.mark.gpu
def many_workgroup_maps(h, w):
    """Seeded detector maps of test_device_decode_is_ordered_over_many_workgroups: ~4 % of the pixels pass 0.5."""
    rng = np.random.default_rng(h * 1000 + w)
    segm = (rng.random((h, w)) * 0.52).astype(np.float32)
    geo = rng.uniform(0, 12, (h, w, 4)).astype(np.float32)
    a = rng.uniform(-1.5, 1.5, (h, w))
    ang = np.stack([np.sin(a), np.cos(a)]).astype(np.float32)
    return rng, segm, geo, ang


def passing_on_both_sides_of_slab_1024(mask):
    """A slab is 1024 pixels in raster order and one workgroup; workgroup i sums slab_counts[0 .. i) 1024 at a time, so
    the workgroups of slabs 1025 and above take a second trip.  True if pixels pass in slabs 0 .. 1023 AND in 1025 ..."""
    flat = np.asarray(mask).reshape(-1)
    return bool(flat[:1024 * 1024].any() and flat[1025 * 1024:].any())


def test_the_1030_slab_map_passes_pixels_on_both_sides_of_slab_1024():
    """CPU: the regime of the (1030, 1024) decode case below, without a GPU."""
    h, w = 1030, 1024
    _, segm, _, _ = many_workgroup_maps(h, w)
    assert (h * w + 1023) // 1024 == 1030
    mask = segm > 0.5
    assert passing_on_both_sides_of_slab_1024(mask)
    assert 0.03 < mask.mean() < 0.05
    assert not passing_on_both_sides_of_slab_1024(many_workgroup_maps(600, 610)[1] > 0.5)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(40, 70), (176, 320), (600, 610), (1030, 1024)])
def test_device_decode_is_ordered_over_many_workgroups(shape):
    """Round 3: the decode runs one workgroup per 1024 pixels (round 2: one workgroup for the whole map);
    the records still come out in raster order -- the merge depends on it -- also on a map large enough
    (> 262144 pixels) for the two-launch path with per-slab counts, and on one of 1030 slabs, where the workgroups of
    slabs 1025 .. 1029 take a second trip through the loop that sums the counts of the slabs before theirs."""
    import torch
    from rroi_align import nms as N
    h, w = shape
    rng, segm, geo, ang = many_workgroup_maps(h, w)              # ~4 % of the pixels pass
    if h * w > 1025 * 1024:
        assert passing_on_both_sides_of_slab_1024(segm > 0.5)
    dev = torch.device("cuda", 0)
    S, G, A = torch.from_numpy(segm).to(dev), torch.from_numpy(geo.transpose(2, 0, 1).copy()).to(dev), torch.from_numpy(ang).to(dev)
    rec, cnt = N.decode(S, G, A, 0.5)
    n = int(cnt.item())
    ys, xs = np.nonzero(segm > 0.5)                                # raster order
    assert n == len(ys) > 0
    got = rec[:n].cpu().numpy().view(N.CANDIDATE).reshape(-1)
    assert np.array_equal(got["y"], ys) and np.array_equal(got["x"], xs)
    assert np.array_equal(got["score"], segm[ys, xs])
    # quads of a sample of the records against the restatement
    sub = np.zeros_like(segm)
    pick = rng.choice(n, min(n, 300), replace=False)
    sub[ys[pick], xs[pick]] = segm[ys[pick], xs[pick]]
    want = _records(NO.decode(sub, geo, ang.swapaxes(0, 1).swapaxes(1, 2), 0.5))
    sel = np.sort(pick)
    assert np.array_equal(got["quad"][sel], want["quad"])
    assert np.array_equal(got["rdist"][sel], want["rdist"])


@pytest.mark.gpu
def test_device_decode_large_map_with_a_small_record_buffer():
    """a map beyond 262144 pixels with a buffer of fewer than h * w + counts records is served (the
    one-launch form, every workgroup counting the pixels before its slab), not refused: *count reports all passing
    pixels, the first `capacity` records are written in raster order and nothing beyond them."""
    import torch
    from rroi_align import nms as N
    from rroi_align._ext import rroi_align as ext
    h, w = 600, 610
    rng = np.random.default_rng(5)
    segm = (rng.random((h, w)) * 0.51).astype(np.float32)        # ~2 % of the pixels pass
    geo = rng.uniform(0, 12, (4, h, w)).astype(np.float32)
    ang = rng.uniform(-1, 1, (2, h, w)).astype(np.float32)
    dev = torch.device("cuda", 0)
    S, G, A = (torch.from_numpy(a).to(dev) for a in (segm, geo, ang))
    ys, xs = np.nonzero(segm > 0.5)
    full, cnt_full = N.decode(S, G, A, 0.5)
    n = int(cnt_full.item())
    assert n == len(ys)
    full = full[:n].cpu().numpy().view(N.CANDIDATE).reshape(-1)
    for cap in (h * w, n + 7, n // 3, 0):
        rec = torch.full((cap + 2, 64), 0xAB, dtype=torch.uint8, device=dev)
        cnt = torch.zeros((1,), dtype=torch.int32, device=dev)
        st = ext._lib.rroi_rbox_decode_hip(S.data_ptr(), G.data_ptr(), A.data_ptr(), h, w, 0.5, rec.data_ptr(), cap,
                                           cnt.data_ptr(), ext._stream())
        assert st == 1, (cap, st)
        assert int(cnt.item()) == n
        k = min(cap, n)
        got = rec[:k].cpu().numpy().view(N.CANDIDATE).reshape(-1)
        assert np.array_equal(got, full[:k]), cap
        assert (rec[max(k, cap):].cpu().numpy() == 0xAB).all(), cap      # nothing behind the caller's records
