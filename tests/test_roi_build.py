"""Callers' ROI construction: CPU checks of the restatement,
GPU parity of the device kernel, and the batched launch against per-box launches."""
import math

import numpy as np
import pytest
import torch

from oracle import roi_build_oracle as RB


def random_quads(n, seed=0, integer=False, size=(1280, 704)):
    """Rotated rectangles as 4 corner points, order 0..3 = bl, tl, tr, br of the text box as in
    rroi_align/test2.py:42-46 (edge 1->2 is the long 'width' edge, 0->1 the 'height' edge)."""
    rng = np.random.default_rng(seed)
    q = np.zeros((n, 4, 2))
    for i in range(n):
        cx, cy = rng.uniform(100, size[0] - 100), rng.uniform(100, size[1] - 100)
        h, w = rng.uniform(12, 60), rng.uniform(40, 400)
        a = rng.uniform(-80, 80) / 180 * math.pi
        ux, uy = math.cos(a), math.sin(a)        # along the text
        vx, vy = -math.sin(a), math.cos(a)       # down
        q[i, 0] = (cx - ux * w / 2 + vx * h / 2, cy - uy * w / 2 + vy * h / 2)
        q[i, 1] = (cx - ux * w / 2 - vx * h / 2, cy - uy * w / 2 - vy * h / 2)
        q[i, 2] = (cx + ux * w / 2 - vx * h / 2, cy + uy * w / 2 - vy * h / 2)
        q[i, 3] = (cx + ux * w / 2 + vx * h / 2, cy + uy * w / 2 + vy * h / 2)
    if integer:
        q = np.round(q)
    return q.reshape(n, 8).astype(np.float32)


def test_restatement_on_the_reference_demo_quad():
    """rroi_align/test2.py:43 quad gt2 -> the numbers its own code (test2.py:50-61) produces."""
    gt = np.asarray([[206, 111], [199, 95], [349, 60], [355, 80]], np.float32)
    rois, gw = RB.rois_from_quads(gt.reshape(1, 8), mode=1)
    center = gt.sum(0) / 4
    w = math.sqrt(150 ** 2 + 35 ** 2)
    h = math.sqrt(7 ** 2 + 16 ** 2)
    ang = -(math.atan2(-35, 150) + math.atan2(-31, 149)) / 2 / 3.1415926535 * 180
    want = np.asarray([0, center[0], center[1], h, w, ang], np.float64).astype(np.float32)
    assert np.array_equal(rois[0], want)
    # inference flavour: truncated centre, single-edge angle, width rule of ocr_utils.py:147-150
    r0, g0 = RB.rois_from_quads(gt.reshape(1, 8), mode=0)
    assert r0[0, 1] == 277.0 and r0[0, 2] == 86.0
    assert np.float32(-math.atan2(-35, 150) / 3.1415926535 * 180) == r0[0, 5]
    assert g0[0] == max(2, (int(w * (11 / h)) + 11) // 32) * 32 == 96


GOLD = __import__("os").path.join(__import__("os").path.dirname(__import__("os").path.abspath(__file__)), "golden", "roi_build.npz")


def test_restatement_equals_the_references_own_statements():
    """VERDICT r01 #6b: `tests/golden/roi_build.npz` holds what the reference's OWN lines
    (tools/ocr_utils.py:133-150, src/ocr_process.py:197-206 and :259-263, executed in place by
    `make_roi_golden.py`) compute for seeded quads: int() truncation of the centre, max(1, h), the
    // 32 rule, the double-precision ground-truth branch with its height jitter, the training
    width rule.  The restatement must reproduce every number, bit for bit."""
    z = np.load(GOLD)
    for tag in ("int", "real"):
        q = z["quads_" + tag]
        rois, gw = RB.rois_from_quads(q, mode=0)
        assert np.array_equal(rois, z["m0_rois_" + tag]) and np.array_equal(gw, z["m0_gw_" + tag])
        for j in (0, -2, 2):
            rois1, _ = RB.rois_from_quads(q[:64], mode=1, jitter=j)
            assert np.array_equal(rois1, z["m1_rois_%s_j%d" % (tag, j)])
            assert RB.train_pooled_width(rois1) == int(z["m1_pw_%s_j%d" % (tag, j)])


def test_pooled_width_rules():
    q = random_quads(64, seed=3)
    rois, gw = RB.rois_from_quads(q, mode=0)
    assert (gw % 32 == 0).all() and (gw >= 64).all()
    # the rule rounds DOWN to a multiple of 32: it may cut a crop (gw < roi_pooled_width = 11*w/h,
    # kernel.cu:68) but never by more than 32 - 11 columns
    rpw = 11 * rois[:, 4] / np.maximum(rois[:, 3], 1)
    assert (gw > rpw - 21).all() and ((gw == 64) | (gw <= rpw + 11)).all()
    assert RB.train_pooled_width(rois) == math.ceil(11 * float((rois[:, 4] / rois[:, 3]).max()))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1])
def test_device_roi_builder_matches_restatement(mode):
    from rroi_align._ext import rroi_align as ext
    for integer in (True, False):
        q = random_quads(2000, seed=11 + mode, integer=integer)
        bidx = (np.arange(2000) % 4).astype(np.float32)
        want, wgw = RB.rois_from_quads(q, bidx, mode=mode)
        got, ggw = ext.quads_to_rois(torch.from_numpy(q).cuda(), torch.from_numpy(bidx).cuda(), mode)
        got, ggw = got.cpu().numpy(), ggw.cpu().numpy()
        # fp64 sqrt is correctly rounded on both sides; atan2 comes from ocml on the device and from
        # glibc in the reference's Python -- both within an ulp of the DOUBLE result, which the
        # rounding of the angle to fp32 absorbs: every field bit-identical
        assert np.array_equal(got, want)
        assert np.array_equal(ggw, wgw)


@pytest.mark.gpu
def test_device_roi_builders_match_the_references_own_output():
    """The device kernels against `roi_build.npz` (the reference's own statements, see above)."""
    from rroi_align._ext import rroi_align as ext
    z = np.load(GOLD)
    for tag in ("int", "real"):
        q = torch.from_numpy(z["quads_" + tag]).cuda()
        got, ggw = ext.quads_to_rois(q, None, 0)
        assert np.array_equal(got.cpu().numpy(), z["m0_rois_" + tag])
        assert np.array_equal(ggw.cpu().numpy(), z["m0_gw_" + tag])
        for j in (0, -2, 2):
            jit = torch.full((64,), float(j), device="cuda")
            rois, ratio = ext.gt_quads_to_rois(q[:64], None, jit if j else None)
            want = z["m1_rois_%s_j%d" % (tag, j)]
            assert np.array_equal(rois.cpu().numpy(), want)
            assert math.ceil(11 * float(ratio.item())) == int(z["m1_pw_%s_j%d" % (tag, j)])


def same_bits(got, want):
    """fp32 arrays equal bit for bit (-0.0 is not 0.0), NaN for NaN."""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    nan = np.isnan(got) & np.isnan(want)
    return got.shape == want.shape and bool(((got.view(np.uint32) == want.view(np.uint32)) | nan).all())


def gt_boxes(n, seed):
    """n ground-truth quads with batch indices and the reference's integer height jitter, and their rows."""
    q = random_quads(n, seed=seed)
    bidx = (np.arange(n) % 3).astype(np.float32)
    jit = np.random.default_rng(seed).integers(-2, 3, n).astype(np.float32)
    return q, bidx, jit, RB.rois_from_quads(q, bidx, mode=1, jitter=jit)[0]


def with_box_at(q, bidx, jit, rows, pos, quad):
    """The same batch with `quad` (no jitter) at index pos -> (quads, jitter, rows)."""
    q, jit, rows = q.copy(), jit.copy(), rows.copy()
    q[pos], jit[pos] = quad, 0.0
    rows[pos] = RB.rois_from_quads(q[pos:pos + 1], bidx[pos:pos + 1], mode=1)[0][0]
    return q, jit, rows


@pytest.mark.gpu
@pytest.mark.parametrize("n", [255, 256, 257, 1000])
def test_gt_quads_to_rois_beyond_one_trip_of_the_block(n):
    """rroi_gt_quads_to_rois_kernel is ONE block of 256 threads that walks the boxes 256 at a time and reduces the
    largest w / h over threads: batches of 255, 256, 257 and 1000 boxes (the test above feeds it 64) with the largest
    ratio at index 0, 255, 256 and n - 1 in turn -- thread 0's first and second trip, thread 255's only one, the last
    box.  Every row bit for bit, the ratio the fp32 maximum of the rows' w / h, the pooled width the reference's."""
    from rroi_align._ext import rroi_align as ext
    q0, bidx, jit0, rows0 = gt_boxes(n, seed=100 + n)
    B = torch.from_numpy(bidx).cuda()
    wide = np.asarray([100, 104, 100, 100, 1300, 100, 1300, 104], np.float32)     # h = 4, w = 1200: w / h = 300
    assert float((rows0[:, 4] / rows0[:, 3]).max()) < 250
    for pos in sorted({0, 255, 256, n - 1}):
        if pos >= n:
            continue
        q, jit, want = with_box_at(q0, bidx, jit0, rows0, pos, wide)
        rois, ratio = ext.gt_quads_to_rois(torch.from_numpy(q).cuda(), B, torch.from_numpy(jit).cuda())
        assert same_bits(rois.cpu().numpy(), want), (n, pos)
        assert int(np.argmax(want[:, 4] / want[:, 3])) == pos
        assert same_bits(ratio.cpu().numpy(), (want[:, 4] / want[:, 3]).max().reshape(1)), (n, pos)
        assert math.ceil(11 * float(ratio.item())) == RB.train_pooled_width(want) == 3300, (n, pos)


@pytest.mark.gpu
def test_gt_quads_to_rois_nan_ratio_wins_at_any_position():
    """A box whose four corners coincide has w = h = 0: w / h = 0 / 0 is NaN, and NaN wins the maximum wherever the box
    stands (src/ocr_process.py:260-262 takes torch.max) -- also at an index only the block's second or third trip reads."""
    from rroi_align._ext import rroi_align as ext
    n = 600
    q0, bidx, jit0, rows0 = gt_boxes(n, seed=7)
    B = torch.from_numpy(bidx).cuda()
    point = np.asarray([300, 200] * 4, np.float32)
    rois, ratio = ext.gt_quads_to_rois(torch.from_numpy(q0).cuda(), B, torch.from_numpy(jit0).cuda())
    assert same_bits(rois.cpu().numpy(), rows0) and float(ratio.item()) == float((rows0[:, 4] / rows0[:, 3]).max())
    for pos in (0, 255, 256, 511, 512, n - 1):
        q, jit, want = with_box_at(q0, bidx, jit0, rows0, pos, point)
        assert want[pos, 3] == 0 and want[pos, 4] == 0
        with np.errstate(invalid="ignore"):
            assert np.isnan((want[:, 4] / want[:, 3]).max())
        rois, ratio = ext.gt_quads_to_rois(torch.from_numpy(q).cuda(), B, torch.from_numpy(jit).cuda())
        assert same_bits(rois.cpu().numpy(), want), pos
        assert math.isnan(float(ratio.item())), pos


def edge_quads():
    """Quads off the well-formed path of random_quads (corners 0..3 = bl, tl, tr, br; edge 1->2 is the width, 0->1 the
    height), every coordinate finite and at most 1e6 in magnitude -> ((n, 8) fp32, what each one is)."""
    z = -0.0
    rows = [
        # axis-aligned, the four orientations: atan2 sees exact zeros, and +-180 degrees where edge 1->2 points to -x
        ("upright", [10, 50, 10, 30, 210, 30, 210, 50]),
        ("quarter turn", [50, 10, 70, 10, 70, 210, 50, 210]),
        ("upside down: atan2(+0, -200)", [210, 30, 210, 50, 10, 50, 10, 30]),
        ("three quarter turn", [70, 210, 50, 210, 50, 10, 70, 10]),
        ("upside down on the x axis: atan2(-0, -200)", [210, -20, 210, 0.0, 10, z, 10, -20]),
        ("upright on the x axis: atan2(-0, +200)", [10, 20, 10, 0.0, 210, z, 210, 20]),
        ("quarter turn on the y axis: atan2(+200, -0)", [20, 10, 0.0, 10, z, 210, 20, 210]),
        # edges of zero length
        ("h == 0", [10, 30, 10, 30, 210, 30, 210, 30]),
        ("w == 0", [10, 50, 10, 30, 10, 30, 10, 50]),
        ("a point", [33, 44, 33, 44, 33, 44, 33, 44]),
        ("h == 0, long: t = 11 w + 11", [0, 7, 0, 7, 30000, 7, 30000, 7]),
        # h < 1: max(1, h)
        ("h = 0.5", [10, 30.5, 10, 30, 90, 30, 90, 30.5]),
        ("h = 0.25, rotated", [10, 30, 10.15, 29.8, 90.15, 89.8, 90, 90]),
        # t // 32 < 2: the floor of 64
        ("w / h = 1", [10, 50, 10, 30, 30, 30, 30, 50]),
        ("t = 63", [0, 11, 0, 0, 52.5, 0, 52.5, 11]),
        ("t = 64", [0, 11, 0, 0, 53, 0, 53, 11]),
        ("w < h", [100, 300, 100, 100, 140, 100, 140, 300]),
        # centres at negative coordinates: int() truncates toward zero, floor does not
        ("centre (-3.75, -0.5)", [-14, 5, -14, -6, 6.5, -6, 6.5, 5]),
        ("centre (-100.25, -7.75)", [-200.5, 2, -200.5, -17.5, 0, -17.5, 0, 2]),
        ("centre (-0.25, 0.75)", [-10, 1, -10, 0, 9, 1, 10, 1]),
        ("far out", [-999000.5, -998000, -999000.5, -998040, -998000, -998040.25, -998000, -998000]),
        ("far out, positive", [999000, 998000, 999000, 997960, 1000000, 997960, 1000000, 998000.5]),
        # mode 1: the angles of edges 1->2 and 0->3 on either side of +-180 degrees
        ("straddle, 1->2 above", [210, 50, 210, 30, 10, 31, 10, 49]),
        ("straddle, 1->2 below", [210, 50, 210, 30, 10, 29, 10, 51]),
        ("straddle, one edge exactly 180", [210, 50, 210, 30, 10, 30, 10, 49]),
        ("straddle, one edge exactly -180", [210, -20, 210, 0.0, 10, z, 10, -19]),
    ]
    q = np.asarray([r[1] for r in rows], np.float32)
    assert np.isfinite(q).all() and np.abs(q).max() <= 1e6
    return q, [r[0] for r in rows]


def test_edge_quads_reach_their_arms():
    """CPU: the restatement takes on edge_quads() the arms the device test below is about."""
    q, names = edge_quads()
    r0, g0 = RB.rois_from_quads(q, mode=0)
    r1, _ = RB.rois_from_quads(q, mode=1)
    assert {-180.0, 180.0, 90.0, -90.0} <= set(r0[:, 5].tolist()) and (np.signbit(r0[:, 5]) & (r0[:, 5] == 0)).any()
    assert (r0[:, 3] == 0).sum() >= 3 and (r0[:, 4] == 0).sum() >= 2 and ((r0[:, 3] > 0) & (r0[:, 3] < 1)).sum() >= 2
    by = dict(zip(names, range(len(names))))
    assert g0[by["t = 63"]] == 64 and g0[by["t = 64"]] == 64 and g0[by["w / h = 1"]] == 64 and g0.max() > 300000
    assert r0[by["centre (-3.75, -0.5)"], 1:3].tolist() == [-3.0, 0.0] and r1[by["centre (-3.75, -0.5)"], 1:3].tolist() == [-3.75, -0.5]
    assert r0[by["centre (-100.25, -7.75)"], 1:3].tolist() == [-100.0, -7.0]
    for k in ("straddle, 1->2 above", "straddle, 1->2 below"):     # the mean of two angles near +180 and -180 is near 0
        assert abs(r0[by[k], 5]) > 179 and abs(r1[by[k], 5]) < 1
    assert abs(r1[by["straddle, one edge exactly 180"], 5]) < 1 and abs(r1[by["straddle, one edge exactly -180"], 5]) < 1


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1])
def test_device_roi_builder_on_edge_quads(mode):
    """rroi_quads_to_rois_kernel on edge_quads(), with per-quad batch indices: rows and pooled widths bit for bit."""
    from rroi_align._ext import rroi_align as ext
    q, names = edge_quads()
    bidx = (np.arange(len(q)) % 5).astype(np.float32)
    want, wgw = RB.rois_from_quads(q, bidx, mode=mode)
    got, ggw = ext.quads_to_rois(torch.from_numpy(q).cuda(), torch.from_numpy(bidx).cuda(), mode)
    got, ggw = got.cpu().numpy(), ggw.cpu().numpy()
    for i, name in enumerate(names):
        assert same_bits(got[i], want[i]), (name, got[i].tolist(), want[i].tolist())
        assert ggw[i] == wgw[i], (name, int(ggw[i]), int(wgw[i]))


@pytest.mark.gpu
def test_ground_truth_module_and_degenerate_jitter(oracle):
    """src/ocr_process.py:196-221, :253-267 through `GroundTruthRRoiAlign`: crops equal the oracle on
    the module's rows and width; a jitter that drives h negative gives all-zero crops (the op's mask,
    kernel.cu:107); h == 0 raises, as the reference's math.ceil(inf) does."""
    from rroi_align.batched import GroundTruthRRoiAlign
    rng = np.random.default_rng(9)
    feats_np = rng.standard_normal((2, 64, 120, 160), dtype=np.float32)
    feats = torch.from_numpy(feats_np).cuda()
    q = random_quads(40, seed=13, size=(640, 480))
    q[3] = np.asarray([100, 101, 100, 100, 160, 100, 160, 101], np.float32)   # h = 1: jitter -2 -> h = -1
    bidx = (np.arange(40) % 2).astype(np.float32)
    jit = np.where(np.arange(40) == 3, -2.0, 1.0).astype(np.float32)
    m = GroundTruthRRoiAlign(11, 0.25)
    crops, rois = m(feats, torch.from_numpy(q).cuda(), torch.from_numpy(bidx).cuda(), torch.from_numpy(jit).cuda())
    want_rois, _ = RB.rois_from_quads(q[:32], bidx[:32], mode=1, jitter=jit[:32])
    assert np.array_equal(rois.cpu().numpy(), want_rois) and rois.shape[0] == 32  # :253-255 keeps 32 rows
    pw = RB.train_pooled_width(want_rois)
    assert crops.shape == (32, 64, 11, pw)
    assert np.array_equal(crops.cpu().numpy(), oracle.forward_c(feats_np, want_rois, 11, pw, 0.25, threads=8))
    assert want_rois[3, 3] == -1.0 and not crops[3].any()
    jit[3] = -1.0                                                              # h == 0 -> w / h = inf
    with pytest.raises(ValueError):
        m(feats, torch.from_numpy(q).cuda(), torch.from_numpy(bidx).cuda(), torch.from_numpy(jit).cuda())
    # the reference's own order -- filter ('##' labels, boxes that leave the image, :212-219),
    # THEN keep 32 rows (:253-255) -- and its one jitter draw PER IMAGE (:204), looked up through batch_index
    keep = np.ones(40, bool)
    keep[[0, 3, 5, 17]] = False
    per_image = np.asarray([2.0, -1.0], np.float32)
    crops2, rois2 = m(feats, torch.from_numpy(q).cuda(), torch.from_numpy(bidx).cuda(), torch.from_numpy(per_image).cuda(),
                      keep=torch.from_numpy(keep).cuda())
    want2, _ = RB.rois_from_quads(q[keep][:32], bidx[keep][:32], mode=1, jitter=per_image[bidx.astype(int)][keep][:32])
    assert np.array_equal(rois2.cpu().numpy(), want2) and rois2.shape[0] == 32
    pw2 = RB.train_pooled_width(want2)
    assert np.array_equal(crops2.cpu().numpy(), oracle.forward_c(feats_np, want2, 11, pw2, 0.25, threads=8))
    # as many boxes as images -- the length alone cannot decide: per box by default, with a warning.  Two boxes, both of image 1:
    # read per image the jitter of both is per_image[1], read per box it is per_image[0] and per_image[1]
    q2, b2 = q[[10, 11]], np.asarray([1.0, 1.0], np.float32)
    args = (feats, torch.from_numpy(q2).cuda(), torch.from_numpy(b2).cuda(), torch.from_numpy(per_image).cuda())
    import rroi_align.batched as _B
    _B._warned_ambiguous_jitter = False
    with pytest.warns(UserWarning, match="per BOX"):     # the per-box default stays, with one warning
        _, r_default = m(*args)
    _, r_img = m(*args, per_image_jitter=True)
    _, r_box = m(*args, per_image_jitter=False)
    assert np.array_equal(r_img.cpu().numpy(), RB.rois_from_quads(q2, b2, mode=1, jitter=per_image[[1, 1]])[0])
    assert np.array_equal(r_box.cpu().numpy(), RB.rois_from_quads(q2, b2, mode=1, jitter=per_image)[0])
    assert not np.array_equal(r_img.cpu().numpy(), r_box.cpu().numpy())
    assert np.array_equal(r_default.cpu().numpy(), r_box.cpu().numpy())


@pytest.mark.gpu
def test_callers_follow_the_features_layout():
    """Round 5: the two callers' modules hand the crops over in the FEATURES' layout by default
    -- channels_last features give channels_last crops (same values, element for element), autograd brings the
    gradient back channels_last and the feature gradient is written channels_last in place: no copy on either side.
    NCHW features keep the reference's contract.  True / False force the layout."""
    from rroi_align.batched import BatchedRRoiAlign, GroundTruthRRoiAlign
    rng = np.random.default_rng(21)
    f = rng.standard_normal((2, 64, 60, 80), dtype=np.float32)
    q = torch.from_numpy(random_quads(24, seed=5, size=(320, 240))).cuda()
    b = torch.from_numpy((np.arange(24) % 2).astype(np.float32)).cuda()
    res = {}
    for tag, fmt in (("nchw", torch.contiguous_format), ("cl", torch.channels_last)):
        F = torch.from_numpy(f).cuda().contiguous(memory_format=fmt).requires_grad_(True)
        crops, rois = GroundTruthRRoiAlign(11, 0.25)(F, q, b)
        assert crops.is_contiguous(memory_format=fmt), tag
        (crops * crops).sum().backward()
        assert F.grad.is_contiguous(memory_format=fmt), tag
        res[tag] = (crops.detach().clone(), F.grad.detach().clone())
        c2, gw = BatchedRRoiAlign(11, 0.25, pooled_width=96)(F.detach(), q[:, :8], b)
        assert c2.is_contiguous(memory_format=fmt), tag
    assert torch.equal(res["nchw"][0], res["cl"][0])
    scale = max(1.0, float(res["nchw"][1].abs().max()))
    assert float((res["nchw"][1] - res["cl"][1]).abs().max()) <= 1e-4 * scale
    Fc = torch.from_numpy(f).cuda().contiguous(memory_format=torch.channels_last)
    forced, _ = GroundTruthRRoiAlign(11, 0.25, channels_last_out=False)(Fc, q, b)
    assert forced.is_contiguous() and torch.equal(forced, res["nchw"][0])


@pytest.mark.gpu
def test_batched_launch_equals_per_box_launches(oracle):
    """One launch for all boxes of an image == the reference's loop of R = 1 launches
    (tools/ocr_utils.py:147-177): identical on each box's own width target_gw[i].  Beyond it the
    batched crop continues up to the box's roi_pooled_width (the per-box width rounds down to a
    multiple of 32 and may cut the word) and is zero after that (kernel.cu:107)."""
    from rroi_align.batched import BatchedRRoiAlign
    from rroi_align.modules.rroi_align import _RRoiAlign
    rng = np.random.default_rng(5)
    feats_np = rng.standard_normal((1, 64, 176, 320), dtype=np.float32)   # focr: 64 ch at 1/4 of 1280x704
    feats = torch.from_numpy(feats_np).cuda()
    q = random_quads(24, seed=7)
    crops, gw = BatchedRRoiAlign(11, 1.0 / 4)(feats, torch.from_numpy(q).cuda())
    rois, wgw = RB.rois_from_quads(q, mode=0)
    assert crops.shape == (24, 64, 11, int(wgw.max()))
    for i in range(24):
        single = _RRoiAlign(11, int(wgw[i]), 1.0 / 4)(feats, torch.from_numpy(rois[i:i + 1]).cuda())
        assert torch.equal(crops[i:i + 1, :, :, :int(wgw[i])], single)
        rpw = 11 * rois[i, 4] / rois[i, 3]
        assert not crops[i, :, :, int(math.floor(rpw)) + 1:].any()
    # and against the oracle, element for element
    want = oracle.forward_c(feats_np, rois, 11, int(wgw.max()), 0.25, threads=4)
    assert np.array_equal(crops.cpu().numpy(), want)
