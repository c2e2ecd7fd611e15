"""GPU (MI355X): the caller-owned workspace -- bounds, stale contents, base address (DESIGN "workspace contract").

Every row of tests/workspace_cases.py runs through the raw C ABI (never ext.forward / ext.backward: their per-stream
cache hands every call a buffer far larger than it asked for) inside one uint8 device buffer

    [ guard 1 MiB | slack: up to 4 KiB + offset | workspace: EXACTLY the bytes the size query returned | guard 1 MiB ]

whose workspace starts `offset` bytes after a 4 KiB boundary.  The whole buffer is poisoned before the call and the
output is pre-filled with a NaN pattern no finite input produces.  A row runs 4 poisons x 4 offsets:

    poisons   0xFF (fp32 NaN, counters at -1), 0x00, 0x7F (3.4e38, huge positive counters), and the buffer as the
              PREVIOUS row of the table left it (that row is run first, into the same buffer, and nothing is refilled)
    offsets   0, 256, 2304, 3840: carve_bwd's first rounding to 4 KiB of the address adds a different amount at each (the
              second starts from a page boundary: it varies with the row, not with the offset)

and every call must (a) leave every byte outside [base, base + nbytes) as it was -- compared on the device, both guards
whole -- and also the tail of a backward workspace behind its last sub-array (the size holds a flat 8192 bytes for the
two roundings, which add less; workspace_cases.backward_used_bytes restates the carve on the host), so that an overrun
of the last array by one line shows; and (b, c) give the project's own result: the forward the oracle's bits, the ORDERED backward
oracle.backward_c's bits (16-bit: rounded once), the other backward plans within workloads.check_backward_elementwise
(16-bit: test_gpu_half.check_half_backward); forward and ORDERED results are also bit-identical across the 16 calls.
The LISTS plan is not asserted to repeat its bits: it hands out list slots with integer atomics, so the order it sums a
pixel's list in depends on scheduling -- two plain calls are not promised the same bits either.

Then: the size and pointer checks of every entry-point family (one byte short, NULL: 0 and nothing launched; 4 KiB more:
the same bits), the plans that take no workspace (NULL / 0 accepted; a workspace that is handed over stays untouched),
the two stages of the forward run as two calls on one arena, and -- last -- coverage over what actually ran.

Every call uses real device buffers of full size; no pointer is fabricated here."""
import numpy as np
import pytest
import torch

import plan_cases as PC
import workloads as Wk
import workspace_cases as WC
from test_gpu_bucketed import NAN_PATTERN
from test_gpu_half import check_half_backward
from test_gpu_plan_coverage import distinct_bins_per_pixel

pytestmark = pytest.mark.gpu

GUARD = 1 << 20
PAGE = 4096
OFFSETS = WC.OFFSETS
POISONS = (0xFF, 0x00, 0x7F, "left")
FULL = [(p, o) for p in POISONS for o in OFFSETS]
DIAGONAL = list(zip(POISONS, OFFSETS))
# rows that run the diagonal of poison x offset (4 calls) instead of all 16: for a row whose 16 calls take more than
# about 5 s on the MI355X; its shape stays
DIAGONAL_ROWS = ()
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
RAN = {"fp32": set(), "bf16": set(), "fp16": set(), "bucketed": set(), "none": set(), "stages": set(), "checks": set()}


@pytest.fixture(scope="module")
def ext():
    from rroi_align._ext import rroi_align as e
    return e


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def stream():
    return torch.cuda.current_stream().cuda_stream


def itype(dtype):
    return torch.int32 if dtype == torch.float32 else torch.int16


# ---------------------------------------------------------------- the arena
class Arena:
    """One uint8 device buffer; place() puts a workspace of nbytes `offset` bytes after the first 4 KiB boundary behind
    the leading guard.  The checked buffer of a call is buf[:end] = guard | slack | workspace | guard."""

    def __init__(self, nbytes):
        self.buf = torch.empty(GUARD + 2 * PAGE + nbytes + GUARD, dtype=torch.uint8, device="cuda")

    def place(self, nbytes, offset):
        p = self.buf.data_ptr()
        lo = ((p + GUARD + PAGE - 1) & ~(PAGE - 1)) + offset - p
        hi = lo + nbytes
        end = hi + GUARD
        assert offset < PAGE and lo >= GUARD and end <= self.buf.numel()
        assert (p + lo) % 256 == 0 and (p + lo) % PAGE == offset
        return lo, hi, end

    def untouched(self, src, spans, what, lo, hi):
        """Every byte of the spans still equals `src` (a poison byte, or a snapshot of the buffer)."""
        for a, b in spans:
            seg = self.buf[a:b]
            same = (seg == src) if isinstance(src, int) else (seg == src[a:b])
            if not bool(same.all()):
                i = int((~same).nonzero()[0]) + a
                n = int((~same).sum())
                pytest.fail(f"{what}: {n} bytes outside the workspace changed; the first at workspace end {i - hi:+d} "
                            f"(workspace start {i - lo:+d}), now {int(self.buf[i]):#04x}")


# ---------------------------------------------------------------- a dense row bound to its inputs and its oracle
class Job:
    def __init__(self, ext, oracle, row, dtype=torch.float32, entry=None, with_oracle=True):
        self.ext, self.row, self.dtype = ext, row, dtype
        c = self.c = row.case
        self.code = ext.dtype_code(dtype)
        self.entry = entry or ("layout" if dtype == torch.float32 else "typed")
        self.word = c.path | (ext.PATH_DETERMINISTIC if row.det else 0)
        self.name = f"{c.name}[{str(dtype).replace('torch.', '')}]"
        self.nbytes = WC.workspace_bytes(ext, row)          # the FP32 query, whatever the dtype
        self.key = WC.row_key(ext, row, self.code)
        f, r = PC.inputs(c)
        self.rois = dev(r)
        self.exact = c.kind == "fwd" or row.det             # the result is a pure function of the inputs, bit for bit
        if c.kind == "fwd":
            src = dev(f).to(dtype)
            wide = src.float().cpu().numpy()
            self.src = src.contiguous(memory_format=torch.channels_last) if c.fl == PC.NHWC else src
            self.shape = (c.R, c.C, c.ph, c.pw)
            if with_oracle:
                want = torch.from_numpy(oracle.forward_c(wide, r, c.ph, c.pw, PC.SCALE, threads=16)).to(dtype)
                assert not bool(want.isnan().any())
                self.want_bits = want.view(itype(dtype)).cuda()
        else:
            g = torch.from_numpy(np.random.default_rng(7).standard_normal((c.R, c.C, c.ph, c.pw)).astype(np.float32)).to(dtype)
            wide = g.float().numpy()
            src = g.cuda()
            self.src = src.contiguous(memory_format=torch.channels_last) if c.fl == PC.NHWC else src
            self.shape = f.shape
            if with_oracle:
                self.want = oracle.backward_c(wide, r, f.shape, PC.SCALE, threads=16)
                assert np.isfinite(self.want).all()
                if row.det:
                    self.want_bits = torch.from_numpy(self.want).to(dtype).view(itype(dtype)).cuda()
                else:
                    self.S, self.n = oracle.backward_bound_c(wide, r, f.shape, PC.SCALE, threads=16)
                if c.name == "b_buckets_chains":   # some pixel's list is longer than its bucket: the chains are walked
                    kshift = WC.plan_of(ext, row).kshift
                    longest = int(distinct_bins_per_pixel(oracle, f.shape, r, c.ph, c.pw).max())
                    assert longest > (1 << kshift), (longest, kshift)
                if c.name == "b_ordered_queue":    # some pixel's list is longer than the register sort takes: it is queued
                    longest = int(distinct_bins_per_pixel(oracle, f.shape, r, c.ph, c.pw).max())
                    assert longest > WC.SORT_REGISTER_CAP, longest
        self.out = torch.empty(int(np.prod(self.shape)), dtype=itype(dtype), device="cuda")
        self.refill()

    def refill(self):
        self.out.fill_(NAN_PATTERN[self.dtype])

    def used(self, offset):
        return WC.row_used_bytes(self.ext, self.row, offset)

    def launch(self, ws, nbytes, stages=None):
        c, L = self.c, self.ext._lib
        dims = (c.B, c.R, c.H, c.W, c.C, c.ph, c.pw)
        tail = (self.rois.data_ptr(), self.out.data_ptr(), ws, nbytes, self.word)
        if c.kind == "fwd":
            if self.entry == "stages":
                assert c.tl == PC.NCHW and self.code == 0
                return L.rroi_align_forward_stages_hip(self.src.data_ptr(), c.fl, PC.SCALE, *dims, *tail,
                                                       self.ext.STAGE_ALL if stages is None else stages, stream())
            if self.entry == "typed":
                return L.rroi_align_forward_typed_hip(self.src.data_ptr(), self.code, c.fl, c.tl, PC.SCALE, *dims, *tail, stream())
            return L.rroi_align_forward_layout_hip(self.src.data_ptr(), c.fl, c.tl, PC.SCALE, *dims, *tail, stream())
        if self.entry == "typed":
            return L.rroi_align_backward_typed_hip(self.src.data_ptr(), self.code, c.fl, c.tl, PC.SCALE, *dims, *tail, stream())
        return L.rroi_align_backward_layout_hip(self.src.data_ptr(), c.fl, c.tl, PC.SCALE, *dims, *tail, stream())

    def logical(self):
        """The output as its (N, C, H, W) tensor, whatever its storage."""
        t = self.out.view(self.dtype)
        n, ch, h, w = self.shape
        return t.view(n, h, w, ch).permute(0, 3, 1, 2) if self.c.tl == PC.NHWC else t.view(n, ch, h, w)

    def bits(self):
        return self.logical().contiguous().view(itype(self.dtype))

    def check(self, what):
        """The project's own bar for this plan."""
        if self.exact:
            got = self.bits()
            if not torch.equal(got, self.want_bits):
                bad = got != self.want_bits
                unwritten = int((got[bad] == NAN_PATTERN[self.dtype]).sum())
                pytest.fail(f"{what}: {int(bad.sum())} elements differ from the oracle's bits ({unwritten} of them never "
                            f"written); the first at {tuple(int(v) for v in bad.nonzero()[0])}")
        elif self.dtype == torch.float32:
            Wk.check_backward_elementwise(self.logical().cpu().numpy(), self.want, self.S, self.n, what=what)
        else:
            check_half_backward(self.logical().contiguous(), self.want, self.S, self.n, self.dtype, what)


# ---------------------------------------------------------------- a bucketed row
class BJob:
    """A bucketed call on real, exactly sized crops: one buffer, bucket after bucket, every crop on a 256-byte boundary
    with a gap of pattern behind it."""

    def __init__(self, ext, oracle, b, with_oracle=True):
        self.ext, self.b, self.dtype = ext, b, torch.float32
        self.name = b.name
        self.widths = WC.bucketed_widths(b)
        self.mx = max(self.widths)
        self.nbytes = WC.bucketed_workspace_bytes(ext, b) if b.path != PC.DIRECT else 0
        self.key = WC.bucketed_key(ext, b)
        self.word = b.path | (ext.PATH_DETERMINISTIC if b.det else 0)
        self.exact = b.kind == "fwd" or b.det
        c = WC.bucketed_case(b)
        f, r = PC.inputs(c)
        self.rois = dev(r)
        layout = ext.bucket_layout(self.widths)
        offs, at = [0] * b.R, 0                       # element offset of every crop
        for w, idx in layout:
            for i in idx:
                offs[i] = at
                at = (at + b.C * b.ph * w + 64 + 63) // 64 * 64      # 256-byte aligned, at least 256 bytes of gap
        self.offs, self.total = offs, at
        if b.kind == "fwd":
            self.src = dev(f)
            self.crops = torch.empty(at, dtype=torch.int32, device="cuda")
            self.shape = None
            if with_oracle:
                full = oracle.forward_c(f, r, b.ph, self.mx, PC.SCALE, threads=16)
                assert np.isfinite(full).all()
                self.want_bits = self.image(lambda i, w: torch.from_numpy(np.ascontiguousarray(full[i, :, :, :w])))
                dense = {}
                for w, idx in layout:   # the dense op at the bucket's width (the reference only: through the binding)
                    d = ext.forward(self.src, self.rois[torch.tensor(idx, device="cuda")], b.ph, w, PC.SCALE).cpu()
                    dense.update({i: d[j] for j, i in enumerate(idx)})
                self.dense_bits = self.image(lambda i, w: dense[i])
        else:
            g = np.random.default_rng(7).standard_normal((b.R, b.C, b.ph, self.mx)).astype(np.float32)
            for i, w in enumerate(self.widths):
                g[i, :, :, w:] = 0
            self.crops = self.image(lambda i, w: torch.from_numpy(np.ascontiguousarray(g[i, :, :, :w])))
            self.shape = f.shape
            self.out = torch.empty(int(np.prod(f.shape)), dtype=torch.int32, device="cuda")
            if with_oracle:
                self.want = oracle.backward_c(g, r, f.shape, PC.SCALE, threads=16)     # on the zero-padded gradients
                if b.det:
                    self.want_bits = torch.from_numpy(self.want).view(torch.int32).reshape(-1).cuda()
                else:
                    self.S, self.n = oracle.backward_bound_c(g, r, f.shape, PC.SCALE, threads=16)
        self.table = ext.crop_table([self.crops.data_ptr() + 4 * o for o in offs], self.widths, "cuda")
        self.refill()

    def image(self, crop_of):
        """The crops' buffer with crop i = crop_of(i, width): the pattern everywhere else."""
        b = self.b
        img = torch.full((self.total,), NAN_PATTERN[torch.float32], dtype=torch.int32)
        for i, (o, w) in enumerate(zip(self.offs, self.widths)):
            img[o:o + b.C * b.ph * w] = crop_of(i, w).contiguous().view(torch.int32).reshape(-1)
        return img.cuda()

    def refill(self):
        (self.crops if self.b.kind == "fwd" else self.out).fill_(NAN_PATTERN[torch.float32])

    def used(self, offset):
        return WC.bucketed_used_bytes(self.ext, self.b, offset)

    def launch(self, ws, nbytes, stages=None):
        b, L = self.b, self.ext._lib
        if b.kind == "fwd":
            g = 0
            for w in self.widths:
                g = int(np.gcd(g, w))
            return L.rroi_align_forward_bucketed_hip(self.src.data_ptr(), 0, PC.SCALE, b.B, b.R, b.H, b.W, b.C, b.ph, self.mx,
                                                     sum(self.widths), g, 256, self.rois.data_ptr(), self.table.data_ptr(),
                                                     ws, nbytes, self.word, stream())
        return L.rroi_align_backward_bucketed_hip(self.table.data_ptr(), 0, 0, PC.SCALE, b.B, b.R, b.H, b.W, b.C, b.ph, self.mx,
                                                  self.rois.data_ptr(), self.out.data_ptr(), ws, nbytes, self.word, stream())

    def bits(self):
        return (self.crops if self.b.kind == "fwd" else self.out).clone()

    def check(self, what):
        if self.b.kind == "fwd":   # every crop, and every gap between the crops
            assert torch.equal(self.crops, self.dense_bits), f"{what}: differs from the dense op's bits (or a gap was written)"
            assert torch.equal(self.crops, self.want_bits), f"{what}: differs from the oracle's bits"
        elif self.exact:
            assert torch.equal(self.out, self.want_bits), f"{what}: differs from oracle.backward_c's bits"
        else:
            got = self.out.view(torch.float32).view(self.shape).cpu().numpy()
            Wk.check_backward_elementwise(got, self.want, self.S, self.n, what=what)


# ---------------------------------------------------------------- poisons x offsets
def run_variants(job, prev, variants):
    """Every (poison, offset): the call inside the guarded arena, the guards, the result."""
    need = max(job.nbytes, prev.nbytes)
    arena = Arena(need)
    left = None
    first = None
    for poison, offset in variants:
        what = f"{job.name} poison {poison if isinstance(poison, str) else hex(poison)} offset {offset}"
        lo, hi, end = arena.place(job.nbytes, offset)
        if poison == "left":
            if left is None:   # the previous row of the table, run once into this buffer: what it left is the poison
                plo, phi, _ = arena.place(prev.nbytes, 0)
                arena.buf.fill_(0xFF)
                assert prev.launch(arena.buf.data_ptr() + plo, prev.nbytes) == 1, (what, "the previous row")
                torch.cuda.synchronize()
                left = arena.buf.clone()
            arena.buf.copy_(left)
            src = left
        else:
            arena.buf.fill_(poison)
            src = poison
        job.refill()
        st = job.launch(arena.buf.data_ptr() + lo, job.nbytes)
        torch.cuda.synchronize()
        assert st == 1, (what, "status", st)
        arena.untouched(src, ((0, lo), (hi, end)), what, lo, hi)
        # the backward's size holds a flat 8192 bytes for two roundings that add less: what is left behind the last
        # sub-array belongs to nothing, and is checked like a guard (an overrun of that array would land there)
        used = job.used(offset)
        assert 0 < used <= job.nbytes
        arena.untouched(src, ((lo + used, hi),), what + " (the unused tail of the workspace)", lo, lo + used)
        if job.exact:
            cur = job.bits()
            if first is None:
                first = (what, cur.clone())
            else:
                assert torch.equal(cur, first[1]), f"{what}: the result differs from that of [{first[0]}]"
        job.check(what)


def variants_of(name):
    return DIAGONAL if name in DIAGONAL_ROWS else FULL


@pytest.mark.parametrize("i", range(len(WC.ROWS)), ids=[r.case.name for r in WC.ROWS])
def test_row(ext, oracle, i):
    row, prev = WC.ROWS[i], WC.ROWS[i - 1]
    job = Job(ext, oracle, row)
    assert job.key == (row.case.kind,) + tuple(row.want)
    run_variants(job, Job(ext, oracle, prev, with_oracle=False), variants_of(row.case.name))
    RAN["fp32"].add(job.key)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("i", range(len(WC.HALF_ROWS)), ids=[r.case.name for r in WC.HALF_ROWS])
def test_half_row(ext, oracle, i, dtype):
    row, prev = WC.HALF_ROWS[i], WC.HALF_ROWS[i - 1]
    job = Job(ext, oracle, row, DTYPES[dtype])
    assert job.key == (row.case.kind,) + tuple(row.want)
    run_variants(job, Job(ext, oracle, prev, DTYPES[dtype], with_oracle=False), variants_of(row.case.name))
    RAN[dtype].add(job.key)


@pytest.mark.parametrize("i", range(len(WC.BUCKETED)), ids=[b.name for b in WC.BUCKETED])
def test_bucketed_row(ext, oracle, i):
    b, prev = WC.BUCKETED[i], WC.BUCKETED[i - 1]
    job = BJob(ext, oracle, b)
    assert job.key[:len(b.want) + 1] == (b.kind,) + tuple(b.want)
    run_variants(job, BJob(ext, oracle, prev, with_oracle=False), FULL)
    RAN["bucketed"].add(job.key)


# ---------------------------------------------------------------- (d) size and pointer checks
def _family(ext, oracle, family):
    bf16 = torch.bfloat16
    if family == "layout":
        return [Job(ext, oracle, WC.ROW["f_cl_out_13x18"]), Job(ext, oracle, WC.ROW["b_ordered_nhwc"])]
    if family == "typed":
        return [Job(ext, oracle, WC.ROW["f_shift_13x18"], bf16), Job(ext, oracle, WC.ROW["b_ordered_nchw"], bf16)]
    if family == "stages":
        return [Job(ext, oracle, WC.ROW["f_strided_13x18"], entry="stages")]
    return [BJob(ext, oracle, WC.BUCKETED[0]), BJob(ext, oracle, WC.BUCKETED[3])]


@pytest.mark.parametrize("family", ["layout", "typed", "stages", "bucketed"])
def test_size_and_pointer_checks(ext, oracle, family):
    """The arena is real and fully sized throughout: only the stated number, or the pointer handed over, changes -- so
    nothing can run out of bounds even where a check is missing."""
    for job in _family(ext, oracle, family):
        assert job.exact and job.nbytes > 0
        arena = Arena(job.nbytes + PAGE)
        lo, hi, end = arena.place(job.nbytes + PAGE, 0)
        base = arena.buf.data_ptr() + lo
        arena.buf.fill_(0xFF)
        assert job.launch(base, job.nbytes) == 1
        torch.cuda.synchronize()
        job.check(f"{job.name} exact size")
        exact = job.bits().clone()
        for what, ws, n in (("one byte short", base, job.nbytes - 1), ("NULL workspace", None, job.nbytes)):
            arena.buf.fill_(0xFF)
            job.refill()
            before = job.bits().clone()
            st = job.launch(ws, n)
            torch.cuda.synchronize()
            assert st == 0, (job.name, what, st)
            arena.untouched(0xFF, ((0, arena.buf.numel()),), f"{job.name} {what}", lo, hi)
            assert torch.equal(job.bits(), before), f"{job.name} {what}: the output was written"
        arena.buf.fill_(0xFF)
        job.refill()
        assert job.launch(base, job.nbytes + PAGE) == 1
        torch.cuda.synchronize()
        arena.untouched(0xFF, ((0, lo), (hi, end)), f"{job.name} 4 KiB more", lo, hi)
        assert torch.equal(job.bits(), exact), f"{job.name}: 4 KiB more of workspace changed the result"
    RAN["checks"].add(family)


# ---------------------------------------------------------------- (e) plans that take no workspace
def _no_workspace(job):
    assert job.launch(None, 0) == 1
    torch.cuda.synchronize()
    job.check(f"{job.name} NULL / 0")
    plain = job.bits().clone()
    arena = Arena(65536)
    lo, hi, end = arena.place(65536, 256)
    arena.buf.fill_(0x7F)
    job.refill()
    assert job.launch(arena.buf.data_ptr() + lo, 65536) == 1
    torch.cuda.synchronize()
    arena.untouched(0x7F, ((0, arena.buf.numel()),), f"{job.name} handed a workspace", lo, hi)
    job.check(f"{job.name} handed a workspace")
    if job.exact:   # (the direct backward adds with fp32 atomics: its bits may differ from run to run, its bound holds)
        assert torch.equal(job.bits(), plain), f"{job.name}: a workspace it does not use changed the result"


@pytest.mark.parametrize("row", WC.NO_WORKSPACE, ids=[r.case.name for r in WC.NO_WORKSPACE])
def test_plans_without_workspace(ext, oracle, row):
    job = Job(ext, oracle, row)
    assert job.key == (row.case.kind,) + tuple(row.want)
    _no_workspace(job)
    RAN["none"].add(job.key)


def test_bucketed_patch_kernel_without_workspace(ext, oracle):
    job = BJob(ext, oracle, WC.NO_WORKSPACE_BUCKETED)
    assert job.key[:3] == ("fwd", "k2p", "-") and job.nbytes == 0
    _no_workspace(job)
    RAN["none"].add(job.key[:3])


# ---------------------------------------------------------------- (f) the two stages as two calls
@pytest.mark.parametrize("name", ["f_strided_13x18", "f_shift_13x18"])
def test_stages_as_two_calls(ext, oracle, name):
    """PROLOGUE, then GATHER, on the same arena.  (A GATHER alone on a poisoned arena is not run: it would read garbage
    affines.)"""
    job = Job(ext, oracle, WC.ROW[name], entry="stages")
    arena = Arena(job.nbytes)
    for poison, offset in DIAGONAL[:3]:
        what = f"{job.name} stages poison {hex(poison)} offset {offset}"
        lo, hi, end = arena.place(job.nbytes, offset)
        arena.buf.fill_(poison)
        job.refill()
        base = arena.buf.data_ptr() + lo
        assert job.launch(base, job.nbytes, ext.STAGE_PROLOGUE) == 1
        torch.cuda.synchronize()
        arena.untouched(poison, ((0, lo), (hi, end)), what + " prologue", lo, hi)
        assert job.launch(base, job.nbytes, ext.STAGE_GATHER) == 1
        torch.cuda.synchronize()
        arena.untouched(poison, ((0, lo), (hi, end)), what + " gather", lo, hi)
        job.check(what)
    RAN["stages"].add(name)


# ---------------------------------------------------------------- coverage over what ran
def test_every_required_plan_ran():
    missing = {
        "fp32": WC.REQUIRED - RAN["fp32"], "bf16": WC.HALF_REQUIRED - RAN["bf16"], "fp16": WC.HALF_REQUIRED - RAN["fp16"],
        "bucketed": WC.BUCKETED_REQUIRED - RAN["bucketed"], "none": WC.NO_WORKSPACE_REQUIRED - RAN["none"],
        "stages": {"f_strided_13x18", "f_shift_13x18"} - RAN["stages"],
        "checks": {"layout", "typed", "stages", "bucketed"} - RAN["checks"],
    }
    missing = {k: sorted(v, key=str) for k, v in missing.items() if v}
    assert not missing, f"required plans that no passing case of this module ran: {missing}"
