"""Every call that works in a caller-provided workspace, run in a packed, guarded arena (tests/arena.py) whose workspace is
poisoned with NaN: the contract of phastft_hip.h's _dev calls --

    the call writes nothing outside [work, work + work_len) and nothing outside its outputs,
    it never depends on what the workspace held before --

for fft_any_batched, r2c_any_batched / c2r_any_batched, dct_batched / dst_batched (types 2 and 3), stft_batched /
istft_batched, conv_batched, czt_batched, fft_nd_batched and r2c_nd_batched / c2r_nd_batched.

One arena per call holds every input plane, every output plane and the workspace, each between bands of 0xA5 bytes: the
packed arena a user would build.  Inputs and planners are the module tests' own (imported, not copied).  Each case is a batch
of 3 at distances above the row and runs at four workspace lengths -- the smallest legal one (workspace_min() where the planner
has one; phastft_hip.h's formula for the N-d planners; workspace_len(1) otherwise), that plus 1, one that gives chunks of two
plus 1, and workspace_len(batch) -- each on a workspace base 0, 1 and 16 / itemsize - 1 elements past a 16-byte boundary.
Per call:

    1. every band is intact (Arena.check() returns nothing);
    2. the input regions are bit-identical to before (the in-place complex planes are the output);
    3. the output regions are bit-identical to those of the same call on a ZERO-filled workspace of the same length and base
       in an arena of its own: same chunking, same alignment path, so what the workspace held is the only difference;
    4. at one length per case (the smallest, one element past the boundary) every transform passes its module's own gate
       against the module's long-double reference -- no tolerance is introduced here;
    5. the gaps between the rows of an output (out_dist > row) keep their sentinel (they are part of 3's regions, and are
       compared with the sentinel itself).

One element below the smallest legal length the call must return code 16 with every byte of the arena unchanged.

That the poison has teeth was shown once on a scratch build whose Bluestein pad sweep (any_pre_kernel, csrc/any_len.hip)
skipped its "0 up to M" stores: every test_any_len case then failed on assertion 3 at its first call (NaN in the planes).

test_checker_sees_an_overrun_on_the_device declares an output region one element short, so that the call's last output
element lies in the band: check() must report exactly that.  It writes only inside the test's own allocation.

TRANSPOSE_ROWS are N-d shapes for the batched planar transpose (csrc/nd.hip), kept out of the modules' SHAPES lists (whose
error-budget files list every entry).  What each is MEANT to reach follows from reading launch_nd_transpose's selection; the
tests do not depend on it (they gate the result against fftn / rfftn / irfftn in long double through the modules' gates).  That the
selection reaches all 4 square and 8 narrow instantiations per type, and that each moves the right bits for every narrow side,
is CHECKED on the host: tests/cpp/block_emu_test.cpp records the instantiation of every launch and fails if one of the 24 never
ran (tests/test_block_emulator.py::test_block_kernels_of[nd]):

    (65, 67)    complex, aligned: an odd total puts the imaginary plane of the transposed copy off a 16-byte boundary, so the
                second transpose is nd_transpose_square<VIN = false, VOUT = false> in f32 too (67 % 4 != 0)
    (29, 70)    narrow R = 29 (f64: a side of 18 .. 31; f32 too)            (70, 31)   narrow C = 31
    (150, 61)   narrow C = 61 (f32: a side of 34 .. 62)                       (47, 150)  narrow R = 47 (f32)
    (5, 6, 70)  a rank-3 rotation: 30 x 70, 350 x 6 and 420 x 5 matrices (narrow on either side)
    each at batch 1 aligned, at batch 2 with an odd dist and from planes one element off a 16-byte boundary: the wide side
    and the flat run of the narrow kernels then run both 16 bytes per lane and element by element (VW, VF), in tiles of
    32 .. 64 wide-side entries, several per matrix, the last one ragged."""
import dataclasses

import numpy as np
import pytest

from tests import test_gpu_any_len as A
from tests import test_gpu_any_real as AR
from tests import test_gpu_conv as CV
from tests import test_gpu_czt as CZ
from tests import test_gpu_dct as D
from tests import test_gpu_nd as N
from tests import test_gpu_real_nd as RN
from tests import test_gpu_stft as ST
from tests.arena import GUARD, SENTINEL, Arena, Region

pytestmark = pytest.mark.gpu

BATCH = 3
DEVICE = "cuda"  # where the arenas live ("cpu" lets drive() be tried on a fake call without a GPU)
IDS = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)  # noqa: E731


def _ndt(dt):
    return np.float64 if dt == "f64" else np.float32


def _torch():
    import torch

    return torch


def _tdt(dt):
    return _torch().float64 if dt == "f64" else _torch().float32


def _vec(dt):
    return 16 // np.dtype(_ndt(dt)).itemsize


def _pow2(n):
    return n & (n - 1) == 0


@dataclasses.dataclass
class Plane:
    name: str
    role: str        # "in" | "out" | "inout"
    row: int         # elements of one transform's row
    dist: int        # elements between rows
    rows: list = None  # the input rows (in, inout)

    def length(self, batch):
        return (batch - 1) * self.dist + self.row


@dataclasses.dataclass
class Case:
    tag: str
    dt: str
    m: int           # the largest inner convolution length (the bands are max(4096, 2 m) elements)
    planes: list
    lengths: list    # (label, work_len): smallest legal, + 1, chunks of two + 1, the whole batch
    call: object     # call(t: name -> 1-D tensor, work): the entry point under test
    gate: object     # gate(got: name -> list of rows): the module's check against its reference
    batch: int = BATCH
    plane_off: int = 0


def _lengths(smallest, two_plus_1, whole):
    return [("smallest", smallest), ("smallest + 1", smallest + 1), ("chunks of two + 1", two_plus_1), ("whole batch", whole)]


def _packed(case, work_len, work_off, work_fill, short=None):
    """the arena of one call: inputs, outputs, then the workspace; `short`: an output region declared one element short"""
    regions = []
    for p in case.planes:
        n = p.length(case.batch)
        if p.role == "out":
            regions.append(Region(p.name, n - (p.name == short), case.plane_off, "sentinel"))
            continue
        data = np.full(n, SENTINEL, _ndt(case.dt))
        for b, row in enumerate(p.rows[:case.batch]):
            data[b * p.dist:b * p.dist + p.row] = row
        if p.name == short:
            data = data[:-1]
        regions.append(Region(p.name, len(data), case.plane_off, "data", data))
    if work_fill == "zero":
        regions.append(Region("work", work_len, work_off, "data", np.zeros(work_len, _ndt(case.dt))))
    else:
        regions.append(Region("work", work_len, work_off, "poison"))
    return Arena(_tdt(case.dt), regions, m=case.m, device=DEVICE)


def _run(case, work_len, work_off, work_fill):
    a = _packed(case, work_len, work_off, work_fill)
    before = {p.name: a.bytes_of(p.name).clone() for p in case.planes if p.role == "in"}
    case.call({p.name: a[p.name] for p in case.planes}, a["work"])
    return a, before


def _rows(case, a):
    got = {}
    for p in case.planes:
        if p.role != "in":
            flat = a[p.name].cpu().numpy()
            got[p.name] = [flat[b * p.dist:b * p.dist + p.row] for b in range(case.batch)]
    return got


def _gaps_keep_the_sentinel(case, a, where):
    for p in case.planes:
        if p.role == "in" or p.dist == p.row:
            continue
        flat = a[p.name].cpu().numpy()
        for b in range(case.batch - 1):
            gap = flat[b * p.dist + p.row:(b + 1) * p.dist]
            assert (gap == SENTINEL).all(), (where, p.name, b)


def drive(P, case, offsets=None, gate_at=("smallest", 1)):
    """assertions 1 - 5 of the module docstring for every (length, base) of the case, and the refusal below the smallest"""
    import torch

    offsets = tuple(dict.fromkeys((0, 1, _vec(case.dt) - 1))) if offsets is None else offsets
    gated = False
    for label, work_len in case.lengths:
        for off in offsets:
            where = (case.tag, case.dt, label, work_len, off)
            a, before = _run(case, work_len, off, "poison")
            hits = a.check()
            assert hits == [], (where, hits)                                                # 1
            for name, kept in before.items():
                assert torch.equal(a.bytes_of(name), kept), (where, name)                   # 2
            z, _ = _run(case, work_len, off, "zero")
            hits = z.check()
            assert hits == [], (where, "zero-filled", hits)
            assert a["work"].data_ptr() % 16 == z["work"].data_ptr() % 16 == off * a.itemsize
            for p in case.planes:
                if p.role != "in":
                    assert torch.equal(a.bytes_of(p.name), z.bytes_of(p.name)), (where, p.name)  # 3
            _gaps_keep_the_sentinel(case, a, where)                                         # 5
            if (label, off) == gate_at:
                case.gate(_rows(case, a))                                                   # 4
                gated = True
    assert gated, case.tag
    label, smallest = case.lengths[0]
    if label == "smallest":
        a = _packed(case, smallest - 1, 1, "poison")
        keep = a.snapshot()
        with pytest.raises(P.PhastPanic) as e:
            case.call({p.name: a[p.name] for p in case.planes}, a["work"])
        assert e.value.code == 16, case.tag
        torch.cuda.synchronize()
        assert torch.equal(a.raw, keep), (case.tag, "a refused call wrote")


def overrun(P, case, name):
    """the call on an arena whose region `name` is declared one element short: exactly that element is reported -- the bytes
    of the value the call left there that differ from the band's fill (all of them, from offset 0, unless one happens to be
    0xA5)"""
    a = _packed(case, case.lengths[-1][1], 0, "poison", short=name)
    t = {p.name: a.view(p.name, extra=int(p.name == name)) for p in case.planes}
    case.call(t, a["work"])
    last = a.view(name, extra=1)[-1:].view(_torch().uint8).cpu().numpy()
    changed = np.nonzero(last != GUARD)[0]
    assert changed.size >= a.itemsize - 2, (case.tag, case.dt, last)
    assert a.check() == [(name, "after", int(changed[0]), int(changed.size))], (case.tag, case.dt)


# ---------------------------------------------------------------------------------------------
# the cases, one builder per entry point
# ---------------------------------------------------------------------------------------------
def any_len_case(P, dt, n):
    pl = A._planner(P, dt, n)
    m = pl.m
    assert not _pow2(n) and pl.workspace_len(1) == 2 * m
    dist = n + 3
    xs = [A._input(n, dt, seed=10 + b) for b in range(BATCH)]

    def call(t, work):
        P.fft_any_batched(t["re"], t["im"], n, P.Direction.Forward, pl, dist=dist, workspace=work)

    def gate(got):
        for b, (re, im) in enumerate(xs):
            A._check(f"guard:any:{n}", dt, n, got["re"][b], got["im"][b], A._ref(re, im, 1))

    planes = [Plane("re", "inout", n, dist, [x[0] for x in xs]), Plane("im", "inout", n, dist, [x[1] for x in xs])]
    return Case(f"any:{n}", dt, m, planes, _lengths(2 * m, 4 * m + 1, pl.workspace_len(BATCH)), call, gate)


def any_real_case(P, dt, n, c2r):
    pl = AR._planner(P, dt, n)
    m, h1 = pl.m, n // 2 + 1
    assert m > 0 and pl.workspace_len(1) == 2 * m
    rd, cd = (n + 5) | 1, (h1 + 3) | 1
    lengths = _lengths(2 * m, 4 * m + 1, pl.workspace_len(BATCH))
    if not c2r:
        xs = [AR._signal(n, dt, seed=10 + b) for b in range(BATCH)]

        def call(t, work):
            P.r2c_any_batched(t["x"], t["out_re"], t["out_im"], pl, BATCH, in_dist=rd, out_dist=cd, workspace=work)

        def gate(got):
            for b, x in enumerate(xs):
                AR._check_r2c(dt, n, (got["out_re"][b], got["out_im"][b]), x)

        planes = [Plane("x", "in", n, rd, xs), Plane("out_re", "out", h1, cd), Plane("out_im", "out", h1, cd)]
        return Case(f"r2c_any:{n}", dt, m, planes, lengths, call, gate)
    specs = [AR._spectrum(n, dt, seed=10 + b) for b in range(BATCH)]

    def call(t, work):
        P.c2r_any_batched(t["in_re"], t["in_im"], t["out"], pl, BATCH, in_dist=cd, out_dist=rd, workspace=work)

    def gate(got):
        for b, (re, im) in enumerate(specs):
            AR._check_c2r(dt, n, got["out"][b], re, im)

    planes = [Plane("in_re", "in", h1, cd, [s[0] for s in specs]), Plane("in_im", "in", h1, cd, [s[1] for s in specs]),
              Plane("out", "out", n, rd)]
    return Case(f"c2r_any:{n}", dt, m, planes, lengths, call, gate)


def dct_case(P, dt, n, kind, t, pl=None):
    pl = pl or D.planner(P, dt, n)
    m = 0 if _pow2(n) else D.inner_m(n)
    in_dist, out_dist = (n + 5) | 1, n + 4
    xs = [D._signal(n, dt, seed=10 + b) for b in range(BATCH)]
    fn = P.dct_batched if kind == "dct" else P.dst_batched

    def call(tn, work):
        fn(tn["x"], tn["out"], pl, BATCH, type=t, in_dist=in_dist, out_dist=out_dist, workspace=work)

    def gate(got):
        for b, x in enumerate(xs):
            D.check(f"guard:{kind}{t}:{n}", dt, n, got["out"][b], D.ref(kind, t, x, None))

    planes = [Plane("x", "in", n, in_dist, xs), Plane("out", "out", n, out_dist)]
    lengths = _lengths(pl.workspace_len(1), pl.workspace_len(2) + 1, pl.workspace_len(BATCH))
    return Case(f"{kind}{t}:{n}", dt, m, planes, lengths, call, gate)


def stft_case(P, dt, shape, inverse):
    length, f, h = shape
    refs = [ST.reference(dt, length, f, h, True, "reflect", "hann", seed=20 + b) for b in range(BATCH)]
    pl = ST.planner(P, dt, length, f, h, refs[0][0], True, "reflect")
    m = 0 if _pow2(f) else ST.inner_m(f)
    pts, dist, vec = pl.frames * pl.bins, length + 5, _vec(dt)
    per = pl.workspace_min() - (vec - 1)
    if not inverse:
        xs = [ST._signal(length, dt, seed=20 + b) for b in range(BATCH)]

        def call(t, work):
            P.stft_batched(t["x"], t["re"], t["im"], pl, BATCH, sig_dist=dist, workspace=work)

        def gate(got):
            for b in range(BATCH):
                ST.check_forward(f"guard:stft:{shape}", dt, f, got["re"][b], got["im"][b], refs[b][1])

        planes = [Plane("x", "in", length, dist, xs), Plane("re", "out", pts, pts), Plane("im", "out", pts, pts)]
        lengths = _lengths(pl.workspace_min(), 2 * per + vec, pl.workspace_len(BATCH))
        return Case(f"stft:{shape}", dt, m, planes, lengths, call, gate)
    assert all(r[4] is not None for r in refs)

    def call(t, work):
        P.istft_batched(t["re"], t["im"], t["x"], pl, BATCH, sig_dist=dist, workspace=work)

    def gate(got):
        for b in range(BATCH):
            ST.check_signal(f"guard:istft:{shape}", dt, f, got["x"][b], refs[b][4])

    planes = [Plane("re", "in", pts, pts, [r[2] for r in refs]), Plane("im", "in", pts, pts, [r[3] for r in refs]),
              Plane("x", "out", length, dist)]
    lengths = _lengths(pl.workspace_min(True), 2 * pl.frames * per + vec, pl.workspace_len(BATCH))
    return Case(f"istft:{shape}", dt, m, planes, lengths, call, gate)


def conv_case(P, dt, shape, mode, flip):
    length, k, block = shape
    taps = CV._taps("random", k, dt)
    pl = CV.planner(P, dt, length, taps, mode, flip, block)
    b_len = CV.block_of(shape)
    m = 0 if _pow2(b_len) else CV.inner_m(b_len)
    n, vec = pl.out_len, _vec(dt)
    sig_dist, out_dist = (length + 5) | 1, (n + 3) | 1
    xs = [CV._signal(length, dt, seed=20 + i) for i in range(BATCH)]
    per = pl.workspace_min() - (vec - 1)

    def call(t, work):
        P.conv_batched(t["x"], t["out"], pl, BATCH, sig_dist=sig_dist, out_dist=out_dist, workspace=work)

    def gate(got):
        t0, count = CV.R.geometry(length, k, mode)  # every mode is a slice of the full convolution (CV.reference)
        for i in range(BATCH):
            want = CV.R.convolve(xs[i], taps, "full", flip)[t0:t0 + count]
            CV.check(f"guard:conv:{shape}:{mode}:{int(flip)}", dt, b_len, got["out"][i], want)

    planes = [Plane("x", "in", length, sig_dist, xs), Plane("out", "out", n, out_dist)]
    lengths = _lengths(pl.workspace_min(), 2 * per + vec, pl.workspace_len(BATCH))
    return Case(f"conv:{shape}:{mode}:{int(flip)}", dt, m, planes, lengths, call, gate)


def czt_case(P, dt, shape):
    import torch

    n, bins = shape
    step = 0.37 / n
    pl = CZ.planner(P, dt, n, bins, step, CZ.START)
    ell = pl.conv_len
    in_dist, out_dist = (n + 5) | 1, (bins + 3) | 1
    xs = [CZ._signal(n, dt, seed=20 + i) for i in range(BATCH)]

    def call(t, work):
        x = [torch.as_strided(t[k], (BATCH, n), (in_dist, 1)) for k in ("in_re", "in_im")]
        o = tuple(torch.as_strided(t[k], (BATCH, bins), (out_dist, 1)) for k in ("out_re", "out_im"))
        P.czt_batched(x[0], x[1], pl, out=o, work=work)

    def gate(got):
        for i in range(BATCH):
            CZ.check(f"guard:czt:{shape}", dt, n, bins, (got["out_re"][i], got["out_im"][i]),
                     CZ.reference(dt, n, bins, step, CZ.START, seed=20 + i))

    planes = [Plane("in_re", "in", n, in_dist, [x[0] for x in xs]), Plane("in_im", "in", n, in_dist, [x[1] for x in xs]),
              Plane("out_re", "out", bins, out_dist), Plane("out_im", "out", bins, out_dist)]
    return Case(f"czt:{shape}", dt, ell, planes, _lengths(2 * ell, 4 * ell + 1, pl.workspace_len(BATCH)), call, gate)


def _blue(axes):
    """the largest convolution length of the axes that run Bluestein (0: every axis is a power of two)"""
    return max([N.conv_len(n) for n in axes if n > 1 and not _pow2(n)], default=0)


def _real_blue(last):
    """the inner convolution length of the any-length real planner of the last axis (0: a power of two, 1 or 2)"""
    return 0 if _pow2(last) else AR.inner_m(last)


def nd_case(P, dt, shape, batch=BATCH, dist=None, plane_off=0, whole_only=False, seed=10):
    """phastft_hip.h: the smallest legal work_len is the copies of one array (2 prod n_i) plus 2 M of the largest Bluestein axis"""
    assert len([n for n in shape if n > 1]) >= 2
    pl = N._planner(P, dt, shape)
    tot, m = int(np.prod(shape)), _blue(shape)
    dist = tot + 7 if dist is None else dist
    xs = [N._input(shape, dt, seed=seed + b) for b in range(batch)]

    def call(t, work):
        P.fft_nd_batched(t["re"], t["im"], P.Direction.Forward, pl, batch=batch, dist=dist, workspace=work)

    def gate(got):
        for b, (re, im) in enumerate(xs):
            N._check(f"guard:nd:{shape}", dt, shape, got["re"][b], got["im"][b], N._ref(re, im, shape, 1))

    planes = [Plane("re", "inout", tot, dist, [x[0] for x in xs]), Plane("im", "inout", tot, dist, [x[1] for x in xs])]
    smallest = 2 * tot + 2 * m
    lengths = [("whole batch", pl.workspace_len(batch))] if whole_only else \
        _lengths(smallest, 2 * 2 * tot + 2 * m + 1, pl.workspace_len(batch))
    return Case(f"nd:{shape}", dt, m, planes, lengths, call, gate, batch=batch, plane_off=plane_off)


def real_nd_case(P, dt, shape, c2r, batch=BATCH, dists=None, plane_off=0, whole_only=False, seed=10):
    """phastft_hip.h: the copies of one array -- R2C one (2 x the half-spectrum points), C2R two -- plus 2 M of the largest
    Bluestein axis, the real last axis (its inner convolution length) included"""
    assert len([n for n in shape if n > 1]) >= 2 or shape[-1] == 1
    pl = RN._planner(P, dt, shape)
    tot, half = int(np.prod(shape)), RN._half(shape)
    assert pl.half == half
    m = max(_blue(shape[:-1]), _real_blue(shape[-1]))
    rd, cd = (tot + 5, half + 3) if dists is None else dists
    copies = 4 if c2r else 2
    smallest = copies * half + 2 * m
    lengths = [("whole batch", pl.workspace_len(batch))] if whole_only else \
        _lengths(smallest, 2 * copies * half + 2 * m + 1, pl.workspace_len(batch))
    if not c2r:
        xs = [RN._real(shape, dt, seed=seed + b) for b in range(batch)]

        def call(t, work):
            P.r2c_nd_batched(t["x"], t["out_re"], t["out_im"], pl, batch=batch, in_dist=rd, out_dist=cd, workspace=work)

        def gate(got):
            for b, x in enumerate(xs):
                RN._check(f"guard:r2c_nd:{shape}", dt, shape, got["out_re"][b], got["out_im"][b], *RN.ref_r2c(x, shape))

        planes = [Plane("x", "in", tot, rd, xs), Plane("out_re", "out", half, cd), Plane("out_im", "out", half, cd)]
        return Case(f"r2c_nd:{shape}", dt, m, planes, lengths, call, gate, batch=batch, plane_off=plane_off)
    specs = [RN._spectrum(shape, dt, seed=seed + b) for b in range(batch)]

    def call(t, work):
        P.c2r_nd_batched(t["in_re"], t["in_im"], t["out"], pl, batch=batch, in_dist=cd, out_dist=rd, workspace=work)

    def gate(got):
        for b, (re, im) in enumerate(specs):
            want = RN.ref_c2r(re, im, shape)
            RN._check(f"guard:c2r_nd:{shape}", dt, shape, got["out"][b], np.zeros(tot), want, np.zeros(tot))

    planes = [Plane("in_re", "in", half, cd, [s[0] for s in specs]), Plane("in_im", "in", half, cd, [s[1] for s in specs]),
              Plane("out", "out", tot, rd)]
    return Case(f"c2r_nd:{shape}", dt, m, planes, lengths, call, gate, batch=batch, plane_off=plane_off)


# ---------------------------------------------------------------------------------------------
# 3. every entry point in a poisoned, guarded arena
# ---------------------------------------------------------------------------------------------
ANY_LEN = [7, 100, 1000, 4099]
ANY_REAL = [6, 7, 100, 999, 1000, 4098]
# 30, 101, 1000: Bluestein inside; 64 (even) and 1 (odd): no inner workspace, the planner's own rows alone (workspace_len(1) > 0)
DCT = [30, 101, 1000, 64, 1]
STFT = [(1000, 30, 23), (4099, 64, 16), (5000, 1000, 250)]           # test_gpu_stft.py's test_batch_properties
CONV = [(100, 17, 17), (1000, 33, 100), (4099, 64, 256)]
CZT = [(37, 101), (101, 37), (100, 30), (4099, 513)]
ND = [(64, 64), (1009, 17), (3, 5, 7), (65, 63), (3, 4096)]
REAL_ND = [(1009, 17), (3, 5, 7), (9, 1024), (4, 2), (65, 63)]
DTS = ["f64", "f32"]


@pytest.mark.parametrize("n", ANY_LEN)
@pytest.mark.parametrize("dt", DTS)
def test_any_len(gpu, dt, n):
    drive(gpu, any_len_case(gpu, dt, n))


@pytest.mark.parametrize("c2r", [False, True], ids=["r2c", "c2r"])
@pytest.mark.parametrize("n", ANY_REAL)
@pytest.mark.parametrize("dt", DTS)
def test_any_real(gpu, dt, n, c2r):
    drive(gpu, any_real_case(gpu, dt, n, c2r))


@pytest.mark.parametrize("n", DCT)
@pytest.mark.parametrize("dt", DTS)
def test_dct_dst(gpu, dt, n):
    pl = D.planner(gpu, dt, n)
    assert pl.workspace_len(1) > 0
    for kind, t in D.KINDS:
        drive(gpu, dct_case(gpu, dt, n, kind, t, pl))


@pytest.mark.parametrize("inverse", [False, True], ids=["stft", "istft"])
@pytest.mark.parametrize("shape", STFT, ids=IDS)
@pytest.mark.parametrize("dt", DTS)
def test_stft(gpu, dt, shape, inverse):
    drive(gpu, stft_case(gpu, dt, shape, inverse))


@pytest.mark.parametrize("shape", CONV, ids=IDS)
@pytest.mark.parametrize("dt", DTS)
def test_conv(gpu, dt, shape):
    for mode, flip in (("full", False), ("same", True), ("valid", False)):
        drive(gpu, conv_case(gpu, dt, shape, mode, flip))


@pytest.mark.parametrize("shape", CZT, ids=IDS)
@pytest.mark.parametrize("dt", DTS)
def test_czt(gpu, dt, shape):
    drive(gpu, czt_case(gpu, dt, shape))


@pytest.mark.parametrize("shape", ND, ids=IDS)
@pytest.mark.parametrize("dt", DTS)
def test_nd(gpu, dt, shape):
    drive(gpu, nd_case(gpu, dt, shape))


@pytest.mark.parametrize("c2r", [False, True], ids=["r2c", "c2r"])
@pytest.mark.parametrize("shape", REAL_ND, ids=IDS)
@pytest.mark.parametrize("dt", DTS)
def test_real_nd(gpu, dt, shape, c2r):
    drive(gpu, real_nd_case(gpu, dt, shape, c2r))


@pytest.mark.parametrize("dt", DTS)
def test_no_workspace_needed_means_none_read(gpu, dt):
    """where workspace_len(1) is 0 (a power of two on the engine's own path) the call accepts a poisoned one-element workspace
    and leaves it alone: the bits of the call without one, bands whole, the element still the NaN it was"""
    import torch

    P, n = gpu, 64
    cases = []
    pa = A._planner(P, dt, n)
    xs = [A._input(n, dt, seed=10 + b) for b in range(BATCH)]
    cases.append((pa, [Plane("re", "inout", n, n + 4, [x[0] for x in xs]), Plane("im", "inout", n, n + 4, [x[1] for x in xs])],
                  lambda t, w: P.fft_any_batched(t["re"], t["im"], n, P.Direction.Forward, pa, dist=n + 4, workspace=w)))
    pr = AR._planner(P, dt, n)
    sig = [AR._signal(n, dt, seed=10 + b) for b in range(BATCH)]
    cases.append((pr, [Plane("x", "in", n, n + 4, sig), Plane("out_re", "out", n // 2 + 1, n // 2 + 4),
                       Plane("out_im", "out", n // 2 + 1, n // 2 + 4)],
                  lambda t, w: P.r2c_any_batched(t["x"], t["out_re"], t["out_im"], pr, BATCH, in_dist=n + 4,
                                                 out_dist=n // 2 + 4, workspace=w)))
    pn = N._planner(P, dt, (1, n))
    cases.append((pn, [Plane("re", "inout", n, n + 4, [x[0] for x in xs]), Plane("im", "inout", n, n + 4, [x[1] for x in xs])],
                  lambda t, w: P.fft_nd_batched(t["re"], t["im"], P.Direction.Forward, pn, batch=BATCH, dist=n + 4,
                                                workspace=w)))
    for pl, planes, call in cases:
        assert pl.workspace_len(1) == 0 and pl.workspace_len(BATCH) == 0
        case = Case(type(pl).__name__, dt, 0, planes, [("one poisoned element", 1)], call, None)
        a, before = _run(case, 1, 1, "poison")
        nan_bits = a.bytes_of("work").clone()
        assert a.check() == [], case.tag
        for name, kept in before.items():
            assert torch.equal(a.bytes_of(name), kept), (case.tag, name)
        assert torch.equal(a.bytes_of("work"), nan_bits) and bool(torch.isnan(a["work"]).all()), case.tag
        plain = _packed(case, 1, 1, "poison")
        call({p.name: plain[p.name] for p in planes}, None)
        for p in planes:
            if p.role != "in":
                assert torch.equal(a.bytes_of(p.name), plain.bytes_of(p.name)), (case.tag, p.name)
        _gaps_keep_the_sentinel(case, a, case.tag)


@pytest.mark.parametrize("dt", DTS)
def test_checker_sees_an_overrun_on_the_device(gpu, dt):
    """one call per module on an arena whose output region is declared one element short: the last output element lies in the
    band, and check() reports exactly that region, side and offset"""
    P = gpu
    overrun(P, any_len_case(P, dt, 100), "re")
    overrun(P, any_real_case(P, dt, 100, False), "out_im")
    overrun(P, any_real_case(P, dt, 100, True), "out")
    overrun(P, dct_case(P, dt, 101, "dct", 2), "out")
    overrun(P, dct_case(P, dt, 101, "dst", 3), "out")
    overrun(P, stft_case(P, dt, STFT[0], False), "re")
    overrun(P, stft_case(P, dt, STFT[0], True), "x")
    overrun(P, conv_case(P, dt, CONV[0], "full", False), "out")
    overrun(P, czt_case(P, dt, CZT[0]), "out_im")
    overrun(P, nd_case(P, dt, (3, 5, 7)), "im")
    overrun(P, real_nd_case(P, dt, (3, 5, 7), False), "out_re")
    overrun(P, real_nd_case(P, dt, (3, 5, 7), True), "out")


# ---------------------------------------------------------------------------------------------
# 4. shapes for the instantiations of the batched planar transpose that the modules' shapes do not reach
# ---------------------------------------------------------------------------------------------
TRANSPOSE_ROWS = [(29, 70), (70, 31), (150, 61), (47, 150), (5, 6, 70)]


def _variants(tot, half=None):
    """(label, batch, distances, plane offset): batch 1 aligned, batch 2 at odd distances, planes one element off"""
    odd = (tot + 2) | 1
    if half is None:
        return [("aligned", 1, None, 0), ("odd dist", 2, odd, 0), ("one element off", 1, None, 1)]
    return [("aligned", 1, None, 0), ("odd dist", 2, (odd, (half + 2) | 1), 0), ("one element off", 1, None, 1)]


@pytest.mark.parametrize("shape", [(65, 67)] + TRANSPOSE_ROWS, ids=IDS)
@pytest.mark.parametrize("dt", DTS)
def test_transposes_complex(gpu, dt, shape):
    tot = int(np.prod(shape))
    for label, batch, dist, off in _variants(tot):
        if shape == (65, 67) and label != "aligned":
            continue
        case = nd_case(gpu, dt, shape, batch=batch, dist=dist, plane_off=off, whole_only=True, seed=1)
        drive(gpu, case, offsets=(0,), gate_at=("whole batch", 0))


@pytest.mark.parametrize("c2r", [False, True], ids=["r2c", "c2r"])
@pytest.mark.parametrize("shape", TRANSPOSE_ROWS, ids=IDS)
@pytest.mark.parametrize("dt", DTS)
def test_transposes_real(gpu, dt, shape, c2r):
    tot, half = int(np.prod(shape)), RN._half(shape)
    for label, batch, dists, off in _variants(tot, half):
        case = real_nd_case(gpu, dt, shape, c2r, batch=batch, dists=dists, plane_off=off, whole_only=True, seed=1)
        drive(gpu, case, offsets=(0,), gate_at=("whole batch", 0))
