"""NUFFT planners built from points in device memory (``from_device``) and re-pointed in place (``set_points``): DESIGN.md §22.
The device sorts the points into the very tables the host constructor builds, so every comparison here is EQUALITY OF BITS
(``torch.equal``) against a planner the host constructor -- the path every other NUFFT test holds against its reference -- built at
the same points.  No tolerance appears in this file.

Point sets: (u) uniform in [-3, 3); (c) clumped, every point within 1e-7 of 0.3 (M ties in one or two cells); (d) duplicates, M
points drawn from 5 values; (e) the edge list -- signed zeros, the smallest subnormals, -2^-130 (cut to 0), -2^-60 (the last cell, at
1 - 2^-53), 1 - 2^-53, +-1, 0.25, 0.5, +-(2^52 + 0.5), +-1e300, q / n_g for a few q with the doubles just below and above --
padded with (u).  The f32 planners get the same doubles.  Type 1 at (c) and (d) proves the order inside a cell (a sum in another
order rounds differently), type 2 proves perm and the positions.

The largest key width (test_the_largest_key_width): 1-D f32 with N = 2^LOG_N_WIDEST modes; its time on the MI355X is in its docstring."""
import ctypes as C
import math
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = {"f64": 1e-9, "f32": 1e-5}
SHAPES = [((16,), 100), ((1000,), 4096), ((256,), 100003), ((12, 20), 5000), ((5, 7, 3), 40), ((16, 8, 12), 20000)]
SMALL = {1: ((16,), 100), 2: ((12, 20), 5000), 3: ((5, 7, 3), 40)}
SETS = "ucde"
INVALID_ARG, PLANNER_SIZE = 16, 3
LOG_N_WIDEST = 27  # 2^28 was measured and does not fit: test_the_largest_key_width says why


def width(eps):
    d = -math.log10(eps)
    if abs(d - round(d)) < 1e-9:
        d = round(d)
    return min(max(math.ceil(d) + 1, 2), 16)


def grid(n, w):
    g = 8
    while g < 2 * n or g < 2 * w:
        g *= 2
    return g


def edge_list(g):
    e = [0.0, -0.0, 5e-324, -5e-324, -2.0 ** -130, -2.0 ** -60, 1.0 - 2.0 ** -53, 1.0, -1.0, 0.25, 0.5, 2.0 ** 52 + 0.5, -(2.0 ** 52 + 0.5),
         1e300, -1e300]
    for q in (1, 2, g // 2, g - 1):
        v = q / g
        e += [v, float(np.nextafter(v, -1.0)), float(np.nextafter(v, 2.0))]
    return e


def points(which, modes, m, dt, seed=0):
    """one float64 array of M values per coordinate"""
    rng = np.random.default_rng(1000 * seed + 10 * len(modes) + SETS.index(which))
    out = []
    for axis, n in enumerate(modes):
        if which == "u":
            x = rng.uniform(-3, 3, m)
        elif which == "c":
            x = 0.3 + rng.uniform(-1e-7, 1e-7, m)
        elif which == "d":
            x = np.array([0.1, -0.7, 2.3, 1.1, 0.999])[rng.integers(0, 5, m)]
        else:
            x = rng.uniform(-3, 3, m)
            e = np.roll(np.array(edge_list(grid(n, width(EPS[dt])))), 5 * axis)[:m]
            x[:len(e)] = e
        out.append(np.ascontiguousarray(x, dtype=np.float64))
    return out


def classes(P, dims, dt):
    sfx = "64" if dt == "f64" else "32"
    name = {1: "PlannerNufft", 2: "PlannerNufft2d", 3: "PlannerNufft3d"}[dims]
    calls = {1: (P.nufft1_batched, P.nufft2_batched), 2: (P.nufft2d1_batched, P.nufft2d2_batched), 3: (P.nufft3d1_batched, P.nufft3d2_batched)}[dims]
    return getattr(P, name + sfx), calls


def n_arg(modes):
    return modes[0] if len(modes) == 1 else tuple(modes)


def host_planner(P, modes, pts, dt):
    cls, _ = classes(P, len(modes), dt)
    return cls(n_arg(modes), *pts, EPS[dt])


def on_device(pts):
    import torch

    return [torch.from_numpy(p).cuda() for p in pts]


def device_planner(P, modes, pts, dt, stream=None):
    cls, _ = classes(P, len(modes), dt)
    return cls.from_device(n_arg(modes), *on_device(pts), EPS[dt], stream=stream)


_DATA = {}


def data(modes, m, dt):
    """the inputs of a shape, made once and shared: values at the points and at the modes, re and im planes on the device"""
    import torch

    key = (modes, m, dt)
    if key not in _DATA:
        rng = np.random.default_rng(7)
        tdt = torch.float64 if dt == "f64" else torch.float32
        make = lambda n: torch.from_numpy(rng.uniform(-1, 1, n)).to(tdt).cuda()
        n = int(np.prod(modes))
        _DATA[key] = (make(m), make(m), make(n), make(n))
    return _DATA[key]


def outputs(P, planner, modes, m, dt, only_type=None):
    """every output of the planner on the shape's data: types 1 and 2, both directions, complex data; type 1 of real data"""
    import torch

    _, (t1, t2) = classes(P, len(modes), dt)
    c_re, c_im, f_re, f_im = data(modes, m, dt)
    out = []
    for d in (P.Direction.Forward, P.Direction.Reverse):
        if only_type in (None, 1):
            out += t1(c_re, c_im, planner, d)
        if only_type in (None, 2):
            out += t2(f_re, f_im, planner, d)
    if only_type is None:
        out += t1(c_re, None, planner)
    torch.cuda.synchronize()
    return [o.reshape(-1) for o in out]


def assert_equal(got, want, what):
    import torch

    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert torch.equal(g, w), (what, k, int((g != w).sum()), g.numel())


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("which", list(SETS))
@pytest.mark.parametrize("modes,m", SHAPES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_the_bits_of_the_host_built_planner(gpu, modes, m, which, dt):
    P = gpu
    pts = points(which, modes, m, dt)
    host, dev = host_planner(P, modes, pts, dt), device_planner(P, modes, pts, dt)
    assert (dev.n_modes, dev.m_points, dev.grid_len, dev.width, dev.eps) == (host.n_modes, host.m_points, host.grid_len, host.width, host.eps)
    assert dev.device_bytes() == host.device_bytes()  # the sort's temporary memory is gone
    assert_equal(outputs(P, dev, modes, m, dt), outputs(P, host, modes, m, dt), (modes, m, which, dt))


def test_the_largest_key_width(gpu):
    """1-D f32, N = 2^27: n_g = 2^28, 28-bit keys (the widest the 2-D and 3-D planners can have; seven digit passes, where 29 bits
    take eight); M = 1000 edge points, type 2 only.  N = 2^28 (n_g = 2^29, the 1-D limit) was run on the MI355X and took 57 s: 28 s
    to build the planner from device points and 29 s from host points, the transforms 0.01 s each -- nearly all of either build is
    the inner engine planner of 2^29 points, which both paths share, and not the sort.  That is far from the ten seconds this
    case may take, so N = 2^27 runs: 29.6 s on the MI355X -- 14.0 s to build the planner from device points, 14.6 s from host
    points, the transforms under 0.01 s: again the two engine planners (of 2^28 points)."""
    import torch

    P = gpu
    modes, m, dt = (1 << LOG_N_WIDEST,), 1000, "f32"
    pts = points("e", modes, m, dt)
    f = torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, (2, modes[0]))).to(torch.float32).cuda()
    got = []
    t0 = time.perf_counter()
    for build in (device_planner, host_planner):
        t1 = time.perf_counter()
        planner = build(P, modes, pts, dt)
        assert planner.grid_len == 2 << LOG_N_WIDEST
        t2 = time.perf_counter()
        got.append([o.clone() for o in P.nufft2_batched(f[0], f[1], planner)])
        torch.cuda.synchronize()
        print(f"{build.__name__}: built in {t2 - t1:.2f} s, transformed in {time.perf_counter() - t2:.2f} s")
        del planner
    print(f"largest key width: {time.perf_counter() - t0:.2f} s in all")
    assert_equal(got[0], got[1], f"2^{LOG_N_WIDEST + 1} cells")


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("built_by", ["device", "host"])
@pytest.mark.parametrize("modes,m", [((1000,), 4096), ((12, 20), 5000), ((16, 8, 12), 20000)], ids=["1d", "2d", "3d"])
def test_re_pointing(gpu, modes, m, built_by, dt):
    """built at A by either path, set_points(B): the bits of a fresh host-built planner at B; then back to a clumped A"""
    P = gpu
    a, b, c = points("u", modes, m, dt, seed=1), points("e", modes, m, dt, seed=2), points("c", modes, m, dt, seed=3)
    planner = (device_planner if built_by == "device" else host_planner)(P, modes, a, dt)
    bytes_before = planner.device_bytes()
    planner.set_points(*on_device(b))
    assert_equal(outputs(P, planner, modes, m, dt), outputs(P, host_planner(P, modes, b, dt), modes, m, dt), "B")
    planner.set_points(*on_device(c))
    assert_equal(outputs(P, planner, modes, m, dt), outputs(P, host_planner(P, modes, c, dt), modes, m, dt), "C")
    assert planner.device_bytes() == bytes_before


@pytest.mark.parametrize("dims", [1, 3])
def test_a_captured_graph_follows_the_points(gpu, dims):
    """a type 1 call captured through the planner on one stream (no parallel branches), replayed, re-pointed, replayed: the first
    replay has the bits of A, the second those of a fresh planner at B -- the tables were rewritten at the same addresses"""
    import torch

    P = gpu
    modes, m = SMALL[dims] if dims == 1 else ((16, 8, 12), 20000)
    dt = "f64"
    _, (t1, _) = classes(P, dims, dt)
    a, b = points("u", modes, m, dt, seed=4), points("d", modes, m, dt, seed=5)
    planner = device_planner(P, modes, a, dt)
    c_re, c_im, _, _ = data(modes, m, dt)
    n = int(np.prod(modes))
    out = tuple(torch.zeros(n, dtype=torch.float64, device="cuda") for _ in range(2))
    work = torch.empty(planner.workspace_len(1), dtype=torch.float64, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on the capture stream
        t1(c_re, c_im, planner, out=out, work=work)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        t1(c_re, c_im, planner, out=out, work=work)
    for pts in (a, b):
        if pts is b:
            planner.set_points(*on_device(b))
        out[0].zero_()
        out[1].zero_()
        g.replay()
        torch.cuda.synchronize()
        want = t1(c_re, c_im, host_planner(P, modes, pts, dt))
        torch.cuda.synchronize()
        assert_equal([o.reshape(-1) for o in out], [w.reshape(-1) for w in want], "A" if pts is a else "B")


@pytest.mark.parametrize("dims", [1, 2, 3])
def test_points_that_are_not_finite(gpu, dims):
    """NaN or an infinity at the first, a middle or the last point of each coordinate array: from_device raises and leaves no
    planner; set_points raises and the planner still gives the bits of its old points"""
    P = gpu
    modes, m = SMALL[dims]
    dt = "f64"
    cls, _ = classes(P, dims, dt)
    good = points("u", modes, m, dt, seed=6)
    planner = device_planner(P, modes, good, dt)
    want = outputs(P, planner, modes, m, dt)
    bad_values = (float("nan"), float("inf"), -float("inf"))
    for axis in range(dims):
        for k, at in enumerate((0, m // 2, m - 1)):
            bad = [p.copy() for p in good]
            bad[axis][at] = bad_values[(axis + k) % 3]
            with pytest.raises(P.PhastPanic) as e:
                cls.from_device(n_arg(modes), *on_device(bad), EPS[dt])
            assert e.value.code == INVALID_ARG
            with pytest.raises(P.PhastPanic) as e:
                planner.set_points(*on_device(bad))
            assert e.value.code == INVALID_ARG
            assert_equal(outputs(P, planner, modes, m, dt), want, (axis, at))


@pytest.mark.parametrize("dims", [1, 2, 3])
def test_what_is_not_a_point_set_in_device_memory(gpu, dims):
    """another M is PHAST_ERR_PLANNER_SIZE; a host tensor, a non-contiguous tensor or a float32 tensor is a TypeError, never a
    silent copy"""
    import torch

    P = gpu
    modes, m = SMALL[dims]
    dt = "f32"
    cls, _ = classes(P, dims, dt)
    good = points("u", modes, m, dt, seed=7)
    planner = device_planner(P, modes, good, dt)
    want = outputs(P, planner, modes, m, dt)
    for other in (m - 1, m + 1):
        with pytest.raises(P.PhastPanic) as e:
            planner.set_points(*on_device(points("u", modes, other, dt)))
        assert e.value.code == PLANNER_SIZE
    dev = on_device(good)
    wrong = {"host": torch.from_numpy(good[-1]), "strided": torch.from_numpy(np.repeat(good[-1], 2)).cuda()[::2], "float32": dev[-1].float(),
             "numpy": good[-1]}
    assert not wrong["strided"].is_contiguous()
    for what, v in wrong.items():
        with pytest.raises(TypeError):
            planner.set_points(*dev[:-1], v)
        with pytest.raises(TypeError):
            cls.from_device(n_arg(modes), *dev[:-1], v)
    assert_equal(outputs(P, planner, modes, m, dt), want, "untouched")


def test_null_pointers_and_a_capturing_stream_through_the_c_abi(gpu):
    import torch

    from phastft_amd import _lib

    P = gpu
    lib = _lib.lib()
    m = 100
    x, y, z = on_device(points("u", (5, 7, 3), m, "f64", seed=8))
    h = C.c_void_p()
    null = None
    for sfx in ("64", "32"):
        eps = EPS["f64" if sfx == "64" else "f32"]
        new1, new2, new3 = (getattr(lib, f"phast_planner_nufft{d}{sfx}_new_dev") for d in ("", "2d", "3d"))
        set1, set2, set3 = (getattr(lib, f"phast_planner_nufft{d}{sfx}_set_points_dev") for d in ("", "2d", "3d"))
        px, py, pz = (C.c_void_p(v.data_ptr()) for v in (x, y, z))
        assert new1(16, null, m, eps, null, C.byref(h)) == INVALID_ARG and not h.value
        assert new1(16, px, m, eps, null, null) == INVALID_ARG
        assert new2(5, 7, px, null, m, eps, null, C.byref(h)) == INVALID_ARG and not h.value
        assert new3(5, 7, 3, px, py, null, m, eps, null, C.byref(h)) == INVALID_ARG and not h.value
        assert new1(0, px, m, eps, null, C.byref(h)) == INVALID_ARG and not h.value     # the size rules of _new
        assert new1(16, px, m, 0.5, null, C.byref(h)) == INVALID_ARG and not h.value
        p1, p3 = device_planner(P, (16,), [v.cpu().numpy() for v in (x,)], "f64" if sfx == "64" else "f32"), None
        p3 = device_planner(P, (5, 7, 3), [v.cpu().numpy() for v in (x, y, z)], "f64" if sfx == "64" else "f32")
        assert set1(null, px, m, null) == INVALID_ARG
        assert set1(p1._h, null, m, null) == INVALID_ARG
        assert set3(p3._h, px, null, pz, m, null) == INVALID_ARG
        assert set3(p3._h, px, py, pz, m + 1, null) == PLANNER_SIZE
        # a stream that is capturing: refused, and the capture goes on undisturbed
        side = torch.cuda.Stream()
        g = torch.cuda.CUDAGraph()
        filled = torch.zeros(8, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=side):
            s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            rc_set = set1(p1._h, px, m, s)
            rc_new = new1(16, px, m, eps, s, C.byref(h))
            rc_set3 = set3(p3._h, px, py, pz, m, s)
            filled.add_(1.0)
        assert (rc_set, rc_new, rc_set3) == (INVALID_ARG, INVALID_ARG, INVALID_ARG) and not h.value
        g.replay()
        torch.cuda.synchronize()
        assert float(filled.sum()) == 8.0
        assert set1(p1._h, px, m, null) == 0 and set2 is not None


def test_points_made_on_a_side_stream(gpu):
    """the points are written by work queued on a side stream, and the planner is built (then re-pointed) with that stream and no
    synchronisation by the caller: the call orders itself after the stream's earlier work"""
    import torch

    P = gpu
    modes, m, dt = (256,), 100003, "f64"
    a, b = points("u", modes, m, dt, seed=9), points("c", modes, m, dt, seed=10)
    src_a, src_b = on_device(a)[0], on_device(b)[0]
    pts = torch.zeros(m, dtype=torch.float64, device="cuda")
    busy = torch.randn(2048, 2048, device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(20):  # the points arrive late on this stream
            busy = busy @ busy * 1e-3
        pts.copy_(src_a)
    planner = P.PlannerNufft64.from_device(modes[0], pts, EPS[dt], stream=side)
    assert_equal(outputs(P, planner, modes, m, dt), outputs(P, host_planner(P, modes, a, dt), modes, m, dt), "A")
    with torch.cuda.stream(side):
        for _ in range(20):
            busy = busy @ busy * 1e-3
        pts.copy_(src_b)
    planner.set_points(pts, stream=side)
    assert_equal(outputs(P, planner, modes, m, dt), outputs(P, host_planner(P, modes, b, dt), modes, m, dt), "B")
