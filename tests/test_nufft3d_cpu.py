"""The three-dimensional non-uniform FFT (csrc/nufft_nd.hpp, csrc/planner_nufft_nd.hpp) without a GPU: the host half of nufft_nd.hpp
compiled with plain g++ (tests/cpp/nufft3d_test.cpp) and held against Python integers -- the argument rule and the binning by
the combined cell; a numpy model of the schedule against tests/nufft3d_reference.py at every shape of tests/test_gpu_nufft3d.py;
the new C ABI exported and listed, with every argument rule returned before the device is touched.

The gate of a transform asked for eps on a fine grid of G = g1 g2 g3 points (nufft3d_gate): C_EPS_3D[dt] * eps +
tolerances.rel_gate(dt, log2 G) for the rel-L2 and C_EPS_3D[dt] * eps + tolerances.bin_gate(dt, log2 G) for the worst element /
rms.  C_EPS_3D is one number per type and comes from the MODEL, not from the device: the smallest of 8, 10, 12, 16, 20, 24, 32,
40, 48, 64, 96, 128 that leaves every entry of the numpy model of the schedule against the long double direct sum -- every shape,
eps, type, direction, complex and real data -- a factor 2 (test_gates_keep_their_margin here asserts exactly that; the model's
need is 11.66 for f64, at (2, 3, 4, 5) and eps = 1e-3, and 7.55 for f32, at the same shape and eps = 1e-2).  The device's own
entries (tests/golden/nufft3d_error_budget.json, measured on the MI355X) are held to the same factor 2 by the same test once the
file exists."""
import ctypes as C
import functools
import json
import os
import subprocess

import numpy as np
import pytest

from tests import nufft3d_reference as R
from tests import tolerances as tol
from tests.test_nufft_cpu import _exact

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = os.path.join(ROOT, "tests", "golden", "nufft3d_error_budget.json")
NEW = [f"phast_planner_nufft3d{s}_{w}" for s in ("64", "32")
       for w in ("new", "free", "describe", "device_bytes", "grid_len", "grid_dim", "width", "workspace_len", "time_stages")]
NEW += [f"phast_nufft3d{t}_{s}{suffix}" for t in (1, 2) for s in ("64", "32") for suffix in ("", "_with_planner", "_dev")]
OK, NO_DEVICE, INVALID_ARG = 0, 15, 16
C_EPS_3D = {"f64": 12.0, "f32": 8.0}
SERIES = (8, 10, 12, 16, 20, 24, 32, 40, 48, 64, 96, 128)
DTS = ["f64", "f32"]
# (direction, real data, seed) of the model's runs: both directions, complex and real data, both seeds -- what the device's budget
# takes its worst over (tests/test_gpu_nufft3d.py: measure)
MODEL_RUNS = tuple((d, real, seed) for seed in R.SEEDS for d in (R.FORWARD, R.REVERSE) for real in (False, True))


def nufft3d_gate(dt, grid_len, eps):
    """(rel-L2, worst element / rms) of a transform asked for eps on a fine grid of grid_len = g1 g2 g3 points"""
    log_g = grid_len.bit_length() - 1
    return C_EPS_3D[dt] * eps + tol.rel_gate(dt, log_g), C_EPS_3D[dt] * eps + tol.bin_gate(dt, log_g)


def grid_len(shape, eps):
    w = R.width(eps)
    return R.grid(shape[0], w) * R.grid(shape[1], w) * R.grid(shape[2], w)


@functools.lru_cache(maxsize=None)
def reference(shape):
    """the long double reference of a shape: computed once, shared, left unchanged"""
    ref = R.Reference(shape)
    for pair in ref.ref.values():
        for a in pair:
            a.flags.writeable = False
    return ref


@functools.lru_cache(maxsize=None)
def model_entry(shape, dt, eps, t):
    """(worst rel-L2, worst element / rms) of the numpy model of the schedule against the direct sum over MODEL_RUNS: double
    arithmetic for f64, float32 kernel values, grid and tables for f32"""
    ref = reference(shape)
    n1, n2, n3 = shape[:3]
    rel = worst = 0.0
    for d, real, seed in MODEL_RUNS:
        got = R.model(t, ref.x, ref.y, ref.z, ref.inp(t, real, seed), n1, n2, n3, eps, d, np.float64 if dt == "f64" else np.float32)
        want = ref.ref[(t, d, real, seed)]
        rel, worst = max(rel, tol.rel_l2(got.real, got.imag, *want)), max(worst, tol.max_bin_err(got.real, got.imag, *want))
    return rel, worst


def need(dt, glen, eps, rel, worst):
    """the constant an entry asks of the gate for a factor 2"""
    log_g = glen.bit_length() - 1
    return max((2 * rel - tol.rel_gate(dt, log_g)) / eps, (2 * worst - tol.bin_gate(dt, log_g)) / eps)


@pytest.fixture(scope="module")
def helpers(tmp_path_factory):
    so = tmp_path_factory.mktemp("nufft3d_helpers") / "libnufft3dhelpers.so"
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-shared", "-fPIC", "-I", os.path.join(ROOT, "phastft_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "nufft3d_test.cpp"), "-o", str(so)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    h = C.CDLL(str(so))
    u, d, p = C.c_ulonglong, C.c_double, C.c_void_p
    h.nufft3d_t_bad_args.argtypes = [u, u, u, u, p, p, p, d, C.c_int]
    h.nufft3d_t_bin.argtypes, h.nufft3d_t_bin.restype = [p, p, p, C.c_size_t, C.c_uint, C.c_uint, C.c_uint, p, p, p, p, p], None
    h.nufft3d_t_tile.argtypes, h.nufft3d_t_tile.restype = [p], None
    return h


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


NAN, INF = float("nan"), float("inf")
P1 = ([0.1], [0.2], [0.3])
BAD = [  # (n1, n2, n3, (x, y, z) each a list or None, m_points or None for len(x), eps, f32)
    (0, 4, 4, P1, None, 1e-6, False), (4, 0, 4, P1, None, 1e-6, False), (4, 4, 0, P1, None, 1e-6, False),
    (2 ** 9, 2 ** 9, 2 ** 8, P1, None, 1e-6, False),               # G = 2^10 2^10 2^9 = 2^29: just above
    (2 ** 9, 2 ** 8, 2 ** 9, P1, None, 1e-6, False), (2 ** 8, 2 ** 9, 2 ** 9, P1, None, 1e-6, False),
    (2 ** 21, 1, 1, P1, None, 1e-6, False),                        # G = 2^22 16 16 = 2^30: the width's 2w rules the short axes
    (2 ** 19, 1, 1, P1, None, 1e-14, False),                       # G = 2^20 32 32 = 2^30: the same modes pass at eps = 1e-1
    (2 ** 40, 2 ** 40, 2 ** 40, P1, None, 1e-6, False), (2 ** 63, 1, 1, P1, None, 1e-6, False), (1, 1, 2 ** 63, P1, None, 1e-6, False),
    (2 ** 28, 2 ** 28, 2 ** 28, P1, None, 1e-1, False),            # every g_i = 2^29: the product overflows 64 bits
    (4, 4, 4, P1, 0, 1e-6, False), (4, 4, 4, P1, 2 ** 30 + 1, 1e-6, False),
    (4, 4, 4, (None, [0.2], [0.3]), 1, 1e-6, False), (4, 4, 4, ([0.1], None, [0.3]), 1, 1e-6, False), (4, 4, 4, ([0.1], [0.2], None), 1, 1e-6, False),
    (4, 4, 4, P1, None, 0.9e-14, False), (4, 4, 4, P1, None, 0.11, False), (4, 4, 4, P1, None, NAN, False),
    (4, 4, 4, P1, None, 0.0, False), (4, 4, 4, P1, None, -1e-3, False), (4, 4, 4, P1, None, 0.9e-6, True),
    (4, 4, 4, ([0.1, NAN], [0.2, 0.3], [0.4, 0.5]), None, 1e-6, False), (4, 4, 4, ([0.1, 0.2], [INF, 0.3], [0.4, 0.5]), None, 1e-6, False),
    (4, 4, 4, ([0.1, 0.2, 0.3], [0.1, 0.2, 0.3], [0.1, 0.2, -INF]), None, 1e-3, True),
    (4, 4, 4, ([0.1, 0.2], [0.1, 0.2], [NAN, 0.3]), None, 1e-3, False)]
GOOD = [(1, 1, 1, ([0.0], [0.0], [0.0]), None, 1e-14, False),
        (2 ** 9, 2 ** 8, 2 ** 8, ([1e300, -5.0], [0.5, -1e300], [-0.0, 3.25]), None, 1e-1, False),   # G = 2^10 2^9 2^9 = 2^28: at the limit
        (2 ** 8, 2 ** 8, 2 ** 9, P1, None, 1e-6, False),                # at the limit, the long axis last
        (2 ** 21, 1, 1, P1, None, 1e-1, False),                         # G = 2^22 8 8 = 2^28
        (2 ** 17, 1, 1, P1, None, 1e-14, False),                        # G = 2^18 32 32 = 2^28: w = 15 widens the one-mode axes
        (1, 1, 2 ** 19, P1, None, 1e-6, False),                         # G = 16 16 2^20 = 2^28
        (4, 4, 4, P1, None, 1e-6, True)]


def _bad_case(h, case):
    n1, n2, n3, pts, m, eps, f32 = case
    x, y, z = (None if v is None else np.array(v, np.float64) for v in pts)
    count = m if m is not None else len(pts[0])
    return bool(h.nufft3d_t_bad_args(n1, n2, n3, count, ptr(x), ptr(y), ptr(z), eps, int(f32)))


def test_argument_rule(helpers):
    """N_i >= 1, G <= 2^28 without overflow (just above and at the limit), the count of points, the three arrays, eps and
    every coordinate finite"""
    for case in BAD:
        assert _bad_case(helpers, case), case
    for case in GOOD:
        assert not _bad_case(helpers, case), case
    for n1, n2, n3, _, _, eps, _ in GOOD:   # the rule is G <= 2^28, with Python integers
        w = R.width(eps)
        assert R.grid(n1, w) * R.grid(n2, w) * R.grid(n3, w) <= 2 ** 28
    for n1, n2, n3, _, _, eps, _ in BAD[3:8]:
        w = R.width(eps)
        assert R.grid(n1, w) * R.grid(n2, w) * R.grid(n3, w) > 2 ** 28


def test_tile_constants(helpers):
    """the spread kernel's tile is one 256-thread workgroup of powers of two <= 8 per axis (every grid is whole tiles, g_i >= 8)
    and a pass through LDS stages at most one point per thread"""
    t = (C.c_uint * 4)()
    helpers.nufft3d_t_tile(t)
    t1, t2, t3, chunk = list(t)
    assert t1 * t2 * t3 == 256 and all(v in (1, 2, 4, 8) for v in (t1, t2, t3)) and 1 <= chunk <= 256


def test_every_bad_argument_is_refused_before_the_device():
    """PHAST_ERR_INVALID_ARG from _new and the one-shot forms whether or not a GPU is there; a good call gets past the check
    (here: to the device, or to PHAST_ERR_NO_DEVICE); null-handle getters return 0"""
    from phastft_amd import _lib

    lib = _lib.lib()
    for sfx, dt in (("64", np.float64), ("32", np.float32)):
        new = getattr(lib, f"phast_planner_nufft3d{sfx}_new")
        v, o = np.zeros(64, dt), np.zeros(64, dt)
        for n1, n2, n3, pts, m, eps, f32 in BAD:
            if eps == 0.9e-6 and sfx == "64":
                continue  # inside f64's range
            x, y, z = (None if a is None else np.array(a, np.float64) for a in pts)
            count = m if m is not None else len(pts[0])
            h = C.c_void_p(1)
            assert new(n1, n2, n3, ptr(x), ptr(y), ptr(z), count, eps, C.byref(h)) == INVALID_ARG, (sfx, n1, n2, n3, pts, m, eps)
            assert h.value is None
            for t in (1, 2):
                shot = getattr(lib, f"phast_nufft3d{t}_{sfx}")
                assert shot(ptr(x), ptr(y), ptr(z), count, ptr(v), ptr(v), ptr(o), ptr(o), n1, n2, n3, eps, 1) == INVALID_ARG
        x, y, z = (np.array(a, np.float64) for a in ([0.1, 0.2], [0.3, 0.4], [0.5, 0.6]))
        assert new(2, 2, 2, ptr(x), ptr(y), ptr(z), 2, 1e-3, None) == INVALID_ARG
        h = C.c_void_p()
        rc = new(2, 2, 2, ptr(x), ptr(y), ptr(z), 2, 1e-3, C.byref(h))
        assert rc in (OK, NO_DEVICE)
        if rc == OK:
            getattr(lib, f"phast_planner_nufft3d{sfx}_free")(h)
        for t in (1, 2):
            assert getattr(lib, f"phast_nufft3d{t}_{sfx}")(ptr(x), ptr(y), ptr(z), 2, None, ptr(v), ptr(o), ptr(o), 2, 2, 2, 1e-3, 1) == INVALID_ARG
            assert getattr(lib, f"phast_nufft3d{t}_{sfx}_with_planner")(ptr(v), ptr(v), 2, ptr(o), ptr(o), 8, 1, None) == INVALID_ARG
            assert getattr(lib, f"phast_nufft3d{t}_{sfx}_dev")(ptr(v), ptr(v), 2, ptr(o), ptr(o), 8, 1, 1, None, ptr(o), 8, None) == INVALID_ARG
        for name in ("grid_len", "width", "device_bytes"):
            assert getattr(lib, f"phast_planner_nufft3d{sfx}_{name}")(None) == 0
        assert getattr(lib, f"phast_planner_nufft3d{sfx}_grid_dim")(None, 1) == 0
        assert getattr(lib, f"phast_planner_nufft3d{sfx}_workspace_len")(None, 3) == 0


def test_new_symbols_are_exported_and_listed():
    from phastft_amd import _lib

    lib = _lib.lib()
    for name in NEW:
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    import phastft_amd as P

    for name in ("PlannerNufft3d64", "PlannerNufft3d32", "nufft3d1_batched", "nufft3d2_batched", "nufft3d1", "nufft3d2"):
        assert name in P.__all__ and hasattr(P, name), name
    for t in (1, 2):
        for sfx in ("64", "32"):
            for tail in ("", "_with_planner"):
                assert f"nufft3d{t}_{sfx}{tail}" in P.__all__ and hasattr(P, f"nufft3d{t}_{sfx}{tail}")


def binning_points(gs, count=2000):
    """points on cell edges of every axis, both wraps, a clump inside one cell, a narrow band that leaves most cells empty"""
    rng = np.random.default_rng(7)
    edges = [np.concatenate([np.arange(g) / g, (np.arange(g) + 1) / g - 2.0 ** -53, -np.arange(1, g + 1) / g]) for g in gs]
    k = max(len(e) for e in edges)
    edges = [np.resize(e if i == 0 else e[::-1] if i == 1 else np.roll(e, 3), k) for i, e in enumerate(edges)]
    spot = (0.3, 0.7, 0.55)
    clump = [(int(s * g) + 0.001 + 0.998 * rng.random(300)) / g + 4.0 - 3.0 * i for i, (s, g) in enumerate(zip(spot, gs))]
    band = [rng.uniform(-3, 3, count), 0.61 + 0.01 * rng.uniform(-3, 3, count) * (rng.random(count) < 0.5), rng.uniform(-3, 3, count)]
    tail = [0.0, 1e-300, -1e-300, 0.5, 2.0 ** -60, -(2.0 ** -60), 1 - 2.0 ** -53]
    sp = [R.SPECIALS, R.SPECIALS[::-1], list(np.roll(R.SPECIALS, -2))]
    tails = [tail, tail[::-1], tail[2:] + tail[:2]]
    return tuple(np.concatenate([sp[i], edges[i], clump[i], band[i], tails[i]]) for i in range(3))


@pytest.mark.parametrize("logs", [(3, 3, 3), (3, 5, 4), (6, 3, 4)], ids=lambda s: f"{s[0]}_{s[1]}_{s[2]}")
def test_binning(helpers, logs):
    """nufft_nd_bin<3> against a numpy stable argsort of the combined cell (q1 g2 + q2) g3 + q3, q_i = floor(frac(coordinate) g_i)
    with frac exact in Python integers: the permutation, the cell starts and the kept positions (in the same cell, below 1)"""
    gs = tuple(1 << v for v in logs)
    pts = binning_points(gs)
    m, cells = len(pts[0]), gs[0] * gs[1] * gs[2]
    kept = [np.zeros(m) for _ in range(3)]
    perm, start = np.zeros(m, np.uint32), np.zeros(cells + 1, np.uint32)
    helpers.nufft3d_t_bin(ptr(pts[0]), ptr(pts[1]), ptr(pts[2]), m, logs[0], logs[1], logs[2], ptr(kept[0]), ptr(kept[1]), ptr(kept[2]), ptr(perm),
                          ptr(start))
    exact = [[_exact(v) for v in p] for p in pts]
    q = [np.array([f >> (128 - lg) for f in ex], np.int64) for ex, lg in zip(exact, logs)]
    cell = (q[0] * gs[1] + q[1]) * gs[2] + q[2]
    assert np.array_equal(perm, np.argsort(cell, kind="stable"))
    counts = np.bincount(cell, minlength=cells)
    assert np.array_equal(start, np.concatenate([[0], np.cumsum(counts)]))
    assert counts.max() >= 300 and all(qi.min() == 0 and qi.max() == g - 1 for qi, g in zip(q, gs))
    for i in range(m):
        j = perm[i]
        for axis in range(3):
            v, f, g = kept[axis][i], exact[axis][j], gs[axis]
            assert 0.0 <= v < 1.0 and int(v * g) == q[axis][j]
            k = int(v * 2.0 ** 64) << 64 if v >= 2.0 ** -11 else None   # (exact: v has 53 bits at most)
            assert k is None or (k <= f and f - k < max(1, f >> 52)), (i, axis, pts[axis][j])
    # points on cell edges lie in the cell they open; the last double below an edge in the cell it closes
    g1 = gs[0]
    assert np.array_equal(q[0][5:5 + g1], np.arange(g1)) and np.array_equal(q[0][5 + g1:5 + 2 * g1], np.arange(g1))
    assert np.array_equal(q[0][5 + 2 * g1:5 + 3 * g1], (g1 - np.arange(1, g1 + 1)) % g1)   # the negative edges wrap
    assert q[0][0] == 0 and q[1][0] == 0 and q[0][1] == g1 - 1 and q[1][3] == gs[1] - 1 and q[2][4] == gs[2] - 1


@pytest.mark.parametrize("shape", R.SHAPES, ids=R.shape_id)
def test_schedule_model_against_the_reference(shape):
    """the schedule in numpy against the direct sum, both types, both directions, complex and real data, within nufft3d_gate"""
    for dt in DTS:
        for eps in R.EPS[dt]:
            g_rel, g_bin = nufft3d_gate(dt, grid_len(shape, eps), eps)
            for t in (1, 2):
                rel, worst = model_entry(shape, dt, eps, t)
                print(f"model nufft3d{t} {R.shape_id(shape)} {dt} eps {eps:g}: rel {rel:.3e} / {g_rel:.3e}, element {worst:.3e} / {g_bin:.3e}")
                assert rel <= g_rel and worst <= g_bin, (shape, dt, eps, t, rel, g_rel, worst, g_bin)


def test_gates_keep_their_margin():
    """C_EPS_3D is the smallest number of its series that leaves every entry of the MODEL a factor 2 -- the constant is fixed
    here, on the CPU, independent of the kernels -- and once the device's budget is recorded every entry of it keeps the same
    factor 2 and none is missing"""
    model_need = {dt: 0.0 for dt in DTS}
    for dt in DTS:
        for shape in R.SHAPES:
            for eps in R.EPS[dt]:
                for t in (1, 2):
                    rel, worst = model_entry(shape, dt, eps, t)
                    g_rel, g_bin = nufft3d_gate(dt, grid_len(shape, eps), eps)
                    assert g_rel >= 2 * rel and g_bin >= 2 * worst, (shape, dt, eps, t, rel, g_rel, worst, g_bin)
                    model_need[dt] = max(model_need[dt], need(dt, grid_len(shape, eps), eps, rel, worst))
    print("the model asks for", model_need)
    for dt in DTS:
        assert C_EPS_3D[dt] == min(c for c in SERIES if c >= model_need[dt]), (dt, model_need[dt], C_EPS_3D[dt])
    if not os.path.exists(BUDGET):
        return
    budget = json.load(open(BUDGET))
    want = {(dt, *shape, eps, t) for dt in DTS for shape in R.SHAPES for eps in R.EPS[dt] for t in (1, 2)}
    have = {(e["dt"], e["n1"], e["n2"], e["n3"], e["m"], e["kind"], e["eps"], e["type"]) for e in budget["entries"]}
    assert have == want and len(budget["entries"]) == len(want)
    for e in budget["entries"]:
        g_rel, g_bin = nufft3d_gate(e["dt"], e["grid_len"], e["eps"])
        assert g_rel >= 2 * e["rel"] and g_bin >= 2 * e["bin"], e


def test_reference_special_cases():
    """the direct sum on the grid points (j1 / N1, j2 / N2, j3 / N3) is numpy's fftn, its type 2 Reverse numpy's ifftn * N1 N2 N3;
    with N3 = 1 it is the two-dimensional direct sum of (x, y), with N2 = N3 = 1 the one-dimensional one of x"""
    from tests import nufft2d_reference as R2
    from tests import nufft_reference as R1

    ns = (3, 5, 4)
    j = np.meshgrid(*(np.arange(n) for n in ns), indexing="ij")
    x, y, z = ((ji / n).reshape(-1) for ji, n in zip(j, ns))
    c = R.data(60, 0, "c")
    re, im = R.nufft3d1(x, y, z, c, *ns)
    assert np.max(np.abs(re.astype(np.float64) + 1j * im.astype(np.float64) - np.fft.fftn(c.reshape(ns)).reshape(-1))) < 1e-13
    re, im = R.nufft3d2(x, y, z, c, *ns, R.REVERSE)
    assert np.max(np.abs(re.astype(np.float64) + 1j * im.astype(np.float64) - np.fft.ifftn(c.reshape(ns)).reshape(-1) * 60)) < 1e-13
    x, y, z = R.points(9, 4, 1, 50)
    c, f = R.data(50, 1, "c"), R.data(36, 1, "f")
    a, b = R.nufft3d1(x, y, z, c, 9, 4, 1), R2.nufft2d1(x, y, c, 9, 4)
    assert max(np.max(np.abs(a[0] - b[0])), np.max(np.abs(a[1] - b[1]))) < 1e-15   # another order of the same long double sum
    a, b = R.nufft3d2(x, y, z, f, 9, 4, 1), R2.nufft2d2(x, y, f, 9, 4)
    assert max(np.max(np.abs(a[0] - b[0])), np.max(np.abs(a[1] - b[1]))) < 1e-15
    a, b = R.nufft3d1(x, y, z, c, 9, 1, 1), R1.nufft1(x, c, 9)
    assert max(np.max(np.abs(a[0] - b[0])), np.max(np.abs(a[1] - b[1]))) < 1e-15
