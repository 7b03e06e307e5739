"""The two-dimensional non-uniform FFT (csrc/nufft_nd.hpp, csrc/planner_nufft_nd.hpp) without a GPU: the host half of nufft_nd.hpp
compiled with plain g++ (tests/cpp/nufft2d_test.cpp) and held against Python integers -- the argument rule and the binning by
the combined cell; a numpy model of the schedule against tests/nufft2d_reference.py at every shape of tests/test_gpu_nufft2d.py
(the CPU leg of the gate); the new C ABI exported and listed, with every argument rule returned before the device is touched.

The gate of a transform asked for eps on a fine grid of G = g1 g2 points (nufft2d_gate): C_EPS_2D[dt] * eps +
tolerances.rel_gate(dt, log2 G) for the rel-L2 and C_EPS_2D[dt] * eps + tolerances.bin_gate(dt, log2 G) for the worst element /
rms.  C_EPS_2D is one number per type: the smallest of 8, 10, 12, 16, 20, 24, 32, 40, 48, 64 that leaves every entry of
tests/golden/nufft2d_error_budget.json (measured on the MI355X) a factor 2 (tests/test_gpu_nufft2d.py:
test_gates_keep_their_margin); the model here stays below the same gates."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import nufft2d_reference as R
from tests import tolerances as tol
from tests.test_nufft_cpu import _exact

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = [f"phast_planner_nufft2d{s}_{w}" for s in ("64", "32")
       for w in ("new", "free", "describe", "device_bytes", "grid_len", "grid_rows", "grid_cols", "width", "workspace_len", "time_stages")]
NEW += [f"phast_nufft2d{t}_{s}{suffix}" for t in (1, 2) for s in ("64", "32") for suffix in ("", "_with_planner", "_dev")]
OK, NO_DEVICE, INVALID_ARG = 0, 15, 16
C_EPS_2D = {"f64": 32.0, "f32": 16.0}


def nufft2d_gate(dt, grid_len, eps):
    """(rel-L2, worst element / rms) of a transform asked for eps on a fine grid of grid_len = g1 g2 points"""
    log_g = grid_len.bit_length() - 1
    return C_EPS_2D[dt] * eps + tol.rel_gate(dt, log_g), C_EPS_2D[dt] * eps + tol.bin_gate(dt, log_g)


@functools.lru_cache(maxsize=None)
def reference(shape):
    """the long double reference of a shape: computed once, shared, left unchanged"""
    ref = R.Reference(shape)
    for pair in ref.ref.values():
        for a in pair:
            a.flags.writeable = False
    return ref


@pytest.fixture(scope="module")
def helpers(tmp_path_factory):
    so = tmp_path_factory.mktemp("nufft2d_helpers") / "libnufft2dhelpers.so"
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-shared", "-fPIC", "-I", os.path.join(ROOT, "phastft_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "nufft2d_test.cpp"), "-o", str(so)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    h = C.CDLL(str(so))
    u, d, p = C.c_ulonglong, C.c_double, C.c_void_p
    h.nufft2d_t_bad_args.argtypes = [u, u, u, p, p, d, C.c_int]
    h.nufft2d_t_bin.argtypes, h.nufft2d_t_bin.restype = [p, p, C.c_size_t, C.c_uint, C.c_uint, p, p, p, p], None
    return h


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


NAN, INF = float("nan"), float("inf")
BAD = [  # (n1, n2, x or None, y or None, m_points or None for len(x), eps, f32)
    (0, 4, [0.1], [0.2], None, 1e-6, False), (4, 0, [0.1], [0.2], None, 1e-6, False),
    (2 ** 13, 2 ** 14, [0.1], [0.2], None, 1e-6, False),          # G = 2^14 2^15 = 2^29
    (2 ** 27, 2, [0.1], [0.2], None, 1e-6, False),                # G = 2^28 2^4: the width's 2w rules the short axis
    (1, 2 ** 26, [0.1], [0.2], None, 1e-6, False),                # G = 16 2^27
    (2 ** 23, 1, [0.1], [0.2], None, 1e-14, False),               # G = 2^24 32: the same modes pass at eps = 1e-1
    (2 ** 40, 2 ** 40, [0.1], [0.2], None, 1e-6, False), (2 ** 63, 1, [0.1], [0.2], None, 1e-6, False),
    (4, 4, [0.1], [0.2], 0, 1e-6, False), (4, 4, [0.1], [0.2], 2 ** 30 + 1, 1e-6, False),
    (4, 4, None, [0.2], 1, 1e-6, False), (4, 4, [0.1], None, 1, 1e-6, False),
    (4, 4, [0.1], [0.2], None, 0.9e-14, False), (4, 4, [0.1], [0.2], None, 0.11, False), (4, 4, [0.1], [0.2], None, NAN, False),
    (4, 4, [0.1], [0.2], None, 0.0, False), (4, 4, [0.1], [0.2], None, -1e-3, False), (4, 4, [0.1], [0.2], None, 0.9e-6, True),
    (4, 4, [0.1, NAN], [0.2, 0.3], None, 1e-6, False), (4, 4, [0.1, 0.2], [INF, 0.3], None, 1e-6, False),
    (4, 4, [0.1, 0.2, 0.3], [0.1, 0.2, -INF], None, 1e-3, True)]
GOOD = [(1, 1, [0.0], [0.0], None, 1e-14, False), (2 ** 13, 2 ** 13, [1e300, -5.0], [0.5, -1e300], None, 1e-1, False),
        (1, 2 ** 24, [0.1], [0.2], None, 1e-1, False),            # G = 8 2^25
        (2 ** 22, 1, [0.1], [0.2], None, 1e-14, False),           # G = 2^23 32 = 2^28: w = 15 widens the one-mode axis
        (2 ** 23, 1, [0.1], [0.2], None, 1e-1, False),            # G = 2^24 8
        (4, 4, [0.1], [0.2], None, 1e-6, True)]


def _bad_case(h, case):
    n1, n2, xs, ys, m, eps, f32 = case
    x, y = (None if v is None else np.array(v, np.float64) for v in (xs, ys))
    count = m if m is not None else len(xs)
    return bool(h.nufft2d_t_bad_args(n1, n2, count, ptr(x), ptr(y), eps, int(f32)))


def test_argument_rule(helpers):
    for case in BAD:
        assert _bad_case(helpers, case), case
    for case in GOOD:
        assert not _bad_case(helpers, case), case
    for n1, n2, eps in ((2 ** 13, 2 ** 13, 1e-6), (100, 70, 1e-12), (1, 1, 1e-14), (2 ** 22, 1, 1e-14)):   # the rule is G <= 2^28
        w = R.width(eps)
        assert R.grid(n1, w) * R.grid(n2, w) <= 2 ** 28


def test_every_bad_argument_is_refused_before_the_device():
    """PHAST_ERR_INVALID_ARG from _new and the one-shot forms whether or not a GPU is there; a good call gets past the check
    (here: to the device, or to PHAST_ERR_NO_DEVICE); null-handle getters return 0"""
    from phastft_amd import _lib

    lib = _lib.lib()
    for sfx, dt in (("64", np.float64), ("32", np.float32)):
        new = getattr(lib, f"phast_planner_nufft2d{sfx}_new")
        v, o = np.zeros(16, dt), np.zeros(16, dt)
        for n1, n2, xs, ys, m, eps, f32 in BAD:
            if eps == 0.9e-6 and sfx == "64":
                continue  # inside f64's range
            x, y = (None if a is None else np.array(a, np.float64) for a in (xs, ys))
            count = m if m is not None else len(xs)
            h = C.c_void_p(1)
            assert new(n1, n2, ptr(x), ptr(y), count, eps, C.byref(h)) == INVALID_ARG, (sfx, n1, n2, xs, ys, m, eps)
            assert h.value is None
            for t in (1, 2):
                shot = getattr(lib, f"phast_nufft2d{t}_{sfx}")
                assert shot(ptr(x), ptr(y), count, ptr(v), ptr(v), ptr(o), ptr(o), n1, n2, eps, 1) == INVALID_ARG
        x, y = np.array([0.1, 0.2], np.float64), np.array([0.3, 0.4], np.float64)
        assert new(2, 2, ptr(x), ptr(y), 2, 1e-3, None) == INVALID_ARG
        h = C.c_void_p()
        rc = new(2, 2, ptr(x), ptr(y), 2, 1e-3, C.byref(h))
        assert rc in (OK, NO_DEVICE)
        if rc == OK:
            getattr(lib, f"phast_planner_nufft2d{sfx}_free")(h)
        for t in (1, 2):
            assert getattr(lib, f"phast_nufft2d{t}_{sfx}")(ptr(x), ptr(y), 2, None, ptr(v), ptr(o), ptr(o), 2, 2, 1e-3, 1) == INVALID_ARG
            assert getattr(lib, f"phast_nufft2d{t}_{sfx}_with_planner")(ptr(v), ptr(v), 2, ptr(o), ptr(o), 4, 1, None) == INVALID_ARG
            assert getattr(lib, f"phast_nufft2d{t}_{sfx}_dev")(ptr(v), ptr(v), 2, ptr(o), ptr(o), 4, 1, 1, None, ptr(o), 8, None) == INVALID_ARG
        for name in ("grid_len", "grid_rows", "grid_cols", "width", "device_bytes"):
            assert getattr(lib, f"phast_planner_nufft2d{sfx}_{name}")(None) == 0
        assert getattr(lib, f"phast_planner_nufft2d{sfx}_workspace_len")(None, 3) == 0


def test_new_symbols_are_exported_and_listed():
    from phastft_amd import _lib

    lib = _lib.lib()
    for name in NEW:
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    import phastft_amd as P

    for name in ("PlannerNufft2d64", "PlannerNufft2d32", "nufft2d1_batched", "nufft2d2_batched", "nufft2d1", "nufft2d2"):
        assert name in P.__all__ and hasattr(P, name), name
    for t in (1, 2):
        for sfx in ("64", "32"):
            for tail in ("", "_with_planner"):
                assert f"nufft2d{t}_{sfx}{tail}" in P.__all__ and hasattr(P, f"nufft2d{t}_{sfx}{tail}")


def binning_points(g1, g2, count=2000):
    """points on cell edges of both axes, both wraps, a clump inside one cell, a narrow band that leaves most cells empty"""
    rng = np.random.default_rng(7)
    edge_x = np.concatenate([np.arange(g1) / g1, (np.arange(g1) + 1) / g1 - 2.0 ** -53, -np.arange(1, g1 + 1) / g1])
    edge_y = np.concatenate([np.arange(g2) / g2, (np.arange(g2) + 1) / g2 - 2.0 ** -53, -np.arange(1, g2 + 1) / g2])
    k = max(len(edge_x), len(edge_y))
    edge_x, edge_y = np.resize(edge_x, k), np.resize(edge_y[::-1], k)
    clump = ((int(0.3 * g1) + 0.001 + 0.998 * rng.random(300)) / g1 + 4.0, (int(0.7 * g2) + 0.001 + 0.998 * rng.random(300)) / g2 - 2.0)
    band = (rng.uniform(-3, 3, count), 0.61 + 0.01 * rng.uniform(-3, 3, count) * (rng.random(count) < 0.5))
    tail = [0.0, 1e-300, -1e-300, 0.5, 2.0 ** -60, -(2.0 ** -60), 1 - 2.0 ** -53]
    x = np.concatenate([R.SPECIALS, edge_x, clump[0], band[0], tail])
    y = np.concatenate([R.SPECIALS[::-1], edge_y, clump[1], band[1], tail[::-1]])
    return x, y


@pytest.mark.parametrize("logs", [(3, 3), (3, 6), (7, 4)], ids=lambda s: f"{s[0]}_{s[1]}")
def test_binning(helpers, logs):
    """nufft_nd_bin<2> against a numpy stable argsort of the combined cell q1 g2 + q2, q_i = floor(frac(coordinate) g_i) with frac
    exact in Python integers: the permutation, the cell starts and the kept positions (in the same cell, below 1)"""
    log_g1, log_g2 = logs
    g1, g2 = 1 << log_g1, 1 << log_g2
    x, y = binning_points(g1, g2)
    m = len(x)
    xs, ys, perm, start = np.zeros(m), np.zeros(m), np.zeros(m, np.uint32), np.zeros(g1 * g2 + 1, np.uint32)
    helpers.nufft2d_t_bin(ptr(x), ptr(y), m, log_g1, log_g2, ptr(xs), ptr(ys), ptr(perm), ptr(start))
    ex, ey = [_exact(v) for v in x], [_exact(v) for v in y]
    q1 = np.array([f >> (128 - log_g1) for f in ex], np.int64)
    q2 = np.array([f >> (128 - log_g2) for f in ey], np.int64)
    cell = q1 * g2 + q2
    assert np.array_equal(perm, np.argsort(cell, kind="stable"))
    counts = np.bincount(cell, minlength=g1 * g2)
    assert np.array_equal(start, np.concatenate([[0], np.cumsum(counts)]))
    assert counts.max() >= 300 and q1.min() == 0 and q1.max() == g1 - 1 and q2.min() == 0 and q2.max() == g2 - 1
    for i in range(m):
        j = perm[i]
        for kept, f, q, g in ((xs[i], ex[j], q1[j], g1), (ys[i], ey[j], q2[j], g2)):
            assert 0.0 <= kept < 1.0 and int(kept * g) == q
            k = int(kept * 2.0 ** 64) << 64 if kept >= 2.0 ** -11 else None   # (exact: kept has 53 bits at most)
            assert k is None or (k <= f and f - k < max(1, f >> 52)), (i, x[j], y[j])
    # points on cell edges lie in the cell they open; the last double below an edge in the cell it closes
    assert np.array_equal(q1[5:5 + g1], np.arange(g1)) and np.array_equal(q1[5 + g1:5 + 2 * g1], np.arange(g1))
    assert np.array_equal(q1[5 + 2 * g1:5 + 3 * g1], (g1 - np.arange(1, g1 + 1)) % g1)   # the negative edges wrap
    assert q1[0] == 0 and q2[0] == 0 and q1[1] == g1 - 1 and q2[3] == g2 - 1


@pytest.mark.parametrize("shape", R.SHAPES, ids=R.shape_id)
def test_schedule_model_against_the_reference(shape):
    """the CPU leg of the gate: the schedule in numpy (double arithmetic for f64's eps, float32 kernel values, grid and tables
    for f32's) against the direct sum, both types, both directions, complex and real data, within nufft2d_gate"""
    ref = reference(shape)
    n1, n2, m, _ = shape
    worst = {}
    for dt, arith in (("f64", np.float64), ("f32", np.float32)):
        for eps in R.EPS[dt]:
            w = R.width(eps)
            g_rel, g_bin = nufft2d_gate(dt, R.grid(n1, w) * R.grid(n2, w), eps)
            for t in (1, 2):
                for d, real, seed in ((R.FORWARD, False, 0), (R.REVERSE, False, 1), (R.FORWARD, True, 1), (R.REVERSE, True, 0)):
                    got = R.model(t, ref.x, ref.y, ref.inp(t, real, seed), n1, n2, eps, d, arith)
                    want = ref.ref[(t, d, real, seed)]
                    rel, worst_bin = tol.rel_l2(got.real, got.imag, *want), tol.max_bin_err(got.real, got.imag, *want)
                    key = (dt, eps, t)
                    worst[key] = max(worst.get(key, (0, 0)), (rel / eps, worst_bin / eps))
                    assert rel <= g_rel and worst_bin <= g_bin, (shape, dt, eps, t, d, real, rel, g_rel, worst_bin, g_bin)
    print(shape, {k: (round(v[0], 2), round(v[1], 2)) for k, v in worst.items()})


def test_reference_special_cases():
    """the direct sum on the grid points (j1 / N1, j2 / N2) is numpy's fft2, its type 2 Reverse numpy's ifft2 * N1 N2; with
    N2 = 1 it is the one-dimensional direct sum of x"""
    from tests import nufft_reference as R1

    n1, n2 = 6, 10
    j1, j2 = np.meshgrid(np.arange(n1), np.arange(n2), indexing="ij")
    x, y = (j1 / n1).reshape(-1), (j2 / n2).reshape(-1)
    c = R.data(n1 * n2, 0, "c")
    re, im = R.nufft2d1(x, y, c, n1, n2)
    assert np.max(np.abs(re.astype(np.float64) + 1j * im.astype(np.float64) - np.fft.fft2(c.reshape(n1, n2)).reshape(-1))) < 1e-13
    re, im = R.nufft2d2(x, y, c, n1, n2, R.REVERSE)
    assert np.max(np.abs(re.astype(np.float64) + 1j * im.astype(np.float64) - np.fft.ifft2(c.reshape(n1, n2)).reshape(-1) * n1 * n2)) < 1e-13
    x, y = R.points(9, 1, 50)
    c = R.data(50, 1, "c")
    a, b = R.nufft2d1(x, y, c, 9, 1), R1.nufft1(x, c, 9)
    assert max(np.max(np.abs(a[0] - b[0])), np.max(np.abs(a[1] - b[1]))) < 1e-15   # another order of the same long double sum
