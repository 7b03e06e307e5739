"""The non-uniform FFT (csrc/nufft.hpp, csrc/planner_nufft.hpp) without a GPU: the host half of nufft.hpp compiled with plain g++
(tests/cpp/nufft_test.cpp) and held against Python integers and numpy -- the argument rules, the width and grid table, the
quadrature of phi^, the truncated positions, the binning; the reference's own integer arithmetic against Python's; a numpy
model of the schedule in double against tests/nufft_reference.py at every shape of tests/test_gpu_nufft.py (the CPU leg of the
gate); the new C ABI exported and listed, with every argument rule returned before the device is touched.

The gate of a transform asked for eps on a grid of n_g points (nufft_gate): C_EPS[dt] * eps + tolerances.rel_gate(dt, log2 n_g)
for the rel-L2 and C_EPS[dt] * eps + tolerances.bin_gate(dt, log2 n_g) for the worst element / rms.  C_EPS is one number per
type, chosen so that every entry of tests/golden/nufft_error_budget.json (measured on the MI355X) keeps a factor 2
(tests/test_gpu_nufft.py: test_gates_keep_their_margin); the model here, in double, stays below the same gates."""
import ctypes as C
import functools
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from tests import nufft_reference as R
from tests import tolerances as tol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = [f"phast_planner_nufft{s}_{w}" for s in ("64", "32")
       for w in ("new", "free", "describe", "device_bytes", "grid_len", "width", "workspace_len", "time_stages")]
NEW += [f"phast_nufft{t}_{s}{suffix}" for t in (1, 2) for s in ("64", "32") for suffix in ("", "_with_planner", "_dev")]
OK, NO_DEVICE, INVALID_ARG = 0, 15, 16
C_EPS = {"f64": 32.0, "f32": 10.0}


def nufft_gate(dt, n_g, eps):
    """(rel-L2, worst element / rms) of a transform asked for eps on a fine grid of n_g points"""
    log_g = n_g.bit_length() - 1
    return C_EPS[dt] * eps + tol.rel_gate(dt, log_g), C_EPS[dt] * eps + tol.bin_gate(dt, log_g)


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
    so = tmp_path_factory.mktemp("nufft_helpers") / "libnuffthelpers.so"
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-shared", "-fPIC", "-I", os.path.join(ROOT, "phastft_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "nufft_test.cpp"), "-o", str(so)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    h = C.CDLL(str(so))
    u, ll, d, p = C.c_ulonglong, C.c_longlong, C.c_double, C.c_void_p
    h.nufft_t_bad_args.argtypes = [u, u, p, d, C.c_int]
    h.nufft_t_width.argtypes = [d]
    h.nufft_t_grid.argtypes, h.nufft_t_grid.restype = [u, C.c_int], u
    h.nufft_t_slot.argtypes, h.nufft_t_slot.restype = [u, u, u], u
    h.nufft_t_first.argtypes, h.nufft_t_first.restype = [C.c_int, d], ll
    h.nufft_t_turns.argtypes, h.nufft_t_turns.restype = [d], d
    h.nufft_t_weight.argtypes, h.nufft_t_weight.restype = [ll, d, C.c_int], d
    h.nufft_t_phi_hat.argtypes, h.nufft_t_phi_hat.restype = [C.c_int, u, p, C.c_size_t, p], None
    h.nufft_t_bin.argtypes, h.nufft_t_bin.restype = [p, C.c_size_t, C.c_uint, p, p, p], None
    return h


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


BAD = [  # (n_modes, points or None, m_points or None for len(points), eps, f32)
    (0, [0.1], None, 1e-6, False), (2 ** 28 + 1, [0.1], None, 1e-6, False), (4, [0.1], 0, 1e-6, False),
    (4, [0.1], 2 ** 30 + 1, 1e-6, False), (4, None, 1, 1e-6, False), (4, [0.1], None, 0.9e-14, False), (4, [0.1], None, 0.11, False),
    (4, [0.1], None, float("nan"), False), (4, [0.1], None, 0.0, False), (4, [0.1], None, -1e-3, False),
    (4, [0.1], None, 0.9e-6, True), (4, [0.1, float("nan")], None, 1e-6, False), (4, [float("inf"), 0.1], None, 1e-6, False),
    (4, [0.1, 0.2, -float("inf")], None, 1e-3, True)]
GOOD = [(1, [0.0], None, 1e-14, False), (2 ** 28, [1e300, -5.0], None, 1e-1, False), (4, [0.1], None, 1e-6, True)]


def test_argument_rule(helpers):
    for n, pts, m, eps, f32 in BAD + GOOD:
        x = None if pts is None else np.array(pts, np.float64)
        count = m if m is not None else len(pts)
        got = helpers.nufft_t_bad_args(n, count, None if x is None else ptr(x), eps, int(f32))
        assert bool(got) == ((n, pts, m, eps, f32) in BAD), (n, pts, m, eps, f32)


def test_every_bad_argument_is_refused_before_the_device():
    """PHAST_ERR_INVALID_ARG from _new and the one-shot forms whether or not a GPU is there; a good call gets past the check
    (here: to the device, or to PHAST_ERR_NO_DEVICE)"""
    from phastft_amd import _lib

    lib = _lib.lib()
    for sfx, dt in (("64", np.float64), ("32", np.float32)):
        new = getattr(lib, f"phast_planner_nufft{sfx}_new")
        v, o = np.zeros(8, dt), np.zeros(8, dt)
        for n, pts, m, eps, f32 in BAD:
            if eps == 0.9e-6 and sfx == "64":
                continue  # inside f64's range
            x = None if pts is None else np.array(pts, np.float64)
            count = m if m is not None else len(pts)
            h = C.c_void_p(1)
            assert new(n, None if x is None else ptr(x), count, eps, C.byref(h)) == INVALID_ARG, (sfx, n, pts, m, eps)
            assert h.value is None
            for t in (1, 2):
                shot = getattr(lib, f"phast_nufft{t}_{sfx}")
                assert shot(None if x is None else ptr(x), count, ptr(v), ptr(v), ptr(o), ptr(o), n, eps, 1) == INVALID_ARG
        x = np.array([0.1, 0.2], np.float64)
        assert new(4, ptr(x), 2, 1e-3, None) == INVALID_ARG
        h = C.c_void_p()
        rc = new(4, ptr(x), 2, 1e-3, C.byref(h))
        assert rc in (OK, NO_DEVICE)
        if rc == OK:
            getattr(lib, f"phast_planner_nufft{sfx}_free")(h)
        for t in (1, 2):
            assert getattr(lib, f"phast_nufft{t}_{sfx}")(ptr(x), 2, None, ptr(v), ptr(o), ptr(o), 4, 1e-3, 1) == INVALID_ARG
            assert getattr(lib, f"phast_nufft{t}_{sfx}_with_planner")(ptr(v), ptr(v), 2, ptr(o), ptr(o), 4, 1, None) == INVALID_ARG
            assert getattr(lib, f"phast_nufft{t}_{sfx}_dev")(ptr(v), ptr(v), 2, ptr(o), ptr(o), 4, 1, 1, None, ptr(o), 8, None) == INVALID_ARG
        for name in ("grid_len", "width", "device_bytes"):
            assert getattr(lib, f"phast_planner_nufft{sfx}_{name}")(None) == 0
        assert getattr(lib, f"phast_planner_nufft{sfx}_workspace_len")(None, 3) == 0


def test_new_symbols_are_exported_and_listed():
    from phastft_amd import _lib

    lib = _lib.lib()
    for name in NEW:
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    import phastft_amd as P

    for name in ("PlannerNufft64", "PlannerNufft32", "nufft1_batched", "nufft2_batched", "nufft1", "nufft2", "nufft1_64",
                 "nufft2_32_with_planner"):
        assert name in P.__all__ and hasattr(P, name), name


# eps -> w: ceil(log10(1 / eps)) + 1 clamped to [2, 16]; decades are exact
WIDTHS = {1e-1: 2, 0.5e-1: 3, 1e-2: 3, 1e-3: 4, 1e-4: 5, 3e-5: 6, 1e-6: 7, 1e-9: 10, 1e-12: 13, 2e-13: 14, 1e-14: 15, 1e-15: 16, 1e-30: 16,
          0.5: 2, 1.0: 2}
# (N, w) -> n_g: the smallest power of two >= max(2N, 2w, 8)
GRIDS = {(1, 2): 8, (2, 3): 8, (4, 2): 8, (5, 2): 16, (7, 16): 32, (16, 4): 32, (16, 15): 32, (16, 16): 32, (17, 16): 64,
         (101, 13): 256, (256, 7): 512, (1000, 4): 2048, (4099, 15): 16384, (2 ** 28, 2): 2 ** 29, (1, 16): 32, (3, 5): 16}


def test_width_and_grid_table(helpers):
    for eps, w in WIDTHS.items():
        assert helpers.nufft_t_width(eps) == w == R.width(eps), eps
    for (n, w), g in GRIDS.items():
        assert helpers.nufft_t_grid(n, w) == g == R.grid(n, w), (n, w)
    for n, g in ((1, 8), (2, 8), (7, 32), (16, 32), (101, 256)):
        slots = [helpers.nufft_t_slot(m, n, g) for m in range(n)]
        assert slots == [int(k) % g for k in R.modes(n)], n


def test_quadrature_of_phi_hat(helpers):
    """phi^ of the library (32 Gauss-Legendre nodes in theta) against a 4096-node trapezoid sum (tanh-sinh) at every k a plan
    can ask for, |k| <= n_g / 4, for every width: 1e-13 relative, element by element (phi^(k) >= 0.1 phi^(0) there)"""
    worst = 0.0
    for w in range(2, 17):
        for n_g in (R.grid(1, w), 256, 2 ** 20):
            top = n_g // 4
            k = np.unique(np.concatenate([np.arange(0, min(top, 64) + 1), np.linspace(0, top, 97).astype(np.int64), -np.arange(1, 9)]))
            k = k[np.abs(k) <= top].astype(np.int64)
            got = np.zeros(len(k))
            helpers.nufft_t_phi_hat(w, n_g, ptr(k), len(k), ptr(got))
            want = R.phi_hat_trapezoid(k, n_g, w)
            assert (want > 0.1 * want.max()).all()
            rel = float(np.max(np.abs(got - want) / want))
            worst = max(worst, rel)
            assert rel <= 1e-13, (w, n_g, rel)
            assert np.max(np.abs(R.phi_hat(k, n_g, w) - want) / want) <= 1e-13  # the model's own
    print(f"phi^: worst relative difference {worst:.2e}")


def _exact(v):
    """x mod 1 of a double as an integer on the 2^-128 grid, as czt_frac defines it: the magnitude is cut towards zero below
    the grid, then the sign is applied mod 1 (so -1e-300 is 0, not 1 - 2^-128)"""
    f = int(abs(Fraction(float(v))) * (1 << 128)) % (1 << 128)
    return f if v >= 0 else (-f) % (1 << 128)


def binning_points(n_g, count=3000):
    rng = np.random.default_rng(5)
    cell = (0.3 * n_g + 0.001 + 0.998 * rng.random(1000)) / n_g + 4.0          # a clump of 1000 points inside one cell
    rest = rng.uniform(-3, 3, count) * (rng.random(count) < 0.5) * 0.01 + 0.61  # a narrow band: most cells stay empty
    return np.concatenate([R.SPECIALS, cell, rest, [0.0, 1e-300, -1e-300, 0.5, 2.0 ** -60, -(2.0 ** -60), 1 - 2.0 ** -53]])


@pytest.mark.parametrize("log_g", [3, 8, 14, 20])
def test_binning(helpers, log_g):
    """nufft_bin against a numpy stable argsort of floor(frac(x) n_g), frac exact in Python integers: the permutation, the
    cell starts and the kept positions (x mod 1 cut to 53 significant bits, in the same cell, below 1)"""
    n_g = 1 << log_g
    x = binning_points(n_g)
    m = len(x)
    xs, perm, start = np.zeros(m), np.zeros(m, np.uint32), np.zeros(n_g + 1, np.uint32)
    helpers.nufft_t_bin(ptr(x), m, log_g, ptr(xs), ptr(perm), ptr(start))
    exact = [_exact(v) for v in x]
    cell = np.array([f >> (128 - log_g) for f in exact], np.int64)
    want = np.argsort(cell, kind="stable")
    assert np.array_equal(perm, want)
    counts = np.bincount(cell, minlength=n_g)
    assert np.array_equal(start, np.concatenate([[0], np.cumsum(counts)]))
    assert counts.max() >= 1000 and ((counts == 0).sum() > n_g // 2 or log_g == 3)
    for i in range(m):
        f = exact[perm[i]]
        assert 0.0 <= xs[i] < 1.0
        kept = int(Fraction(float(xs[i])) * (1 << 128))
        assert kept <= f and f - kept < max(1, f >> 52), (i, x[perm[i]])       # cut, by less than one part in 2^52
        assert int(xs[i] * n_g) == cell[perm[i]]
        assert helpers.nufft_t_turns(float(x[perm[i]])) == xs[i]
    assert cell[list(x).index(1 - 2.0 ** -53)] == n_g - 1 and cell[0] == 0
    assert exact[list(x).index(1e-300)] == 0 and cell[list(x).index(7.5)] == n_g // 2 and cell[list(x).index(-0.25)] == 3 * n_g // 4


def test_support(helpers):
    """the w grid points from nufft_first on hold every point of the support, and the kernel value is phi of the distance"""
    rng = np.random.default_rng(3)
    for w in range(2, 17):
        for t in list(rng.random(50)) + [0.0, 0.5, 0.25, 1 - 2.0 ** -53, 2.0 ** -60]:
            first = helpers.nufft_t_first(w, t)
            inside = [dq for dq in range(-20, 21) if abs(dq - t) < w / 2]
            assert set(inside) <= set(range(first, first + w)), (w, t)
            for dq in range(first - 1, first + w + 1):
                want = float(R.phi(np.array([(dq - t) * 2.0 / w]), 2.30 * w)[0])
                assert abs(helpers.nufft_t_weight(dq, t, w) - want) <= 1e-12 * want, (w, t, dq)  # and 0 where phi is 0


def test_reference_integers_against_python():
    """the two-limb product of the reference is Python's own integer product, cut to its top 64 bits"""
    x = np.concatenate([R.points(101, 1000), R.points(1000, 4096, "clump")[:50]])
    hi, lo = R.limbs(x)
    for k in (0, 1, 3, 50, 2047, 2 ** 27, 2 ** 31 - 1):
        top = R.phase_top(k, hi, lo)
        for j in list(range(8)) + [500, 1020, 1049]:
            assert int(top[j]) == ((k * _exact(x[j])) % (1 << 128)) >> 64, (k, j)
    # the DFT: x_j = j / N, M = N is numpy's transform
    n = 30
    c = R.data(n, 0, "c")
    re, im = R.nufft1(np.arange(n) / n, c, n)
    want = np.fft.fft(c)
    assert np.max(np.abs(re.astype(np.float64) + 1j * im.astype(np.float64) - want)) < 1e-13
    re, im = R.nufft2(np.arange(n) / n, c, R.REVERSE)
    assert np.max(np.abs(re.astype(np.float64) + 1j * im.astype(np.float64) - np.fft.ifft(c) * n)) < 1e-13


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}{s[2]}")
def test_schedule_model_against_the_reference(shape):
    """the CPU leg of the gate: the schedule in numpy (double arithmetic for f64's eps, float32 kernel values, grid and table
    for f32's) against the direct sum, both types, both directions, complex and real data, within nufft_gate"""
    ref = reference(shape)
    n, m, _ = shape
    worst = {}
    for dt, arith in (("f64", np.float64), ("f32", np.float32)):
        for eps in R.EPS[dt]:
            n_g = R.grid(n, R.width(eps))
            g_rel, g_bin = nufft_gate(dt, n_g, eps)
            for t in (1, 2):
                for d, real, seed in ((R.FORWARD, False, 0), (R.REVERSE, False, 1), (R.FORWARD, True, 1), (R.REVERSE, True, 0)):
                    got = R.model(t, ref.x, ref.inp(t, real, seed), n, eps, d, arith)
                    want = ref.ref[(t, d, real, seed)]
                    rel, worst_bin = tol.rel_l2(got.real, got.imag, *want), tol.max_bin_err(got.real, got.imag, *want)
                    key = (dt, eps, t)
                    worst[key] = max(worst.get(key, (0, 0)), (rel / eps, worst_bin / eps))
                    assert rel <= g_rel and worst_bin <= g_bin, (shape, dt, eps, t, d, real, rel, g_rel, worst_bin, g_bin)
    print(shape, {k: (round(v[0], 2), round(v[1], 2)) for k, v in worst.items()})
