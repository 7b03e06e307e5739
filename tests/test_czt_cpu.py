"""The chirp-Z transform (csrc/czt.hpp, csrc/planner_czt.hpp) without a GPU: czt.hpp's fixed-point conversion and exact phase
compiled with g++ and checked against Python integers; the schedule run in numpy in double on those phases around pocketfft,
against tests/czt_reference.py (the GPU tests' reference) at every shape of tests/test_gpu_czt.py; the reference against
scipy.signal.czt / zoom_fft; the new C ABI exported and listed, with every argument rule returned before the device is
touched; the C++ and Rust mirrors."""
import ctypes as C
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from tests import czt_reference as R
from tests import tolerances as tol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = [f"phast_planner_czt{s}_{w}" for s in ("64", "32")
       for w in ("new", "free", "describe", "device_bytes", "conv_len", "workspace_len", "time_stages")]
NEW += [f"phast_czt_{s}{suffix}" for s in ("64", "32") for suffix in ("", "_with_planner", "_dev")]
OK, LEN_MISMATCH, NO_DEVICE, INVALID_ARG = 0, 2, 15, 16
ANY_FACTOR = 2.0
START = 0.123456789
# (N, M, step or None for 0.37 / N, start): the shapes of tests/test_gpu_czt.py
SHAPES = [(1, 1, None, START), (1, 5, None, START), (5, 1, None, START), (37, 101, None, START), (101, 37, None, START),
          (100, 29, None, START), (100, 30, None, START), (64, 64, 1 / 64, 0.0), (1000, 1000, None, START),
          (4099, 513, None, START), (100003, 16, None, START), (100003, 16, 0.3183098861837907, START),
          (3, 100003, None, START), (1000, 1000, -0.37 / 1000, -0.4)]
NS = [0, 1, 2, 2 ** 15 + 1, 10 ** 6 + 3, 2 ** 29 - 1, 2 ** 30 - 1]
STEPS = [1 / 3, 0.37 / 100003, 0.3183098861837907, 1e-12, 1 - 2.0 ** -53, -0.25, 7.75]
STARTS = [0.0, START, -0.4, 0.5, 1e-12, 12345.678, -(1 - 2.0 ** -53)]


def step_of(shape):
    n, _, step, _ = shape
    return 0.37 / n if step is None else step


def conv_len(n, m):
    return max(8, 1 << (n + m - 2).bit_length())


def czt_gate(dt, n, m):
    """tests/tolerances.py's formulas on log2 L, times the any-length factor 2: (rel-L2, per bin)"""
    log_l = conv_len(n, m).bit_length() - 1
    return ANY_FACTOR * tol.rel_gate(dt, log_l), ANY_FACTOR * tol.bin_gate(dt, log_l)


HELPERS = r"""
#include "czt.hpp"
using phast::CztFrac;
extern "C" {
void frac(double v, int down, unsigned long long *hi, unsigned long long *lo) {
    const CztFrac f = phast::czt_frac(v, down);
    *hi = f.hi;
    *lo = f.lo;
}
double phase(unsigned long long n, unsigned long long h_hi, unsigned long long h_lo, unsigned long long s_hi, unsigned long long s_lo) {
    return phast::czt_phase(n, CztFrac{h_hi, h_lo}, CztFrac{s_hi, s_lo});
}
/* out[i] = the phase of point i < count for (step, start) as the planner forms it */
void phases(unsigned long long count, double step, double start, double *out) {
    const CztFrac h = phast::czt_frac(step, 1), s = phast::czt_frac(start, 0);
    for (unsigned long long i = 0; i < count; ++i) out[i] = phast::czt_phase(i, h, s);
}
unsigned long long conv_len(unsigned long long n, unsigned long long m) { return phast::czt_conv_len(n, m); }
int bad_args(unsigned long long n, unsigned long long m, double step, double start) { return phast::czt_bad_args(n, m, step, start); }
}
"""


@pytest.fixture(scope="module")
def helpers(tmp_path_factory):
    d = tmp_path_factory.mktemp("czt_helpers")
    src, so = d / "helpers.cpp", d / "libczthelpers.so"
    src.write_text(HELPERS)
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-shared", "-fPIC", "-I",
                        os.path.join(ROOT, "phastft_amd", "csrc"), str(src), "-o", str(so)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    h = C.CDLL(str(so))
    u = C.c_ulonglong
    h.frac.argtypes = [C.c_double, C.c_int, C.POINTER(u), C.POINTER(u)]
    h.frac.restype = None
    h.phase.argtypes = [u] * 5
    h.phase.restype = C.c_double
    h.phases.argtypes = [u, C.c_double, C.c_double, C.c_void_p]
    h.phases.restype = None
    h.conv_len.argtypes = [u, u]
    h.conv_len.restype = u
    h.bad_args.argtypes = [u, u, C.c_double, C.c_double]
    return h


def frac(h, v, down):
    hi, lo = C.c_ulonglong(), C.c_ulonglong()
    h.frac(v, down, C.byref(hi), C.byref(lo))
    return (hi.value << 64) | lo.value


def test_fixed_point_conversion(helpers):
    """(v / 2^down) mod 1 on the 2^-128 grid equals the exact value of the double, for every step and start of the tests"""
    for v in STEPS + STARTS + [1.0, -1.0, 2.0 ** 52 + 1, -(2.0 ** 60), 2.0 ** -70, 3 * 2.0 ** -127, 0.75 + 2.0 ** -52]:
        for down in (0, 1):
            want = Fraction(v) / (1 << down) % 1 * (1 << 128)
            assert want.denominator == 1, v  # all of these are on the grid
            assert frac(helpers, v, down) == int(want), (v, down)
    # below the grid the value is cut towards zero by less than 2^-128
    for v in (2.0 ** -130, 1e-300, 5e-324, 1.5 * 2.0 ** -128):
        assert frac(helpers, v, 0) == int(Fraction(v) * (1 << 128)) and frac(helpers, v, 1) == int(Fraction(v) / 2 * (1 << 128))
        assert frac(helpers, -v, 0) == (-int(Fraction(v) * (1 << 128))) % (1 << 128)


def test_phase_against_python_integers(helpers):
    """the angle handed to sincospi is the true n^2 step / 2 + n start mod 1 to within 2^-52 turn, at every n up to 2^30 - 1"""
    worst = Fraction(0)
    mask = (1 << 64) - 1
    for step in STEPS:
        h = frac(helpers, step, 1)
        for start in STARTS:
            s = frac(helpers, start, 0)
            for n in NS:
                got = helpers.phase(n, h >> 64, h & mask, s >> 64, s & mask)
                assert -0.5 <= got <= 0.5
                true = n * n * Fraction(step) / 2 + n * Fraction(start)
                err = (Fraction(got) - true) % 1
                err = min(err, 1 - err)
                worst = max(worst, err)
                assert err <= Fraction(1, 1 << 52), (step, start, n, float(err))
    print(f"worst phase error {float(worst):.3e} turns (2^-52 = {2.0 ** -52:.3e})")


def test_conv_len_and_argument_rules_of_the_helper(helpers):
    for n, m in [(1, 1), (1, 5), (5, 4), (5, 5), (100, 29), (100, 30), (37, 101), (2 ** 29, 2 ** 29), (2 ** 29, 2 ** 29 + 1),
                 (1, 2 ** 30), (100003, 16)]:
        assert helpers.conv_len(n, m) == conv_len(n, m), (n, m)
    assert helpers.conv_len(100, 29) == 128 and helpers.conv_len(100, 30) == 256 and helpers.conv_len(1, 1) == 8
    big = 1 << 30
    for args, bad in (((1, 1, 0.5, 0.0), 0), ((big, 1, 0.5, 0.0), 0), ((1, big, 0.5, 0.0), 0), ((big // 2, big // 2 + 1, 0.5, 0.0), 0),
                      ((0, 1, 0.5, 0.0), 1), ((1, 0, 0.5, 0.0), 1), ((big, 2, 0.5, 0.0), 1), ((2, big, 0.5, 0.0), 1),
                      ((big // 2 + 1, big // 2 + 1, 0.5, 0.0), 1), ((1 << 63, 1 << 63, 0.5, 0.0), 1), ((2 ** 64 - 1, 2, 0.5, 0.0), 1),
                      ((8, 8, float("nan"), 0.0), 1), ((8, 8, 0.5, float("inf")), 1), ((8, 8, float("-inf"), 0.0), 1),
                      ((8, 8, 0.5, float("nan")), 1), ((8, 8, 1e300, -1e300), 0), ((8, 8, 0.0, 0.0), 0)):
        assert bool(helpers.bad_args(*args)) == bool(bad), args


def schedule(h, xr, xi, m, step, start):
    """the five stages of planner_czt.hpp restated in numpy in double on czt.hpp's phases, around pocketfft"""
    n = len(xr)
    ell = h.conv_len(n, m)
    count = max(n, m)
    pre, post = np.empty(count), np.empty(count)
    h.phases(count, step, start, pre.ctypes.data)
    h.phases(count, step, 0.0, post.ctypes.data)
    x = np.asarray(xr, np.float64) + (1j * np.asarray(xi, np.float64) if xi is not None else 0)
    a = np.zeros(ell, np.complex128)
    a[:n] = x * np.exp(-2j * np.pi * pre[:n])                       # pre sweep
    c = np.exp(-2j * np.pi * post)                                   # c[j] = exp(-2 pi i j^2 step / 2)
    b = np.zeros(ell, np.complex128)
    b[:m] = np.conj(c[:m])
    b[ell - np.arange(1, n)] = np.conj(c[1:n])
    bh = np.fft.fft(b) / ell
    w = np.fft.fft(a) * bh                                           # engine, spectrum sweep
    w = np.conj(np.fft.fft(np.conj(w)))                              # L IFFT
    return c[:m] * w[:m]                                             # post sweep


def rel_and_bin(got, ref_re, ref_im):
    e_re, e_im = got.real.astype(R.LD) - ref_re, got.imag.astype(R.LD) - ref_im
    den = np.sqrt(np.sum(ref_re ** 2 + ref_im ** 2))
    rms = np.sqrt(np.mean(ref_re ** 2 + ref_im ** 2))
    rel = float(np.sqrt(np.sum(e_re ** 2 + e_im ** 2)) / (den if den else 1))
    worst = float(np.maximum(np.abs(e_re), np.abs(e_im)).max() / (rms if rms else 1))
    return rel, worst


def test_schedule_against_the_reference(helpers):
    """every GPU test shape, complex and real signals, in double: within the f64 gate (the share used is printed)"""
    usage = 0.0
    for shape in SHAPES:
        n, m, _, start = shape
        step = step_of(shape)
        for real in (False, True):
            xr, xi = R.signal(n, np.float64, 0, real)
            want = R.czt(xr if real else xr + 1j * xi, m, step, start)
            rel, worst = rel_and_bin(schedule(helpers, xr, xi, m, step, start), *want)
            g_rel, g_bin = czt_gate("f64", n, m)
            usage = max(usage, rel / g_rel, worst / g_bin)
            assert rel <= g_rel and worst <= g_bin, (shape, real, rel, g_rel, worst, g_bin)
    print(f"numpy model of the schedule in double: at most {usage:.3f} of the f64 gate")


def test_reference_against_scipy():
    """scipy is the definition here, not the accuracy standard: 1e-9 at N, M <= 300"""
    ss = pytest.importorskip("scipy.signal")
    for n, m, step, start in [(37, 101, 0.37 / 37, START), (101, 37, 0.37 / 101, START), (300, 300, 1 / 300, 0.0), (1, 5, 0.2, 0.3),
                              (64, 64, -0.01, -0.4), (200, 299, 0.0017, 0.25)]:
        for real in (False, True):
            xr, xi = R.signal(n, np.float64, 1, real)
            x = xr if real else xr + 1j * xi
            re, im = R.czt(x, m, step, start)
            want = ss.czt(x, m, w=np.exp(-2j * np.pi * step), a=np.exp(2j * np.pi * start))
            assert np.abs((re + 1j * im).astype(np.complex128) - want).max() <= 1e-9 * max(1.0, np.abs(want).max()), (n, m)
    for fn, m, fs, endpoint in [([0.1, 0.3], 50, 2.0, False), ([0.1, 0.3], 50, 2.0, True), (0.5, 77, 2.0, False),
                                ([100.0, 180.0], 200, 1000.0, True), ([-0.2, 0.2], 33, 1.0, False)]:
        xr, xi = R.signal(300, np.float64, 2)
        x = xr + 1j * xi
        start, step = R.zoom_params(fn, m, fs, endpoint)
        re, im = R.czt(x, m, step, start)
        want = ss.zoom_fft(x, fn, m, fs=fs, endpoint=endpoint)
        assert np.abs((re + 1j * im).astype(np.complex128) - want).max() <= 1e-9 * np.abs(want).max(), (fn, m, fs, endpoint)


def test_reference_is_the_dft_at_the_dft_parameters():
    xr, xi = R.signal(64, np.float64, 3)
    re, im = R.czt(xr + 1j * xi, 64, 1 / 64, 0.0)
    want = np.fft.fft(xr + 1j * xi)
    assert np.abs((re + 1j * im).astype(np.complex128) - want).max() < 1e-13


@pytest.fixture(scope="module")
def lib():
    from phastft_amd import _lib

    return _lib.lib()


def test_new_symbols_are_exported_and_listed(lib):
    from phastft_amd import _lib

    header = open(os.path.join(ROOT, "include", "phastft_hip.h")).read()
    assert len(NEW) == 20
    for name in NEW:
        getattr(lib, name)
        assert name in _lib.SYMBOLS and re.search(r"\b" + name + r"\s*\(", header), name
    import phastft_amd as P

    for name in ("PlannerCzt64", "PlannerCzt32", "czt_batched", "czt_64", "czt_32", "czt_64_with_planner", "czt_32_with_planner",
                 "czt", "zoom_fft"):
        assert name in P.__all__ and callable(getattr(P, name)), name
    assert "PlannerCzt64/32" in P.__doc__


def test_argument_codes(lib):
    """every rule of _new, null planners and null planes come back before the device is touched"""
    big = 1 << 30
    n_ = C.c_size_t
    for sfx, dt in (("64", np.float64), ("32", np.float32)):
        new = getattr(lib, f"phast_planner_czt{sfx}_new")

        def make(n, m, step=0.01, start=0.0, out=True):
            p = C.c_void_p(1)
            rc = new(n_(n), n_(m), C.c_double(step), C.c_double(start), C.byref(p) if out else None)
            assert rc == OK or not p.value or not out
            return rc

        assert make(0, 8) == INVALID_ARG                      # N = 0
        assert make(8, 0) == INVALID_ARG                      # M = 0
        assert make(big, 2) == INVALID_ARG                    # N + M - 1 > 2^30
        assert make(big // 2 + 1, big // 2 + 1) == INVALID_ARG
        assert make(2 ** 64 - 1, 3) == INVALID_ARG            # ... and where the sum wraps
        assert make(8, 8, step=float("nan")) == INVALID_ARG
        assert make(8, 8, step=float("inf")) == INVALID_ARG
        assert make(8, 8, start=float("nan")) == INVALID_ARG
        assert make(8, 8, start=float("-inf")) == INVALID_ARG
        assert make(8, 8, out=False) == INVALID_ARG
        for name in ("device_bytes", "conv_len"):
            fn = getattr(lib, f"phast_planner_czt{sfx}_{name}")
            fn.restype = C.c_size_t
            assert fn(None) == 0
        fn = getattr(lib, f"phast_planner_czt{sfx}_workspace_len")
        fn.restype = C.c_size_t
        assert fn(None, n_(1)) == 0
        assert getattr(lib, f"phast_planner_czt{sfx}_describe")(None, C.create_string_buffer(8), n_(8)) == INVALID_ARG
        ms = (C.c_float * 5)()
        assert getattr(lib, f"phast_planner_czt{sfx}_time_stages")(None, None, None, None, None, n_(1), None, n_(0), 1, ms,
                                                                   None) == INVALID_ARG
        x, y = np.zeros(16, dt), np.zeros(16, dt)
        o_re, o_im = np.zeros(8, dt), np.zeros(8, dt)
        p = lambda v: v.ctypes.data_as(C.c_void_p)  # noqa: E731
        shot = getattr(lib, f"phast_czt_{sfx}")
        d = C.c_double
        assert shot(None, p(y), n_(16), p(o_re), p(o_im), n_(8), d(0.01), d(0.0)) == INVALID_ARG   # null planes
        assert shot(p(x), p(y), n_(16), None, p(o_im), n_(8), d(0.01), d(0.0)) == INVALID_ARG
        assert shot(p(x), p(y), n_(16), p(o_re), None, n_(8), d(0.01), d(0.0)) == INVALID_ARG
        assert shot(p(x), p(y), n_(0), p(o_re), p(o_im), n_(8), d(0.01), d(0.0)) == INVALID_ARG    # the rules of _new
        assert shot(p(x), p(y), n_(16), p(o_re), p(o_im), n_(0), d(0.01), d(0.0)) == INVALID_ARG
        assert shot(p(x), None, n_(16), p(o_re), p(o_im), n_(8), d(float("nan")), d(0.0)) == INVALID_ARG
        assert getattr(lib, f"phast_czt_{sfx}_with_planner")(p(x), p(y), n_(16), p(o_re), p(o_im), n_(8), None) == INVALID_ARG
        assert getattr(lib, f"phast_czt_{sfx}_dev")(p(x), p(y), n_(16), p(o_re), p(o_im), n_(8), n_(1), None, None, n_(0),
                                                    None) == INVALID_ARG


def test_calls_without_a_gpu_fail_loudly(lib):
    """a short workspace and a wrong length against a planner need a planner: tests/test_gpu_czt.py checks those codes"""
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present: tests/test_gpu_czt.py covers the device side")
    h = C.c_void_p()
    n_ = C.c_size_t
    assert lib.phast_planner_czt64_new(n_(1000), n_(100), C.c_double(0.001), C.c_double(0.1), C.byref(h)) == NO_DEVICE
    assert not h.value
    assert lib.phast_planner_czt32_new(n_(5), n_(1), C.c_double(-0.25), C.c_double(0.0), C.byref(h)) == NO_DEVICE
    x, o = np.zeros(16), np.zeros(8)
    p = lambda v: v.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert lib.phast_czt_64(p(x), None, n_(16), p(o), p(o.copy()), n_(8), C.c_double(0.01), C.c_double(0.0)) == NO_DEVICE
    import phastft_amd as P

    with pytest.raises(P.PhastHipError):
        P.PlannerCzt64(1000, 100, 0.001)
    with pytest.raises(P.PhastHipError):
        P.czt_32(x.astype(np.float32), None, o.astype(np.float32), o.astype(np.float32), 0.01)


def test_python_argument_errors():
    import phastft_amd as P

    with pytest.raises(P.PhastPanic):
        P.PlannerCzt64(0, 8, 0.1)
    with pytest.raises(P.PhastPanic):
        P.PlannerCzt32(8, 0, 0.1)
    with pytest.raises(P.PhastPanic):
        P.PlannerCzt64(8, 8, float("nan"))
    with pytest.raises(P.PhastPanic):
        P.PlannerCzt64(8, 8, 0.1, float("inf"))
    with pytest.raises(P.PhastPanic):
        P.PlannerCzt64(1 << 30, 2, 0.1)
    x = np.zeros(16)
    with pytest.raises(P.PhastPanic) as e:
        P.czt_64(x, np.zeros(15), np.zeros(8), np.zeros(8), 0.01)   # planes of two lengths
    assert e.value.code == LEN_MISMATCH
    with pytest.raises(P.PhastPanic) as e:
        P.czt_64(x, None, np.zeros(8), np.zeros(7), 0.01)
    assert e.value.code == LEN_MISMATCH
    with pytest.raises(TypeError):
        P.czt_64(x.astype(np.float32), None, np.zeros(8), np.zeros(8), 0.01)
    with pytest.raises(TypeError):
        P.czt(np.zeros(16))                                          # the conveniences take device tensors
    with pytest.raises(TypeError):
        P.zoom_fft(np.zeros(16), [0.1, 0.2])
    with pytest.raises(ValueError):
        P.zoom_fft(np.zeros(16), [0.1, 0.2, 0.3])


def test_cpp_mirror_without_gpu(tmp_path):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present: tests/test_gpu_czt.py runs the mirror there")
    from phastft_amd import build

    lib = build.build()
    exe = str(tmp_path / "czt_test")
    libdir = os.path.dirname(lib)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "czt_test.cpp"), "-o", exe, "-L", libdir, "-lphastft_hip",
                        f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "czt: ok" in r.stdout, r.stdout + r.stderr


def test_rust_mirror():
    """Parsed textually, as tests/test_rust_shim.py does (no Rust toolchain here)"""
    src = os.path.join(ROOT, "rust", "phastft-hip", "src")
    ffi = open(os.path.join(src, "ffi.rs")).read()
    for name in NEW:
        assert re.search(r"fn " + name + r"\s*\(", ffi), name
    planner = open(os.path.join(src, "planner.rs")).read()
    assert "PlannerCzt64" in planner and "PlannerCzt32" in planner
    czt = open(os.path.join(src, "algorithms", "czt.rs")).read()
    for f in ("czt_64", "czt_32", "czt_64_with_planner", "czt_32_with_planner", "czt_64_dev", "czt_32_dev"):
        assert re.search(r"\b" + f + r"\b", czt), f
    assert "pub mod czt;" in open(os.path.join(src, "algorithms", "mod.rs")).read()
    lib = open(os.path.join(src, "lib.rs")).read()
    assert "PlannerCzt64" in lib and "czt_64_dev" in lib
