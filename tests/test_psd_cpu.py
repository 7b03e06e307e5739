"""Welch spectral estimation (csrc/psd.hpp, csrc/planner_psd.hpp) without a GPU: the header's segment count, slab partition,
argument rules, scale and one-sided factors compiled with g++ against Python integers and floats; the long-double reference
of tests/psd_reference.py against scipy.signal.welch, csd and spectrogram; the planner's schedule (means and sums in double,
slabs, chunks, partial rows, one rounding at the end) restated in numpy against the reference; the new C ABI exported and
listed, with its argument codes returned before the device is touched; the Python names and errors."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.signal as ss

from tests import psd_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
NEW = [f"phast_planner_psd{s}_{w}" for s in ("64", "32")
       for w in ("new", "free", "describe", "device_bytes", "segments", "bins", "slab", "workspace_len", "workspace_min",
                 "time_stages")]
NEW += [f"phast_{k}_{fs}_{suffix}" for k in ("psd", "csd") for fs in ("f64", "f32") for suffix in ("with_planner", "dev")]
OK, LEN_MISMATCH, PLANNER_SIZE, NO_DEVICE, INVALID_ARG = 0, 2, 3, 15, 16
ALL_SHAPES = R.SHAPES + R.slab_shapes()

HELPERS = r"""
#include "psd.hpp"
using u64 = unsigned long long;
extern "C" {
u64 segments(u64 len, u64 p, u64 h) { return phast::psd_segments(len, p, h); }
u64 bins(u64 f) { return phast::psd_bins(f); }
int onesided(u64 k, u64 f) { return phast::psd_onesided(k, f); }
u64 slab_len(u64 s, u64 bins) { return phast::psd_slab_len(s, bins); }
u64 slabs(u64 s, u64 q) { return phast::psd_slabs(s, q); }
void slab_range(u64 s, u64 q, u64 c_lo, u64 c_hi, u64 *lo, u64 *hi) { phast::psd_slab_range(s, q, c_lo, c_hi, lo, hi); }
unsigned mean_threads(u64 p) { return phast::psd_mean_threads(p); }
int bad_args(u64 len, u64 p, u64 h, u64 f, int detrend, int scaling, double fs, unsigned v) {
    return phast::psd_bad_args(len, p, h, f, detrend, scaling, fs, v);
}
int sigma(const double *w, u64 p, int scaling, double fs, double *out) { return phast::psd_sigma(w, p, scaling, fs, out); }
void hann(u64 p, double *w) { for (u64 j = 0; j < p; ++j) w[j] = (double)phast::psd_hann(j, p); }
u64 min_slab() { return phast::kPsdMinSlab; }
}
"""


@pytest.fixture(scope="module")
def helpers(tmp_path_factory):
    d = tmp_path_factory.mktemp("psd_helpers")
    src, so = d / "helpers.cpp", d / "libpsdhelpers.so"
    src.write_text(HELPERS)
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-shared", "-fPIC", "-I",
                        os.path.join(ROOT, "phastft_amd", "csrc"), str(src), "-o", str(so)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lib = C.CDLL(str(so))
    for name in ("segments", "bins", "slab_len", "slabs", "min_slab"):
        getattr(lib, name).restype = C.c_ulonglong
    lib.mean_threads.restype = C.c_uint
    u = C.c_ulonglong
    lib.bad_args.argtypes = [u, u, u, u, C.c_int, C.c_int, C.c_double, C.c_uint]
    lib.sigma.argtypes = [C.c_void_p, u, C.c_int, C.c_double, C.c_void_p]
    lib.slab_range.argtypes = [u, u, u, u, C.c_void_p, C.c_void_p]
    lib.segments.argtypes = [u, u, u]
    lib.slab_len.argtypes = lib.slabs.argtypes = [u, u]
    lib.onesided.argtypes = [u, u]
    lib.bins.argtypes = lib.mean_threads.argtypes = [u]
    lib.hann.argtypes = [u, C.c_void_p]
    return lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def test_segments_bins_and_onesided_factors(helpers):
    for length, p, h, f in ALL_SHAPES + [(1 << 24, 256, 128, 256), (1 << 20, 1024, 256, 1024), (10 ** 6, 1000, 250, 1000)]:
        s = int(helpers.segments(length, p, h))
        assert s == 1 + (length - p) // h == R.segments(length, p, h)
        assert (s - 1) * h + p <= length < s * h + p          # the last segment fits, one more would not
        assert helpers.bins(f) == f // 2 + 1
        c = [helpers.onesided(k, f) for k in range(f // 2 + 1)]
        assert c == [int(v) for v in R.onesided(f)], f
    assert [helpers.onesided(k, 2) for k in range(2)] == [1, 1]   # DC and Nyquist only
    assert [helpers.onesided(k, 1) for k in range(1)] == [1]
    assert [helpers.onesided(k, 9) for k in range(5)] == [1, 2, 2, 2, 2]   # odd F: no Nyquist bin


def test_slab_rule_and_partition(helpers):
    """Q is a function of S and bins alone; the slabs, cut by any chunk boundaries, cover every frame exactly once, in order"""
    assert helpers.min_slab() == R.MIN_SLAB
    for s, b in ((1, 1), (15, 5), (4089, 5), (131071, 129), (1 << 20, 513), (4093, 513)):
        q = int(helpers.slab_len(s, b))
        assert q == max(16, s * b // (1 << 19)), (s, b)
        assert helpers.slabs(s, q) == -(-s // q)
    assert helpers.slab_len(131071, 129) == 32 and helpers.slabs(131071, 32) == 4096   # 2^24 samples, P = 256, H = 128
    lo, hi = C.c_ulonglong(), C.c_ulonglong()
    rng = np.random.default_rng(5)
    for s in list(range(1, 70)) + [255, 256, 257, 1000, 4089, 4999, 5000]:
        for q in {16, int(helpers.slab_len(s, 5)), 7}:
            n = int(helpers.slabs(s, q))
            cuts = [0, s] if s < 3 else sorted({0, s, *rng.integers(1, s, 3).tolist()})
            seen = []
            for c_lo, c_hi in zip(cuts[:-1], cuts[1:]):          # chunk by chunk, slab by slab
                for slab in range(n):
                    helpers.slab_range(slab, q, c_lo, c_hi, C.byref(lo), C.byref(hi))
                    if lo.value < hi.value:
                        assert slab * q <= lo.value and hi.value <= min((slab + 1) * q, s)
                        seen.append((slab, lo.value, hi.value))
            frames = [f for _, a, b in sorted(seen) for f in range(a, b)]
            assert frames == list(range(s)), (s, q, cuts)


def test_mean_threads(helpers):
    for p in (1, 2, 4, 5, 8, 9, 100, 256, 1000, 1024, 1025, 1 << 20):
        t = int(helpers.mean_threads(p))
        assert t & (t - 1) == 0 and 1 <= t <= 256
        assert t == 256 or 4 * t >= p
        assert t == 1 or 4 * (t // 2) < p


def test_argument_rules(helpers):
    ok = (1000, 100, 63, 128, 1, 0, 2.5, 2)
    assert helpers.bad_args(*ok) == 0
    bad = {"H = 0": (1000, 100, 0, 128), "H > P": (1000, 100, 101, 128), "P > F": (1000, 100, 50, 99), "L < P": (99, 100, 50, 128),
           "P = 0": (1000, 0, 0, 128), "F too long": (1 << 29, 100, 50, (1 << 29) + 1), "L too long": ((1 << 29) + 1, 100, 50, 128)}
    for why, sizes in bad.items():
        assert helpers.bad_args(*sizes, 1, 0, 1.0, 2) == 1, why
    assert helpers.bad_args(1 << 29, 1 << 29, 1 << 29, 1 << 29, 1, 0, 1.0, 2) == 0
    assert helpers.bad_args(1 << 24, 256, 128, 256, 1, 0, 1.0, 4) == 0          # S fd = 131071 * 256 < 2^30
    assert helpers.bad_args(1 << 29, 8, 1, 8, 1, 0, 1.0, 4) == 1                # S fd > 2^30
    assert helpers.bad_args(1 << 27, 8, 1, 8, 1, 0, 1.0, 4) == 0                # (2^27 - 7) * 8 <= 2^30
    assert helpers.bad_args((1 << 27) + 7, 7, 1, 7, 1, 0, 1.0, 2) == 1          # fd = 8 for f64: (2^27 + 1) * 8 > 2^30
    assert helpers.bad_args((1 << 27) + 6, 7, 1, 7, 1, 0, 1.0, 2) == 0
    for detrend, scaling, fs in ((2, 0, 1.0), (-1, 0, 1.0), (1, 2, 1.0), (1, 0, 0.0), (1, 0, -1.0), (1, 0, float("nan")),
                                 (1, 0, float("inf"))):
        assert helpers.bad_args(1000, 100, 63, 128, detrend, scaling, fs, 2) == 1, (detrend, scaling, fs)


def test_sigma_and_hann(helpers):
    out = C.c_double()
    for p in (1, 2, 7, 100, 256):
        w = np.zeros(p)
        helpers.hann(p, _ptr(w))
        assert np.array_equal(w, R.hann(p).astype(np.float64)), p
        # scipy builds its window in double: the rounding of the angle 2 pi j / P alone moves cos by up to pi eps / 2
        assert np.max(np.abs(w - ss.get_window("hann", p))) <= 4 * np.finfo(np.float64).eps, p
        for win in (w, R.window_of("random", p)):
            for code, scaling in ((0, "density"), (1, "spectrum")):
                assert helpers.sigma(_ptr(win), p, code, 2.5, C.byref(out)) == 0
                want = float(R.sigma(win, scaling, 2.5))
                # a serial double sum of P positive terms: (P - 1) u at worst, and the product, the square and the reciprocal
                assert abs(out.value - want) <= (p + 4) * 1.2e-16 * want, (p, scaling)
    zero, alt = np.zeros(4), np.array([1.0, -1.0, 1.0, -1.0])
    assert helpers.sigma(_ptr(zero), 4, 0, 1.0, C.byref(out)) == 1              # sum w^2 = 0
    assert helpers.sigma(_ptr(alt), 4, 1, 1.0, C.byref(out)) == 1               # sum w = 0
    assert helpers.sigma(_ptr(alt), 4, 0, 1.0, C.byref(out)) == 0 and out.value == 0.25


CONFIGS = [(det, sc, win) for det in (True, False) for sc in ("density", "spectrum") for win in ("hann", "random")]


def _signals(length, seed=0):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, length), rng.uniform(-1, 1, length)


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_reference_is_scipys(shape):
    """welch, csd and spectrogram in double: <= 1e-13 relative to the largest value"""
    length, p, h, f = shape
    x, y = _signals(length)
    for det, sc, win in CONFIGS:
        w = R.window_of(win, p)
        kw = dict(fs=2.5, window="hann" if w is None else w, nperseg=p, noverlap=p - h, nfft=f, detrend="constant" if det else False,
                  scaling=sc)
        pxy, pxx, pyy = R.psd(x, p, h, f, w, det, sc, 2.5, y=y)
        freqs, want = ss.welch(x, **kw)
        assert np.array_equal(freqs, np.fft.rfftfreq(f, 1 / 2.5))
        assert want.shape == pxx.shape
        assert np.max(np.abs(pxx - want)) <= 1e-13 * max(np.max(np.abs(want)), 1e-300), (shape, det, sc, win)
        assert np.max(np.abs(R.psd(x, p, h, f, w, det, sc, 2.5) - pxx)) == 0
        _, want = ss.csd(x, y, **kw)
        assert np.max(np.abs(pxy - want)) <= 1e-13 * max(np.max(np.abs(want)), 1e-300), (shape, det, sc, win)
        _, want = ss.welch(y, **kw)
        assert np.max(np.abs(pyy - want)) <= 1e-13 * max(np.max(np.abs(want)), 1e-300)
        _, times, want = ss.spectrogram(x, mode="psd", **kw)
        got = R.psd(x, p, h, f, w, det, sc, 2.5, average=False)
        assert got.shape == want.T.shape == (R.segments(length, p, h), f // 2 + 1)
        assert np.max(np.abs(got - want.T)) <= 1e-13 * max(np.max(np.abs(want)), 1e-300), (shape, det, sc, win)
        assert np.allclose(times, (np.arange(got.shape[0]) * h + p / 2) / 2.5, rtol=1e-15, atol=0)


def test_detrended_single_sample_segments_are_exactly_zero():
    x, _ = _signals(64)
    assert np.all(R.psd(x, 1, 1, 1) == 0) and np.all(ss.welch(x, nperseg=1, noverlap=0)[1] == 0)


def schedule(helpers, x, shape, window, detrend, scaling, fs, dtype, chunk, y=None):
    """planner_psd.hpp restated: per chunk of `chunk` frames the means in double, rows rounded to T, a long-double rfft rounded to
    T (the real planner's output type), slab sums in double into partial rows that live from chunk to chunk, and one rounding
    to T after the last slab"""
    length, p, h, f = shape
    s, nb = int(helpers.segments(length, p, h)), f // 2 + 1
    q = int(helpers.slab_len(s, nb))
    n = int(helpers.slabs(s, q))
    w = (R.hann(p) if window is None else np.asarray(window)).astype(np.float64)
    sig = C.c_double()
    assert helpers.sigma(_ptr(w), p, 0 if scaling == "density" else 1, fs, C.byref(sig)) == 0
    planes = 1 if y is None else 4
    partial = np.full((planes, n, nb), np.nan)                    # poison: a slab must start from 0, not from what is there
    lo, hi = C.c_ulonglong(), C.c_ulonglong()
    for q0 in range(0, s, chunk):
        c = min(chunk, s - q0)
        spec = []
        for v in (x,) if y is None else (x, y):
            seg = v[(q0 + np.arange(c))[:, None] * h + np.arange(p)[None, :]].astype(np.float64)
            rows = np.zeros((c, f), dtype)
            if detrend:   # the mean as the pair (first sample, mean of the differences from it)
                diff = seg - seg[:, :1]
                rows[:, :p] = ((diff - diff.sum(axis=1, keepdims=True) / p) * w).astype(dtype)
            else:
                rows[:, :p] = (seg * w).astype(dtype)
            spec.append(np.fft.rfft(rows.astype(LD), axis=1).astype(np.complex64 if dtype == np.float32 else np.complex128))
        for slab in range(n):
            helpers.slab_range(slab, q, q0, q0 + c, C.byref(lo), C.byref(hi))
            if lo.value >= hi.value:
                continue
            acc = np.zeros((planes, nb)) if lo.value == slab * q else partial[:, slab].copy()
            for fr in range(lo.value, hi.value):
                a = spec[0][fr - q0].astype(np.complex128)
                if y is None:
                    acc[0] += a.real * a.real + a.imag * a.imag
                else:
                    b = spec[1][fr - q0].astype(np.complex128)
                    acc[0] += a.real * b.real + a.imag * b.imag
                    acc[1] += a.real * b.imag - a.imag * b.real
                    acc[2] += a.real * a.real + a.imag * a.imag
                    acc[3] += b.real * b.real + b.imag * b.imag
            partial[:, slab] = acc
    total = np.zeros((planes, nb))
    for slab in range(n):
        total += partial[:, slab]
    ck = np.array([helpers.onesided(k, f) for k in range(nb)], np.float64)
    return (total * (sig.value / s * ck)).astype(dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_schedule_against_the_reference(helpers, shape, dtype):
    """the restated schedule is the reference to a few roundings of T, whole and in chunks, and its bits do not depend on the
    chunking"""
    length, p, h, f = shape
    x, y = (v.astype(dtype) for v in _signals(length, 1))
    eps = float(np.finfo(dtype).eps)
    s = R.segments(length, p, h)
    for det, sc, win in CONFIGS[::3] + CONFIGS[1:2]:
        w = R.window_of(win, p)
        want = R.psd(x, p, h, f, w, det, sc, 2.5)
        whole = schedule(helpers, x, shape, w, det, sc, 2.5, dtype, s)[0]
        scale = float(np.linalg.norm(want.astype(np.float64)))
        if scale == 0:
            assert np.all(whole == 0)
        else:
            assert np.linalg.norm(whole - want.astype(np.float64)) <= 8 * eps * scale, (shape, det, sc, win)
        for chunk in {1, 5, 17} if s <= 300 else {37}:
            assert np.array_equal(schedule(helpers, x, shape, w, det, sc, 2.5, dtype, chunk)[0], whole), (shape, chunk)
    pxy, pxx, pyy = R.psd(x, p, h, f, None, True, "density", 2.5, y=y)
    got = schedule(helpers, x, shape, None, True, "density", 2.5, dtype, s, y=y)
    den = float(np.linalg.norm(np.sqrt((pxx * pyy).astype(np.float64))))
    if den:
        assert np.linalg.norm((got[0] + 1j * got[1]) - pxy.astype(np.complex128)) <= 8 * eps * den
        assert np.linalg.norm(got[2] - pxx.astype(np.float64)) <= 8 * eps * np.linalg.norm(pxx.astype(np.float64))
        assert np.linalg.norm(got[3] - pyy.astype(np.float64)) <= 8 * eps * np.linalg.norm(pyy.astype(np.float64))


def test_a_float_mean_misses_what_a_double_mean_keeps(helpers):
    """x = uniform(-1, 1) + 1000 in f32, P = 256, H = 128, Hann: the error of the estimate with the mean carried in double
    against the same schedule with the mean rounded to f32"""
    shape = (8192, 256, 128, 256)
    x = (np.random.default_rng(3).uniform(-1, 1, shape[0]) + 1000).astype(np.float32)
    want = R.psd(x, 256, 128, 256).astype(np.float64)
    got = schedule(helpers, x, shape, None, True, "density", 1.0, np.float32, 63)[0]
    err = np.linalg.norm(got - want) / np.linalg.norm(want)
    assert err <= 4.2e-6 / 10, err
    x64 = np.random.default_rng(3).uniform(-1, 1, shape[0]) + 1000       # f64: the offset costs nothing either
    want64 = R.psd(x64, 256, 128, 256).astype(np.float64)
    got64 = schedule(helpers, x64, shape, None, True, "density", 1.0, np.float64, 63)[0]
    assert np.linalg.norm(got64 - want64) / np.linalg.norm(want64) <= 4 * 8e-16 * 7 / 3
    seg = x[np.arange(63)[:, None] * 128 + np.arange(256)[None, :]]
    rows = ((seg - seg.mean(axis=1, keepdims=True, dtype=np.float32)) * R.hann(256).astype(np.float32)).astype(np.float32)
    bad = (np.abs(np.fft.rfft(rows.astype(np.float64), axis=1)) ** 2).mean(axis=0) * float(R.sigma(R.hann(256), "density", 1.0)) * R.onesided(256).astype(np.float64)
    assert np.linalg.norm(bad - want) / np.linalg.norm(want) > 4.2e-6


@pytest.fixture(scope="module")
def lib():
    from phastft_amd import _lib

    return _lib.lib()


def test_new_symbols_are_exported_and_listed(lib):
    from phastft_amd import _lib

    header = open(os.path.join(ROOT, "include", "phastft_hip.h")).read()
    assert len(NEW) == 28
    for name in NEW:
        getattr(lib, name)
        assert name in _lib.SYMBOLS and re.search(r"\b" + name + r"\s*\(", header), name
    for const in ("PHAST_DETREND_NONE 0", "PHAST_DETREND_CONSTANT 1", "PHAST_PSD_DENSITY 0", "PHAST_PSD_SPECTRUM 1"):
        assert "#define " + const in header
    import phastft_amd as P

    for name in ("PlannerPsd64", "PlannerPsd32", "psd_batched", "csd_batched", "psd_f64_with_planner", "psd_f32_with_planner",
                 "csd_f64_with_planner", "csd_f32_with_planner", "welch", "csd", "spectrogram", "periodogram", "coherence"):
        assert name in P.__all__ and callable(getattr(P, name)), name
    assert "PlannerPsd64/32" in P.__doc__
    from phastft_amd import build

    assert "psd" in build.UNITS


def test_argument_codes(lib):
    """sizes out of range, unknown detrend and scaling, fs <= 0, a window that sums to zero, null pointers and a null planner
    come back before the device is touched"""
    sz = C.c_size_t
    for sfx, fs, dt in (("64", "f64", np.float64), ("32", "f32", np.float32)):
        new = getattr(lib, f"phast_planner_psd{sfx}_new")
        for ln, p, h, f, det, sc, rate in ((1000, 100, 0, 128, 1, 0, 1.0), (1000, 100, 101, 128, 1, 0, 1.0), (1000, 100, 50, 99, 1, 0, 1.0),
                                           (99, 100, 50, 128, 1, 0, 1.0), (1000, 0, 0, 8, 1, 0, 1.0), (1000, 8, 4, (1 << 29) + 1, 1, 0, 1.0),
                                           ((1 << 29) + 1, 8, 4, 8, 1, 0, 1.0), (1 << 29, 8, 1, 8, 1, 0, 1.0), (1000, 100, 50, 128, 2, 0, 1.0),
                                           (1000, 100, 50, 128, 1, 2, 1.0), (1000, 100, 50, 128, 1, 0, 0.0), (1000, 100, 50, 128, 1, 0, -2.0)):
            h_ = C.c_void_p(1)
            assert new(sz(ln), sz(p), sz(h), sz(f), None, det, sc, rate, C.byref(h_)) == INVALID_ARG and not h_.value, (ln, p, h, f)
        zero, alt = np.zeros(4), np.array([1.0, -1.0, 1.0, -1.0])
        h_ = C.c_void_p(1)
        assert new(sz(100), sz(4), sz(2), sz(4), _ptr(zero), 1, 0, 1.0, C.byref(h_)) == INVALID_ARG and not h_.value
        h_ = C.c_void_p(1)
        assert new(sz(100), sz(4), sz(2), sz(4), _ptr(alt), 1, 1, 1.0, C.byref(h_)) == INVALID_ARG and not h_.value
        assert new(sz(100), sz(8), sz(4), sz(8), None, 1, 0, 1.0, None) == INVALID_ARG
        for q in ("workspace_len",):
            assert getattr(lib, f"phast_planner_psd{sfx}_{q}")(None, 1, 0) == 0
        assert getattr(lib, f"phast_planner_psd{sfx}_workspace_min")(None, 1) == 0
        for q in ("segments", "bins", "slab", "device_bytes"):
            assert getattr(lib, f"phast_planner_psd{sfx}_{q}")(None) == 0
        assert getattr(lib, f"phast_planner_psd{sfx}_describe")(None, C.create_string_buffer(8), sz(8)) == INVALID_ARG
        ms = (C.c_float * 3)()
        assert getattr(lib, f"phast_planner_psd{sfx}_time_stages")(None, None, None, sz(1), 1, sz(0), None, sz(0), 1, ms, None) == INVALID_ARG
        x, o = np.zeros(100, dt), np.zeros(5, dt)
        assert getattr(lib, f"phast_psd_{fs}_with_planner")(_ptr(x), sz(100), _ptr(o), sz(5), 1, None) == INVALID_ARG
        assert getattr(lib, f"phast_psd_{fs}_dev")(_ptr(x), _ptr(o), sz(100), sz(1), sz(100), 1, None, None, sz(0), None) == INVALID_ARG
        assert getattr(lib, f"phast_csd_{fs}_with_planner")(_ptr(x), sz(100), _ptr(x), sz(100), _ptr(o), sz(5), _ptr(o), sz(5), None, sz(0),
                                                             None, sz(0), 1, None) == INVALID_ARG
        assert getattr(lib, f"phast_csd_{fs}_dev")(_ptr(x), _ptr(x), _ptr(o), _ptr(o), None, None, sz(100), sz(1), sz(100), 1, None, None,
                                                    sz(0), None) == INVALID_ARG


def test_calls_without_a_gpu_fail_loudly(lib):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present: tests/test_gpu_psd.py covers the device side")
    h = C.c_void_p()
    sz = C.c_size_t
    assert lib.phast_planner_psd64_new(sz(1000), sz(100), sz(50), sz(128), None, 1, 0, 1.0, C.byref(h)) == NO_DEVICE and not h.value
    import phastft_amd as P

    with pytest.raises(P.PhastHipError):
        P.PlannerPsd32(1000, 100)


def test_python_argument_errors():
    import phastft_amd as P

    with pytest.raises(P.PhastPanic):
        P.PlannerPsd64(1000, 100, hop=101)            # INVALID_ARG before the device is touched
    with pytest.raises(P.PhastPanic):
        P.PlannerPsd64(1000, 100, nfft=64)
    with pytest.raises(P.PhastPanic):
        P.PlannerPsd64(1000, 100, fs=0.0)
    with pytest.raises(P.PhastPanic):
        P.PlannerPsd32(1000, 4, window=np.zeros(4))
    with pytest.raises(ValueError):
        P.PlannerPsd64(1000, 100, window=np.ones(99))
    with pytest.raises(ValueError):
        P.PlannerPsd64(1000, 100, detrend="linear")   # out of scope
    with pytest.raises(ValueError):
        P.PlannerPsd64(1000, 100, scaling="power")
    with pytest.raises(TypeError):
        P.welch(np.zeros(1000))                        # the conveniences take device tensors
    from phastft_amd import _psd_window

    assert _psd_window("hann", 8) is None and _psd_window(None, 8) is None
    assert np.array_equal(_psd_window("boxcar", 5), np.ones(5))
    assert np.array_equal(_psd_window(("tukey", 0.25), 16), ss.get_window(("tukey", 0.25), 16))   # scipy is here: any name it takes


def test_rust_mirror():
    """Parsed textually, as tests/test_rust_shim.py does (no Rust toolchain here)"""
    src = os.path.join(ROOT, "rust", "phastft-hip", "src")
    ffi = open(os.path.join(src, "ffi.rs")).read()
    for name in NEW:
        assert re.search(r"fn " + name + r"\s*\(", ffi), name
    planner = open(os.path.join(src, "planner.rs")).read()
    assert "PlannerPsd64" in planner and "PlannerPsd32" in planner and "pub fn slab" in planner and "pub enum Detrend" in planner
    psd = open(os.path.join(src, "algorithms", "psd.rs")).read()
    for f in ("psd_f64_with_planner", "csd_f64_with_planner", "psd_f32_dev", "csd_f32_dev"):
        assert re.search(r"impl_psd!\([^;]*\b" + f + r"\b", psd), f  # the functions are stamped out by impl_psd!
    assert "pub mod psd;" in open(os.path.join(src, "algorithms", "mod.rs")).read()
    lib = open(os.path.join(src, "lib.rs")).read()
    assert "PlannerPsd64" in lib and "algorithms::psd" in lib
