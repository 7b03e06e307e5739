"""Overlap-save convolution and correlation (csrc/conv.hpp, csrc/planner_conv.hpp) without a GPU: conv.hpp's geometry, automatic
block and argument rules compiled with g++ and checked against Python integers; the overlap-save schedule run in numpy through
those helpers around pocketfft's double rfft / irfft, against scipy.signal.convolve / correlate(method="direct") and against
tests/conv_reference.py (the GPU tests' reference); the new C ABI exported and listed, with every argument rule returned
before the device is touched; the C++ and Rust mirrors."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.fft as sf
import scipy.signal as ss

from tests import conv_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = [f"phast_planner_conv{s}_{w}" for s in ("64", "32")
       for w in ("new", "free", "describe", "device_bytes", "out_len", "block", "segments", "workspace_len", "workspace_min",
                 "time_stages")]
NEW += [f"phast_conv_{fs}{suffix}" for fs in ("f64", "f32") for suffix in ("_with_planner", "_dev")]
OK, LEN_MISMATCH, NO_DEVICE, INVALID_ARG = 0, 2, 15, 16
MODE = {"full": 0, "same": 1, "valid": 2}
# the GPU tests' shapes (L, K, B), and a few more where out_len is an exact multiple of S in some mode
SHAPES = [(1, 1, 1), (37, 1, 8), (64, 5, 8), (100, 17, 17), (101, 7, 16), (10, 30, 64), (1000, 30, 64), (1000, 33, 100),
          (4099, 64, 256), (5000, 251, 1000), (5000, 1000, 4096), (5000, 1000, 1024), (40, 5, 12), (36, 5, 12), (24, 1, 8)]

HELPERS = r"""
#include "conv.hpp"
extern "C" {
unsigned long long t0(unsigned long long k, int mode) { return phast::conv_t0(k, mode); }
unsigned long long out_len(unsigned long long len, unsigned long long k, int mode) { return phast::conv_out_len(len, k, mode); }
unsigned long long segments(unsigned long long n, unsigned long long k, unsigned long long b) { return phast::conv_segments(n, k, b); }
unsigned long long row(unsigned long long b, unsigned long long vec) { return phast::conv_row(b, vec); }
unsigned long long auto_block(unsigned long long len, unsigned long long k) { return phast::conv_auto_block(len, k); }
int bad_args(unsigned long long len, unsigned long long k, int mode, int flip, unsigned long long block, unsigned long long vec) {
    return phast::conv_bad_args(len, k, mode, flip, block, vec);
}
}
"""


@pytest.fixture(scope="module")
def helpers(tmp_path_factory):
    d = tmp_path_factory.mktemp("conv_helpers")
    src, so = d / "helpers.cpp", d / "libconvhelpers.so"
    src.write_text(HELPERS)
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-shared", "-fPIC", "-I",
                        os.path.join(ROOT, "phastft_amd", "csrc"), str(src), "-o", str(so)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    h = C.CDLL(str(so))
    for name, argtypes in (("t0", [C.c_ulonglong, C.c_int]), ("out_len", [C.c_ulonglong] * 2 + [C.c_int]),
                           ("segments", [C.c_ulonglong] * 3), ("row", [C.c_ulonglong] * 2), ("auto_block", [C.c_ulonglong] * 2)):
        getattr(h, name).restype = C.c_ulonglong
        getattr(h, name).argtypes = argtypes
    h.bad_args.argtypes = [C.c_ulonglong] * 2 + [C.c_int] * 2 + [C.c_ulonglong] * 2
    return h


def test_helpers_against_python_integers(helpers):
    """t0, out_len and the segment count over a grid with K = 1, B = K (S = 1), K > L, and out_len a multiple and a
    non-multiple of S; the segments cover [0, out_len) exactly once and read inside the row"""
    multiples = ragged = 0
    for length in (1, 2, 5, 10, 31, 32, 33, 64, 97):
        for k in (1, 2, 3, 7, 8, 30, 40):
            for b in sorted({k, k + 1, k + 2, 2 * k, 4 * k + 3, 64}):
                if b < k:
                    continue
                for mode, m in MODE.items():
                    t0, n = {"full": (0, length + k - 1), "same": ((k - 1) // 2, length), "valid": (k - 1, length - k + 1)}[mode]
                    assert helpers.t0(k, m) == t0
                    if mode == "valid" and length < k:
                        assert helpers.out_len(length, k, m) == 0 and helpers.bad_args(length, k, m, 0, b, 2)
                        continue
                    assert helpers.out_len(length, k, m) == n
                    assert not helpers.bad_args(length, k, m, 0, b, 2) and not helpers.bad_args(length, k, m, 1, b, 4)
                    s = b - k + 1
                    segs = helpers.segments(n, k, b)
                    assert segs == -(-n // s) and (segs - 1) * s < n <= segs * s
                    multiples += n % s == 0
                    ragged += n % s != 0
                    # the last sample a segment saves is element K - 1 + S - 1 = B - 1 of its row
                    assert k - 1 + min(s, n - (segs - 1) * s) - 1 <= b - 1
    assert multiples > 100 and ragged > 100
    for b, vec, want in ((1, 2, 2), (1, 4, 4), (8, 4, 8), (17, 2, 18), (17, 4, 20), (1000, 4, 1000), (1 << 29, 4, 1 << 29)):
        assert helpers.row(b, vec) == want


def test_automatic_block(helpers):
    """the smallest power of two >= 4 (K - 1), at least 1024 and at most 2^29; the smallest power of two >= L + K - 1 where
    that is smaller"""

    def pow2(v):
        return 1 << max(v - 1, 0).bit_length()

    for length, k in ((1, 1), (2, 1), (10, 30), (5000, 251), (5000, 1000), (1 << 24, 32), (1 << 24, 1000), (1 << 24, 16384),
                      (1 << 24, 257), (1 << 24, 258), (1 << 29, 1 << 29), (1 << 29, (1 << 27) + 2), (300, 300)):
        want = min(max(pow2(4 * (k - 1)), 1024), 1 << 29, pow2(length + k - 1))
        got = helpers.auto_block(length, k)
        assert got == want and got >= k and got & (got - 1) == 0, (length, k, got, want)
    assert helpers.auto_block(1, 1) == 1 and helpers.auto_block(10, 30) == 64
    assert helpers.auto_block(1 << 24, 1000) == 4096 and helpers.auto_block(1 << 24, 16384) == 65536


def test_argument_rules_of_the_helper(helpers):
    big = 1 << 29
    for args, bad in (((100, 16, 0, 0, 64, 2), 0), ((100, 16, 2, 1, 16, 4), 0), ((100, 16, 0, 0, 0, 2), 0),
                      ((15, 16, 2, 0, 64, 2), 1),        # valid with L < K
                      ((15, 16, 1, 0, 64, 2), 0),        # ... same and full take K > L
                      ((100, 16, 0, 0, 15, 2), 1),       # B < K
                      ((100, 0, 0, 0, 64, 2), 1),        # K = 0
                      ((0, 16, 0, 0, 64, 2), 1),         # L = 0
                      ((big + 1, 16, 1, 0, 64, 2), 1),   # L > 2^29
                      ((100, big + 1, 1, 0, 0, 2), 1),   # K > 2^29
                      ((big, 16, 0, 0, 1 << 20, 2), 1),  # out_len = L + K - 1 > 2^29
                      ((big, 16, 1, 0, 1 << 20, 2), 0),
                      ((100, 16, 0, 0, big + 1, 2), 1),  # B > 2^29
                      ((100, 16, 3, 0, 64, 2), 1), ((100, 16, -1, 0, 64, 2), 1),  # the mode
                      ((100, 16, 0, 2, 64, 2), 1),       # flip is 0 or 1
                      ((100, 16, 0, 0, 64, 3), 1),       # 16 bytes hold 2 or 4 elements
                      ((big, 16, 1, 0, 16, 2), 1),       # S = 1: segments * fd = 2^33
                      ((1 << 26, 1, 1, 0, 16, 2), 0),    # segments * fd = 2^22 * 16
                      ((big, 17, 1, 0, 32, 4), 0),       # S = 16: 2^25 segments * 32 = 2^30 exactly
                      ((big, 18, 1, 0, 33, 4), 1)):      # ... and * 36, the row of 33 floats rounded up to 16 bytes
        assert bool(helpers.bad_args(*args)) == bool(bad), args


def overlap_save(h, x, taps, b, mode, flip, dtype=np.float64):
    """the three sweeps of conv.hip restated in numpy on conv.hpp's helpers, around pocketfft's rfft / irfft per row"""
    length, k = len(x), len(taps)
    t0, n = h.t0(k, MODE[mode]), h.out_len(length, k, MODE[mode])
    s, segs = b - k + 1, h.segments(n, k, b)
    g = np.asarray(taps[::-1] if flip else taps, np.float64)
    spec = sf.rfft(np.pad(g, (0, b - k))).astype(np.complex64 if dtype == np.float32 else np.complex128)
    idx = t0 - (k - 1) + np.arange(segs)[:, None] * s + np.arange(b)[None, :]          # segment sweep
    rows = np.where((idx >= 0) & (idx < length), np.asarray(x, dtype)[np.clip(idx, 0, length - 1)], dtype(0))
    y = sf.irfft(sf.rfft(rows, axis=1) * spec[None, :], n=b, axis=1)                    # R2C, spectrum sweep, C2R
    assert y.dtype == dtype
    i = np.arange(n)                                                                    # save sweep
    return y[i // s, k - 1 + i % s]


def test_schedule_against_scipy_and_the_reference(helpers):
    """every mode and both flips over all shapes and both tap kinds, in double: against scipy's direct sums and against
    tests/conv_reference.py; the worst difference is printed (DESIGN.md §16 quotes it)"""
    worst_ref = worst_scipy = ref_vs_scipy = 0.0
    for length, k, b in SHAPES:
        x = R.signal(length)
        for kind in R.TAPS:
            taps = R.taps(kind, k)
            for mode in R.MODES:
                if mode == "valid" and length < k:
                    assert R.geometry(length, k, mode)[1] == 0
                    continue
                for flip in (False, True):
                    want = R.convolve(x, taps, mode, flip)
                    direct = (ss.correlate if flip else ss.convolve)(x, taps, mode=mode, method="direct")
                    got = overlap_save(helpers, x, taps, b, mode, flip)
                    assert got.shape == want.shape == direct.shape, (length, k, b, mode, flip)
                    scale = float(np.sqrt(np.mean(want.astype(np.float64) ** 2))) or 1.0
                    worst_ref = max(worst_ref, float(np.abs(got - want).max()) / scale)
                    worst_scipy = max(worst_scipy, float(np.abs(got - direct).max()) / scale)
                    ref_vs_scipy = max(ref_vs_scipy, float(np.abs(direct - want).max()) / scale)
    print(f"overlap-save in double, worst |difference| / rms of the output: vs conv_reference {worst_ref:.3e}, vs scipy direct "
          f"{worst_scipy:.3e}; conv_reference vs scipy direct {ref_vs_scipy:.3e}")
    # a direct sum of K <= 1000 products in double and a double transform of B <= 4096 both stay far below this
    assert worst_ref < 1e-12 and worst_scipy < 1e-12 and ref_vs_scipy < 1e-12


def test_schedule_with_the_automatic_block(helpers):
    for length, k in ((5000, 251), (10, 30), (1, 1), (3000, 300)):
        b = helpers.auto_block(length, k)
        x, taps = R.signal(length, seed=1), R.taps("random", k, seed=1)
        for mode in ("full", "same"):
            got = overlap_save(helpers, x, taps, b, mode, True)
            assert np.abs(got - R.convolve(x, taps, mode, True)).max() < 1e-11


@pytest.fixture(scope="module")
def lib():
    from phastft_amd import _lib

    return _lib.lib()


def test_new_symbols_are_exported_and_listed(lib):
    from phastft_amd import _lib

    header = open(os.path.join(ROOT, "include", "phastft_hip.h")).read()
    assert len(NEW) == 24
    for name in NEW:
        getattr(lib, name)
        assert name in _lib.SYMBOLS and re.search(r"\b" + name + r"\s*\(", header), name
    for const in ("PHAST_CONV_FULL 0", "PHAST_CONV_SAME 1", "PHAST_CONV_VALID 2"):
        assert "#define " + const in header
    import phastft_amd as P

    for name in ("PlannerConv64", "PlannerConv32", "conv_batched", "conv_f64_with_planner", "conv_f32_with_planner",
                 "fftconvolve", "correlate"):
        assert name in P.__all__ and callable(getattr(P, name)), name
    assert "PlannerConv64/32" in P.__doc__


def test_argument_codes(lib):
    """every rule of _new, null planners and null pointers come back before the device is touched"""
    big = 1 << 29
    for sfx, fs, dt in (("64", "f64", np.float64), ("32", "f32", np.float32)):
        new = getattr(lib, f"phast_planner_conv{sfx}_new")
        taps = np.ones(16, dt)
        tp = taps.ctypes.data_as(C.c_void_p)

        def make(length, k, mode, flip, block, out=True, h=tp):
            p = C.c_void_p(1)
            rc = new(C.c_size_t(length), h, C.c_size_t(k), C.c_int(mode), C.c_int(flip), C.c_size_t(block),
                     C.byref(p) if out else None)
            assert rc == OK or not p.value or not out
            return rc

        assert make(15, 16, 2, 0, 64) == INVALID_ARG           # valid with L < K
        assert make(100, 16, 0, 0, 15) == INVALID_ARG          # B < K
        assert make(100, 0, 0, 0, 64) == INVALID_ARG           # K = 0
        assert make(0, 16, 0, 0, 64) == INVALID_ARG            # L = 0
        assert make(big + 1, 16, 1, 0, 64) == INVALID_ARG      # L > 2^29
        assert make(100, big + 1, 1, 0, 0) == INVALID_ARG      # K > 2^29 (the taps are not read)
        assert make(big, 16, 0, 0, 1 << 20) == INVALID_ARG     # out_len > 2^29
        assert make(100, 16, 0, 0, big + 1) == INVALID_ARG     # B > 2^29
        assert make(big, 16, 1, 0, 16) == INVALID_ARG          # segments * fd > 2^30
        assert make(100, 16, 3, 0, 64) == INVALID_ARG          # the mode
        assert make(100, 16, 0, 2, 64) == INVALID_ARG          # flip is 0 or 1
        assert make(100, 16, 0, 0, 64, h=None) == INVALID_ARG  # no taps
        assert make(100, 16, 0, 0, 64, out=False) == INVALID_ARG
        fn = getattr(lib, f"phast_planner_conv{sfx}_workspace_len")
        fn.restype = C.c_size_t
        assert fn(None, C.c_size_t(1)) == 0
        for name in ("device_bytes", "out_len", "block", "segments", "workspace_min"):
            assert getattr(lib, f"phast_planner_conv{sfx}_{name}")(None) == 0
        assert getattr(lib, f"phast_planner_conv{sfx}_describe")(None, C.create_string_buffer(8), C.c_size_t(8)) == INVALID_ARG
        ms = (C.c_float * 5)()
        assert getattr(lib, f"phast_planner_conv{sfx}_time_stages")(None, None, None, C.c_size_t(1), None, C.c_size_t(0), 1, ms,
                                                                    None) == INVALID_ARG
        x, y = np.zeros(100, dt), np.zeros(115, dt)
        p = lambda v: v.ctypes.data_as(C.c_void_p)  # noqa: E731
        n = C.c_size_t
        assert getattr(lib, f"phast_conv_{fs}_with_planner")(p(x), n(100), p(y), n(115), None) == INVALID_ARG
        assert getattr(lib, f"phast_conv_{fs}_dev")(p(x), p(y), n(100), n(1), n(100), n(115), None, None, n(0), None) == INVALID_ARG


def test_calls_without_a_gpu_fail_loudly(lib):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present: tests/test_gpu_conv.py covers the device side")
    h = C.c_void_p()
    taps = np.ones(16)
    tp = taps.ctypes.data_as(C.c_void_p)
    assert lib.phast_planner_conv64_new(C.c_size_t(1000), tp, C.c_size_t(16), 0, 0, C.c_size_t(0), C.byref(h)) == NO_DEVICE
    assert not h.value
    taps32 = np.ones(16, np.float32)
    assert lib.phast_planner_conv32_new(C.c_size_t(1000), taps32.ctypes.data_as(C.c_void_p), C.c_size_t(16), 1, 1, C.c_size_t(100),
                                        C.byref(h)) == NO_DEVICE
    import phastft_amd as P

    with pytest.raises(P.PhastHipError):
        P.PlannerConv64(1000, taps)


def test_python_argument_errors():
    import phastft_amd as P

    with pytest.raises(ValueError):
        P.PlannerConv64(100, np.ones(16), mode="wrap")
    with pytest.raises(P.PhastPanic):
        P.PlannerConv64(15, np.ones(16), mode="valid")   # L < K: INVALID_ARG before the device is touched
    with pytest.raises(P.PhastPanic):
        P.PlannerConv32(100, np.ones(16), block=15)      # B < K
    with pytest.raises(P.PhastPanic):
        P.PlannerConv32(100, np.ones(0))                 # no taps


def test_cpp_mirror_without_gpu(tmp_path):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present: tests/test_gpu_conv.py runs the mirror there")
    from phastft_amd import build

    lib = build.build()
    exe = str(tmp_path / "conv_test")
    libdir = os.path.dirname(lib)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "conv_test.cpp"), "-o", exe, "-L", libdir, "-lphastft_hip",
                        f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "conv: ok" in r.stdout, r.stdout + r.stderr


def test_rust_mirror():
    """Parsed textually, as tests/test_rust_shim.py does (no Rust toolchain here)"""
    src = os.path.join(ROOT, "rust", "phastft-hip", "src")
    ffi = open(os.path.join(src, "ffi.rs")).read()
    for name in NEW:
        assert re.search(r"fn " + name + r"\s*\(", ffi), name
    planner = open(os.path.join(src, "planner.rs")).read()
    assert "PlannerConv64" in planner and "PlannerConv32" in planner
    conv = open(os.path.join(src, "algorithms", "conv.rs")).read()
    for f in ("conv_f64_with_planner", "conv_f32_with_planner", "conv_f64_dev", "conv_f32_dev"):
        assert re.search(r"\b" + f + r"\b", conv), f
    lib = open(os.path.join(src, "lib.rs")).read()
    assert "PlannerConv64" in lib and "conv" in lib
