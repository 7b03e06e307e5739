"""The STFT and its inverse (csrc/stft.hpp, csrc/planner_stft.hpp) without a GPU: stft.hpp's frame count, reflected index, tap
range and envelope minimum compiled with g++ and checked against Python integers; both schedules run in numpy through those
helpers around a long-double rfft / irfft against torch.stft / torch.istft; tests/stft_reference.py (the GPU tests' reference)
against torch as well; the new C ABI exported and listed, with every argument rule returned before the device is touched; the
C++ and Rust mirrors.

An inverse through a planner whose envelope minimum is 0 needs a planner, hence a device: tests/test_gpu_stft.py and
tests/cpp/stft_test.cpp check that refusal; here the same verdict is checked on stft_envelope_min, which is all the planner
consults."""
import ctypes as C
import itertools
import os
import re
import subprocess
import warnings

import numpy as np
import pytest
import scipy.fft as sf

from tests import stft_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = [f"phast_planner_stft{s}_{w}" for s in ("64", "32")
       for w in ("new", "free", "describe", "device_bytes", "frames", "bins", "workspace_len", "workspace_min", "envelope_min",
                 "time_stages")]
NEW += [f"phast_{k}_{fs}{suffix}" for k in ("stft", "istft") for fs in ("f64", "f32") for suffix in ("_with_planner", "_dev")]
OK, LEN_MISMATCH, NO_DEVICE, INVALID_ARG = 0, 2, 15, 16
GRID_L, GRID_F, GRID_H = (37, 64, 101), (1, 2, 7, 16, 30), (1, 3, 5, 16, 23)

HELPERS = r"""
#include "stft.hpp"
extern "C" {
unsigned long long frames(unsigned long long len, unsigned long long f, unsigned long long h, unsigned long long p) {
    return phast::stft_frames(len, f, h, p);
}
long long reflect(long long i, long long len) { return phast::stft_reflect(i, len); }
void taps(unsigned long long u, unsigned long long f, unsigned long long h, unsigned long long frames, long long *lo, long long *hi) {
    phast::stft_taps(u, f, h, frames, lo, hi);
}
int bad_args(unsigned long long len, unsigned long long f, unsigned long long h, int center, int pad) {
    return phast::stft_bad_args(len, f, h, center, pad);
}
double envelope_min(const double *w, unsigned long long len, unsigned long long f, unsigned long long h, unsigned long long p,
                    unsigned long long frames) {
    return phast::stft_envelope_min(w, len, f, h, p, frames);
}
}
"""


@pytest.fixture(scope="module")
def helpers(tmp_path_factory):
    d = tmp_path_factory.mktemp("stft_helpers")
    src, so = d / "helpers.cpp", d / "libstfthelpers.so"
    src.write_text(HELPERS)
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-shared", "-fPIC", "-I",
                        os.path.join(ROOT, "phastft_amd", "csrc"), str(src), "-o", str(so)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    h = C.CDLL(str(so))
    h.frames.restype = C.c_ulonglong
    h.frames.argtypes = [C.c_ulonglong] * 4
    h.reflect.restype = C.c_longlong
    h.reflect.argtypes = [C.c_longlong] * 2
    h.taps.argtypes = [C.c_ulonglong] * 4 + [C.POINTER(C.c_longlong)] * 2
    h.bad_args.argtypes = [C.c_ulonglong] * 3 + [C.c_int] * 2
    h.envelope_min.restype = C.c_double
    h.envelope_min.argtypes = [C.c_void_p] + [C.c_ulonglong] * 5
    return h


def _taps(h, u, f, hop, frames):
    lo, hi = C.c_longlong(), C.c_longlong()
    h.taps(u, f, hop, frames, C.byref(lo), C.byref(hi))
    return lo.value, hi.value


def test_helpers_against_python_integers(helpers):
    """frame count, reflected indices in range, and tap ranges that cover exactly the (f, j) with f H - p + j = t"""
    for f in (1, 2, 3, 7, 8, 16, 31, 32):
        for hop in sorted(v for v in {1, 2, 3, f // 2, f - 1, f} if 1 <= v <= f):
            for length in (1, 2, 5, 31, 32, 33, 64, 97, 120):
                for center in (0, 1):
                    p = f // 2 if center else 0
                    if (center and p >= length) or (not center and length < f):
                        assert helpers.bad_args(length, f, hop, center, 0)
                        continue
                    assert not helpers.bad_args(length, f, hop, center, 0)
                    frames = 1 + (length + 2 * p - f) // hop
                    assert helpers.frames(length, f, hop, p) == frames
                    for i in range(-p, (frames - 1) * hop - p + f):
                        r = helpers.reflect(i, length)
                        assert 0 <= r < length
                        assert r == (-i if i < 0 else 2 * (length - 1) - i if i >= length else i)
                    for t in range(length):
                        want = [k for k in range(frames) if 0 <= t + p - k * hop < f]
                        lo, hi = _taps(helpers, t + p, f, hop, frames)
                        assert list(range(lo, hi + 1)) == want, (length, f, hop, center, t)


def test_argument_rules_of_the_helper(helpers):
    big = 1 << 29
    for args, bad in (((100, 16, 4, 1, 0), 0), ((100, 16, 17, 1, 0), 1), ((100, 16, 0, 1, 0), 1), ((0, 16, 4, 1, 0), 1),
                      ((100, 0, 0, 1, 0), 1), ((big + 1, 16, 4, 1, 0), 1), ((big, big + 1, 4, 1, 1), 1),
                      ((8, 16, 4, 1, 0), 1),   # p = 8 >= L with reflect
                      ((8, 16, 4, 1, 1), 0),   # ... zeros may pad beyond the signal
                      ((9, 16, 4, 1, 0), 0), ((15, 16, 4, 0, 0), 1), ((16, 16, 4, 0, 7), 1), ((16, 16, 4, 0, 1), 0),
                      ((100, 16, 4, 2, 0), 1), ((100, 16, 4, 1, 2), 1),
                      ((big, 1024, 1, 1, 0), 1),   # frames * F > 2^30
                      ((1 << 20, 1024, 1, 1, 0), 1), ((1 << 20, 1024, 2, 1, 0), 0)):
        assert bool(helpers.bad_args(*args)) == bool(bad), args


class Schedule:
    """the two sweeps of stft.hip restated in numpy on stft.hpp's helpers, around a long-double rfft / irfft"""

    def __init__(self, h, length, f, hop, center, pad):
        self.h, self.len, self.f, self.hop, self.pad = h, length, f, hop, pad
        self.p = f // 2 if center else 0
        self.frames = h.frames(length, f, hop, self.p)

    def forward(self, x, w):
        i = np.arange(self.frames)[:, None] * self.hop - self.p + np.arange(self.f)[None, :]
        out = (i < 0) | (i >= self.len)
        src = i.copy()
        for v in np.unique(i[out]):  # only the first and last frames reflect or zero-fill
            src[i == v] = self.h.reflect(int(v), self.len) if self.pad == "reflect" else 0
        assert src.min() >= 0 and src.max() < self.len
        a = np.asarray(x, np.longdouble)[src]
        if self.pad != "reflect":
            a[out] = 0
        return sf.rfft(a * np.asarray(w, np.longdouble)[None, :], axis=1)

    def inverse(self, spec, w):
        y = sf.irfft(np.asarray(spec, np.clongdouble), n=self.f, axis=1)
        out = np.zeros(self.len, np.longdouble)
        for t in range(self.len):
            u = t + self.p
            lo, hi = _taps(self.h, u, self.f, self.hop, self.frames)
            num = den = np.longdouble(0)
            for k in range(lo, hi + 1):
                j = u - k * self.hop
                num += np.longdouble(w[j]) * y[k, j]
                den += np.longdouble(w[j]) ** 2
            out[t] = num / den if hi >= lo else 0
        return out

    def envelope_min(self, w):
        w = np.ascontiguousarray(w, np.float64)
        return self.h.envelope_min(w.ctypes.data_as(C.c_void_p), self.len, self.f, self.hop, self.p, self.frames)


def _grid():
    for length, f, hop, center, pad, win in itertools.product(GRID_L, GRID_F, GRID_H, (False, True), ("reflect", "zero"),
                                                              R.WINDOWS):
        if hop <= f:
            yield length, f, hop, center, pad, win


def test_schedules_and_reference_match_torch(helpers):
    """forward and inverse of the restated schedules and of tests/stft_reference.py against torch.stft / torch.istft on the
    whole grid; the NOLA verdict of stft_envelope_min and of the reference is torch's in every case"""
    import torch

    worst_f = worst_i = 0.0
    inverted = 0
    for length, f, hop, center, pad, win in _grid():
        case = (length, f, hop, center, pad, win)
        x = np.random.default_rng([length, f, hop]).uniform(-1, 1, length)
        w = R.window(win, f)
        sch = Schedule(helpers, length, f, hop, center, pad)
        want = torch.stft(torch.from_numpy(x), f, hop, window=torch.from_numpy(w), center=center,
                          pad_mode="reflect" if pad == "reflect" else "constant", return_complex=True).numpy().T
        got = sch.forward(x, w)
        assert got.shape == want.shape == (sch.frames, f // 2 + 1), case
        ref = R.stft(x, w, f, hop, center, pad)
        worst_f = max(worst_f, float(np.abs(got - want).max()), float(np.abs(ref - want).max()))
        env = sch.envelope_min(w)
        ok = R.invertible(w, length, f, hop, center)
        assert (env > R.NOLA_MIN) == ok, case
        den, cnt = R.envelope(w, length, f, hop, center)
        assert abs(env - den[cnt > 0].min()) <= 1e-14 * max(1.0, env), case
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")  # torch warns where length reaches past the last frame: the zero tail
                back = torch.istft(torch.from_numpy(want.T.copy()), f, hop, window=torch.from_numpy(w), center=center,
                                   length=length).numpy()
            torch_ok = True
        except RuntimeError:
            torch_ok = False
        assert torch_ok == ok, case
        if ok:
            inverted += 1
            worst_i = max(worst_i, float(np.abs(sch.inverse(want, w) - back).max()),
                          float(np.abs(R.istft(want, w, length, f, hop, center) - back).max()))
    print(f"forward worst {worst_f:.2e}, inverse worst {worst_i:.2e}, {inverted} inverted")
    assert worst_f < 2e-14 and worst_i < 2e-14, (worst_f, worst_i)
    assert inverted > 300


def test_a_window_that_starts_at_zero_does_not_invert_uncentred(helpers):
    """Hann with center = 0: w[0] = 0 is the only tap of sample 0, so the envelope minimum is exactly 0 -- the inverse refuses"""
    for f, hop in ((16, 4), (30, 23), (1024, 256)):
        sch = Schedule(helpers, 4 * f, f, hop, False, "reflect")
        assert sch.envelope_min(R.window("hann", f)) == 0.0
        assert sch.envelope_min(R.window("rect", f)) >= 1.0
        assert helpers.envelope_min(None, 4 * f, f, hop, 0, sch.frames) >= 1.0  # NULL: all ones


def test_envelope_minimum_is_linear_work(helpers):
    """L = 2^18, F = 4096, H = 1: 10^9 taps by the definition, a blink by the prefix sums.  With H = 1 the envelope is a
    running sum of w^2 that is complete in the interior, so the minimum sits at one of the two ends"""
    import time

    length, f, hop = 1 << 18, 4096, 1
    w = R.window("hann", f)
    t0 = time.perf_counter()
    got = helpers.envelope_min(w.ctypes.data_as(C.c_void_p), length, f, hop, f // 2, 1 + length // hop)
    assert time.perf_counter() - t0 < 1.0
    first, last = np.sum(w[:f // 2 + 1] ** 2), np.sum(w[f // 2 - 1:] ** 2)  # t = 0 and t = L - 1
    assert abs(got - min(first, last)) < 1e-9


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
    for const in ("PHAST_PAD_REFLECT 0", "PHAST_PAD_ZERO 1"):
        assert "#define " + const in header
    import phastft_amd as P

    for name in ("PlannerStft64", "PlannerStft32", "stft_batched", "istft_batched", "stft_f64_with_planner",
                 "stft_f32_with_planner", "istft_f64_with_planner", "istft_f32_with_planner"):
        assert name in P.__all__ and callable(getattr(P, name)), name
    assert "PlannerStft64/32" in P.__doc__


def test_argument_codes(lib):
    """every rule of _new, null planners and null outputs come back before the device is touched"""
    big = 1 << 29
    for sfx, fs, dt in (("64", "f64", np.float64), ("32", "f32", np.float32)):
        new = getattr(lib, f"phast_planner_stft{sfx}_new")
        w = np.ones(16, dt)
        wp = w.ctypes.data_as(C.c_void_p)

        def make(length, f, hop, center, pad, out=True, win=wp):
            h = C.c_void_p(1)
            rc = new(C.c_size_t(length), C.c_size_t(f), C.c_size_t(hop), win, C.c_int(center), C.c_int(pad),
                     C.byref(h) if out else None)
            assert rc == OK or not h.value or not out
            return rc

        assert make(100, 16, 17, 1, 0) == INVALID_ARG          # H > F
        assert make(100, 16, 0, 1, 0) == INVALID_ARG           # H = 0
        assert make(100, 0, 0, 1, 0) == INVALID_ARG            # F = 0
        assert make(0, 16, 4, 1, 0) == INVALID_ARG             # L = 0
        assert make(big + 1, 16, 4, 1, 0) == INVALID_ARG       # L > 2^29
        assert make(big, big + 1, 4, 1, 1) == INVALID_ARG      # F > 2^29
        assert make(8, 16, 4, 1, 0) == INVALID_ARG             # p >= L with center and reflect
        assert make(15, 16, 4, 0, 0) == INVALID_ARG            # L < F without center
        assert make(1 << 20, 1024, 1, 1, 0, win=None) == INVALID_ARG  # frames * F > 2^30
        assert make(100, 16, 4, 2, 0) == INVALID_ARG           # center is 0 or 1
        assert make(100, 16, 4, 1, 2) == INVALID_ARG           # pad_mode is PHAST_PAD_REFLECT or PHAST_PAD_ZERO
        assert make(100, 16, 4, 1, 0, out=False) == INVALID_ARG
        for name, one in (("workspace_len", C.c_size_t(1)), ("workspace_min", C.c_int(1))):  # (p, size_t batch), (p, int inverse)
            fn = getattr(lib, f"phast_planner_stft{sfx}_{name}")
            fn.restype = C.c_size_t
            assert fn(None, one) == 0
        for name in ("device_bytes", "frames", "bins"):
            assert getattr(lib, f"phast_planner_stft{sfx}_{name}")(None) == 0
        assert getattr(lib, f"phast_planner_stft{sfx}_envelope_min")(None) == 0.0
        assert getattr(lib, f"phast_planner_stft{sfx}_describe")(None, C.create_string_buffer(8), C.c_size_t(8)) == INVALID_ARG
        ms = (C.c_float * 2)()
        assert getattr(lib, f"phast_planner_stft{sfx}_time_stages")(None, 0, None, None, None, C.c_size_t(1), None,
                                                                    C.c_size_t(0), 1, ms, None) == INVALID_ARG
        x, a, b = np.zeros(100, dt), np.zeros(9 * 26, dt), np.zeros(9 * 26, dt)
        p = lambda v: v.ctypes.data_as(C.c_void_p)  # noqa: E731
        n = C.c_size_t
        assert getattr(lib, f"phast_stft_{fs}_with_planner")(p(x), n(100), p(a), n(a.size), p(b), n(b.size), None) == INVALID_ARG
        assert getattr(lib, f"phast_istft_{fs}_with_planner")(p(a), n(a.size), p(b), n(b.size), p(x), n(100), None) == INVALID_ARG
        assert getattr(lib, f"phast_stft_{fs}_dev")(p(x), p(a), p(b), n(100), n(1), n(100), None, None, n(0), None) == INVALID_ARG
        assert getattr(lib, f"phast_istft_{fs}_dev")(p(a), p(b), p(x), n(100), n(1), n(100), None, None, n(0), None) == INVALID_ARG


def test_calls_without_a_gpu_fail_loudly(lib):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present: tests/test_gpu_stft.py covers the device side")
    h = C.c_void_p()
    assert lib.phast_planner_stft64_new(C.c_size_t(1000), C.c_size_t(16), C.c_size_t(4), None, 1, 0, C.byref(h)) == NO_DEVICE
    assert not h.value
    assert lib.phast_planner_stft32_new(C.c_size_t(1000), C.c_size_t(30), C.c_size_t(23), None, 0, 1, C.byref(h)) == NO_DEVICE
    import phastft_amd as P

    with pytest.raises(P.PhastHipError):
        P.PlannerStft64(1000, 16, 4)


def test_python_argument_errors():
    import phastft_amd as P

    with pytest.raises(ValueError):
        P.PlannerStft64(100, 16, 4, pad_mode="edge")
    with pytest.raises(ValueError):
        P.PlannerStft32(100, 16, 4, window=np.ones(17))
    with pytest.raises(P.PhastPanic):
        P.PlannerStft64(100, 16, 17)       # H > F: INVALID_ARG before the device is touched
    with pytest.raises(P.PhastPanic):
        P.PlannerStft32(8, 16, 4)          # p >= L


def test_cpp_mirror_without_gpu(tmp_path):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present: tests/test_gpu_stft.py runs the mirror there")
    from phastft_amd import build

    lib = build.build()
    exe = str(tmp_path / "stft_test")
    libdir = os.path.dirname(lib)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "stft_test.cpp"), "-o", exe, "-L", libdir, "-lphastft_hip",
                        f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "stft: ok" in r.stdout, r.stdout + r.stderr


def test_rust_mirror():
    """Parsed textually, as tests/test_rust_shim.py does (no Rust toolchain here)"""
    src = os.path.join(ROOT, "rust", "phastft-hip", "src")
    ffi = open(os.path.join(src, "ffi.rs")).read()
    for name in NEW:
        assert re.search(r"fn " + name + r"\s*\(", ffi), name
    planner = open(os.path.join(src, "planner.rs")).read()
    assert "PlannerStft64" in planner and "PlannerStft32" in planner
    stft = open(os.path.join(src, "algorithms", "stft.rs")).read()
    for f in ("stft_f64_with_planner", "stft_f32_with_planner", "istft_f64_with_planner", "istft_f32_with_planner"):
        assert re.search(r"\b" + f + r"\b", stft), f
    lib = open(os.path.join(src, "lib.rs")).read()
    assert "PlannerStft64" in lib and "stft" in lib
