"""DCT / DST of types II and III (csrc/dct.hpp, csrc/planner_dct.hpp) without a GPU: dct.hpp's index, sign and scale helpers
compiled with g++ and run step by step around a long-double rfft / irfft against scipy.fft.dct / dst, the new C ABI exported
and listed with its argument codes returned before the device is touched, the Python idct / idst mapping, the C++ and Rust
mirrors, and gates of tests/test_gpu_dct.py that a wrong twiddle fails."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.fft as sf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = [f"phast_planner_dct{s}_{w}" for s in ("64", "32")
       for w in ("new", "free", "describe", "device_bytes", "workspace_len", "time_stages")]
NEW += [f"phast_{k}_{fs}{suffix}" for k in ("dct", "dst") for fs in ("f64", "f32") for suffix in ("", "_with_planner", "_dev")]
OK, LEN_MISMATCH, NO_DEVICE, INVALID_ARG = 0, 2, 15, 16
KINDS = [("dct", 2), ("dct", 3), ("dst", 2), ("dst", 3)]
NORMS = [None, "ortho", "forward"]
NORM_CODE = {None: 0, "ortho": 1, "forward": 2}

HELPERS = r"""
#include "dct.hpp"
extern "C" {
void perm(unsigned long long n, int dst, unsigned long long *src, double *sign) {
    for (unsigned long long i = 0; i < n; ++i) { src[i] = phast::dct_perm_src(i, n); sign[i] = phast::dct_perm_sign(dst, i, n); }
}
void twiddle(int type, unsigned long long n, double *turns) {
    for (unsigned long long k = 0; k <= n / 2; ++k) turns[k] = phast::dct_turns(type, k, n);
}
void scales(int type, int norm, unsigned long long n, double *s) { s[0] = phast::dct_scale(type, norm, n); s[1] = phast::dct_scale0(type, norm, n); }
void ii_index(int dst, unsigned long long n, unsigned long long *re, unsigned long long *im) {
    for (unsigned long long k = 0; k <= n / 2; ++k) { re[k] = phast::dct2_re_index(dst, k, n); im[k] = k ? phast::dct2_im_index(dst, k, n) : 0; }
}
void iii_index(int dst, unsigned long long n, unsigned long long *a, unsigned long long *b) {
    for (unsigned long long k = 0; k <= n / 2; ++k) { a[k] = phast::dct3_a_index(dst, k, n); b[k] = k ? phast::dct3_b_index(dst, k, n) : 0; }
}
}
"""


@pytest.fixture(scope="module")
def helpers(tmp_path_factory):
    d = tmp_path_factory.mktemp("dct_helpers")
    src, so = d / "helpers.cpp", d / "libdcthelpers.so"
    src.write_text(HELPERS)
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-shared", "-fPIC", "-I",
                        os.path.join(ROOT, "phastft_amd", "csrc"), str(src), "-o", str(so)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return C.CDLL(str(so))


def _u64(n):
    return np.zeros(n, np.uint64)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class Schedule:
    """the four sweeps of planner_dct.hpp restated in numpy on dct.hpp's helpers, around a long-double rfft / irfft; `phase`
    replaces the twiddle angle (the gate-sensitivity test)"""

    def __init__(self, h, n, phase=None):
        self.h, self.n, self.phase = h, n, phase

    def _perm(self, dst):
        src, sign = _u64(self.n), np.zeros(self.n)
        self.h.perm(C.c_ulonglong(self.n), C.c_int(dst), _ptr(src), _ptr(sign))
        return src.astype(np.int64), sign

    def _tw(self, t, norm):
        n, hh = self.n, self.n // 2
        turns, s = np.zeros(hh + 1), np.zeros(2)
        self.h.twiddle(C.c_int(t), C.c_ulonglong(n), _ptr(turns))
        self.h.scales(C.c_int(t), C.c_int(NORM_CODE[norm]), C.c_ulonglong(n), _ptr(s))
        if self.phase is not None:
            turns = self.phase(t, np.arange(hh + 1), n)
        ang = np.pi * turns.astype(np.longdouble)
        sc = np.full(hh + 1, s[0], np.longdouble)
        sc[0] = s[1]
        return np.cos(ang), np.sin(ang), sc

    def ii(self, x, dst, norm):
        n, hh, e = self.n, self.n // 2, (self.n + 1) // 2
        src, sign = self._perm(dst)
        v = x[src].astype(np.longdouble) * sign                     # II-pre: permute (DST: odd samples negated)
        V = sf.rfft(v)                                                # the real planner's R2C
        c, s, sc = self._tw(2, norm)
        zr = sc * (V.real * c - V.imag * s)
        zi = -sc * (V.real * s + V.imag * c)
        re_i, im_i = _u64(hh + 1), _u64(hh + 1)
        self.h.ii_index(C.c_int(dst), C.c_ulonglong(n), _ptr(re_i), _ptr(im_i))
        y = np.full(n, np.nan, np.longdouble)
        y[re_i.astype(np.int64)] = zr                                 # II-post: bins 0 .. h from the real part
        k = np.arange(1, e)
        y[im_i.astype(np.int64)[k]] = zi[k]                           # ... and N - k (DST: k - 1) from the imaginary part
        return y

    def iii(self, X, dst, norm):
        n, hh = self.n, self.n // 2
        a_i, b_i = _u64(hh + 1), _u64(hh + 1)
        self.h.iii_index(C.c_int(dst), C.c_ulonglong(n), _ptr(a_i), _ptr(b_i))
        A = X[a_i.astype(np.int64)].astype(np.longdouble)
        B = X[b_i.astype(np.int64)].astype(np.longdouble)
        B[0] = 0                                                      # X'[N] := 0
        c, s, sc = self._tw(3, norm)
        Vr, Vi = sc * (c * A + s * B), sc * (s * A - c * B)
        Vi[0] = 0                                                     # exact zeros
        if n % 2 == 0:
            Vi[hh] = 0
        v = sf.irfft(Vr + 1j * Vi, n)                                 # the real planner's C2R (1/N)
        src, sign = self._perm(dst)
        x = np.full(n, np.nan, np.longdouble)
        x[src] = v * sign                                             # III-post: un-permute (DST: odd outputs negated)
        return x


def _ref(kind, t, x, norm):
    return (sf.dct if kind == "dct" else sf.dst)(x.astype(np.longdouble), type=t, norm=norm)


def _rel(got, want):
    want = np.asarray(want, np.longdouble)
    den = np.sqrt(np.sum(want * want))
    return float(np.sqrt(np.sum((np.asarray(got, np.longdouble) - want) ** 2)) / (den if den else 1))


def test_schedules_match_scipy_for_every_length_up_to_300(helpers):
    worst = 0.0
    for n in range(1, 301):
        x = np.random.default_rng([n, 5]).uniform(-1, 1, n)
        x.flags.writeable = False  # no step writes the caller's input
        sch = Schedule(helpers, n)
        for kind, t in KINDS:
            for norm in NORMS:
                got = (sch.ii if t == 2 else sch.iii)(x, kind == "dst", norm)
                assert not np.isnan(got).any(), (kind, t, norm, n)  # every output written
                e = _rel(got, _ref(kind, t, x, norm))
                worst = max(worst, e)
                assert e < 1e-14, (kind, t, norm, n, e)
    assert worst > 0


def test_gates_catch_wrong_twiddles(helpers):
    """tests/test_gpu_dct.py's gates on the restated schedule: e^{-i pi k / N} in place of e^{-i pi k / (2N)} misses them"""
    from tests.test_gpu_dct import dct_gates

    wrong = lambda t, k, n: (-1.0 if t == 2 else 1.0) * k / n  # noqa: E731
    for n in (16, 17, 1000, 1001):
        x = np.random.default_rng([n, 6]).uniform(-1, 1, n)
        good, bad = Schedule(helpers, n), Schedule(helpers, n, wrong)
        g_rel, _ = dct_gates("f64", n)
        for kind, t in KINDS:
            want = _ref(kind, t, x, None)
            assert _rel((good.ii if t == 2 else good.iii)(x, kind == "dst", None), want) < g_rel / 100
            assert _rel((bad.ii if t == 2 else bad.iii)(x, kind == "dst", None), want) > 100 * dct_gates("f32", n)[0]


def test_helpers_index_every_point_once(helpers):
    """the II-post writes and the III-pre reads cover 0 .. N-1 exactly once; for even N bin N/2 is written once"""
    for n in range(1, 200):
        hh, e = n // 2, (n + 1) // 2
        for dst in (0, 1):
            re_i, im_i = _u64(hh + 1), _u64(hh + 1)
            helpers.ii_index(C.c_int(dst), C.c_ulonglong(n), _ptr(re_i), _ptr(im_i))
            idx = np.concatenate([re_i, im_i[1:e]]).astype(np.int64)
            assert sorted(idx) == list(range(n)), (n, dst)
            src, sign = _u64(n), np.zeros(n)
            helpers.perm(C.c_ulonglong(n), C.c_int(dst), _ptr(src), _ptr(sign))
            assert sorted(src.astype(np.int64)) == list(range(n))


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
    for const in ("PHAST_NORM_BACKWARD 0", "PHAST_NORM_ORTHO 1", "PHAST_NORM_FORWARD 2"):
        assert "#define " + const in header
    import phastft_amd as P

    for name in ("PlannerDct64", "PlannerDct32", "dct_f64", "dct_f32", "dst_f64", "dst_f32", "dct_f64_with_planner",
                 "dct_f32_with_planner", "dst_f64_with_planner", "dst_f32_with_planner", "dct_batched", "dst_batched",
                 "idct", "idst"):
        assert name in P.__all__ and callable(getattr(P, name)), name
    assert "PlannerDct64/32" in P.__doc__


def test_argument_codes(lib):
    """type, norm, null pointers, N out of range and unequal host lengths come back before the device is touched"""
    for sfx, fs, dt in (("64", "f64", np.float64), ("32", "f32", np.float32)):
        new = getattr(lib, f"phast_planner_dct{sfx}_new")
        h = C.c_void_p(1)
        assert new(C.c_size_t(0), C.byref(h)) == INVALID_ARG and not h.value
        assert new(C.c_size_t((1 << 29) + 1), C.byref(h)) == INVALID_ARG
        assert new(C.c_size_t(1000), None) == INVALID_ARG
        assert getattr(lib, f"phast_planner_dct{sfx}_workspace_len")(None, C.c_size_t(4)) == 0
        assert getattr(lib, f"phast_planner_dct{sfx}_device_bytes")(None) == 0
        assert getattr(lib, f"phast_planner_dct{sfx}_describe")(None, C.create_string_buffer(8), C.c_size_t(8)) == INVALID_ARG
        ms = (C.c_float * 3)()
        assert getattr(lib, f"phast_planner_dct{sfx}_time_stages")(None, 0, 2, 0, None, None, C.c_size_t(1), None, C.c_size_t(0),
                                                                   1, ms, None) == INVALID_ARG
        x, y, z = np.zeros(10, dt), np.zeros(10, dt), np.zeros(9, dt)
        p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        for kind in ("dct", "dst"):
            host = getattr(lib, f"phast_{kind}_{fs}")
            assert host(p(x), C.c_size_t(10), p(y), C.c_size_t(10), 4, 0) == INVALID_ARG   # type I / IV reserved
            assert host(p(x), C.c_size_t(10), p(y), C.c_size_t(10), 1, 0) == INVALID_ARG
            assert host(p(x), C.c_size_t(10), p(y), C.c_size_t(10), 2, 3) == INVALID_ARG   # norm out of range
            assert host(p(x), C.c_size_t(10), p(y), C.c_size_t(10), 3, -1) == INVALID_ARG
            assert host(None, C.c_size_t(10), p(y), C.c_size_t(10), 2, 0) == INVALID_ARG
            assert host(p(x), C.c_size_t(10), None, C.c_size_t(10), 2, 0) == INVALID_ARG
            assert host(p(x), C.c_size_t(0), p(y), C.c_size_t(0), 2, 0) == INVALID_ARG     # N = 0
            assert host(p(x), C.c_size_t((1 << 29) + 1), p(y), C.c_size_t((1 << 29) + 1), 2, 0) == INVALID_ARG
            assert host(p(x), C.c_size_t(10), p(z), C.c_size_t(9), 2, 0) == LEN_MISMATCH
            assert getattr(lib, f"phast_{kind}_{fs}_with_planner")(p(x), C.c_size_t(10), p(y), C.c_size_t(10), 2, 0,
                                                                   None) == INVALID_ARG
            assert getattr(lib, f"phast_{kind}_{fs}_dev")(p(x), p(y), C.c_size_t(10), C.c_size_t(1), C.c_size_t(10),
                                                          C.c_size_t(10), 2, 0, None, None, C.c_size_t(0), None) == INVALID_ARG


def test_calls_without_a_gpu_fail_loudly(lib):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present: tests/test_gpu_dct.py covers the device side")
    x, y = np.ones(10), np.zeros(10)
    assert lib.phast_dct_f64(x.ctypes.data_as(C.c_void_p), C.c_size_t(10), y.ctypes.data_as(C.c_void_p), C.c_size_t(10),
                             2, 0) == NO_DEVICE
    h = C.c_void_p()
    assert lib.phast_planner_dct64_new(C.c_size_t(1000), C.byref(h)) == NO_DEVICE and not h.value


def test_python_argument_errors():
    import phastft_amd as P

    x, y = np.ones(10), np.zeros(10)
    with pytest.raises(ValueError):
        P.dct_f64(x, y, norm="orthonormal")
    with pytest.raises(ValueError):
        P.idct(x, y, type=4)
    with pytest.raises(ValueError):
        P.idst(x, y, norm="both")
    with pytest.raises(P.PhastPanic):
        P.dst_f64(x, np.zeros(9))      # LEN_MISMATCH before the device is touched
    with pytest.raises(P.PhastPanic):
        P.dct_f32(x.astype(np.float32), y.astype(np.float32), type=1)


def test_idct_idst_mapping():
    """scipy's idct / idst of type t and norm n is its dct / dst of type 5 - t with norm backward <-> forward; _inverse
    gives exactly that, and the mapping holds in scipy itself"""
    import phastft_amd as P

    x = np.random.default_rng(3).uniform(-1, 1, 37).astype(np.longdouble)
    for t in (2, 3):
        for norm in NORMS + ["backward"]:
            t2, n2 = P._inverse(t, norm)
            assert t2 == 5 - t and n2 == {None: "forward", "backward": "forward", "ortho": "ortho", "forward": "backward"}[norm]
            for fwd, inv in ((sf.dct, sf.idct), (sf.dst, sf.idst)):
                assert np.allclose(inv(x, type=t, norm=norm), fwd(x, type=t2, norm=n2), rtol=0, atol=1e-15)


def test_cpp_mirror_without_gpu(tmp_path):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present: tests/test_gpu_dct.py runs the mirror there")
    from phastft_amd import build

    lib = build.build()
    exe = str(tmp_path / "dct_test")
    libdir = os.path.dirname(lib)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "dct_test.cpp"), "-o", exe, "-L", libdir, "-lphastft_hip",
                        f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "dct: ok" in r.stdout, r.stdout + r.stderr


def test_rust_mirror():
    """Parsed textually, as tests/test_rust_shim.py does (no Rust toolchain here)"""
    src = os.path.join(ROOT, "rust", "phastft-hip", "src")
    ffi = open(os.path.join(src, "ffi.rs")).read()
    used = [f"phast_planner_dct{s}_{w}" for s in ("64", "32") for w in ("new", "free", "workspace_len")]
    used += [f"phast_{k}_{fs}{suffix}" for k in ("dct", "dst") for fs in ("f64", "f32") for suffix in ("_with_planner", "_dev")]
    for name in used:
        assert re.search(r"fn " + name + r"\s*\(", ffi), name
    planner = open(os.path.join(src, "planner.rs")).read()
    assert "PlannerDct64" in planner and "PlannerDct32" in planner
    r2r = open(os.path.join(src, "algorithms", "r2r.rs")).read()
    for f in ("dct_f64", "dct_f32", "dst_f64", "dst_f32", "dct_f64_with_planner", "dst_f32_with_planner", "idct_f64", "idst_f32"):
        assert re.search(r"impl_r2r!\([^;]*\b" + f + r"\b", r2r), f  # the functions are stamped out by impl_r2r!
    lib = open(os.path.join(src, "lib.rs")).read()
    assert "PlannerDct64" in lib and "r2r" in lib
