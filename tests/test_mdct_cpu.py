"""The MDCT and its inverse (csrc/mdct.hpp, csrc/dct4.hpp, csrc/planner_mdct.hpp) without a GPU: the headers' index, twiddle
and window helpers compiled with g++ and the four sweeps restated on them in numpy around a long-double FFT, against the two
references of tests/mdct_reference.py; every coefficient and every output sample written exactly once; the windows' TDAC
defect; the round trip; gates that wrong twiddles miss; the new C ABI exported and listed, with its argument codes returned
before the device is touched; the Python names."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.fft as sf

from tests import mdct_reference as ref
from tests import tolerances as tol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
NEW = [f"phast_planner_mdct{s}_{w}" for s in ("64", "32")
       for w in ("new", "free", "describe", "device_bytes", "frames", "workspace_len", "workspace_min", "tdac_defect",
                 "time_stages")]
NEW += [f"phast_{k}_{fs}_{suffix}" for k in ("mdct", "imdct") for fs in ("f64", "f32") for suffix in ("with_planner", "dev")]
OK, LEN_MISMATCH, PLANNER_SIZE, NO_DEVICE, INVALID_ARG = 0, 2, 3, 15, 16
WINDOWS = ("sine", "vorbis", "kbd")

HELPERS = r"""
#include "mdct.hpp"
using u64 = unsigned long long;
extern "C" {
u64 frames(u64 len, u64 n, int padded) { return phast::mdct_frames(len, n, padded); }
int bad_args(u64 len, u64 n, int padded) { return phast::mdct_bad_args(len, n, padded); }
double defect(const double *w, u64 n) { return phast::mdct_tdac_defect(w, n); }
void fold(u64 n, u64 *a, u64 *b, int *sign) {
    for (u64 i = 0; i < n; ++i) { a[i] = phast::mdct_fold_a(i, n / 2); b[i] = phast::mdct_fold_b(i, n / 2, &sign[i]); }
}
void unfold(u64 n, u64 *src, int *sign) { for (u64 i = 0; i < 2 * n; ++i) src[i] = phast::mdct_unfold(i, n / 2, &sign[i]); }
void dct4_index(u64 n, u64 *re_src, u64 *im_src, u64 *re_dst, u64 *im_dst) {
    for (u64 m = 0; m < n / 2; ++m) {
        re_src[m] = phast::dct4_re_src(m); im_src[m] = phast::dct4_im_src(m, n);
        re_dst[m] = phast::dct4_re_dst(m); im_dst[m] = phast::dct4_im_dst(m, n);
    }
}
void dct4_tables(u64 n, long double *pre_c, long double *pre_s, long double *post_c, long double *post_s) {
    for (u64 m = 0; m < n / 2; ++m) {
        phast::dct4_twiddle(phast::dct4_pre_num(m), 4 * n, &pre_c[m], &pre_s[m]);
        phast::dct4_twiddle(phast::dct4_post_num(m), 4 * n, &post_c[m], &post_s[m]);
    }
}
}
"""


@pytest.fixture(scope="module")
def helpers(tmp_path_factory):
    d = tmp_path_factory.mktemp("mdct_helpers")
    src, so = d / "helpers.cpp", d / "libmdcthelpers.so"
    src.write_text(HELPERS)
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-shared", "-fPIC", "-I",
                        os.path.join(ROOT, "phastft_amd", "csrc"), str(src), "-o", str(so)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lib = C.CDLL(str(so))
    lib.frames.restype = C.c_ulonglong
    lib.defect.restype = C.c_double
    return lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _u64(n):
    return np.zeros(n, np.uint64)


class Schedule:
    """the four sweeps of planner_mdct.hpp restated in numpy on the headers' helpers, around a long-double FFT of h points.
    `pre` / `post` replace a twiddle table (the gate-sensitivity test).  `writes` counts what the last call stored where."""

    def __init__(self, hl, n, pre=None, post=None):
        self.hl, self.n, self.h = hl, n, n // 2
        n64, h = C.c_ulonglong(n), self.h
        a, b, sg = _u64(n), _u64(n), np.zeros(n, np.int32)
        hl.fold(n64, _ptr(a), _ptr(b), _ptr(sg))
        self.fold_a, self.fold_b, self.fold_sign = a.astype(np.int64), b.astype(np.int64), sg.astype(LD)
        us, usg = _u64(2 * n), np.zeros(2 * n, np.int32)
        hl.unfold(n64, _ptr(us), _ptr(usg))
        self.unfold_src, self.unfold_sign = us.astype(np.int64), usg.astype(LD)
        idx = [_u64(h) for _ in range(4)]
        hl.dct4_index(n64, *(_ptr(i) for i in idx))
        self.re_src, self.im_src, self.re_dst, self.im_dst = (i.astype(np.int64) for i in idx)
        tabs = [np.zeros(h, LD) for _ in range(4)]
        hl.dct4_tables(n64, *(_ptr(t) for t in tabs))
        self.pre = tabs[0] - 1j * tabs[1] if pre is None else pre(np.arange(h), n)
        self.post = tabs[2] - 1j * tabs[3] if post is None else post(np.arange(h), n)

    def dct4(self, u, scale=LD(1)):
        z = (u[self.re_src] + 1j * u[self.im_src]) * self.pre        # pre
        c = (sf.fft(z) if self.h > 1 else z) * self.post * scale      # the complex planner's transform, then post
        out = np.full(self.n, np.nan, LD)
        self.writes = np.zeros(self.n, np.int64)
        np.add.at(self.writes, self.re_dst, 1)
        np.add.at(self.writes, self.im_dst, 1)
        out[self.re_dst] = c.real
        out[self.im_dst] = -c.imag
        return out

    def forward(self, x, w, padded):
        n, length = self.n, x.size
        f = int(self.hl.frames(C.c_ulonglong(length), C.c_ulonglong(n), C.c_int(padded)))
        x, w = x.astype(LD), np.asarray(w, LD)
        out = np.zeros((f, n), LD)
        for t in range(f):
            s = (t - padded) * n + np.arange(2 * n)
            inside = (s >= 0) & (s < length)
            xw = np.where(inside, w * x[np.clip(s, 0, length - 1)], 0)
            u = -xw[self.fold_a] + self.fold_sign * xw[self.fold_b]    # the fold
            out[t] = self.dct4(u)
            assert (self.writes == 1).all(), (n, t)                     # every coefficient once
        return out

    def inverse(self, X, length, w, padded):
        n, f = self.n, X.shape[0]
        w = np.asarray(w, LD)
        v = np.stack([self.dct4(X[t].astype(LD), LD(2) / n) for t in range(f)]) if f else np.zeros((0, n), LD)
        s = np.arange(length)
        q, r = s // n, s % n
        out, wrote = np.zeros(length, LD), np.zeros(length, np.int64)
        for half in (1, 0):                                             # frame q - 1 + padded (second half) first
            t, j = q - half + padded, r + half * n
            ok = (t >= 0) & (t < f)
            y = w[j[ok]] * self.unfold_sign[j[ok]] * v[t[ok], self.unfold_src[j[ok]]]
            out[ok] += y
        wrote += 1                                                      # one store per sample, zeros included
        self.sample_writes = wrote
        return out


def _cases(n):
    return [(ln, p) for ln in (1, n - 1, n, n + 1, 3 * n + 5) for p in (1, 0) if ln >= 1 and (p or ln >= 2 * n)]


def test_schedule_matches_the_definition_for_every_even_n_up_to_64(helpers):
    worst = 0.0
    for n in range(2, 65, 2):
        sch = Schedule(helpers, n)
        for ln, padded in _cases(n):
            rng = np.random.default_rng([n, ln, padded])
            x, w = rng.uniform(-1, 1, ln), rng.uniform(-1, 1, 2 * n)
            x.flags.writeable = False
            X = sch.forward(x, w, padded)
            assert X.shape[0] == ref.frames_of(ln, n, bool(padded))
            e = ref.errors(X, ref.mdct_direct(x, n, w, bool(padded)))[0]
            assert e < 1e-14, ("forward", n, ln, padded, e)
            worst = max(worst, e)
            back = sch.inverse(X, ln, w, padded)
            assert (sch.sample_writes == 1).all()
            e = ref.errors(back, ref.imdct_direct(X, ln, n, w, bool(padded)))[0]
            assert e < 1e-14, ("inverse", n, ln, padded, e)
    assert worst > 0


@pytest.mark.parametrize("n", [2, 4, 6, 30, 960, 1024, 2050])
def test_schedule_matches_the_fast_reference(helpers, n):
    sch = Schedule(helpers, n)
    for ln, padded in _cases(n):
        rng = np.random.default_rng([n, ln, padded, 1])
        x, w = rng.uniform(-1, 1, ln), rng.uniform(-1, 1, 2 * n)
        X = sch.forward(x, w, padded)
        want = ref.mdct_fast(x, n, w, bool(padded))
        assert X.shape == want.shape
        assert ref.errors(X, want)[0] < 1e-14, ("forward", n, ln, padded)
        back = sch.inverse(X, ln, w, padded)
        assert ref.errors(back, ref.imdct_fast(X, ln, n, w, bool(padded)))[0] < 1e-14, ("inverse", n, ln, padded)


def test_the_two_references_agree():
    for n in (2, 6, 16, 30):
        for ln, padded in _cases(n):
            rng = np.random.default_rng([n, ln, padded, 2])
            x, w = rng.uniform(-1, 1, ln), rng.uniform(-1, 1, 2 * n)
            a, b = ref.mdct_direct(x, n, w, bool(padded)), ref.mdct_fast(x, n, w, bool(padded))
            assert ref.errors(a, b)[0] < 1e-15
            assert ref.errors(ref.imdct_direct(a, ln, n, w, bool(padded)), ref.imdct_fast(a, ln, n, w, bool(padded)))[0] < 1e-15


def test_helpers_index_every_point_once(helpers):
    for n in range(2, 130, 2):
        sch = Schedule(helpers, n)
        assert sorted(np.concatenate([sch.re_src, sch.im_src])) == list(range(n))
        assert sorted(np.concatenate([sch.re_dst, sch.im_dst])) == list(range(n))
        assert sorted(np.concatenate([sch.fold_a, sch.fold_b])) == list(range(2 * n))  # every windowed sample is folded once
        assert np.bincount(sch.unfold_src, minlength=n).tolist() == [2] * n


def test_tdac_defect(helpers):
    import phastft_amd as P

    for n in (2, 6, 30, 960, 1024):
        for name in WINDOWS:
            w = np.ascontiguousarray(P.mdct_window(name, n, np.float64))
            assert np.abs(w - ref.window(name, n).astype(np.float64)).max() < 2e-16, (name, n)
            d = helpers.defect(_ptr(w), C.c_ulonglong(n))
            assert d < 1e-15 and d == ref.tdac_defect(w, n), (name, n, d)
        assert abs(helpers.defect(_ptr(np.ones(2 * n)), C.c_ulonglong(n)) - 1.0) < 1e-15  # 1 + 1 - 1
        for height in (0.5, np.sqrt(0.75)):                                                # rectangular, 2 height^2 - 1 = -+0.5
            assert abs(helpers.defect(_ptr(np.full(2 * n, height)), C.c_ulonglong(n)) - 0.5) < 1e-15


@pytest.mark.parametrize("name", WINDOWS)
def test_round_trip(helpers, name):
    for n in (2, 6, 30, 960):
        sch = Schedule(helpers, n)
        w = ref.window(name, n)
        for ln, padded in _cases(n):
            x = np.random.default_rng([n, ln, 3]).uniform(-1, 1, ln)
            back = sch.inverse(sch.forward(x, w, padded), ln, w, padded).astype(np.float64)
            lo, hi = (0, ln) if padded else (n, ref.frames_of(ln, n, False) * n)
            assert np.abs(back[lo:hi] - x[lo:hi]).max() <= tol.ROUNDTRIP_ABS["f64"], (name, n, ln, padded)


def test_gates_catch_wrong_twiddles(helpers):
    """mdct_gates on the restated schedule: e^{-i pi 4m / (4N)} in place of (4m + 1), and a post-twiddle evaluated in f32
    under the f64 gate, each miss by 100 x"""
    n = 1000
    x, w = np.random.default_rng(7).uniform(-1, 1, 3 * n + 5), np.random.default_rng(8).uniform(-1, 1, 2 * n)
    want = ref.mdct_fast(x, n, w)
    g64, g32 = ref.mdct_gates("f64", n)[0], ref.mdct_gates("f32", n)[0]
    assert ref.errors(Schedule(helpers, n).forward(x, w, 1), want)[0] < g64 / 100
    shifted = lambda m, nn: np.exp(-1j * ref.PI * (4 * m).astype(LD) / (4 * nn))  # noqa: E731
    assert ref.errors(Schedule(helpers, n, pre=shifted).forward(x, w, 1), want)[0] > 100 * g32
    f32 = lambda k, nn: np.exp(-1j * np.float32(np.pi) * k.astype(np.float32) / np.float32(nn)).astype(np.complex64).astype(np.clongdouble)  # noqa: E731
    assert ref.errors(Schedule(helpers, n, post=f32).forward(x, w, 1), want)[0] > 100 * g64


def test_frames_and_argument_rules(helpers):
    u = C.c_ulonglong
    for n in (2, 6, 30):
        for ln in range(1, 5 * n):
            assert helpers.frames(u(ln), u(n), 1) == ref.frames_of(ln, n, True)
            assert helpers.bad_args(u(ln), u(n), 1) == 0
            assert helpers.bad_args(u(ln), u(n), 0) == (ln < 2 * n)
            if ln >= 2 * n:
                assert helpers.frames(u(ln), u(n), 0) == ref.frames_of(ln, n, False)
    for bad in ((10, 3, 1), (10, 0, 1), (10, (1 << 29) + 2, 1), (0, 4, 1), ((1 << 29) + 1, 4, 1), (10, 4, 2), (10, 4, -1)):
        assert helpers.bad_args(u(bad[0]), u(bad[1]), C.c_int(bad[2])) == 1, bad
    assert helpers.bad_args(u(1 << 29), u(1 << 29), 1) == 0


@pytest.fixture(scope="module")
def lib():
    from phastft_amd import _lib

    return _lib.lib()


def test_new_symbols_are_exported_and_listed(lib):
    from phastft_amd import _lib

    header = open(os.path.join(ROOT, "include", "phastft_hip.h")).read()
    assert len(NEW) == 26
    for name in NEW:
        getattr(lib, name)
        assert name in _lib.SYMBOLS and re.search(r"\b" + name + r"\s*\(", header), name
    import phastft_amd as P

    for name in ("PlannerMdct64", "PlannerMdct32", "mdct_batched", "imdct_batched", "mdct_f64_with_planner",
                 "mdct_f32_with_planner", "imdct_f64_with_planner", "imdct_f32_with_planner", "mdct", "imdct", "mdct_window"):
        assert name in P.__all__ and callable(getattr(P, name)), name
    assert "PlannerMdct64/32" in P.__doc__
    from phastft_amd import build

    assert "mdct" in build.UNITS


def test_argument_codes(lib):
    """odd N, N = 0, N and L out of range, padded = 0 with L < 2N, null pointers and a null planner come back before the
    device is touched"""
    sz = C.c_size_t
    for sfx, fs, dt in (("64", "f64", np.float64), ("32", "f32", np.float32)):
        new = getattr(lib, f"phast_planner_mdct{sfx}_new")
        h = C.c_void_p(1)
        assert new(sz(100), sz(7), None, 1, C.byref(h)) == INVALID_ARG and not h.value   # odd N
        for ln, n, padded in ((100, 0, 1), (100, (1 << 29) + 2, 1), (0, 8, 1), ((1 << 29) + 1, 8, 1), (15, 8, 0), (100, 8, 2)):
            h = C.c_void_p(1)
            assert new(sz(ln), sz(n), None, padded, C.byref(h)) == INVALID_ARG and not h.value, (ln, n, padded)
        assert new(sz(100), sz(8), None, 1, None) == INVALID_ARG
        for q in ("workspace_len", "workspace_min"):
            assert getattr(lib, f"phast_planner_mdct{sfx}_{q}")(None, 1) == 0
        assert getattr(lib, f"phast_planner_mdct{sfx}_frames")(None) == 0
        assert getattr(lib, f"phast_planner_mdct{sfx}_device_bytes")(None) == 0
        assert getattr(lib, f"phast_planner_mdct{sfx}_tdac_defect")(None) == 0.0
        assert getattr(lib, f"phast_planner_mdct{sfx}_describe")(None, C.create_string_buffer(8), sz(8)) == INVALID_ARG
        ms = (C.c_float * 3)()
        assert getattr(lib, f"phast_planner_mdct{sfx}_time_stages")(None, 0, None, None, sz(1), None, sz(0), 1, ms,
                                                                    None) == INVALID_ARG
        x, y = np.zeros(100, dt), np.zeros(112, dt)
        for name, a, b in (("mdct", x, y), ("imdct", y, x)):
            assert getattr(lib, f"phast_{name}_{fs}_with_planner")(_ptr(a), sz(a.size), _ptr(b), sz(b.size), None) == INVALID_ARG
            assert getattr(lib, f"phast_{name}_{fs}_dev")(_ptr(a), _ptr(b), sz(100), sz(1), sz(100), None, None, sz(0),
                                                          None) == INVALID_ARG


def test_calls_without_a_gpu_fail_loudly(lib):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present: tests/test_gpu_mdct.py covers the device side")
    h = C.c_void_p()
    assert lib.phast_planner_mdct64_new(C.c_size_t(100), C.c_size_t(8), None, 1, C.byref(h)) == NO_DEVICE and not h.value
    import phastft_amd as P

    with pytest.raises(P.PhastHipError):
        P.PlannerMdct32(100, 8)


def test_python_argument_errors():
    import phastft_amd as P

    with pytest.raises(P.PhastPanic):
        P.PlannerMdct64(100, 7)                      # odd N: INVALID_ARG before the device is touched
    with pytest.raises(P.PhastPanic):
        P.PlannerMdct64(15, 8, padded=False)
    with pytest.raises(ValueError):
        P.PlannerMdct64(100, 8, window=np.ones(8))  # a window of N values, not 2N
    with pytest.raises(ValueError):
        P.mdct_window("hann", 8)
    assert P.mdct_window("kbd", 8, np.float32).dtype == np.float32 and P.mdct_window("sine", 8).size == 16


def test_rust_mirror():
    """Parsed textually, as tests/test_rust_shim.py does (no Rust toolchain here)"""
    src = os.path.join(ROOT, "rust", "phastft-hip", "src")
    ffi = open(os.path.join(src, "ffi.rs")).read()
    for name in NEW:
        assert re.search(r"fn " + name + r"\s*\(", ffi), name
    planner = open(os.path.join(src, "planner.rs")).read()
    assert "PlannerMdct64" in planner and "PlannerMdct32" in planner and "pub fn tdac_defect" in planner
    mdct = open(os.path.join(src, "algorithms", "mdct.rs")).read()
    for f in ("mdct_f64_with_planner", "imdct_f64_with_planner", "mdct_f32_dev", "imdct_f32_dev"):
        assert re.search(r"impl_mdct!\([^;]*\b" + f + r"\b", mdct), f  # the functions are stamped out by impl_mdct!
    assert "pub mod mdct;" in open(os.path.join(src, "algorithms", "mod.rs")).read()
    lib = open(os.path.join(src, "lib.rs")).read()
    assert "PlannerMdct64" in lib and "algorithms::mdct" in lib
