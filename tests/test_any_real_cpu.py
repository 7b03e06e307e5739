"""Arbitrary-length real transforms (csrc/any_real.hpp, csrc/planner_any_real.hpp) without a GPU: the new C ABI is exported
and listed, argument errors come back as their codes before the device is touched (NO_DEVICE for calls that need one), Python
raises PhastPanic with the reference texts, the C++ and Rust mirrors carry the new names, and the gates of
tests/test_gpu_any_real.py catch a naive chirp phase."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import tolerances as tol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = [f"phast_planner_r2c_any{s}_{w}" for s in ("64", "32")
       for w in ("new", "free", "describe", "device_bytes", "workspace_len", "time_stages", "time_c2r_stages")]
NEW += [f"phast_{k}_fft_{fs}_any{suffix}" for k in ("r2c", "c2r") for fs in ("f64", "f32") for suffix in ("", "_with_planner", "_dev")]
OK, PLANNER_SIZE, NO_DEVICE, INVALID_ARG = 0, 3, 15, 16
R2C_INPUT_LEN, R2C_OUT_RE_LEN, R2C_OUT_IM_LEN, C2R_OUTPUT_LEN, C2R_IN_RE_LEN, C2R_IN_IM_LEN = 5, 6, 7, 8, 9, 10
TEXTS = {6: "output_re must have length N/2 + 1", 7: "output_im must have length N/2 + 1",
         9: "input_re must have length N/2 + 1", 10: "input_im must have length N/2 + 1", 16: "invalid argument"}


@pytest.fixture(scope="module")
def lib():
    from phastft_amd import _lib

    return _lib.lib()


def _no_gpu():
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present: tests/test_gpu_any_real.py covers the device side")


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_new_symbols_are_exported_and_listed(lib):
    from phastft_amd import _lib

    header = open(os.path.join(ROOT, "include", "phastft_hip.h")).read()
    assert len(NEW) == 26
    for name in NEW:
        getattr(lib, name)
        assert name in _lib.SYMBOLS and re.search(r"\b" + name + r"\s*\(", header), name
    import phastft_amd as P

    for name in ("PlannerR2cAny64", "PlannerR2cAny32", "r2c_fft_f64_any", "r2c_fft_f32_any", "r2c_fft_f64_any_with_planner",
                 "r2c_fft_f32_any_with_planner", "c2r_fft_f64_any", "c2r_fft_f32_any", "c2r_fft_f64_any_with_planner",
                 "c2r_fft_f32_any_with_planner", "r2c_any_batched", "c2r_any_batched"):
        assert name in P.__all__ and callable(getattr(P, name)), name
    for row in ("PlannerR2cAny64/32", "r2c_fft_f64/f32_any[_with_planner]", "c2r_fft_f64/f32_any[_with_planner]",
                "r2c_any_batched", "c2r_any_batched"):
        assert row in P.__doc__, row


def test_planner_argument_codes(lib):
    for sfx in ("64", "32"):
        new = getattr(lib, f"phast_planner_r2c_any{sfx}_new")
        h = C.c_void_p(1)
        assert new(C.c_size_t(0), C.byref(h)) == INVALID_ARG and not h.value          # N = 0
        assert new(C.c_size_t((1 << 29) + 1), C.byref(h)) == INVALID_ARG              # above the limit
        assert new(C.c_size_t(1 << 30), C.byref(h)) == INVALID_ARG
        assert new(C.c_size_t(1000), None) == INVALID_ARG                              # null out
        assert getattr(lib, f"phast_planner_r2c_any{sfx}_workspace_len")(None, C.c_size_t(4)) == 0
        assert getattr(lib, f"phast_planner_r2c_any{sfx}_device_bytes")(None) == 0
        assert getattr(lib, f"phast_planner_r2c_any{sfx}_describe")(None, C.create_string_buffer(8), C.c_size_t(8)) == INVALID_ARG
        ms = (C.c_float * 5)()
        assert getattr(lib, f"phast_planner_r2c_any{sfx}_time_stages")(None, None, None, None, C.c_size_t(1), None,
                                                                       C.c_size_t(0), 1, ms, None) == INVALID_ARG


def test_call_argument_codes(lib):
    """every length mismatch, null pointers and N out of range, before the device is touched (no GPU needed for any of them)"""
    for fs, dt in (("f64", np.float64), ("f32", np.float32)):
        r2c = getattr(lib, f"phast_r2c_fft_{fs}_any")
        c2r = getattr(lib, f"phast_c2r_fft_{fs}_any")
        x, a, b, short = np.zeros(1001, dt), np.zeros(501, dt), np.zeros(501, dt), np.zeros(500, dt)
        z = C.c_size_t
        assert r2c(None, z(1001), _p(a), z(501), _p(b), z(501)) == INVALID_ARG
        assert r2c(_p(x), z(1001), None, z(501), _p(b), z(501)) == INVALID_ARG
        assert r2c(_p(x), z(0), _p(a), z(1), _p(b), z(1)) == INVALID_ARG               # N = 0
        assert r2c(_p(x), z((1 << 29) + 2), _p(a), z((1 << 28) + 2), _p(b), z((1 << 28) + 2)) == INVALID_ARG
        assert r2c(_p(x), z(1001), _p(short), z(500), _p(b), z(501)) == R2C_OUT_RE_LEN
        assert r2c(_p(x), z(1001), _p(a), z(501), _p(short), z(500)) == R2C_OUT_IM_LEN
        assert r2c(_p(x), z(1000), _p(a), z(501), _p(b), z(502)) == R2C_OUT_IM_LEN     # floor(N/2) + 1 = 501
        assert c2r(_p(a), z(501), _p(b), z(501), None, z(1001)) == INVALID_ARG
        assert c2r(_p(a), z(1), _p(b), z(1), _p(x), z(0)) == INVALID_ARG
        assert c2r(_p(short), z(500), _p(b), z(501), _p(x), z(1001)) == C2R_IN_RE_LEN
        assert c2r(_p(a), z(501), _p(short), z(500), _p(x), z(1001)) == C2R_IN_IM_LEN
        assert c2r(_p(a), z(501), _p(b), z(501), _p(x), z(1003)) == C2R_IN_RE_LEN
        # no planner
        withp = getattr(lib, f"phast_r2c_fft_{fs}_any_with_planner")
        assert withp(_p(x), z(1001), _p(a), z(501), _p(b), z(501), None) == INVALID_ARG
        withp = getattr(lib, f"phast_c2r_fft_{fs}_any_with_planner")
        assert withp(_p(a), z(501), _p(b), z(501), _p(x), z(1001), None) == INVALID_ARG
        for kind in ("r2c", "c2r"):
            dev = getattr(lib, f"phast_{kind}_fft_{fs}_any_dev")
            assert dev(_p(x), _p(a), _p(b), z(1001), z(1), z(1001), z(501), None, _p(x), z(4096), None) == INVALID_ARG
        assert np.all(x == 0) and np.all(a == 0) and np.all(b == 0)


def test_python_raises_the_reference_texts(lib):
    """the Python layer: PhastPanic with the library's messages, raised before any device work"""
    import phastft_amd as P

    for r2c, c2r, dt in ((P.r2c_fft_f64_any, P.c2r_fft_f64_any, np.float64), (P.r2c_fft_f32_any, P.c2r_fft_f32_any, np.float32)):
        for call, code in ((lambda: r2c(np.zeros(7, dt), np.zeros(3, dt), np.zeros(4, dt)), R2C_OUT_RE_LEN),
                           (lambda: r2c(np.zeros(8, dt), np.zeros(5, dt), np.zeros(4, dt)), R2C_OUT_IM_LEN),
                           (lambda: c2r(np.zeros(3, dt), np.zeros(4, dt), np.zeros(7, dt)), C2R_IN_RE_LEN),
                           (lambda: c2r(np.zeros(4, dt), np.zeros(5, dt), np.zeros(7, dt)), C2R_IN_IM_LEN),
                           (lambda: r2c(np.zeros(0, dt), np.zeros(1, dt), np.zeros(1, dt)), INVALID_ARG)):
            with pytest.raises(P.PhastPanic) as ei:
                call()
            assert ei.value.code == code and str(ei.value) == TEXTS[code], (code, str(ei.value))
    with pytest.raises(P.PhastPanic) as ei:
        P.PlannerR2cAny32(0)
    assert ei.value.code == INVALID_ARG
    with pytest.raises(P.PhastPanic):
        P.PlannerR2cAny64((1 << 29) + 1)
    with pytest.raises(TypeError):
        P.r2c_fft_f64_any(np.zeros(8, np.float32), np.zeros(5), np.zeros(5))


def test_device_calls_fail_loudly_without_a_gpu(lib):
    _no_gpu()
    import phastft_amd as P

    for fs, sfx, dt in (("f64", "64", np.float64), ("f32", "32", np.float32)):
        for n in (1, 2, 1000, 1001, 1024):   # direct, even, odd, power of two
            h = C.c_void_p()
            assert getattr(lib, f"phast_planner_r2c_any{sfx}_new")(C.c_size_t(n), C.byref(h)) == NO_DEVICE and not h.value
        x = np.arange(1000, dtype=dt)
        a, b = np.zeros(501, dt), np.zeros(501, dt)
        assert getattr(lib, f"phast_r2c_fft_{fs}_any")(_p(x), C.c_size_t(1000), _p(a), C.c_size_t(501), _p(b),
                                                       C.c_size_t(501)) == NO_DEVICE
        assert getattr(lib, f"phast_c2r_fft_{fs}_any")(_p(a), C.c_size_t(501), _p(b), C.c_size_t(501), _p(x),
                                                       C.c_size_t(1000)) == NO_DEVICE
        assert np.array_equal(x, np.arange(1000, dtype=dt))
    with pytest.raises(P.PhastHipError):
        P.PlannerR2cAny64(1000)
    with pytest.raises(P.PhastHipError):
        P.r2c_fft_f64_any(np.zeros(1000), np.zeros(501), np.zeros(501))
    with pytest.raises(P.PhastHipError):
        P.c2r_fft_f32_any(np.zeros(4, np.float32), np.zeros(4, np.float32), np.zeros(7, np.float32))


def _naive_bluestein_rfft(x):
    """an odd-N R2C by Bluestein in float64 with the NAIVE chirp exp(-i pi k^2 / N), k^2 / N in double -- the error the exact
    phase (any_len.hpp: chirp_r) removes"""
    n = len(x)
    m = 1 << (2 * n - 2).bit_length()
    k = np.arange(n, dtype=np.float64)
    w = np.exp(-1j * np.pi * (k * k / n))
    b = np.zeros(m, complex)
    b[:n] = np.conj(w)
    b[m - n + 1:] = np.conj(w[1:][::-1])
    a = np.zeros(m, complex)
    a[:n] = x * w
    c = np.fft.ifft(np.fft.fft(a) * np.fft.fft(b))[:n]
    return (w * c)[: (n - 1) // 2 + 1]


def test_gates_catch_a_naive_chirp():
    """tests/test_gpu_any_real.py's f64 gates at N = 1_000_003 (M = 2^21: 2 * 8e-16 * 21 = 3.4e-14) against a Bluestein R2C
    whose only flaw is the naive chirp phase: it misses them by orders of magnitude"""
    from tests.test_gpu_any_real import real_gates

    n = 1_000_003
    x = np.random.default_rng(5).uniform(-1, 1, n)
    got = _naive_bluestein_rfft(x)
    ref = np.fft.rfft(x.astype(np.longdouble))
    r, i = np.asarray(ref.real, np.float64), np.asarray(ref.imag, np.float64)
    rel = tol.rel_l2(got.real, got.imag, r, i)
    g_rel, g_bin = real_gates("f64", n)
    assert g_rel == pytest.approx(2 * 8e-16 * 21)
    assert rel > 100 * g_rel, (rel, g_rel)


def test_rust_safe_wrappers():
    """Parsed textually, as tests/test_rust_shim.py does (no Rust toolchain here); the extern block itself is checked
    against the header by that test."""
    src = os.path.join(ROOT, "rust", "phastft-hip", "src")
    r2c_rs, planner = open(os.path.join(src, "algorithms", "r2c.rs")).read(), open(os.path.join(src, "planner.rs")).read()
    lib_rs = open(os.path.join(src, "lib.rs")).read()
    for t, pl, fs, sfx in (("f64", "PlannerR2cAny64", "f64", "64"), ("f32", "PlannerR2cAny32", "f32", "32")):
        assert re.search(rf"impl_r2c_any!\({t}, {pl}, r2c_fft_{fs}_any, r2c_fft_{fs}_any_with_planner, r2c_fft_{fs}_any_dev, "
                         rf"c2r_fft_{fs}_any,\s*c2r_fft_{fs}_any_with_planner, c2r_fft_{fs}_any_dev, phast_r2c_fft_{fs}_any_with_planner,"
                         rf"\s*phast_r2c_fft_{fs}_any_dev, phast_c2r_fft_{fs}_any_with_planner, phast_c2r_fft_{fs}_any_dev\);", r2c_rs), fs
        assert re.search(rf"impl_planner_r2c_any!\({pl}, phast_planner_r2c_any{sfx}_new, phast_planner_r2c_any{sfx}_free,"
                         rf"\s*phast_planner_r2c_any{sfx}_workspace_len\);", planner), sfx
        for name in (f"r2c_fft_{fs}_any", f"r2c_fft_{fs}_any_with_planner", f"r2c_fft_{fs}_any_dev", f"c2r_fft_{fs}_any",
                     f"c2r_fft_{fs}_any_with_planner", f"c2r_fft_{fs}_any_dev"):
            assert name in lib_rs, name
    assert re.search(r"pub fn \$r2c_p\(input: &\[\$t\], output_re: &mut \[\$t\], output_im: &mut \[\$t\], planner: &\$planner\)", r2c_rs)
    assert re.search(r"pub fn \$c2r_p\(input_re: &\[\$t\], input_im: &\[\$t\], output: &mut \[\$t\], planner: &\$planner\)", r2c_rs)
    assert re.search(r"pub unsafe fn \$r2c_dev\(d_input: \*const \$t, d_output_re: \*mut \$t, d_output_im: \*mut \$t, n: usize,", r2c_rs)
    assert "unsafe impl Send for $any {}" in planner and "unsafe impl Sync for $any {}" in planner
    assert "extension beyond PhastFT 0.3.0" in r2c_rs


def test_cpp_mirror_compiles_and_panics_without_a_device(tmp_path):
    _no_gpu()
    from phastft_amd import build

    lib = build.build()
    header = open(os.path.join(ROOT, "include", "phastft.hpp")).read()
    for name in ("class NAME", "PlannerR2cAny64", "PlannerR2cAny32", "r2c_fft_f64_any_with_planner", "c2r_fft_f32_any"):
        assert name in header, name
    exe = str(tmp_path / "any_real_test")
    libdir = os.path.dirname(lib)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "any_real_test.cpp"), "-o", exe, "-L", libdir, "-lphastft_hip",
                        f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "any_real: ok" in r.stdout, r.stdout + r.stderr
