"""Arbitrary-length transforms (Bluestein; csrc/any_len.hpp, csrc/planner_any.hpp) without a GPU: the new C ABI is exported and
listed, argument errors come back as their codes before the device is touched (NO_DEVICE for calls that need one, as the
power-of-two calls do), the exact chirp phase is exact, and the C++ and Rust mirrors carry the new names."""
import ctypes as C
import os
import random
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["phast_planner_any64_new", "phast_planner_any32_new", "phast_planner_any64_free", "phast_planner_any32_free",
       "phast_planner_any64_describe", "phast_planner_any32_describe", "phast_planner_any64_device_bytes",
       "phast_planner_any32_device_bytes", "phast_planner_any64_workspace_len", "phast_planner_any32_workspace_len",
       "phast_fft_64_any", "phast_fft_32_any", "phast_fft_64_any_with_planner", "phast_fft_32_any_with_planner",
       "phast_fft_64_any_dev", "phast_fft_32_any_dev"]
PI_LD = np.longdouble("3.14159265358979323846264338327950288")
OK, LEN_MISMATCH, PLANNER_SIZE, NO_DEVICE, INVALID_ARG = 0, 2, 3, 15, 16


@pytest.fixture(scope="module")
def lib():
    from phastft_amd import _lib

    return _lib.lib()


def _no_gpu():
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present: tests/test_gpu_any_len.py covers the device side")


def test_new_symbols_are_exported_and_listed(lib):
    from phastft_amd import _lib

    header = open(os.path.join(ROOT, "include", "phastft_hip.h")).read()
    for name in NEW:
        getattr(lib, name)
        assert name in _lib.SYMBOLS and re.search(r"\b" + name + r"\s*\(", header), name


def test_planner_argument_codes(lib):
    for sfx in ("64", "32"):
        new = getattr(lib, f"phast_planner_any{sfx}_new")
        h = C.c_void_p(1)
        assert new(C.c_size_t(0), C.byref(h)) == INVALID_ARG and not h.value          # N = 0
        assert new(C.c_size_t((1 << 29) + 1), C.byref(h)) == INVALID_ARG              # above the limit
        assert new(C.c_size_t(1 << 30), C.byref(h)) == INVALID_ARG
        assert new(C.c_size_t(1000), None) == INVALID_ARG                              # null out
        assert getattr(lib, f"phast_planner_any{sfx}_workspace_len")(None, C.c_size_t(4)) == 0
        assert getattr(lib, f"phast_planner_any{sfx}_device_bytes")(None) == 0
        assert getattr(lib, f"phast_planner_any{sfx}_describe")(None, C.create_string_buffer(8), C.c_size_t(8)) == INVALID_ARG


def test_call_argument_codes(lib):
    for sfx, dt in (("64", np.float64), ("32", np.float32)):
        re_, im_ = np.zeros(1000, dt), np.zeros(1000, dt)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        plain = getattr(lib, f"phast_fft_{sfx}_any")
        withp = getattr(lib, f"phast_fft_{sfx}_any_with_planner")
        dev = getattr(lib, f"phast_fft_{sfx}_any_dev")
        assert plain(None, C.c_size_t(1000), p(im_), C.c_size_t(1000), 1) == INVALID_ARG      # null pointer
        assert plain(p(re_), C.c_size_t(1000), p(im_), C.c_size_t(1000), 2) == INVALID_ARG   # bad direction
        assert plain(p(re_), C.c_size_t(1000), p(im_), C.c_size_t(999), 1) == LEN_MISMATCH
        assert plain(p(re_), C.c_size_t(0), p(im_), C.c_size_t(0), 1) == INVALID_ARG         # N = 0: the planner's code
        assert withp(p(re_), C.c_size_t(1000), p(im_), C.c_size_t(1000), 1, None) == INVALID_ARG  # no planner
        assert dev(p(re_), p(im_), C.c_size_t(1000), C.c_size_t(1), C.c_size_t(1000), 1, None, p(re_), C.c_size_t(4096),
                   None) == INVALID_ARG
        assert np.all(re_ == 0) and np.all(im_ == 0)


def test_device_calls_fail_loudly_without_a_gpu(lib):
    _no_gpu()
    import phastft_amd as P

    for sfx, dt in (("64", np.float64), ("32", np.float32)):
        h = C.c_void_p()
        assert getattr(lib, f"phast_planner_any{sfx}_new")(C.c_size_t(1000), C.byref(h)) == NO_DEVICE and not h.value
        assert getattr(lib, f"phast_planner_any{sfx}_new")(C.c_size_t(1024), C.byref(h)) == NO_DEVICE
        x = np.arange(1000, dtype=dt)
        y = np.zeros(1000, dt)
        assert getattr(lib, f"phast_fft_{sfx}_any")(x.ctypes.data_as(C.c_void_p), C.c_size_t(1000), y.ctypes.data_as(C.c_void_p),
                                                    C.c_size_t(1000), 1) == NO_DEVICE
        assert np.array_equal(x, np.arange(1000, dtype=dt))
    with pytest.raises(P.PhastHipError):
        P.PlannerAny64(1000)
    with pytest.raises(P.PhastHipError):
        P.fft_64_any(np.zeros(1000), np.zeros(1000), P.Direction.Forward)
    with pytest.raises(P.PhastPanic):
        P.PlannerAny32(0)
    with pytest.raises(P.PhastPanic) as ei:
        P.fft_32_any(np.zeros(10, np.float32), np.zeros(9, np.float32), P.Direction.Forward)
    assert ei.value.code == LEN_MISMATCH


PHASE_MAIN = r"""
#include <cstdio>
#include "any_len.hpp"
int main() {
    unsigned long long n, N;
    while (std::scanf("%llu %llu", &n, &N) == 2)
        std::printf("%llu %.17g %llu\n", phast::chirp_r(n, N), phast::chirp_turns(n, N), phast::any_conv_len(N));
    return 0;
}
"""


def test_exact_chirp_phase_on_the_host(tmp_path):
    """any_len.hpp's phase helper (the same code the sweeps run on the device) compiled with g++: r = n^2 mod 2N against
    Python integers on seeded samples up to n = 2^30 - 1, the angle (units of pi) against numpy long double, and the
    naive pi n^2 / N in double shown to be off by orders of magnitude more at N ~ 10^6."""
    src = tmp_path / "phase.cpp"
    src.write_text(PHASE_MAIN)
    exe = str(tmp_path / "phase")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "phastft_amd", "csrc"), str(src),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rng = random.Random(20261015)
    cases = [(0, 1), (1, 1), (5, 3), (999, 1000), *[(1_000_003 - j, 1_000_003) for j in range(1, 40)], ((1 << 30) - 1, 1 << 29), ((1 << 30) - 1, 1),
             ((1 << 30) - 1, 3), (1 << 29, (1 << 29) - 1)]
    for _ in range(3000):
        N = rng.choice([rng.randint(1, 300), rng.randint(1, 1 << 20), rng.randint(1, 1 << 29)])
        n = rng.choice([rng.randrange(N), rng.randrange(1 << 30)])
        cases.append((n, N))
    out = subprocess.run([exe], input="".join(f"{n} {N}\n" for n, N in cases), capture_output=True, text=True, check=True).stdout
    naive_worst = 0.0
    for (n, N), line in zip(cases, out.split("\n")):
        r_s, t_s, m_s = line.split()
        rr = n * n % (2 * N)
        assert int(r_s) == rr, (n, N)
        assert float(t_s) == float(Fraction(-rr, N)), (n, N, t_s)     # the exact angle / pi, correctly rounded
        want = -np.longdouble(rr) / np.longdouble(N)                   # ... and against long double arithmetic
        assert abs(np.longdouble(float(t_s)) - want) <= np.spacing(abs(float(want)) or 1.0), (n, N, t_s, want)
        m = int(m_s)
        assert m == (N if N & (N - 1) == 0 else 1 << (2 * N - 2).bit_length()) and (m == N or m >= 2 * N - 1)
        if N == 1_000_003:   # the naive phase pi n^2 / N in double against the true angle in long double
            naive = np.longdouble(np.pi * float(n) * float(n) / float(N))
            exact = np.longdouble(n * n) / np.longdouble(N) * PI_LD
            naive_worst = max(naive_worst, abs(float(naive - exact)))
    assert naive_worst > 1e-11   # the error the exact phase removes (~1e-10 at n ~ N ~ 10^6)


def test_rust_safe_wrappers():
    """Parsed textually, as tests/test_rust_shim.py does (no Rust toolchain here); the extern block itself is checked
    against the header by that test."""
    src = os.path.join(ROOT, "rust", "phastft-hip", "src")
    lib_rs, planner = open(os.path.join(src, "lib.rs")).read(), open(os.path.join(src, "planner.rs")).read()
    assert re.search(r"pub fn \$with_planner\(reals: &mut \[\$t\], imags: &mut \[\$t\], direction: Direction, planner: &\$planner\)", lib_rs)
    assert re.search(r"pub fn \$plain\(reals: &mut \[\$t\], imags: &mut \[\$t\], direction: Direction\)", lib_rs)
    assert re.search(r"pub unsafe fn \$dev\(d_reals: \*mut \$t, d_imags: \*mut \$t, n: usize, batch: usize, dist: usize, "
                     r"direction: Direction,\s*planner: &\$planner, d_work: \*mut \$t, work_len: usize, stream: \*mut c_void\)", lib_rs)
    for t, pl, sfx in (("f64", "PlannerAny64", "64"), ("f32", "PlannerAny32", "32")):
        assert re.search(rf"impl_fft_any!\({t}, {pl}, fft_{sfx}_any_with_planner, fft_{sfx}_any, phast_fft_{sfx}_any_with_planner, "
                         rf"fft_{sfx}_any_dev,\s*phast_fft_{sfx}_any_dev\);", lib_rs), sfx
        assert re.search(rf"impl_planner_any!\({pl}, phast_planner_any{sfx}_new, phast_planner_any{sfx}_free, "
                         rf"phast_planner_any{sfx}_workspace_len\);", planner), sfx
    assert "unsafe impl Send for $any {}" in planner and "unsafe impl Sync for $any {}" in planner
    assert "pub fn new(n: usize) -> Self" in planner and "pub fn workspace_len(&self, batch: usize) -> usize" in planner
    assert "extension beyond PhastFT 0.3.0" in lib_rs and "extension beyond PhastFT 0.3.0" in planner


def test_cpp_mirror_compiles_and_panics_without_a_device(tmp_path):
    _no_gpu()
    from phastft_amd import build

    lib = build.build()
    exe = str(tmp_path / "any_len_test")
    libdir = os.path.dirname(lib)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "any_len_test.cpp"), "-o", exe, "-L", libdir, "-lphastft_hip",
                        f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "any_len: ok" in r.stdout, r.stdout + r.stderr
