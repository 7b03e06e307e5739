"""Multi-dimensional transforms (csrc/nd.hpp, csrc/planner_nd.hpp) without a GPU: the new C ABI is exported and listed,
shape and argument errors come back as their codes before the device is touched (NO_DEVICE for calls that need one), the
schedule of nd.hpp -- compiled with g++ and executed step by step in numpy -- computes fftn / ifftn / rfftn / irfftn and
lands in the caller's buffer with r transposes for rank r, and the C++ and Rust mirrors carry the new names."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = [f"phast_planner_{k}{s}_{f}" for k in ("nd", "r2c_nd") for s in ("64", "32")
       for f in ("new", "free", "describe", "device_bytes", "workspace_len")]
NEW += [f"phast_fft_{s}_nd{f}" for s in ("64", "32") for f in ("", "_with_planner", "_dev")]
NEW += [f"phast_planner_nd{s}_time_steps" for s in ("64", "32")]
NEW += [f"phast_{k}_fft_{s}_nd{f}" for k in ("r2c", "c2r") for s in ("f64", "f32") for f in ("", "_with_planner", "_dev")]
OK, LEN_MISMATCH, PLANNER_SIZE, NO_DEVICE, INVALID_ARG = 0, 2, 3, 15, 16
R2C_INPUT_LEN, R2C_OUT_RE_LEN, R2C_OUT_IM_LEN, C2R_OUTPUT_LEN, C2R_IN_RE_LEN, C2R_IN_IM_LEN = 5, 6, 7, 8, 9, 10


@pytest.fixture(scope="module")
def lib():
    from phastft_amd import _lib

    return _lib.lib()


def _no_gpu():
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present: tests/test_gpu_nd.py covers the device side")


def _dims(shape):
    return (C.c_size_t * max(1, len(shape)))(*shape), C.c_size_t(len(shape))


BAD_SHAPES = [(), (0,), (4, 0, 3), ((1 << 29) + 1,), (1 << 16, 1 << 15), (2,) * 9]


def test_new_symbols_are_exported_and_listed(lib):
    from phastft_amd import _lib

    header = open(os.path.join(ROOT, "include", "phastft_hip.h")).read()
    assert len(NEW) == 40
    for name in NEW:
        getattr(lib, name)
        assert name in _lib.SYMBOLS and re.search(r"\b" + name + r"\s*\(", header), name


def test_planner_shape_codes(lib):
    """rank 0 or > 8, an axis of 0 or > 2^29, a product > 2^30: INVALID_ARG before the device is touched"""
    for k in ("nd", "r2c_nd"):
        for sfx in ("64", "32"):
            new = getattr(lib, f"phast_planner_{k}{sfx}_new")
            for shape in BAD_SHAPES:
                h = C.c_void_p(1)
                assert new(*_dims(shape), C.byref(h)) == INVALID_ARG and not h.value, (k, shape)
            assert new(None, C.c_size_t(2), C.byref(C.c_void_p())) == INVALID_ARG
            assert new(*_dims((4, 4)), None) == INVALID_ARG
            assert getattr(lib, f"phast_planner_{k}{sfx}_workspace_len")(None, C.c_size_t(1)) == 0


def test_call_argument_codes(lib):
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    for sfx, fs, dt in (("64", "f64", np.float64), ("32", "f32", np.float32)):
        a, b = np.zeros(12, dt), np.zeros(12, dt)
        plain = getattr(lib, f"phast_fft_{sfx}_nd")
        for shape in BAD_SHAPES:
            assert plain(p(a), C.c_size_t(12), p(b), C.c_size_t(12), *_dims(shape), 1) == INVALID_ARG, shape
        assert plain(p(a), C.c_size_t(12), p(b), C.c_size_t(11), *_dims((3, 4)), 1) == LEN_MISMATCH
        assert plain(p(a), C.c_size_t(12), p(b), C.c_size_t(12), *_dims((3, 5)), 1) == PLANNER_SIZE  # wrong element count
        assert plain(p(a), C.c_size_t(12), p(b), C.c_size_t(12), *_dims((3, 4)), 7) == INVALID_ARG   # direction
        assert plain(None, C.c_size_t(12), p(b), C.c_size_t(12), *_dims((3, 4)), 1) == INVALID_ARG
        for name in (f"phast_fft_{sfx}_nd_with_planner",):
            assert getattr(lib, name)(p(a), C.c_size_t(12), p(b), C.c_size_t(12), 1, None) == INVALID_ARG
        dev = getattr(lib, f"phast_fft_{sfx}_nd_dev")
        assert dev(p(a), p(b), C.c_size_t(12), C.c_size_t(1), C.c_size_t(12), 1, None, p(a), C.c_size_t(12), None) == INVALID_ARG
        h = np.zeros(9, dt)  # [3][4 // 2 + 1]
        r2c = getattr(lib, f"phast_r2c_fft_{fs}_nd")
        assert r2c(p(a), C.c_size_t(11), p(h), C.c_size_t(9), p(h), C.c_size_t(9), *_dims((3, 4))) == R2C_INPUT_LEN
        assert r2c(p(a), C.c_size_t(12), p(h), C.c_size_t(8), p(h), C.c_size_t(9), *_dims((3, 4))) == R2C_OUT_RE_LEN
        assert r2c(p(a), C.c_size_t(12), p(h), C.c_size_t(9), p(h), C.c_size_t(10), *_dims((3, 4))) == R2C_OUT_IM_LEN
        assert r2c(p(a), C.c_size_t(12), p(h), C.c_size_t(9), p(h), C.c_size_t(9), *_dims(())) == INVALID_ARG
        c2r = getattr(lib, f"phast_c2r_fft_{fs}_nd")
        assert c2r(p(h), C.c_size_t(9), p(h), C.c_size_t(9), p(a), C.c_size_t(13), *_dims((3, 4))) == C2R_OUTPUT_LEN
        assert c2r(p(h), C.c_size_t(8), p(h), C.c_size_t(9), p(a), C.c_size_t(12), *_dims((3, 4))) == C2R_IN_RE_LEN
        assert c2r(p(h), C.c_size_t(9), p(h), C.c_size_t(7), p(a), C.c_size_t(12), *_dims((3, 4))) == C2R_IN_IM_LEN
        for k in ("r2c", "c2r"):
            assert getattr(lib, f"phast_{k}_fft_{fs}_nd_dev")(p(a), p(h), p(h), C.c_size_t(12), C.c_size_t(1), C.c_size_t(12),
                                                            C.c_size_t(9), None, p(a), C.c_size_t(64), None) == INVALID_ARG


def test_device_calls_fail_loudly_without_a_gpu(lib):
    _no_gpu()
    import phastft_amd as P

    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    for sfx, fs, dt in (("64", "f64", np.float64), ("32", "f32", np.float32)):
        for k in ("nd", "r2c_nd"):
            h = C.c_void_p()
            assert getattr(lib, f"phast_planner_{k}{sfx}_new")(*_dims((30, 40)), C.byref(h)) == NO_DEVICE and not h.value
        a, b, h9 = np.zeros(12, dt), np.zeros(12, dt), np.zeros(9, dt)
        assert getattr(lib, f"phast_fft_{sfx}_nd")(p(a), C.c_size_t(12), p(b), C.c_size_t(12), *_dims((3, 4)), 1) == NO_DEVICE
        assert getattr(lib, f"phast_r2c_fft_{fs}_nd")(p(a), C.c_size_t(12), p(h9), C.c_size_t(9), p(h9), C.c_size_t(9),
                                                      *_dims((3, 4))) == NO_DEVICE
        assert getattr(lib, f"phast_c2r_fft_{fs}_nd")(p(h9), C.c_size_t(9), p(h9), C.c_size_t(9), p(a), C.c_size_t(12),
                                                      *_dims((3, 4))) == NO_DEVICE
    with pytest.raises(P.PhastHipError):
        P.PlannerNd64((8, 8))
    with pytest.raises(P.PhastHipError):
        P.fft_64_nd(np.zeros(12), np.zeros(12), (3, 4), P.Direction.Forward)
    with pytest.raises(P.PhastHipError):
        P.r2c_fft_f32_nd(np.zeros((3, 4), np.float32), np.zeros(9, np.float32), np.zeros(9, np.float32), (3, 4))
    with pytest.raises(P.PhastPanic):
        P.PlannerR2cNd32((0, 4))
    with pytest.raises(P.PhastPanic):
        P.fft_32_nd(np.zeros(12, np.float32), np.zeros(11, np.float32), (3, 4), P.Direction.Forward)


# ---------------------------------------------------------------------------------------------
# the schedule of nd.hpp, run in numpy
# ---------------------------------------------------------------------------------------------
DRIVER = r"""
#include "nd.hpp"
#include <cstdio>
#include <cstdlib>
using namespace phast;
int main(int argc, char **argv) {
    const int kind = atoi(argv[1]);
    size_t dims[16], rank = (size_t)argc - 2, sq[kNdMaxRank];
    for (size_t i = 0; i < rank; ++i) dims[i] = strtoull(argv[i + 2], nullptr, 10);
    unsigned long long total = 0;
    int bad = 1;
    const size_t q = nd_squeeze(dims, rank, kind, sq, &total, &bad);
    if (bad) { printf("bad\n"); return 0; }
    NdStep st[2 * kNdMaxRank + 1];
    const size_t ns = nd_schedule(sq, q, kind, st);
    printf("%zu %llu\n", q, total);
    for (size_t i = 0; i < ns; ++i) printf("%d %d %d %zu %zu %d\n", st[i].op, st[i].src, st[i].dst, st[i].rows, st[i].n, st[i].axis);
    return 0;
}
"""
X, W, W2, R = 0, 1, 2, 3
TRANSFORM, TRANSPOSE, R2C_ROWS, C2R_ROWS = 0, 1, 2, 3


@pytest.fixture(scope="module")
def sched(tmp_path_factory):
    d = tmp_path_factory.mktemp("nd_sched")
    src, exe = d / "sched.cpp", str(d / "sched")
    src.write_text(DRIVER)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "phastft_amd", "csrc"),
                        str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(kind, shape):
        out = subprocess.run([exe, str(kind), *map(str, shape)], capture_output=True, text=True, check=True).stdout.split("\n")
        if out[0] == "bad":
            return None
        q, total = map(int, out[0].split())
        return q, total, [tuple(map(int, line.split())) for line in out[1:] if line]

    return run


def _execute(steps, kind, bufs, inverse):
    """run the steps on flat numpy buffers (one array): X, W, W2 complex, R real"""
    for op, src, dst, rows, n, _axis in steps:
        a = bufs[src]
        if op == TRANSFORM:
            m = a[:rows * n].reshape(rows, n)
            out = np.fft.ifft(m, axis=1) if inverse else np.fft.fft(m, axis=1)
        elif op == TRANSPOSE:
            out = a[:rows * n].reshape(rows, n).T
        elif op == R2C_ROWS:
            assert src == R and dst != R
            out = np.fft.rfft(a[:rows * n].reshape(rows, n), axis=1)
        else:
            assert dst == R
            out = np.fft.irfft(a[:rows * (n // 2 + 1)].reshape(rows, n // 2 + 1), n=n, axis=1)
        out = out.reshape(-1)
        if kind == 2:
            assert dst != X, "C2R writes its input planes"
        if kind == 1:
            assert dst != R, "R2C writes its input"
        bufs[dst][:out.size] = out


RANKS = [(7,), (16,), (1,), (1, 1), (4, 6), (5, 3), (1, 9, 1), (3, 1, 4, 1, 5), (2, 3, 4), (2, 3, 4, 5), (3, 2, 5, 2, 3),
         (1024, 3), (3, 1024), (9, 1), (9, 2), (6, 7), (6, 8), (2, 1, 7), (1, 1, 12), (4, 5, 1)]


@pytest.mark.parametrize("shape", RANKS, ids=lambda s: "x".join(map(str, s)))
def test_complex_schedule_in_numpy(sched, shape):
    q, total, steps = sched(0, shape)
    assert total == int(np.prod(shape)) and q == sum(1 for d in shape if d > 1)
    transposes = sum(1 for s in steps if s[0] == TRANSPOSE)
    assert transposes == (q if q >= 2 else 0)
    rng = np.random.default_rng(len(shape) * 1000 + total)
    x = rng.standard_normal(total) + 1j * rng.standard_normal(total)
    for inverse in (False, True):
        bufs = {X: x.copy(), W: np.full(total, np.nan, complex)}
        _execute(steps, 0, bufs, inverse)
        want = (np.fft.ifftn if inverse else np.fft.fftn)(x.reshape(shape)).reshape(-1)
        np.testing.assert_allclose(bufs[X], want, rtol=0, atol=1e-9 * max(1.0, np.abs(want).max()))


@pytest.mark.parametrize("shape", RANKS, ids=lambda s: "x".join(map(str, s)))
def test_real_schedules_in_numpy(sched, shape):
    q, total, steps = sched(1, shape)
    lead = [d for d in shape[:-1] if d > 1]
    assert q == len(lead) + 1
    assert sum(1 for s in steps if s[0] == TRANSPOSE) == (q if q >= 2 else 0)
    half = total // shape[-1] * (shape[-1] // 2 + 1)
    rng = np.random.default_rng(total + 7)
    x = rng.standard_normal(total)
    bufs = {R: x.copy(), X: np.full(half, np.nan, complex), W: np.full(half, np.nan, complex)}
    _execute(steps, 1, bufs, False)
    want = np.fft.rfftn(x.reshape(shape)).reshape(-1)
    np.testing.assert_allclose(bufs[X], want, rtol=0, atol=1e-9 * max(1.0, np.abs(want).max()))
    q2, _, back = sched(2, shape)
    assert q2 == q and sum(1 for s in back if s[0] == TRANSPOSE) == (q if q >= 2 else 0)
    spec = want.copy()
    bufs = {X: spec, W: np.full(half, np.nan, complex), W2: np.full(half, np.nan, complex), R: np.full(total, np.nan)}
    _execute(back, 2, bufs, True)
    assert np.array_equal(spec, want)
    np.testing.assert_allclose(bufs[R], np.fft.irfftn(want.reshape(shape[:-1] + (shape[-1] // 2 + 1,)), s=shape, axes=list(range(len(shape)))).reshape(-1),
                               rtol=0, atol=1e-9)


def test_schedule_rejects_bad_shapes(sched):
    for kind in (0, 1, 2):
        for shape in [(0,), (4, 0), ((1 << 29) + 1,), (1 << 16, 1 << 15), (2,) * 9]:
            assert sched(kind, shape) is None, (kind, shape)
    assert sched(0, (1 << 29, 2)) is not None  # 2^30 points: the limit itself


def test_cpp_mirror_compiles_and_panics_without_a_device(tmp_path):
    _no_gpu()
    from phastft_amd import build

    lib = build.build()
    exe = str(tmp_path / "nd_test")
    libdir = os.path.dirname(lib)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "nd_test.cpp"), "-o", exe, "-L", libdir, "-lphastft_hip",
                        f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "nd: ok" in r.stdout, r.stdout + r.stderr


def test_rust_safe_wrappers():
    """Parsed textually, as tests/test_rust_shim.py does (no Rust toolchain here); the extern block itself is checked
    against the header by that test."""
    src = os.path.join(ROOT, "rust", "phastft-hip", "src")
    lib_rs, planner = open(os.path.join(src, "lib.rs")).read(), open(os.path.join(src, "planner.rs")).read()
    r2c = open(os.path.join(src, "algorithms", "r2c.rs")).read()
    assert re.search(r"pub fn \$plain\(reals: &mut \[\$t\], imags: &mut \[\$t\], shape: &\[usize\], direction: Direction\)",
                     lib_rs)
    for name in ("fft_64_nd", "fft_32_nd", "fft_64_nd_with_planner", "fft_32_nd_with_planner", "fft_64_nd_dev",
                 "fft_32_nd_dev"):
        assert re.search(r"\b" + name + r"\b", lib_rs), name
    for name in ("PlannerNd64", "PlannerNd32", "PlannerR2cNd64", "PlannerR2cNd32"):
        assert re.search(r"impl_planner_nd!\(" + name + r",", planner), name
    assert "pub fn new(shape: &[usize]) -> Self" in planner
    for fs in ("f64", "f32"):
        for k in ("r2c", "c2r"):
            for f in ("", "_with_planner", "_dev"):
                name = f"{k}_fft_{fs}_nd{f}"
                assert re.search(r"\b" + name + r"\b", r2c) and re.search(r"\b" + name + r"\b", lib_rs), name


def test_cpp_mirror_names():
    hpp = open(os.path.join(ROOT, "include", "phastft.hpp")).read()
    for name in ("PlannerNd64", "PlannerNd32", "PlannerR2cNd64", "PlannerR2cNd32"):
        assert f"PHASTFT_PLANNER_ND({name}," in hpp
    for name in ("fft_64_nd", "fft_32_nd", "r2c_fft_f64_nd", "r2c_fft_f32_nd", "c2r_fft_f64_nd", "c2r_fft_f32_nd"):
        assert f"inline void {name}(" in hpp and f"inline void {name}_with_planner(" in hpp
