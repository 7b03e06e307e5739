"""The polyphase channelizer without a GPU (csrc/channelizer.hpp):

    tests/channelizer_reference.py -- the long double evaluation of the definition the GPU tests compare with -- against the
        definition summed term by term and against the scipy expression, channel k = upfirdn(h, x exp(-2 pi i k n / M), 1, D),
        at double round-off for the nine small cases, real and complex; pfb_prototype against scipy.signal.firwin;
    channelizer.hpp compiled with g++: full_frames, T, the first tap r0 of every (m, p) and a tile's run of the signal against
        brute force for every (L, K, M, D) with L, K <= 12 and M, D <= 7; the schedule's LDS bounds against the numpy model;
        every illegal argument;
    the C ABI's argument rules and exports, which need no device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import channelizer_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG = 16


def test_reference_against_the_definition_and_scipy():
    """taps with a normal distribution.  The scipy expression sums up to K products per output in double, (K + 2) u sum |h x|
    in any order, and its phases exp(-2 pi i (k n mod M) / M) come from a double angle below 2 pi, each within 2 pi 2 u + u <
    14 u: (K + 16) u max_m sum_p sum |h x| bounds both, and the term-by-term long double sum lies far inside it"""
    S = pytest.importorskip("scipy.signal")
    for case in R.SMALL_CASES:
        L, K, M, D = case
        h = np.random.default_rng([K, 5]).normal(size=K)
        n = np.arange(L)
        for cplx in (False, True):
            x = R.signals(case, "f64", cplx)[0]
            y, u, a = R.channelize_ref(h, x.astype(np.complex128), M, D)
            assert y.shape == (R.full_frames(L, K, D), M)
            bound = (K + 16) * 2.0 ** -53 * float(np.max(np.sum(a, axis=1))) + 1e-300
            assert float(np.max(np.abs(y - R.definition_ref(h, x, M, D)))) <= bound, case
            want = np.stack([S.upfirdn(h, x * np.exp(-2j * np.pi * ((k * n) % M) / M), 1, D) for k in range(M)], 1)
            assert want.shape == y.shape and float(np.max(np.abs(y - want))) <= bound, (case, cplx)
            if not cplx:  # the one-sided bins of a real signal are the first of the M
                half = R.channelize_ref(h, x, M, D)[0]
                assert half.shape[1] == M // 2 + 1 and np.array_equal(half, y[:, :M // 2 + 1])
            # a window is a slice of the whole, zeros past full_frames
            w = R.channelize_ref(h, x.astype(np.complex128), M, D, 1, y.shape[0] + 1)[0]
            assert np.array_equal(w[:-2], y[1:]) and not w[-2:].any()


def test_pfb_prototype_against_scipy():
    S = pytest.importorskip("scipy.signal")
    import phastft_amd as P

    for m, t, window in ((8, 4, ("kaiser", 5.0)), (7, 3, "hamming"), (256, 8, ("kaiser", 8.0)), (2, 5, "hann")):
        want = S.firwin(m * t, 1.0 / m, window=window)
        got = P.pfb_prototype(m, t, window)
        assert got.dtype == np.float64 and got.shape == (m * t,) and np.abs(got - want).max() <= 4e-16, (m, t, window)
    assert np.array_equal(P.pfb_prototype(16, 4), P.firwin_lowpass(64, 1 / 16, ("kaiser", 5.0)))
    with pytest.raises(ValueError):
        P.pfb_prototype(1, 4)
    with pytest.raises(ValueError):
        P.pfb_prototype(4, 0)


# ---- channelizer.hpp with g++ ----
@pytest.fixture(scope="module")
def helpers(tmp_path_factory):
    so = tmp_path_factory.mktemp("channelizer_helpers") / "libchannelizerhelpers.so"
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-shared", "-fPIC", "-I", os.path.join(ROOT, "phastft_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "channelizer_geom_test.cpp"), "-o", str(so)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    h = C.CDLL(str(so))
    u, p = C.c_ulonglong, C.c_void_p
    h.ch_t_full_frames.restype = h.ch_t_t.restype = h.ch_t_r0.restype = u
    h.ch_t_full_frames.argtypes = [u] * 3
    h.ch_t_t.argtypes = [u] * 2
    h.ch_t_r0.argtypes = [u] * 4
    h.ch_t_geom.argtypes = [u, u, u, p]
    h.ch_t_span.argtypes = [u] * 8 + [p, p]
    h.ch_t_bad_args.argtypes = [u] * 6
    h.ch_t_const.restype = C.c_uint
    return h


def _geom(h, K, M, D):
    out = (C.c_uint * 7)()
    h.ch_t_geom(K, M, D, out)
    return tuple(out)


def test_geometry_against_brute_force(helpers):
    """per (L, K, M, D): the frames that hold a product, T, r0 of every (m, p), and for tiles of 1 .. 3 frames and column
    runs the periods of the signal the taps j0 .. j0 + jc - 1 meet -- chan_span names every one of them, and no more than the
    kernel's bound"""
    h = helpers
    q_lo, count = C.c_longlong(), C.c_ulonglong()
    for M in range(1, 8):
        for D in range(1, 8):
            for K in range(1, 13):
                T = -(-K // M)
                assert h.ch_t_t(K, M) == T == R.t_of(K, M)
                for L in range(1, 13):
                    # the last frame with a tap on a sample: h[m D - n] with 0 <= m D - n < K, 0 <= n < L
                    last = max(m for m in range(L + K) if any(0 <= m * D - n < K for n in range(L)))
                    assert h.ch_t_full_frames(L, K, D) == last + 1 == R.full_frames(L, K, D), (L, K, D)
                for m in range(0, 9):
                    for p in range(M):
                        r0 = h.ch_t_r0(m, p, M, D)
                        # the taps of column p in frame m: h[i] with (m D - i) = p mod M, i >= 0; the first is r0
                        assert r0 == min(i for i in range(M) if (m * D - i - p) % M == 0), (m, p, M, D)
                for m0 in (0, 2, 5):
                    for n in (1, 2, 3):
                        for p0, c in ((0, M), (0, 1), (M - 1, 1), (M // 2, M - M // 2)):
                            for j0, jc in ((0, T), (0, 1), (T - 1, 1)):
                                met = set()
                                for m in range(m0, m0 + n):
                                    for p in range(p0, p0 + c):
                                        r0 = (m * D - p) % M
                                        for j in range(j0, j0 + jc):
                                            s = m * D - r0 - j * M   # a multiple of M away from p, below or above 0
                                            assert (s - p) % M == 0
                                            met.add((s - p) // M)
                                h.ch_t_span(m0, n, p0, c, M, D, j0, jc, C.byref(q_lo), C.byref(count))
                                assert q_lo.value <= min(met) and max(met) < q_lo.value + count.value, (M, D, K, m0, n, p0, c, j0, jc)
                                assert q_lo.value == min(met) or c < M or n > 1   # tight where one frame has all its columns
                                assert count.value <= ((n - 1) * D + M - 1) // M + 2 + jc - 1


def test_the_schedule_fits_lds_and_matches_the_model(helpers):
    h = helpers
    lds, max_cols, per_thread = (h.ch_t_const(i) for i in range(3))
    assert (lds, max_cols, per_thread) == (R.LDS, R.MAX_COLS, R.PER_THREAD) and max_cols == 256
    shapes = [c[1:] for c in R.CASES] + [(k, m, d) for m in (1, 2, 3, 7, 64, 100, 255, 256, 257, 1000, 4096, 1 << 29)
                                         for d in (1, 3, m, 2 * m + 1, 5000, 1 << 29) for k in (1, m, 8 * m + 3, 1 << 29) if k <= 1 << 29]
    for K, M, D in shapes:
        cols, fpp, per, frames, span, jc, rows = g = _geom(h, K, M, D)
        assert g == R.geom(K, M, D), (K, M, D)
        assert cols == min(M, 256) and 1 <= fpp and fpp * cols <= 256 and 1 <= per <= per_thread and frames == fpp * per
        assert span >= ((frames - 1) * D + M - 1) // M + 2 and 1 <= jc <= R.t_of(K, M)
        assert rows == span + jc - 1 and rows * cols <= lds, (K, M, D)
        assert (frames - 1) * (D // M) < 1 << 32   # the kernel's 32-bit period steps


def test_illegal_arguments_are_refused(helpers):
    h = helpers
    ok = (100, 9, 4, 4, 0, 0)
    big = (1 << 29) + 1
    assert h.ch_t_bad_args(*ok) == 0
    assert h.ch_t_bad_args(1 << 29, 1 << 29, 1, 1 << 29, 0, 0) == 0 and h.ch_t_bad_args(100, 9, 4, 4, 27, 5) == 0  # first = full_frames
    for bad in ((0, 9, 4, 4, 0, 0), (big, 9, 4, 4, 0, 0), (100, 0, 4, 4, 0, 0), (100, big, 4, 4, 0, 0), (100, 9, 0, 4, 0, 0),
                (100, 9, big, 4, 0, 0), (100, 9, 4, 0, 0, 0), (100, 9, 4, big, 0, 0), (100, 9, 4, 4, 28, 1), (100, 9, 4, 4, 27, 0),
                (100, 9, 1 << 20, 4, 0, 1025), (100, 9, 1, 4, 0, (1 << 30) + 1)):
        assert h.ch_t_bad_args(*bad) == 1, bad


# ---- the C ABI before the device is touched ----
def test_argument_codes_and_exports_without_a_device():
    from phastft_amd import _lib

    lib = _lib.lib()
    for sfx, ndt in (("64", np.float64), ("32", np.float32)):
        taps = np.ones(9, ndt)
        tp = taps.ctypes.data_as(C.c_void_p)
        h = C.c_void_p()
        new = getattr(lib, f"phast_planner_channelizer{sfx}_new")
        big = (1 << 29) + 1
        for bad in ((0, tp, 9, 4, 4, 0, 0, 0), (100, None, 9, 4, 4, 0, 0, 0), (100, tp, 0, 4, 4, 0, 0, 1), (100, tp, 9, 0, 4, 0, 0, 0),
                    (100, tp, 9, 4, 0, 0, 0, 1), (100, tp, 9, big, 4, 0, 0, 0), (100, tp, 9, 4, big, 0, 0, 0), (100, tp, 9, 4, 4, 28, 0, 0),
                    (100, tp, 9, 4, 4, 27, 0, 1), (100, tp, 9, 1 << 20, 4, 0, 1025, 0)):
            assert new(*bad, C.byref(h)) == INVALID_ARG and not h.value, bad
        assert new(100, tp, 9, 4, 4, 0, 0, 0, None) == INVALID_ARG
        fs = "f64" if sfx == "64" else "f32"
        for name in (f"phast_channelize_{fs}_dev", f"phast_channelize_{fs}_with_planner", f"phast_planner_channelizer{sfx}_time_stages"):
            fn = getattr(lib, name)
            args = [None] * len(fn.argtypes)
            for i, t in enumerate(fn.argtypes):
                if t is not C.c_void_p:
                    args[i] = 1
            assert fn(*args) == INVALID_ARG   # a null planner
        for name in ("out_frames", "full_frames", "bins", "tile_frames", "tile_cols", "chunk", "periods", "workspace_min",
                     "workspace_len", "device_bytes"):
            fn = getattr(lib, f"phast_planner_channelizer{sfx}_{name}")
            assert fn(None, 1) == 0 if name == "workspace_len" else fn(None) == 0


def test_python_argument_errors():
    import phastft_amd as P

    for name in ("PlannerChannelizer64", "PlannerChannelizer32", "channelize_batched", "channelize_64_with_planner",
                 "channelize_32_with_planner", "channelize_poly", "pfb_prototype"):
        assert name in P.__all__ and hasattr(P, name), name
    with pytest.raises(P.PhastPanic):
        P.PlannerChannelizer64(100, np.ones(9), 0)
    with pytest.raises(P.PhastPanic):
        P.PlannerChannelizer32(100, np.ones(9), 4, 0)
    with pytest.raises(TypeError):
        P.channelize_poly(np.zeros(8), np.ones(3), 4)   # host arrays go through the *_with_planner forms
