"""The host half of sample-rate conversion (csrc/resample.hpp, csrc/planner_resample.hpp), without a GPU:

    the long double references (tests/resample_reference.py) against scipy.signal.upfirdn, resample_poly, resample, decimate
        and firwin at double round-off, and the package's numpy filter design against firwin;
    resample.hpp compiled with g++: full_len, Kp and a tile's run of the signal against brute force for every
        (L, K, up, down) with L, K <= 12 and up, down <= 7, the schedule's LDS bounds, and every illegal argument;
    the numpy model of the kernel's schedule (tiles, tap chunks, phase-major table, fixed order): bit for bit the reference on
        integer-valued data, inside the gate (Kp + 2) u sum |h x| on random data;
    the argument codes of the C ABI before the device is touched, and the exports."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import resample_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG = 16


# ---- the references against scipy ----
def test_upfirdn_reference_against_scipy():
    S = pytest.importorskip("scipy.signal")
    for (L, K, up, down) in R.UPFIRDN_CASES[:10]:
        h, x = R.taps(K, "f64"), R.signal(L, "f64")
        ref, scale = R.upfirdn_ref(h, x, up, down)
        want = S.upfirdn(h, x, up, down)
        assert ref.size == want.size == R.full_len(L, K, up, down)
        assert np.all(np.abs(np.asarray(ref, np.float64) - want) <= R.poly_gate("f64", K, up, scale) + 1e-300), (L, K, up, down)
        # the window: first and a tail of zeros
        part, _ = R.upfirdn_ref(h, x, up, down, 2, ref.size + 3)
        assert np.array_equal(part[:max(ref.size - 2, 0)], ref[2:]) and not part[max(ref.size - 2, 0):].any()


def test_filter_designs_against_scipy():
    S = pytest.importorskip("scipy.signal")
    import phastft_amd as P

    for numtaps, cutoff, window in ((3201, 1 / 160, ("kaiser", 5.0)), (81, 0.25, "hamming"), (41, 0.5, ("kaiser", 5.0)), (7, 1 / 3, "hamming")):
        want = S.firwin(numtaps, cutoff, window=window)
        assert np.abs(np.asarray(R.firwin_ref(numtaps, cutoff, window), np.float64) - want).max() <= 4e-16
        assert np.abs(P.firwin_lowpass(numtaps, cutoff, window) - want).max() <= 4e-16
    with pytest.raises(ValueError):
        P.firwin_lowpass(5, 0.5, "tukey")


def test_resample_poly_decimate_and_resample_references_against_scipy():
    S = pytest.importorskip("scipy.signal")
    for L, up, down in ((300, 160, 147), (300, 147, 160), (50, 3, 2), (50, 2, 3), (64, 4, 1), (64, 1, 4), (33, 6, 4), (7, 5, 5)):
        x = R.signal(L, "f64")
        got, want = np.asarray(R.resample_poly_ref(x, up, down), np.float64), S.resample_poly(x, up, down)
        assert got.shape == want.shape and np.abs(got - want).max() <= 1e-14, (L, up, down)
    x = R.signal(40, "f64")
    b = R.taps(9, "f64")
    assert np.abs(np.asarray(R.resample_poly_ref(x, 3, 2, taps=b), np.float64) - S.resample_poly(x, 3, 2, window=b)).max() <= 1e-14
    for L, q, n in ((200, 4, None), (100, 3, None), (64, 2, 10), (5, 7, None)):
        x = R.signal(L, "f64")
        got, want = np.asarray(R.decimate_ref(x, q, n), np.float64), S.decimate(x, q, n, ftype="fir")
        assert got.shape == want.shape and np.abs(got - want).max() <= 1e-14, (L, q, n)
    for L, num in R.FOURIER_CASES:
        x = R.signal(L, "f64")
        got, want = np.asarray(R.resample_ref(x, num), np.float64), S.resample(x, num)
        assert got.shape == want.shape and np.abs(got - want).max() <= 1e-13 * max(1.0, np.abs(want).max()), (L, num)


# ---- resample.hpp with g++ ----
@pytest.fixture(scope="module")
def helpers(tmp_path_factory):
    so = tmp_path_factory.mktemp("resample_helpers") / "libresamplehelpers.so"
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-shared", "-fPIC", "-I", os.path.join(ROOT, "phastft_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "resample_geom_test.cpp"), "-o", str(so)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    h = C.CDLL(str(so))
    u, p = C.c_ulonglong, C.c_void_p
    h.rs_t_full_len.argtypes, h.rs_t_full_len.restype = [u] * 4, u
    h.rs_t_kp.argtypes, h.rs_t_kp.restype = [u] * 2, u
    h.rs_t_geom.argtypes = [u, u, u, p]
    h.rs_t_span.argtypes = [u] * 6 + [p, p]
    h.rs_t_upfirdn_bad_args.argtypes = [u] * 6
    h.rs_t_resample_bad_args.argtypes = [u] * 2
    h.rs_t_bins.argtypes, h.rs_t_bins.restype = [u] * 2, u
    h.rs_t_nyquist.argtypes, h.rs_t_nyquist.restype = [u] * 2, C.c_double
    h.rs_t_const.argtypes, h.rs_t_const.restype = [C.c_int], C.c_uint
    return h


def _geom(h, K, up, down):
    out = (C.c_uint * 5)()
    h.rs_t_geom(K, up, down, out)
    return tuple(out)


def test_geometry_against_brute_force(helpers):
    h = helpers
    lo, count = C.c_longlong(), C.c_ulonglong()
    for L in range(1, 13):
        for K in range(1, 13):
            for up in range(1, 8):
                for down in range(1, 8):
                    # the pairs (n, i) with m down = n up + i: the outputs that have a product, and the samples they meet
                    reach = {}
                    for n in range(L):
                        for i in range(K):
                            if (n * up + i) % down == 0:
                                reach.setdefault((n * up + i) // down, []).append(n)
                    # every down-th sample of the (L - 1) up + K samples of the filtered, zero-stuffed signal
                    full = len(range(0, (L - 1) * up + K, down))
                    assert max(reach) < full
                    assert h.rs_t_full_len(L, K, up, down) == full, (L, K, up, down)
                    kp = -(-K // up)
                    assert h.rs_t_kp(K, up) == kp
                    for m0, n_out, j0, jc in ((0, full, 0, kp), (1, 2, 0, kp), (full // 2, 3, 0, 1), (full // 2, 3, kp - 1, 1), (0, 1, 0, kp)):
                        h.rs_t_span(m0, n_out, up, down, j0, jc, C.byref(lo), C.byref(count))
                        need = [(m * down) // up - j for m in range(m0, m0 + n_out) for j in range(j0, j0 + jc)]
                        assert lo.value == min(need) and lo.value + count.value - 1 == max(need), (L, K, up, down, m0, n_out, j0, jc)
                        # ... and every sample an output of the tile really multiplies is inside it
                        for m in range(m0, min(m0 + n_out, full)):
                            for n in reach.get(m, []):
                                j = (m * down) // up - n
                                if j0 <= j < j0 + jc:
                                    assert lo.value <= n < lo.value + count.value


def test_the_schedule_fits_lds_and_matches_the_model(helpers):
    h = helpers
    tap_lds, tap_pad, sig_lds, max_tile, per_thread, max_rows = (h.rs_t_const(i) for i in range(6))
    assert (tap_lds, sig_lds, max_tile, max_rows) == (R.TAP_LDS, R.SIG_LDS, R.MAX_TILE, R.MAX_ROWS) and max_tile == 256 * per_thread
    rng = np.random.default_rng(5)
    cases = [(K, up, down) for (_, K, up, down) in R.UPFIRDN_CASES]
    cases += [(1, 1, 1), (1 << 29, 1, 1), (1 << 29, 1 << 20, 1), (1 << 29, 1, 1 << 20), (1, 1 << 20, 1 << 20), (5, 256, 1), (5, 257, 1),
              (4096, 1, 1), (4097, 1, 1), (2048, 1, 4096), (2049, 1, 4095)]
    cases += [(int(rng.integers(1, 1 << 14)), int(rng.integers(1, 600)), int(rng.integers(1, 600))) for _ in range(300)]
    lo, count = C.c_longlong(), C.c_ulonglong()
    for K, up, down in cases:
        rows, jc, stride, tile, by_phase = _geom(h, K, up, down)
        assert (rows, jc, stride, tile, bool(by_phase)) == R.geom(K, up, down), (K, up, down)
        assert 1 <= jc <= -(-K // up) and stride == jc | 1 and 1 <= tile <= (max_tile if by_phase else max_rows)
        assert rows * stride <= tap_lds + tap_pad and (rows == up if by_phase else tile <= rows)
        for m0 in (0, 1, tile - 1, 12345 * tile, (1 << 29) - tile):   # the run of a whole tile, wherever it starts
            h.rs_t_span(m0, tile, up, down, 0, jc, C.byref(lo), C.byref(count))
            assert count.value <= sig_lds, (K, up, down, m0, count.value)
    # the chunks the GPU cases name
    assert R.geom(4200, 7, 5)[1] == 585 and R.geom(6000, 300, 7)[:2] == (256, 16) and R.geom(5000, 1, 1)[1] == 2048


def test_illegal_arguments_are_refused(helpers):
    h = helpers
    ok = (100, 9, 3, 2, 0, 0)
    assert h.rs_t_upfirdn_bad_args(*ok) == 0
    full = R.full_len(100, 9, 3, 2)
    for bad in ((0, 9, 3, 2, 0, 0), ((1 << 29) + 1, 9, 3, 2, 0, 0), (100, 0, 3, 2, 0, 0), (100, (1 << 29) + 1, 3, 2, 0, 0),
                (100, 9, 0, 2, 0, 0), (100, 9, (1 << 20) + 1, 2, 0, 0), (100, 9, 3, 0, 0, 0), (100, 9, 3, (1 << 20) + 1, 0, 0),
                (100, 9, 3, 2, full + 1, 5), (100, 9, 3, 2, full, 0),          # nothing left for out_len = 0
                (100, 9, 3, 2, 0, (1 << 29) + 1), (1 << 29, 9, 1 << 20, 1, 0, 0)):   # full_len > 2^29 needs an out_len
        assert h.rs_t_upfirdn_bad_args(*bad) == 1, bad
    assert h.rs_t_upfirdn_bad_args(100, 9, 3, 2, full, 7) == 0                 # a window of zeros behind the end
    assert h.rs_t_upfirdn_bad_args(1 << 29, 9, 1 << 20, 1, 1 << 40, 1 << 29) == 0
    assert h.rs_t_upfirdn_bad_args((1 << 29) - 512, 1 << 29, 1 << 20, 1 << 20, 0, 0) == 0
    assert h.rs_t_resample_bad_args(1, 1) == 0 and h.rs_t_resample_bad_args(1 << 29, 1 << 29) == 0
    for bad in ((0, 5), (5, 0), ((1 << 29) + 1, 5), (5, (1 << 29) + 1)):
        assert h.rs_t_resample_bad_args(*bad) == 1, bad
    for L, num in R.FOURIER_CASES:
        N = min(L, num)
        assert h.rs_t_bins(L, num) == N // 2 + 1
        assert h.rs_t_nyquist(L, num) == (1.0 if N % 2 or L == num else 2.0 if num < L else 0.5)


# ---- the model of the schedule ----
def _windows(L, K, up, down):
    tile = R.geom(K, up, down)[3]
    full = R.full_len(L, K, up, down)
    yield 0, None
    for n in (tile - 1, tile, tile + 1, 2 * tile + 3):
        if n >= 1:
            yield min(3, full), n


@pytest.mark.parametrize("case", R.UPFIRDN_CASES[:10], ids=lambda c: "L%d_K%d_up%d_down%d" % c)
def test_model_is_the_reference_on_integers_and_inside_the_gate(case):
    L, K, up, down = case
    rng = np.random.default_rng([L, K, up, down])
    for dt in ("f64", "f32"):
        ndt = R.NDT[dt]
        hi, xi = rng.integers(-8, 9, K).astype(ndt), rng.integers(-8, 9, L).astype(ndt)   # sums below 2^24: exact in f32
        h, x = R.taps(K, dt), R.signal(L, dt)
        for first, out_len in _windows(L, K, up, down):
            if K * up > 10 ** 6 and out_len is not None and out_len > 600:
                continue   # (the model is a Python loop: the long windows of the long filters run on the device)
            exact, _ = R.upfirdn_ref(hi, xi, up, down, first, out_len)
            got = R.upfirdn_model(hi, xi, up, down, first, out_len, ndt)
            assert got.dtype == ndt and np.array_equal(got.astype(np.longdouble), exact), (case, dt, first, out_len)
            ref, scale = R.upfirdn_ref(h, x, up, down, first, out_len)
            got = R.upfirdn_model(h, x, up, down, first, out_len, ndt)
            err = np.abs(got.astype(np.longdouble) - ref).astype(np.float64)
            assert np.all(err <= R.poly_gate(dt, K, up, scale)), (case, dt, first, out_len, float((err / np.maximum(R.poly_gate(dt, K, up, scale), 1e-300)).max()))


# ---- the C ABI before the device is touched ----
def test_argument_codes_and_exports_without_a_device():
    from phastft_amd import _lib

    lib = _lib.lib()
    for sfx, ndt in (("64", np.float64), ("32", np.float32)):
        taps = np.ones(9, ndt)
        tp = taps.ctypes.data_as(C.c_void_p)
        h = C.c_void_p()
        new = getattr(lib, f"phast_planner_upfirdn{sfx}_new")
        for bad in ((0, tp, 9, 3, 2, 0, 0), (100, None, 9, 3, 2, 0, 0), (100, tp, 0, 3, 2, 0, 0), (100, tp, 9, 0, 2, 0, 0),
                    (100, tp, 9, 3, 0, 0, 0), (100, tp, 9, 3, (1 << 20) + 1, 0, 0), (100, tp, 9, 3, 2, 10 ** 6, 0),
                    (100, tp, 9, 3, 2, 0, (1 << 29) + 1)):
            assert new(*bad, C.byref(h)) == INVALID_ARG and not h.value, bad
        assert new(100, tp, 9, 3, 2, 0, 0, None) == INVALID_ARG
        new = getattr(lib, f"phast_planner_resample{sfx}_new")
        for bad in ((0, 5), (5, 0), ((1 << 29) + 1, 5), (5, (1 << 29) + 1)):
            assert new(*bad, C.byref(h)) == INVALID_ARG and not h.value, bad
        assert new(8, 5, None) == INVALID_ARG
        fs = "f64" if sfx == "64" else "f32"
        for name in (f"phast_upfirdn_{fs}_dev", f"phast_resample_{fs}_dev", f"phast_upfirdn_{fs}_with_planner", f"phast_resample_{fs}_with_planner"):
            fn = getattr(lib, name)
            args = [None] * len(fn.argtypes)
            for i, t in enumerate(fn.argtypes):
                if t is not C.c_void_p:
                    args[i] = 1
            assert fn(*args) == INVALID_ARG   # a null planner
        for name in ("out_len", "full_len", "tile", "chunk", "workspace_len", "device_bytes"):
            fn = getattr(lib, f"phast_planner_upfirdn{sfx}_{name}")
            assert fn(None, 1) == 0 if name == "workspace_len" else fn(None) == 0
        assert getattr(lib, f"phast_planner_resample{sfx}_workspace_min")(None) == 0


def test_python_argument_errors():
    import phastft_amd as P

    for name in ("PlannerUpfirdn64", "PlannerUpfirdn32", "PlannerResample64", "PlannerResample32", "upfirdn_batched", "resample_batched",
                 "upfirdn_64_with_planner", "upfirdn_32_with_planner", "resample_64_with_planner", "resample_32_with_planner", "upfirdn",
                 "resample_poly", "decimate", "resample"):
        assert name in P.__all__ and hasattr(P, name), name
    with pytest.raises(P.PhastPanic):
        P.PlannerUpfirdn64(100, np.ones(9), 0, 2)
    with pytest.raises(P.PhastPanic):
        P.PlannerResample32(0, 5)
    with pytest.raises(ValueError):
        P.resample_poly(np.zeros(8), 3, 2, padtype="line")
    with pytest.raises(ValueError):
        P.decimate(np.zeros(8), 2, ftype="iir")
    with pytest.raises(ValueError):
        P.decimate(np.zeros(8), 2, zero_phase=False)
    with pytest.raises(TypeError):
        P.resample(np.zeros(8), 4)   # host arrays go through the *_with_planner forms
    with pytest.raises(TypeError):
        P.upfirdn(np.ones(3), np.zeros(8))
