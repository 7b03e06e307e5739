"""The polyphase synthesis bank without a GPU (csrc/synthesizer.hpp):

    tests/synthesizer_reference.py -- the long double evaluation the GPU tests compare with -- against the definition summed
        term by term and against the scipy expression, s = sum_k exp(2 pi i k n / M) upfirdn(g, Y[:, k], D, 1), at double
        round-off for the eight small cases, real and complex;
    the perfect-reconstruction and adjoint identities that tie the bank to the channelizer, in numpy from the two references;
    synthesizer.hpp compiled with g++: full_len, m_lo, m_hi, the column and the tile geometry against brute force for every
        (F, K, M, D) with F, K <= 12 and M, D <= 7; every illegal argument;
    the C ABI's argument rules and exports, which need no device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import channelizer_reference as A
from tests import synthesizer_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG = 16
U = 2.0 ** -53


def test_reference_against_the_definition_and_scipy():
    """taps with a normal distribution.  The scipy expression sums up to ceil(K / D) products per channel and M channels per
    output in double with phases from a double angle below 2 pi (each within 14 u): (ceil(K / D) + M + 16) u sum_m |g| sum_k |Y|
    bounds it, and the polyphase form's 1 / M and once-rounded M g[j] add 3 u"""
    S = pytest.importorskip("scipy.signal")
    for case in R.SMALL_CASES:
        F, K, M, D = case
        g = np.random.default_rng([K, 6]).normal(size=K)
        full = R.full_len(F, K, D)
        n = np.arange(full)
        for real in (False, True):
            Y = R.frames(case, "f64", real)[0]
            Yf = R.hermitian_full(Y, M) if real else Y
            s, a, t, b = R.synth_ref(R.scaled_taps(g, M, "f64"), Y, M, D, real)
            assert s.shape == (full,) and (np.isrealobj(s) == real)
            scale = np.zeros(full)
            for m in range(F):
                scale[m * D:m * D + K] += np.abs(g) * float(np.sum(np.abs(Yf[m])))
            bound = (-(-K // D) + M + 19) * U * scale + 1e-300
            d = R.definition_ref(g, Yf, M, D)
            assert np.all(np.abs(s - d) <= bound), case
            want = sum(np.exp(2j * np.pi * ((k * n) % M) / M) * S.upfirdn(g, Yf[:, k].astype(np.complex128), D, 1) for k in range(M))
            assert want.shape == s.shape and np.all(np.abs(s - want) <= bound), (case, real)
            if real:  # a Hermitian Y gives a real s
                assert np.all(np.abs(d.imag) <= bound)
            # the count of terms is the header's, and an output without one is exactly zero
            assert all(t[i] == max(0, R.m_hi(i, F, D) - R.m_lo(i, K, D) + 1) for i in range(full))
            assert not np.any(s[t == 0])
            # a window is a slice of the whole, zeros past full_len
            w = R.synth_ref(R.scaled_taps(g, M, "f64"), Y, M, D, real, full + 2)[0]
            assert np.array_equal(w[:-2], s) and not w[-2:].any()


def test_perfect_reconstruction_with_the_sine_pair():
    """h[j] = sin(pi (j + 1/2) / M), K = M, D = M / 2, g = (0, h reversed) / M: synthesize(channelize(x)) is x delayed by M, and
    ~0 in front of and behind it"""
    for M, D in ((8, 4), (16, 8), (6, 3)):
        L = 5 * M + 3
        h = np.sin(np.pi * (np.arange(M) + 0.5) / M)
        g = np.concatenate(([0.0], h[::-1])) / M
        for cplx in (False, True):
            x = A.signals((L,), "f64", cplx)[0]
            y = A.channelize_ref(h, x, M, D)[0]
            s = R.synth_ref(R.scaled_taps(g, M, "f64"), y, M, D, not cplx)[0]
            assert s.size >= M + L
            assert float(np.max(np.abs(s[M:M + L] - x))) <= 1e-12, (M, D, cplx)
            assert float(np.max(np.abs(s[:M]))) <= 1e-12 and float(np.max(np.abs(s[M + L:]), initial=0.0)) <= 1e-12


def test_adjoint_of_the_channelizer():
    """K a multiple of M, g = (0, h reversed): <Y, A x> = <(S Y)[K : K + L], x> for the channelizer A with taps h and this
    synthesis S"""
    for L, K, M, D in ((37, 24, 8, 4), (50, 12, 6, 4), (41, 16, 8, 8)):
        h = A.taps(K, "f64")
        g = np.concatenate(([0.0], h[::-1]))
        x = A.signals((L,), "f64", True)[0]
        ax = A.channelize_ref(h, x, M, D)[0]
        rng = np.random.default_rng([L, K, 7])
        Y = rng.uniform(-1, 1, ax.shape) + 1j * rng.uniform(-1, 1, ax.shape)
        s = R.synth_ref(R.scaled_taps(g, M, "f64"), Y, M, D, False, K + L)[0]
        lhs, rhs = np.sum(np.conj(Y) * ax), np.sum(np.conj(s[K:K + L]) * x)
        assert abs(lhs - rhs) <= 1e-12 * abs(lhs), (L, K, M, D, lhs, rhs)


# ---- synthesizer.hpp with g++ ----
@pytest.fixture(scope="module")
def helpers(tmp_path_factory):
    so = tmp_path_factory.mktemp("synthesizer_helpers") / "libsynthesizerhelpers.so"
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-shared", "-fPIC", "-I", os.path.join(ROOT, "phastft_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "synthesizer_geom_test.cpp"), "-o", str(so)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    h = C.CDLL(str(so))
    u, p = C.c_ulonglong, C.c_void_p
    h.sy_t_full_len.restype = h.sy_t_m_lo.restype = h.sy_t_col.restype = u
    h.sy_t_m_hi.restype = C.c_longlong
    h.sy_t_full_len.argtypes = h.sy_t_m_lo.argtypes = h.sy_t_m_hi.argtypes = [u] * 3
    h.sy_t_col.argtypes = [u] * 2
    h.sy_t_geom.argtypes = [u, u, u, p]
    h.sy_t_bad_args.argtypes = [u] * 6
    h.sy_t_const.restype = C.c_uint
    return h


def _geom(h, K, M, D):
    out = (C.c_uint * 8)()
    h.sy_t_geom(K, M, D, out)
    return tuple(out)


def test_geometry_against_brute_force(helpers):
    """per (F, K, M, D): the samples that hold a term, the frames of every sample and its column -- the one whose phase
    exp(2 pi i k n / M) the row of v carries -- and the steps the kernel takes from one of a thread's samples to its next"""
    h = helpers
    for D in range(1, 8):
        for K in range(1, 13):
            for F in range(1, 13):
                terms = {}
                for m in range(F):
                    for j in range(K):
                        terms.setdefault(m * D + j, []).append(m)
                full = max(terms) + 1
                assert h.sy_t_full_len(F, K, D) == full == R.full_len(F, K, D), (F, K, D)
                for n in range(full + 3):
                    lo, hi = h.sy_t_m_lo(n, K, D), h.sy_t_m_hi(n, F, D)
                    assert (lo, hi) == (R.m_lo(n, K, D), R.m_hi(n, F, D))
                    assert list(range(lo, hi + 1)) == terms.get(n, []), (F, K, D, n)
            for M in range(1, 8):
                tile, per, most, sq, sr, sm, kq, kr = g = _geom(h, K, M, D)
                assert g == R.geom(K, M, D)
                assert most == max(len([m for m in range(12) if 0 <= n - m * D < K]) for n in range(12 * D + K))
                for n in range(0, 40):
                    assert h.sy_t_col(n, M) == n % M
                    # the steps: floor, remainder and column of n + 256 from those of n, and m_lo from floor and remainder
                    q, r, c = n // D, n % D, n % M
                    q2, r2, c2 = q + sq, r + sr, c + sm
                    if r2 >= D:
                        q2, r2 = q2 + 1, r2 - D
                    if c2 >= M:
                        c2 -= M
                    assert (q2, r2, c2) == ((n + 256) // D, (n + 256) % D, (n + 256) % M)
                    assert max(0, q - kq - (1 if r < kr else 0) + 1) == R.m_lo(n, K, D)


def test_the_schedule_matches_the_model(helpers):
    h = helpers
    assert (h.sy_t_const(0), h.sy_t_const(1)) == (R.PER_THREAD, R.TILE) and R.TILE == 256 * R.PER_THREAD
    shapes = [c[1:] for c in R.CASES] + [(k, m, d) for m in (1, 2, 3, 7, 64, 100, 255, 256, 257, 1000, 4096, 1 << 29)
                                         for d in (1, 3, m, 2 * m + 1, 5000, 1 << 29) for k in (1, m, 8 * m + 3, 1 << 29) if k <= 1 << 29]
    for K, M, D in shapes:
        assert _geom(h, K, M, D) == R.geom(K, M, D), (K, M, D)


def test_illegal_arguments_are_refused(helpers):
    h = helpers
    ok = (10, 9, 4, 4, 0, 0)   # full_len 45
    big = (1 << 29) + 1
    assert h.sy_t_bad_args(*ok) == 0
    assert h.sy_t_bad_args(1 << 29, 1 << 29, 1, 1 << 29, 0, 1 << 30) == 0 and h.sy_t_bad_args(10, 9, 4, 4, 45, 5) == 0  # first = full_len
    assert h.sy_t_bad_args(1 << 10, 9, 1 << 20, 4, 0, 0) == 0   # F M = 2^30
    for bad in ((0, 9, 4, 4, 0, 0), (big, 9, 1, 4, 0, 0), (10, 0, 4, 4, 0, 0), (10, big, 4, 4, 0, 0), (10, 9, 0, 4, 0, 0),
                (10, 9, big, 4, 0, 0), (10, 9, 4, 0, 0, 0), (10, 9, 4, big, 0, 0), (10, 9, 4, 4, 46, 1), (10, 9, 4, 4, 45, 0),
                ((1 << 10) + 1, 9, 1 << 20, 4, 0, 0), (10, 9, 4, 4, 0, (1 << 30) + 1), (1 << 29, 9, 1, 4, 0, 0)):
        assert h.sy_t_bad_args(*bad) == 1, bad


# ---- the C ABI before the device is touched ----
def test_argument_codes_and_exports_without_a_device():
    from phastft_amd import _lib

    lib = _lib.lib()
    for sfx, ndt in (("64", np.float64), ("32", np.float32)):
        taps = np.ones(9, ndt)
        tp = taps.ctypes.data_as(C.c_void_p)
        h = C.c_void_p()
        new = getattr(lib, f"phast_planner_synthesizer{sfx}_new")
        big = (1 << 29) + 1
        for bad in ((0, tp, 9, 4, 4, 0, 0, 0), (10, None, 9, 4, 4, 0, 0, 0), (10, tp, 0, 4, 4, 0, 0, 1), (10, tp, 9, 0, 4, 0, 0, 0),
                    (10, tp, 9, 4, 0, 0, 0, 1), (10, tp, 9, big, 4, 0, 0, 0), (10, tp, 9, 4, big, 0, 0, 0), (10, tp, 9, 4, 4, 46, 0, 0),
                    (10, tp, 9, 4, 4, 45, 0, 1), (2048, tp, 9, 1 << 20, 4, 0, 0, 0), (10, tp, 9, 4, 4, 0, (1 << 30) + 1, 1)):
            assert new(*bad, C.byref(h)) == INVALID_ARG and not h.value, bad
        assert new(10, tp, 9, 4, 4, 0, 0, 0, None) == INVALID_ARG
        fs = "f64" if sfx == "64" else "f32"
        for name in (f"phast_synthesize_{fs}_dev", f"phast_synthesize_{fs}_with_planner", f"phast_planner_synthesizer{sfx}_time_stages"):
            fn = getattr(lib, name)
            args = [None] * len(fn.argtypes)
            for i, t in enumerate(fn.argtypes):
                if t is not C.c_void_p:
                    args[i] = 1
            assert fn(*args) == INVALID_ARG   # a null planner
        for name in ("out_len", "full_len", "bins", "tile_samples", "per_thread", "max_terms", "workspace_min", "workspace_len",
                     "device_bytes"):
            fn = getattr(lib, f"phast_planner_synthesizer{sfx}_{name}")
            assert fn(None, 1) == 0 if name == "workspace_len" else fn(None) == 0


def test_python_argument_errors():
    import phastft_amd as P

    for name in ("PlannerSynthesizer64", "PlannerSynthesizer32", "synthesize_batched", "synthesize_64_with_planner",
                 "synthesize_32_with_planner", "synthesize_poly"):
        assert name in P.__all__ and hasattr(P, name), name
    with pytest.raises(P.PhastPanic):
        P.PlannerSynthesizer64(10, np.ones(9), 0)
    with pytest.raises(P.PhastPanic):
        P.PlannerSynthesizer32(10, np.ones(9), 4, 0)
    with pytest.raises(TypeError):
        P.synthesize_poly(np.zeros((3, 4), np.complex128), np.ones(3), 4)   # host arrays go through the *_with_planner forms
