"""CPU checks of the continuous wavelet transform (csrc/cwt.hpp), none of which needs a device:

    tests/cwt_reference.py (the definition in long double, direct sums) against independent anchors: scipy.signal.hilbert for
        the STEP family, the time-domain Morlet and Mexican hat for the impulse responses, a unit sinusoid at the centre
        frequency for the PEAK norm, the closed-form maxima against a fine grid, linearity, real against complex input;
    cwt.hpp compiled with g++: tiles, scale groups, rows per chunk and the workspace need against brute force for every
        L <= P <= 12 and S <= 9, the constants and gains against the reference, every illegal argument;
    the Python conveniences cwt_scales and cwt_fourier_period against their formulas;
    the C ABI's argument rules, which come back before the device is touched."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest
import scipy.signal

from tests import cwt_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAM = {"morlet": 0, "paul": 1, "dog": 2, "step": 3}
NORM = {"l2": 0, "peak": 1}


# ---- the reference against independent anchors ----
@pytest.mark.parametrize("L,P", [(7, 7), (8, 8), (7, 12), (8, 11)])
def test_step_is_scipys_hilbert(L, P):
    x = R.signal(L, 1)
    got = R.cwt(x, [1.0], "step", P=P)[0].astype(np.complex128)
    want = scipy.signal.hilbert(x, N=P)[:L]
    assert np.max(np.abs(got - want)) <= 1e-15   # measured 2e-16
    both = R.cwt(x, [0.3, 5.0], "step", norm="peak", P=P)   # no scale, no norm
    assert np.array_equal(both[0], both[1]) and np.array_equal(both[0].astype(np.complex128), got)


def _impulse(P, n0):
    x = np.zeros(P)
    x[n0] = 1.0
    return x


def test_morlet_impulse_response_is_the_time_domain_wavelet():
    """W = s^(-1/2) psi0((n - n0) / s), psi0(t) = pi^(-1/4) exp(i w0 t) exp(-t^2 / 2), up to the mass exp(-w0^2 / 2) = 1.5e-8 that
    the Heaviside factor cuts off (measured 2.4e-10)"""
    P, n0, s, w0 = 1024, 500, 20.0, 6.0
    got = R.cwt(_impulse(P, n0), [s], "morlet", w0, "l2")[0].astype(np.complex128)
    t = (np.arange(P) - n0) / s
    want = math.pi ** -0.25 * np.exp(1j * w0 * t) * np.exp(-t * t / 2) / math.sqrt(s)
    assert np.max(np.abs(got - want)) <= math.exp(-w0 * w0 / 2)


def test_dog2_impulse_response_is_the_mexican_hat():
    P, n0, s = 1024, 500, 20.0
    got = R.cwt(_impulse(P, n0), [s], "dog", 2, "l2")[0].astype(np.complex128)
    t = (np.arange(P) - n0) / s
    want = -(t * t - 1) * np.exp(-t * t / 2) / math.sqrt(math.gamma(2.5) * s)
    assert np.max(np.abs(got.real - want)) <= 1e-14   # measured 8e-17
    assert np.max(np.abs(got.imag)) <= 1e-16


@pytest.mark.parametrize("family,param", [("morlet", 6.0), ("paul", 4)])
def test_peak_norm_gives_unit_modulus_at_the_centre_frequency(family, param):
    """cos(2 pi 0.05 n): the negative-frequency leak is exp(-72) and the edges are more than 70 widths away"""
    L, f = 4096, 0.05
    x = np.cos(2 * math.pi * f * np.arange(L))
    s = (param if family == "morlet" else float(param)) / (2 * math.pi * f)
    w = R.cwt_fft(x, [s], family, param, "peak")[0]
    assert np.max(np.abs(np.abs(w[1500:2500]) - 1)) <= 1e-9   # measured 1.4e-11 (Paul)


@pytest.mark.parametrize("family,param", [("morlet", 6.0), ("morlet", 4.5), ("paul", 1), ("paul", 4), ("paul", 85), ("dog", 1), ("dog", 2),
                                          ("dog", 6), ("dog", 170)])
def test_closed_form_maxima_against_a_fine_grid(family, param):
    top = {"morlet": param, "paul": float(param), "dog": math.sqrt(param)}[family]
    x = np.linspace(top * 0.9, top * 1.1, 200001).astype(R.LD)
    grid = np.max(np.abs(R.psi_hat(family, param, x)))
    assert abs(grid / R.peak(family, param) - 1) <= 1e-11


def test_linearity_and_the_two_input_kinds():
    L, P = 20, 24
    sc = [0.7, 2.0, 5.0]
    a, b = R.signal(L, 1, True), R.signal(L, 2, True)
    for family in R.FAMILIES:
        wa, wb = R.cwt(a, sc, family, P=P), R.cwt(b, sc, family, P=P)
        wab = R.cwt(2 * a - 3j * b, sc, family, P=P)
        assert np.max(np.abs(wab - (2 * wa - R.CLD(3j) * wb))) <= 1e-17 * 50
        x = R.signal(L, 3)
        assert np.array_equal(R.cwt(x, sc, family, P=P), R.cwt(x + 0j, sc, family, P=P))
    # a real wavelet of a real signal is real (even m) or imaginary-free up to the unit factor
    w = R.cwt(R.signal(L, 3), sc, "dog", 2, P=P)
    assert np.max(np.abs(w.imag)) <= 1e-18
    # conj(-(i^1)) = i times an odd real filter: real again, where the bins pair up (an odd P: for an even one the bin P / 2
    # counts as positive and has no partner)
    w = R.cwt(R.signal(L, 3), sc, "dog", 1, P=P - 1)
    assert np.max(np.abs(w.imag)) <= 1e-18


def test_no_reference_row_of_the_gpu_cases_is_zero():
    """... except where it must be: with P = 1 the only bin is k = 0, where every family but STEP is 0"""
    for L, P, S in R.SHAPES:
        sc = R.case_scales(L, S)
        assert len(sc) == S and np.all(sc > 0)
        if L > 2:
            assert sc[0] < 1
        for family in R.FAMILIES:
            for cplx in (False, True):
                if P > 300 and (family != "morlet" or cplx):
                    continue   # the long case once: the rows' norms depend on the filter's support, not on the data
                w = R.cwt(R.signal(L, 0, cplx), sc, family, P=P)
                norms = np.sqrt(np.sum(np.abs(w) ** 2, axis=1))
                if P == 1 and family != "step":
                    assert np.all(norms == 0)
                else:
                    assert np.all(norms > 1e-8), (L, P, S, family, norms)


# ---- cwt.hpp with g++ ----
@pytest.fixture(scope="module")
def helpers(tmp_path_factory):
    so = tmp_path_factory.mktemp("cwt_helpers") / "libcwthelpers.so"
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-shared", "-fPIC", "-I", os.path.join(ROOT, "phastft_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "cwt_geom_test.cpp"), "-o", str(so)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    h = C.CDLL(str(so))
    u, d, i = C.c_ulonglong, C.c_double, C.c_int
    for name, args, res in (("geom", [u, u, i, C.c_uint, C.c_void_p], None), ("first_signal", [u, u], u), ("signals", [u, u, u], u),
                            ("max_signals", [u, u, u], u), ("first_group", [u, u, u], u), ("groups", [u, u, u, u], u),
                            ("need", [u, u, u, u, u, C.c_uint], u), ("rows_per_chunk", [u, u, u, u, u, u, C.c_uint], u),
                            ("signed_bin", [u, u], C.c_longlong), ("step_gain", [u, u], d), ("bad_args", [u, u, u, i, d, i], i),
                            ("bad_scale", [d], i), ("family_const", [i, d], d), ("family_peak", [i, d], d), ("gain", [i, d, i, d], d),
                            ("group_const", [], C.c_uint)):
        f = getattr(h, "cw_t_" + name)
        f.argtypes, f.restype = args, res
    return h


def test_geometry_against_brute_force(helpers):
    h = helpers
    G = h.cw_t_group_const()
    assert G == 8
    for esz, V in ((8, 2), (4, 4)):
        for P in range(1, 13):
            for S in range(1, 10):
                for real in (0, 1):
                    out = (C.c_ulonglong * 8)()
                    h.cw_t_geom(P, S, real, esz, out)
                    v, tile, group, tiles, ngrp, bins, xd, rd = out
                    assert (v, tile, group) == (V, 256 * V, G)
                    assert tiles == len(range(0, P, tile)) and ngrp == len(range(0, S, G))
                    assert bins == (P // 2 + 1 if real else P)
                    assert xd >= bins and xd % V == 0 and xd - bins < V and rd >= P and rd % V == 0 and rd - P < V
        for k in range(13):
            for P in range(max(1, k + 1), 13):
                assert h.cw_t_signed_bin(k, P) == (k if k <= P // 2 else k - P)
                want = 1.0 if k == 0 or 2 * k == P else 2.0 if 2 * k < P else 0.0
                assert h.cw_t_step_gain(k, P) == want == float(R.step_gain(P)[k])
    # rows, chunks and the workspace: every start and length of a chunk in calls of up to 3 signals
    for S in range(1, 10):
        ngrp = -(-S // G)
        for batch in (1, 2, 3):
            total = batch * S
            groups_of = [(row // S) * ngrp + (row % S) // G for row in range(total)]
            for r in range(1, total + 1):
                worst = 0
                for row0 in range(0, total - r + 1):
                    sigs = sorted({row // S for row in range(row0, row0 + r)})
                    assert h.cw_t_first_signal(row0, S) == sigs[0] and h.cw_t_signals(row0, r, S) == len(sigs)
                    grp = sorted({groups_of[row] for row in range(row0, row0 + r)})
                    assert h.cw_t_first_group(row0, S, ngrp) == grp[0] and h.cw_t_groups(row0, r, S, ngrp) == len(grp)
                    assert grp == list(range(grp[0], grp[0] + len(grp)))   # a launch covers consecutive groups
                    worst = max(worst, len(sigs))
                bound = h.cw_t_max_signals(r, S, batch)
                assert worst <= bound <= batch
                if batch == 3 and r <= S:   # ... and the bound is met wherever a chunk can start at any row
                    assert bound == min(batch, max(len({row // S for row in range(o, o + r)}) for o in range(S)))
                for sig_per, row_per, V in ((10, 0, 2), (24, 16, 2), (7, 36, 4)):
                    assert h.cw_t_need(r, S, batch, sig_per, row_per, V) == bound * sig_per + r * row_per + V - 1
            for sig_per, row_per, V in ((10, 0, 2), (24, 16, 2), (7, 36, 4)):
                needs = [h.cw_t_need(r, S, batch, sig_per, row_per, V) for r in range(1, total + 1)]
                assert needs == sorted(needs)
                for length in range(0, needs[-1] + 3):
                    fits = [r for r in range(1, total + 1) if needs[r - 1] <= length]
                    assert h.cw_t_rows_per_chunk(length, total, S, batch, sig_per, row_per, V) == (fits[-1] if fits else 0)


def test_constants_and_gains_match_the_reference(helpers):
    h = helpers
    for family, params in (("morlet", (6.0, 4.5, 12.0)), ("paul", (1, 2, 4, 20, 85)), ("dog", (1, 2, 3, 4, 6, 40, 170))):
        for param in params:
            assert abs(h.cw_t_family_const(FAM[family], param) / float(R.family_const(family, param)) - 1) <= 4e-16
            assert abs(h.cw_t_family_peak(FAM[family], param) / float(R.peak(family, param)) - 1) <= 4e-16
            for s in (0.3, 2.0, 77.7):
                for norm in R.NORMS:
                    c = np.sqrt(2 * R.PI * R.LD(s)) if norm == "l2" else 2 / R.peak(family, param)
                    want = float(c * R.family_const(family, param))
                    got = h.cw_t_gain(FAM[family], param, NORM[norm], s)
                    assert math.isfinite(got) and got > 0 and abs(got / want - 1) <= 4e-16, (family, param, norm, s)
    assert h.cw_t_gain(3, 0.0, 1, 5.0) == 1.0


def test_illegal_arguments_are_refused(helpers):
    h = helpers
    ok = (8, 8, 3, 0, 6.0, 0)
    assert h.cw_t_bad_args(*ok) == 0
    assert h.cw_t_bad_args(8, 1 << 29, 1 << 20, 3, 0.0, 1) == 0
    assert h.cw_t_bad_args(8, 12, 1, 1, 85.0, 1) == 0 and h.cw_t_bad_args(8, 12, 1, 2, 170.0, 1) == 0
    for bad in ((0, 8, 3, 0, 6.0, 0), (8, 7, 3, 0, 6.0, 0), (8, (1 << 29) + 1, 3, 0, 6.0, 0), (8, 8, 0, 0, 6.0, 0),
                (8, 8, (1 << 20) + 1, 0, 6.0, 0), (8, 8, 3, 4, 6.0, 0), (8, 8, 3, -1, 6.0, 0), (8, 8, 3, 0, 6.0, 2), (8, 8, 3, 0, 6.0, -1),
                (8, 8, 3, 0, 0.0, 0), (8, 8, 3, 0, -1.0, 0), (8, 8, 3, 0, float("nan"), 0), (8, 8, 3, 0, float("inf"), 0),
                (8, 8, 3, 1, 0.0, 0), (8, 8, 3, 1, 2.5, 0), (8, 8, 3, 1, 86.0, 0), (8, 8, 3, 1, float("nan"), 0),
                (8, 8, 3, 2, 0.0, 0), (8, 8, 3, 2, 1.5, 0), (8, 8, 3, 2, 171.0, 0), (8, 8, 3, 3, 0.0, 2)):
        assert h.cw_t_bad_args(*bad) == 1, bad
    for s in (1e-300, 0.5, 1.0, 1e300):
        assert h.cw_t_bad_scale(s) == 0
    for s in (0.0, -0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        assert h.cw_t_bad_scale(s) == 1, s


# ---- the Python conveniences ----
def test_cwt_scales_and_fourier_period():
    import phastft_amd as P

    sc = P.cwt_scales(1000)
    J = math.floor(math.log2(1000 / 2.0) / 0.25)
    assert sc.dtype == np.float64 and len(sc) == J + 1 == 36
    assert np.allclose(sc, [2.0 * 2 ** (j * 0.25) for j in range(J + 1)], rtol=1e-15)
    assert sc[-1] <= 1000 < sc[-1] * 2 ** 0.25
    sc = P.cwt_scales(64, s0=1.5, dj=0.5, J=4)
    assert np.allclose(sc, 1.5 * 2 ** (0.5 * np.arange(5)), rtol=1e-15)
    for bad in (dict(L=1), dict(L=8, s0=0.0), dict(L=8, dj=0.0), dict(L=0)):
        with pytest.raises(ValueError):
            P.cwt_scales(**bad)
    assert P.cwt_fourier_period() == pytest.approx(4 * math.pi / (6 + math.sqrt(38)), rel=1e-15)   # 1.033 (Torrence & Compo)
    assert P.cwt_fourier_period("morlet", 5.0) == pytest.approx(4 * math.pi / (5 + math.sqrt(27)), rel=1e-15)
    assert P.cwt_fourier_period("paul") == pytest.approx(4 * math.pi / 9, rel=1e-15)
    assert P.cwt_fourier_period("paul", 2) == pytest.approx(4 * math.pi / 5, rel=1e-15)
    assert P.cwt_fourier_period("dog") == pytest.approx(2 * math.pi / math.sqrt(2.5), rel=1e-15)
    assert P.cwt_fourier_period("dog", 6) == pytest.approx(2 * math.pi / math.sqrt(6.5), rel=1e-15)
    with pytest.raises(ValueError):
        P.cwt_fourier_period("step")
    with pytest.raises(ValueError):
        P.cwt_fourier_period("haar")


# ---- the C ABI without a device ----
def test_new_refuses_bad_arguments_before_the_device_is_touched():
    from phastft_amd import _lib

    lib = _lib.lib()
    sc = (C.c_double * 3)(1.0, 2.0, 4.0)
    for sfx in ("64", "32"):
        new = getattr(lib, f"phast_planner_cwt{sfx}_new")
        h = C.c_void_p()
        for args in ((0, 0, sc, 3, 0, 6.0, 0, 1), (8, 7, sc, 3, 0, 6.0, 0, 1), (8, 8, None, 3, 0, 6.0, 0, 1), (8, 8, sc, 0, 0, 6.0, 0, 1),
                     (8, 8, sc, 3, 9, 6.0, 0, 1), (8, 8, sc, 3, 0, 6.0, 7, 1), (8, 8, sc, 3, 1, 2.5, 0, 1), (8, 8, sc, 3, 2, 171.0, 0, 0),
                     (8, (1 << 29) + 1, sc, 3, 0, 6.0, 0, 1)):
            assert new(*args, C.byref(h)) == 16 and not h.value, args   # PHAST_ERR_INVALID_ARG, not a device error
        for bad in (0.0, -2.0, float("nan"), float("inf")):
            sb = (C.c_double * 3)(1.0, bad, 4.0)
            assert new(8, 8, sb, 3, 0, 6.0, 0, 1, C.byref(h)) == 16 and not h.value, bad
        assert new(8, 8, sc, 3, 0, 6.0, 0, 1, None) == 16
        for name in ("workspace_min", "pad_len", "num_scales", "tile_bins", "scale_group", "device_bytes"):
            assert getattr(lib, f"phast_planner_cwt{sfx}_{name}")(None) == 0
        assert getattr(lib, f"phast_cwt_{sfx}_dev")(None, None, None, None, 8, 1, 8, 24, None, None, 0, None) == 16
        assert getattr(lib, f"phast_cwt_{sfx}_with_planner")(None, None, 8, None, None, 24, None) == 16


def test_python_refuses_unknown_names():
    import phastft_amd as P

    with pytest.raises(ValueError):
        P.PlannerCwt64(8, [1.0], "haar")
    with pytest.raises(ValueError):
        P.PlannerCwt64(8, [1.0], "morlet", norm="l1")
