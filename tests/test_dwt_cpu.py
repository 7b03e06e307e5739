"""The host half of the discrete wavelet transform (csrc/dwt.hpp, csrc/planner_dwt.hpp, phastft_amd.wavelet_filters), without a
GPU:

    dwt.hpp compiled with g++: level lengths, offsets, a tile's run and the extension map against brute force for every
        L <= 12, F in {2, 4, 6, 8, 14}, J <= 4 and all six modes, and the LDS bounds of the tile;
    the long double reference (tests/dwt_reference.py): perfect reconstruction for haar and db2 .. db10 and the LeGall pair,
        the Haar known answer PyWavelets documents;
    the built-in filters: the db2 closed form, orthonormality sum_k h[k] h[k + 2q] = delta_q and sum h = sqrt 2 to 1e-13;
    dwt_max_level, dwt_coeff_lens, and every refusal of the C ABI and of the Python layer before the device is touched."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import dwt_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG = 16
NAMES = ["haar"] + [f"db{i}" for i in range(1, 11)]
FS = (2, 4, 6, 8, 14)


@pytest.fixture(scope="module")
def helpers(tmp_path_factory):
    so = tmp_path_factory.mktemp("dwt_helpers") / "libdwthelpers.so"
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-shared", "-fPIC", "-I", os.path.join(ROOT, "phastft_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "dwt_geom_test.cpp"), "-o", str(so)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    h = C.CDLL(str(so))
    u, i, ll, p = C.c_ulonglong, C.c_int, C.c_longlong, C.c_void_p
    h.dwt_t_level_len.argtypes, h.dwt_t_level_len.restype = [u, C.c_uint, i], u
    h.dwt_t_synth_len.argtypes, h.dwt_t_synth_len.restype = [u, C.c_uint, i], u
    h.dwt_t_max_level.argtypes, h.dwt_t_max_level.restype = [u, C.c_uint], C.c_uint
    h.dwt_t_ext_index.argtypes, h.dwt_t_ext_index.restype = [i, ll, ll], ll
    h.dwt_t_synth_index.argtypes, h.dwt_t_synth_index.restype = [i, ll, ll], ll
    h.dwt_t_bad_args.argtypes = [u, u, u, i]
    h.dwt_t_geom.argtypes = [u, C.c_uint, C.c_uint, i, p, p, p]
    h.dwt_t_analysis_span.argtypes = [u, u, C.c_uint, i, p, p]
    h.dwt_t_synth_pairs.argtypes = [u, C.c_uint, i, p, p]
    h.dwt_t_synth_span.argtypes = [ll, u, C.c_uint, p, p]
    h.dwt_t_shift.argtypes, h.dwt_t_shift.restype = [i, C.c_uint, i], ll
    h.dwt_t_const.argtypes, h.dwt_t_const.restype = [i], C.c_uint
    return h


def _brute_ext(mode, n, t):
    """ext(x, t) by walking the extended signal outwards from [0, n), one period at a time"""
    if mode == "zero":
        return t if 0 <= t < n else -1
    if mode == "constant":
        return min(max(t, 0), n - 1)
    if mode == "periodization":
        period = list(range(n)) + ([n - 1] if n % 2 else [])
    elif mode == "periodic":
        period = list(range(n))
    elif mode == "symmetric":
        period = list(range(n)) + list(range(n - 1, -1, -1))
    else:  # reflect: the end points are not repeated
        period = list(range(n)) + list(range(n - 2, 0, -1)) if n > 1 else [0]
    while t < 0:
        t += len(period)
    while t >= len(period):
        t -= len(period)
    return period[t]


def test_extension_map_against_brute_force(helpers):
    for mi, mode in enumerate(R.MODES):
        for n in range(1, 13):
            for t in range(-3 * 14 - 5, 3 * 14 + n + 5):
                want = _brute_ext(mode, n, t)
                assert helpers.dwt_t_ext_index(mi, n, t) == want, (mode, n, t)
                assert int(R.ext_index(mode, n, t)) == want, (mode, n, t)


def test_geometry_against_brute_force(helpers):
    h = helpers
    tile = h.dwt_t_const(0)
    assert (tile, h.dwt_t_const(1), h.dwt_t_const(2)) == (1024, 4, 1168)
    assert tile == 256 * h.dwt_t_const(1) and tile + h.dwt_t_const(3) // 2 - 1 <= h.dwt_t_const(2)   # the arrays hold the longest run
    n, off, rest = (C.c_ulonglong * 33)(), (C.c_ulonglong * 33)(), (C.c_ulonglong * 4)()
    lo, count, q_first = C.c_longlong(), C.c_ulonglong(), C.c_longlong()
    for mi, mode in enumerate(R.MODES):
        per = mode == "periodization"
        for f in FS:
            for L in range(1, 13):
                for J in range(1, 5):
                    h.dwt_t_geom(L, f, J, mi, n, off, rest)
                    # level lengths: count the coefficients whose taps the definitions name
                    lens = [L]
                    for _ in range(J):
                        prev = lens[-1]
                        lens.append(len(range(0, prev + prev % 2, 2)) if per else len([i for i in range(prev + f) if 2 * i + 1 - (f - 1) <= prev - 1]))
                    assert list(n[:J + 1]) == lens == R.level_lens(L, f, J, mode), (mode, f, L, J)
                    # the packed row: cA_J, cD_J, .., cD_1
                    at, offs = lens[J], {}
                    for l in range(J, 0, -1):
                        offs[l] = at
                        at += lens[l]
                    assert [off[l] for l in range(1, J + 1)] == [offs[l] for l in range(1, J + 1)] and off[0] == 0
                    assert rest[0] == at == sum(R.level_lens(L, f, J, mode)[1:]) + lens[J]
                    assert rest[1] == max([lens[l] for l in range(1, J) if l % 2], default=0)
                    assert rest[2] == max([lens[l] for l in range(1, J) if l % 2 == 0], default=0)
                    assert rest[3] == tile
                # a tile's run of the signal: the samples its coefficients' taps name, before the extension
                shift = f // 2 if per else 1
                assert h.dwt_t_shift(0, f, mi) == shift
                for i0 in (0, 3):
                    for cnt in (1, 2, 5):
                        h.dwt_t_analysis_span(i0, cnt, f, mi, C.byref(lo), C.byref(count))
                        named = [2 * i + shift - j for i in range(i0, i0 + cnt) for j in range(f)]
                        assert lo.value == min(named) and lo.value + count.value - 1 == max(named), (mode, f, i0, cnt)
                # the synthesis pairs of a level that keeps out_len samples, and a tile's run of the coefficients
                s = f // 2 - 1 if per else f - 2
                assert h.dwt_t_shift(1, f, mi) == s
                for out_len in range(1, 13):
                    h.dwt_t_synth_pairs(out_len, f, mi, C.byref(q_first), C.byref(count))
                    qs = sorted({(r + s) // 2 for r in range(out_len)})
                    assert (q_first.value, count.value) == (qs[0], len(qs)), (mode, f, out_len)
                    assert qs == list(range(qs[0], qs[0] + len(qs)))
                    pairs = count.value
                    h.dwt_t_synth_span(q_first.value, pairs, f, C.byref(lo), C.byref(count))
                    named = [(r + s - t) // 2 for r in range(2 * qs[0] - s, 2 * (qs[-1] + 1) - s) for t in range(f) if (r + s - t) % 2 == 0]
                    assert lo.value == min(named) and lo.value + count.value - 1 == max(named), (mode, f, out_len)
                    if not per:   # the extension modes never leave [0, m) for the samples a level keeps
                        m = (out_len + f - 1) // 2
                        assert lo.value >= 0 and lo.value + count.value <= m, (mode, f, out_len)
        for m in range(1, 8):
            for k in range(-20, 20):
                want = k % m if per else (k if 0 <= k < m else -1)
                assert h.dwt_t_synth_index(mi, m, k) == want


def test_synthesis_length_undoes_the_analysis_length(helpers):
    for mi, mode in enumerate(R.MODES):
        for f in FS + (256,):
            for n in list(range(1, 40)) + [4100, 1 << 29]:
                m = helpers.dwt_t_level_len(n, f, mi)
                assert helpers.dwt_t_synth_len(m, f, mi) in (n, n + 1), (mode, f, n)


def test_reference_reconstructs_perfectly():
    import phastft_amd as P

    rng = np.random.default_rng(5)
    banks = {name: P.wavelet_filters(name) for name in ["haar"] + [f"db{i}" for i in range(2, 11)]}
    banks["legall"] = R.legall53()
    for name, bank in banks.items():
        for L in (1, 2, 3, 5, 8, 9, 17, 40):
            for mode in R.MODES:
                for J in (1, 3):
                    x = rng.standard_normal(L)
                    coeffs = R.wavedec(x, bank, J, mode)
                    assert [c.size for c in coeffs] == P.dwt_coeff_lens(L, len(bank[0]), J, mode)
                    y = R.waverec(coeffs, bank, mode, L)
                    assert float(np.abs(y - x).max()) <= 2e-13, (name, L, mode, J)   # the taps are doubles: not exact


def test_haar_known_answer():
    import phastft_amd as P

    cA, cD = R.analysis_level(np.arange(1.0, 9.0), *P.wavelet_filters("haar")[:2], "symmetric")
    assert np.allclose(np.asarray(cA, float), [2.12132034, 4.94974747, 7.77817459, 10.60660172], atol=5e-9, rtol=0)
    assert np.allclose(np.asarray(cD, float), [-0.70710678] * 4, atol=5e-9, rtol=0)


def test_builtin_filters():
    import phastft_amd as P

    s3 = np.sqrt(3.0)
    dec_lo, dec_hi, rec_lo, rec_hi = P.wavelet_filters("db2")
    assert np.abs(rec_lo - np.array([1 + s3, 3 + s3, 3 - s3, 1 - s3]) / (4 * np.sqrt(2.0))).max() <= 1e-15
    assert np.array_equal(P.wavelet_filters("haar")[2], P.wavelet_filters("db1")[2])
    for name in NAMES:
        dec_lo, dec_hi, rec_lo, rec_hi = P.wavelet_filters(name)
        f = rec_lo.size
        assert f == 2 * (1 if name == "haar" else int(name[2:]))
        assert abs(rec_lo.sum() - np.sqrt(2.0)) <= 1e-13, name
        for q in range(f // 2):
            assert abs(np.dot(rec_lo[:f - 2 * q], rec_lo[2 * q:]) - (q == 0)) <= 1e-13, (name, q)
        assert np.array_equal(dec_lo, rec_lo[::-1]) and np.array_equal(dec_hi, rec_hi[::-1])
        assert np.array_equal(rec_hi, [(-1) ** k * rec_lo[f - 1 - k] for k in range(f)])
    for bad in ("db0", "db11", "sym4", "bior2.2", "", "dbx"):
        with pytest.raises(ValueError):
            P.wavelet_filters(bad)


def test_max_level_and_coeff_lens(helpers):
    import phastft_amd as P

    for f in (2, 4, 8, 20, 256):
        for L in list(range(1, 70)) + [1000, 4100, 1 << 20]:
            want = int(np.floor(np.log2(L / (f - 1)))) if L >= f - 1 else 0
            assert P.dwt_max_level(L, f) == want == helpers.dwt_t_max_level(L, f) == R.max_level(L, f), (L, f)
    assert P.dwt_max_level(1000, "db4") == 7 and P.dwt_max_level(1024, "haar") == 10
    assert P.dwt_coeff_lens(17, "db2", 3) == [4, 4, 6, 10] and P.dwt_coeff_lens(9, 4, 4, "zero") == [3, 3, 3, 4, 6]
    assert P.dwt_coeff_lens(17, 4, 3, "periodization") == [3, 3, 5, 9]
    for bad in (lambda: P.dwt_coeff_lens(0, 4), lambda: P.dwt_coeff_lens(8, 3), lambda: P.dwt_coeff_lens(8, 4, 0),
                lambda: P.dwt_coeff_lens(8, 4, 33), lambda: P.dwt_coeff_lens(8, 4, 1, "smooth"), lambda: P.dwt_max_level(0, 4)):
        with pytest.raises(ValueError):
            bad()


def test_every_refusal_comes_before_the_device(helpers):
    """header rules and the C ABI: the same answers, and no handle comes back"""
    from phastft_amd import _lib

    lib = _lib.lib()
    taps = {np.float64: np.ones(258, np.float64), np.float32: np.ones(258, np.float32)}
    cases = [(0, 4, 1, 2), ((1 << 29) + 1, 4, 1, 2), (16, 0, 1, 2), (16, 3, 1, 2), (16, 258, 1, 2), (16, 4, 0, 2), (16, 4, 33, 2),
             (16, 4, 1, -1), (16, 4, 1, 6), (16, 4, 1, 7)]
    for L, f, J, mode in cases:
        assert helpers.dwt_t_bad_args(L, f, J, mode) == 1, (L, f, J, mode)
        for sfx, dt in (("64", np.float64), ("32", np.float32)):
            ptr, h = taps[dt].ctypes.data_as(C.c_void_p), C.c_void_p(1)
            assert getattr(lib, f"phast_planner_dwt{sfx}_new")(L, ptr, ptr, ptr, ptr, f, J, mode, C.byref(h)) == INVALID_ARG
            assert not h.value
    for L, f, J, mode in [(1, 2, 1, 0), (1 << 29, 256, 32, 5), (5, 8, 4, 3)]:
        assert helpers.dwt_t_bad_args(L, f, J, mode) == 0
    ptr, h = taps[np.float64].ctypes.data_as(C.c_void_p), C.c_void_p(1)
    for hole in range(4):   # a null filter
        args = [ptr] * 4
        args[hole] = None
        assert lib.phast_planner_dwt64_new(16, *args, 4, 1, 2, C.byref(h)) == INVALID_ARG and not h.value
    assert lib.phast_planner_dwt64_new(16, ptr, ptr, ptr, ptr, 4, 1, 2, None) == INVALID_ARG
    # a null planner: codes and zeros, never a crash
    for sfx, fs in (("64", "f64"), ("32", "f32")):
        for name in ("workspace_len", "workspace_min", "coeff_len", "tile", "device_bytes"):
            fn = getattr(lib, f"phast_planner_dwt{sfx}_{name}")
            assert (fn(None, 1) if name == "workspace_len" else fn(None)) == 0
        assert getattr(lib, f"phast_planner_dwt{sfx}_level_len")(None, 1) == 0
        assert getattr(lib, f"phast_planner_dwt{sfx}_level_offset")(None, 1) == 0
        for name in ("wavedec", "waverec"):
            assert getattr(lib, f"phast_{name}_{fs}_dev")(ptr, ptr, 16, 1, 16, 16, None, None, 0, None) == INVALID_ARG
            assert getattr(lib, f"phast_{name}_{fs}_with_planner")(ptr, 16, ptr, 16, None) == INVALID_ARG


def test_python_refusals():
    import phastft_amd as P

    for mode in ("smooth", "antisymmetric", "antireflect", "sym", None, 2):
        with pytest.raises(ValueError):
            P.PlannerDwt64(16, "db2", 1, mode)
    with pytest.raises(ValueError):
        P.PlannerDwt64(16, "coif1")
    with pytest.raises(ValueError):
        P.PlannerDwt64(16, (np.ones(4), np.ones(4), np.ones(4)))            # three filters
    with pytest.raises(ValueError):
        P.PlannerDwt32(16, (np.ones(4), np.ones(4), np.ones(4), np.ones(6)))   # unequal lengths
    with pytest.raises(ValueError):
        P.PlannerDwt64(16, (np.ones(3),) * 4)                               # odd
    with pytest.raises(ValueError):
        P.PlannerDwt64(16, (np.ones(258),) * 4)                             # too long
    for level in (0, 33):
        with pytest.raises(P.PhastPanic):
            P.PlannerDwt64(16, "db2", level)
    with pytest.raises(P.PhastPanic):
        P.PlannerDwt32(0, "haar")
    with pytest.raises(ValueError):
        P.idwt(None, None, "haar")
    for name in ("PlannerDwt64", "PlannerDwt32", "wavedec_batched", "waverec_batched", "wavedec_64_with_planner", "wavedec_32_with_planner",
                 "waverec_64_with_planner", "waverec_32_with_planner", "dwt", "idwt", "wavedec", "waverec", "wavelet_filters",
                 "dwt_max_level", "dwt_coeff_lens"):
        assert name in P.__all__ and hasattr(P, name), name
