"""czt_frac (csrc/czt.hpp) and nufft_turns (csrc/nufft.hpp) are plain arithmetic on the bits of the double, so that the host's
nufft_bin and the device's sort (csrc/nufft_sort.hip) share one statement of "x mod 1".  Compiled with plain g++ -- no GPU, no
HIP -- and held against a big-integer statement (fractions.Fraction, as tests/nufft_reference.py reduces its points):

    czt_frac(v, down)   |v| / 2^down truncated onto the 2^-128 grid, mod 1; a negative v as the two's complement, so a negative
                        value below 2^-128 is cut to 0
    nufft_turns(f)      f truncated to its 53 leading significant bits, never rounded: always below 1

on the edge list of the device-point tests (signed zeros, subnormals, -2^-130, -2^-60, 1 - 2^-53, +-1, 0.25, 0.5, +-(2^52 + 0.5),
+-1e300, q / n_g with its two neighbours), on powers of two across the whole exponent range and on random doubles."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = 1 << 128


def edge_list(log_g):
    g = float(1 << log_g)
    e = [0.0, -0.0, 5e-324, -5e-324, -2.0 ** -130, -2.0 ** -60, 1.0 - 2.0 ** -53, 1.0, -1.0, 0.25, 0.5, 2.0 ** 52 + 0.5, -(2.0 ** 52 + 0.5),
         1e300, -1e300]
    for q in (1.0, 2.0, g / 2, g - 1):
        v = q / g
        e += [v, float(np.nextafter(v, -1.0)), float(np.nextafter(v, 2.0))]
    return e


def points():
    rng = np.random.default_rng(22)
    pts = [v for log_g in (3, 9, 20, 29) for v in edge_list(log_g)]
    pts += [s * 2.0 ** e for e in range(-1074, 1024, 7) for s in (1.0, -1.0)]
    pts += [s * (2.0 ** e) * (1 + 2.0 ** -52) for e in range(-140, 70) for s in (1.0, -1.0)]
    pts += [float(v) for v in rng.uniform(-3, 3, 400)]
    pts += [float(v) for v in rng.standard_normal(200) * 10.0 ** rng.integers(-45, 20, 200)]
    pts += [float(np.ldexp(v, -int(k))) for v, k in zip(rng.uniform(-1, 1, 200), rng.integers(60, 140, 200))]
    return pts


def frac_of(v, down):
    """the big-integer statement: the numerator over 2^128"""
    a = int(abs(Fraction(v)) / (1 << down) * ONE) % ONE  # int() truncates
    return (ONE - a) % ONE if v < 0 else a


def turns_of(t):
    if t == 0:
        return 0.0
    drop = max(t.bit_length() - 53, 0)
    return float(Fraction((t >> drop) << drop, ONE))  # 53 bits: the conversion is exact


@pytest.fixture(scope="module")
def helpers(tmp_path_factory):
    so = tmp_path_factory.mktemp("nufft_frac") / "libnufftfrac.so"
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-shared", "-fPIC", "-I", os.path.join(ROOT, "phastft_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "nufft_frac_test.cpp"), "-o", str(so)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    h = C.CDLL(str(so))
    h.frac_t_frac.argtypes, h.frac_t_frac.restype = [C.c_double, C.c_int, C.c_void_p, C.c_void_p], None
    h.frac_t_turns.argtypes, h.frac_t_turns.restype = [C.c_double], C.c_double
    h.frac_t_turns_of.argtypes, h.frac_t_turns_of.restype = [C.c_ulonglong, C.c_ulonglong], C.c_double
    return h


@pytest.mark.parametrize("down", [0, 1])
def test_the_fraction_is_the_big_integer_statement(helpers, down):
    hi, lo = C.c_ulonglong(), C.c_ulonglong()
    for v in points():
        helpers.frac_t_frac(v, down, C.byref(hi), C.byref(lo))
        assert (hi.value << 64) | lo.value == frac_of(v, down), (v.hex(), down)


def test_the_position_is_the_truncated_fraction(helpers):
    for v in points():
        got = helpers.frac_t_turns(v)
        assert got.hex() == turns_of(frac_of(v, 0)).hex(), v.hex()
        assert 0.0 <= got < 1.0
    # -2^-60 lands in the last cell at 1 - 2^-53, -2^-130 is cut to 0, and the signed zeros and subnormals are 0
    assert helpers.frac_t_turns(-2.0 ** -60) == 1.0 - 2.0 ** -53
    for v in (-2.0 ** -130, 0.0, -0.0, 5e-324, -5e-324):
        assert helpers.frac_t_turns(v) == 0.0 and np.signbit(helpers.frac_t_turns(v)) == 0


def test_the_position_of_any_fraction_word(helpers):
    """fractions no double gives: all ones, one bit, a low word only"""
    rng = np.random.default_rng(5)
    words = [(0, 0), (0, 1), (1, 0), (2 ** 64 - 1, 2 ** 64 - 1), (0, 2 ** 64 - 1), (2 ** 63, 1), (1, 2 ** 63), (2 ** 11 - 1, 2 ** 64 - 1)]
    words += [(int(a) >> int(s), int(b)) for a, b, s in zip(rng.integers(0, 2 ** 64, 300, dtype=np.uint64),
                                                           rng.integers(0, 2 ** 64, 300, dtype=np.uint64), rng.integers(0, 65, 300))]
    for hi, lo in words:
        hi &= 2 ** 64 - 1
        assert helpers.frac_t_turns_of(hi, lo).hex() == turns_of((hi << 64) | lo).hex(), (hi, lo)
