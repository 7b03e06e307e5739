"""The chirp-Z transform on the unit circle by the definition, in long double with exact phases:

    X[k] = sum_{n < N} x[n] exp(-2 pi i n (start + k step)),  k < M,   start and step in turns.

The CPU reference of tests/test_gpu_czt.py, tests/test_czt_cpu.py and tests/golden/make_czt_error_budget.py.  It shares no code
with csrc/czt.hpp: the phase n (start + k step) is reduced mod 1 in Python integers on a 2^-160 grid from the exact value of
the two doubles (fractions.Fraction), and only the reduced phase, cut to its top 64 bits, becomes a long double.  The sum is
vectorised over the longer of N and M."""
from __future__ import annotations

from fractions import Fraction

import numpy as np

GRID = 160
MOD = 1 << GRID
LD = np.longdouble
TWO_PI = LD(8) * np.arctan(LD(1))  # numpy.pi is a double


def turns(v: float) -> int:
    """v mod 1 on the 2^-160 grid, exact (raises where the double has bits below the grid)"""
    f = Fraction(float(v)) % 1 * MOD
    if f.denominator != 1:
        raise ValueError(f"{v!r} is not on the 2^-{GRID} grid")
    return int(f)


def unit(phase):
    """exp(-2 pi i p / 2^160) of an object array of Python integers in [0, 2^160), as (cos, -sin) in long double"""
    top = (phase >> (GRID - 64)).astype(np.uint64)           # 2^-64 turns: below the long double's last bit of an angle < pi
    t = top.view(np.int64).astype(LD) * LD(2) ** -64          # the signed turn in [-1/2, 1/2)
    a = TWO_PI * t
    return np.cos(a), -np.sin(a)


def czt(x, m: int, step: float, start: float = 0.0):
    """(re, im) of the M bins in long double; x real or complex, of any float type (taken as it is: round it first)"""
    x = np.asarray(x)
    n = x.shape[0]
    xr = x.real.astype(LD)
    xi = x.imag.astype(LD) if np.iscomplexobj(x) else None
    s, t = turns(start), turns(step)
    out_re, out_im = np.zeros(m, LD), np.zeros(m, LD)
    if n >= m:
        idx = np.arange(n).astype(object)
        for k in range(m):
            c, ms = unit(idx * ((s + k * t) % MOD) % MOD)
            out_re[k] = np.dot(xr, c) - (np.dot(xi, ms) if xi is not None else 0)
            out_im[k] = np.dot(xr, ms) + (np.dot(xi, c) if xi is not None else 0)
    else:
        idx = np.arange(m).astype(object)
        for j in range(n):
            c, ms = unit((j * s + idx * (j * t % MOD)) % MOD)
            out_re += xr[j] * c
            out_im += xr[j] * ms
            if xi is not None:
                out_re -= xi[j] * ms
                out_im += xi[j] * c
    return out_re, out_im


def signal(n: int, dtype=np.float64, seed: int = 0, real: bool = False):
    """uniform [-1, 1) planes rounded to `dtype`: (re, im), im None for a real signal"""
    rng = np.random.default_rng([seed, n, 17])
    re = rng.uniform(-1, 1, n).astype(dtype)
    im = None if real else rng.uniform(-1, 1, n).astype(dtype)
    return re, im


def zoom_params(fn, m: int, fs: float = 2.0, endpoint: bool = False):
    """(start, step) of scipy.signal.zoom_fft(x, fn, m, fs=fs, endpoint=endpoint)"""
    f1, f2 = (0.0, float(fn)) if np.ndim(fn) == 0 else (float(fn[0]), float(fn[1]))
    return f1 / fs, (f2 - f1) / (fs * ((m - 1) if endpoint else m))
