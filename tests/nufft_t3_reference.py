"""The non-uniform FFT of type 3 by the definition, in long double with exact phases:

    f_k = sum_j c_j exp(-+2 pi i s_k x_j),   j < M, k < K,   s_k x_j in turns, - for Forward and + for Reverse.

The CPU reference of tests/test_gpu_nufft_t3.py, tests/test_nufft_t3_cpu.py and tests/golden/make_nufft_t3_error_budget.py.  It
shares no code with csrc/nufft_t3.hpp: every double is taken as the exact ratio n / 2^a that it is (fractions.Fraction), the
product s_k x_j is formed in integers and reduced mod 1 there, and only the reduced phase, cut to its top 64 bits, becomes a
long double -- as tests/nufft_reference.py treats k x_j.  The integers are Python's own, in numpy object arrays."""
from __future__ import annotations

from fractions import Fraction

import numpy as np

from tests.nufft_reference import EPS, FORWARD, LD, REVERSE, SEEDS, TWO_PI, data  # noqa: F401  (shared with the callers)

# (M, K, X, S) of the GPU tests: the half-widths keep n_f <= 2^14
SHAPES = [(1, 1, 1.0, 1.0), (5, 3, 0.7, 3.0), (100, 37, 2.0, 8.0), (1000, 257, 0.5, 150.0), (4096, 1000, 3.0, 400.0)]
# the point sets: uniform; both centres off; the sources' centre far off; sources / targets clumped within 1e-7 of the
# half-width plus two outliers; all sources / all targets / both equal
KINDS = ["u", "off", "far", "xclump", "sclump", "xeq", "seq", "eq"]
# every shape uniform, the two middle shapes through every other set
CASES = [s + ("u",) for s in SHAPES] + [s + (k,) for s in SHAPES[2:4] for k in KINDS[1:]]
BIG = (1 << 16, 1 << 15, 4.0, 2040.0, "u")  # n_f = 2^16 at every eps; compared on BIG_PICK outputs
BIG_PICK = 64


def case_id(c):
    return f"{c[0]}x{c[1]}{c[4]}"


def _spread(rng, count, half, clump):
    if clump:
        v = half * (0.3 + 1e-7 * rng.random(count))
        v[:2] = [-half, half]
        return v
    v = rng.uniform(-half, half, count)
    if count >= 2:
        v[:2] = [-half, half]   # the half-widths are what the case says
    return v


def points(case):
    """(x, s) of a case as float64; the same for every seed, eps and direction"""
    m, k, X, S, kind = case
    rng = np.random.default_rng([m, k, 37])
    x = _spread(rng, m, X, kind == "xclump")
    s = _spread(rng, k, S, kind == "sclump")
    if kind == "off":
        x, s = x + 1000 * X, s - 300 * S
    if kind == "far":
        x = x + 1e6 * X
    if kind in ("xeq", "eq"):
        x = np.full(m, 0.37 * X)
    if kind in ("seq", "eq"):
        s = np.full(k, -0.81 * S)
    return x, s


def conditioning(x, s):
    """Q = 2 pi (|C_s| + S) X of the point sets as given (no degenerate replacement: X = 0 has Q = 0)"""
    cx, cs = (x.min() + x.max()) / 2, (s.min() + s.max()) / 2
    return 2 * np.pi * (abs(cs) + np.abs(s - cs).max()) * np.abs(x - cx).max()


def _ratio(v):
    """the doubles v as integers n over one power of two 2^a"""
    pairs = [Fraction(float(t)) for t in v]
    a = max(p.denominator.bit_length() - 1 for p in pairs)
    return np.array([p.numerator * ((1 << a) // p.denominator) for p in pairs], dtype=object), a


def turns(x, s_k, ratio=None):
    """s_k x_j mod 1 as the signed turn in [-1/2, 1/2) in long double, exact to the 2^-64 cut"""
    nx, ax = ratio if ratio is not None else _ratio(x)
    f = Fraction(float(s_k))
    a_s = f.denominator.bit_length() - 1
    a = ax + a_s
    prod = (nx * f.numerator) & ((1 << a) - 1)       # (n_x n_s) mod 2^a: Python's & of a negative integer is the residue
    top = (prod >> (a - 64)) if a >= 64 else (prod << (64 - a))
    return top.astype(np.uint64).view(np.int64).astype(LD) * LD(2) ** -64


def direct(x, s, cs, pick=None):
    """Forward sums of the vectors cs at the targets s (or at s[pick]): [(re, im)] in long double"""
    ratio = _ratio(x)
    cr = np.array([np.asarray(c).real for c in cs], LD).T   # (M, a)
    ci = np.array([np.asarray(c).imag for c in cs], LD).T
    ks = range(len(s)) if pick is None else pick
    o_re, o_im = np.zeros((len(ks), len(cs)), LD), np.zeros((len(ks), len(cs)), LD)
    for i, k in enumerate(ks):
        a = TWO_PI * turns(x, s[k], ratio)
        e_re, e_im = np.cos(a), -np.sin(a)
        o_re[i] = e_re @ cr - e_im @ ci
        o_im[i] = e_im @ cr + e_re @ ci
    return [(o_re[:, j], o_im[:, j]) for j in range(len(cs))]


def nufft3(x, s, c, direction: int = FORWARD):
    """(re, im) in long double; Reverse is the conjugate of Forward on the conjugate data"""
    c = np.asarray(c, np.complex128)
    (re, im), = direct(np.asarray(x, np.float64), np.asarray(s, np.float64), [c if direction == FORWARD else c.conj()])
    return re, (im if direction == FORWARD else -im)


class Reference:
    """every reference value of one case, from one pass: ref[(direction, real, seed)] = (re, im) in float64, as
    tests/nufft_reference.py builds them from v and conj v of every seed"""

    def __init__(self, case, pick=None):
        self.case = case
        self.x, self.s = points(case)
        self.q = conditioning(self.x, self.s)
        self.pick = pick
        self.c = {sd: data(case[0], sd, "c") for sd in SEEDS}
        out = direct(self.x, self.s, [v for sd in SEEDS for v in (self.c[sd], self.c[sd].conj())], pick)
        self.ref = {}
        for i, sd in enumerate(SEEDS):
            (a_re, a_im), (b_re, b_im) = out[2 * i], out[2 * i + 1]   # Forward of v and of conj v
            self.ref[(FORWARD, False, sd)] = (a_re.astype(np.float64), a_im.astype(np.float64))
            self.ref[(REVERSE, False, sd)] = (b_re.astype(np.float64), (-b_im).astype(np.float64))
            h_re, h_im = (a_re + b_re) / 2, (a_im + b_im) / 2
            self.ref[(FORWARD, True, sd)] = (h_re.astype(np.float64), h_im.astype(np.float64))
            self.ref[(REVERSE, True, sd)] = (h_re.astype(np.float64), (-h_im).astype(np.float64))

    def inp(self, real: bool, seed: int):
        v = self.c[seed]
        return v.real.astype(np.complex128) if real else v
