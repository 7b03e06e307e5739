"""Non-uniform FFTs of types 1 and 2 by the definition, in long double with exact phases, and a numpy model of
the library's schedule in double:

    type 1   F[m] = sum_j c_j exp(-+2 pi i k(m) x_j)        type 2   c_j = sum_m F[m] exp(-+2 pi i k(m) x_j)

k(m) = m for m < ceil(N / 2) and m - N otherwise, x_j in turns, - for Forward and + for Reverse.  The CPU reference of
tests/test_gpu_nufft.py, tests/test_nufft_cpu.py and tests/golden/make_nufft_error_budget.py.  The direct sum shares no code
with csrc/nufft.hpp: every x_j is reduced mod 1 exactly from the value of the double (fractions.Fraction) onto a 2^-128
grid (a point with bits below it, such as 1e-300, is cut towards zero there), the product k x_j is formed mod 1 in integers
on that grid, and only the reduced phase, cut to its top 64 bits, becomes a long double -- as tests/czt_reference.py does.
The integers are two uint64 limbs, so the sum stays vectorised; test_nufft_cpu.py holds them against Python's own."""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

LD = np.longdouble
TWO_PI = LD(8) * np.arctan(LD(1))
FORWARD, REVERSE = 0, 1

# (N, M, kind) of the GPU tests: uniform random points with the binning test's specials mixed in, or every point within 1e-7
# of 0.3 (the long-cell-list case)
SHAPES = [(1, 1, "u"), (2, 5, "u"), (7, 3, "u"), (16, 100, "u"), (101, 1000, "u"), (256, 37, "u"), (1000, 4096, "u"),
          (1000, 4096, "clump"), (4099, 2000, "u")]
EPS = {"f64": [1e-3, 1e-6, 1e-9, 1e-12, 1e-14], "f32": [1e-2, 1e-4, 1e-6]}
SEEDS = (0, 1)
SPECIALS = [0.0, 1 - 2.0 ** -53, -0.25, 7.5, 1e-300]


def modes(n: int):
    m = np.arange(n)
    return np.where(m < (n + 1) // 2, m, m - n)


def points(n: int, m: int, kind: str = "u"):
    """the M points of a shape, in turns (float64); the same for every seed, eps and type"""
    rng = np.random.default_rng([n, m, 29])
    if kind == "clump":
        return 0.3 + 1e-7 * rng.random(m)
    x = rng.uniform(-1.0, 2.0, m)
    k = min(m, len(SPECIALS)) if m >= 3 else 0
    x[:k] = SPECIALS[:k]
    return x


def data(count: int, seed: int, what: str):
    """complex uniform [-1, 1) values that are exact in float32, so that both dtypes share one reference"""
    rng = np.random.default_rng([seed, count, 31, 1 if what == "c" else 2])
    re = rng.uniform(-1, 1, count).astype(np.float32).astype(np.float64)
    im = rng.uniform(-1, 1, count).astype(np.float32).astype(np.float64)
    return re + 1j * im


# ---------------------------------------------------------------------------------------------
# the direct sum
# ---------------------------------------------------------------------------------------------
def limbs(x):
    """x mod 1 on the 2^-128 grid as (hi, lo) uint64 arrays, exact from the doubles (cut towards zero below the grid)"""
    hi, lo = np.empty(len(x), np.uint64), np.empty(len(x), np.uint64)
    for j, v in enumerate(x):
        f = int(Fraction(float(v)) % 1 * (1 << 128))
        hi[j], lo[j] = f >> 64, f & ((1 << 64) - 1)
    return hi, lo


def phase_top(k: int, hi, lo):
    """the top 64 bits of (|k| x mod 1) on the grid, for |k| < 2^31: uint64, wrapping"""
    k = np.uint64(abs(int(k)))
    l0, l1 = lo & np.uint64(0xFFFFFFFF), lo >> np.uint64(32)
    carry = ((k * l0 >> np.uint64(32)) + k * l1) >> np.uint64(32)   # floor(k lo / 2^64); every term < 2^64
    with np.errstate(over="ignore"):
        return k * hi + carry


def unit_row(k: int, hi, lo):
    """exp(-2 pi i k x_j) for every point as (cos, -sin) in long double"""
    t = phase_top(k, hi, lo).view(np.int64).astype(LD) * LD(2) ** -64   # the signed turn of |k| x in [-1/2, 1/2)
    a = TWO_PI * t
    c, s = np.cos(a), np.sin(a)
    return c, (-s if k >= 0 else s)


def direct(x, n: int, cs=(), fs=()):
    """Forward sums of both types in ONE pass over the frequencies k >= 0 (the row of -k is the conjugate of the row of k): cs
    are vectors of M point values, fs vectors of N mode values.  Returns ([F of every c], [c of every f]) as (re, im) pairs
    in long double."""
    hi, lo = limbs(x)
    m = len(x)
    cr = np.array([np.asarray(c).real for c in cs], LD).reshape(len(cs), m).T   # (M, a)
    ci = np.array([np.asarray(c).imag for c in cs], LD).reshape(len(cs), m).T
    fr = np.array([np.asarray(f).real for f in fs], LD).reshape(len(fs), n)     # (b, N)
    fi = np.array([np.asarray(f).imag for f in fs], LD).reshape(len(fs), n)
    o1_re, o1_im = np.zeros((n, len(cs)), LD), np.zeros((n, len(cs)), LD)
    o2_re, o2_im = np.zeros((m, len(fs)), LD), np.zeros((m, len(fs)), LD)
    for k in range(n // 2 + 1):
        e_re, e_im = unit_row(k, hi, lo)
        for i, sign in ((k, 1), (n - k, -1)):   # the mode indices of k and of -k
            if (sign == 1 and k >= (n + 1) // 2) or (sign == -1 and (k == 0 or i < (n + 1) // 2)):
                continue
            s_im = e_im if sign == 1 else -e_im
            o1_re[i] = e_re @ cr - s_im @ ci
            o1_im[i] = s_im @ cr + e_re @ ci
            o2_re += np.outer(e_re, fr[:, i]) - np.outer(s_im, fi[:, i])
            o2_im += np.outer(s_im, fr[:, i]) + np.outer(e_re, fi[:, i])
    return ([(o1_re[:, j], o1_im[:, j]) for j in range(len(cs))], [(o2_re[:, j], o2_im[:, j]) for j in range(len(fs))])


def nufft1(x, c, n: int, direction: int = FORWARD):
    """(re, im) in long double; Reverse is the conjugate of Forward on the conjugate data"""
    c = np.asarray(c, np.complex128)
    (re, im), = direct(x, n, cs=[c if direction == FORWARD else c.conj()])[0]
    return re, (im if direction == FORWARD else -im)


def nufft2(x, f, direction: int = FORWARD):
    f = np.asarray(f, np.complex128)
    (re, im), = direct(x, len(f), fs=[f if direction == FORWARD else f.conj()])[1]
    return re, (im if direction == FORWARD else -im)


class Reference:
    """every reference value of one shape, from one pass: ref[(type, direction, real, seed)] = (re, im) in float64.  Reverse
    is the conjugate of Forward on the conjugate data, and real data Re v = (v + conj v) / 2, so the pass carries v and
    conj v of every seed and nothing else."""

    def __init__(self, shape):
        n, m, kind = shape
        self.n, self.m, self.x = n, m, points(n, m, kind)
        self.c = {s: data(m, s, "c") for s in SEEDS}
        self.f = {s: data(n, s, "f") for s in SEEDS}
        cs = [v for s in SEEDS for v in (self.c[s], self.c[s].conj())]
        fs = [v for s in SEEDS for v in (self.f[s], self.f[s].conj())]
        o1, o2 = direct(self.x, n, cs, fs)
        self.ref = {}
        for t, o in ((1, o1), (2, o2)):
            for i, s in enumerate(SEEDS):
                (a_re, a_im), (b_re, b_im) = o[2 * i], o[2 * i + 1]   # Forward of v and of conj v
                self.ref[(t, FORWARD, False, s)] = (a_re.astype(np.float64), a_im.astype(np.float64))
                self.ref[(t, REVERSE, False, s)] = (b_re.astype(np.float64), (-b_im).astype(np.float64))
                h_re, h_im = (a_re + b_re) / 2, (a_im + b_im) / 2
                self.ref[(t, FORWARD, True, s)] = (h_re.astype(np.float64), h_im.astype(np.float64))
                self.ref[(t, REVERSE, True, s)] = (h_re.astype(np.float64), (-h_im).astype(np.float64))

    def inp(self, t: int, real: bool, seed: int):
        v = (self.c if t == 1 else self.f)[seed]
        return v.real.astype(np.complex128) if real else v


# ---------------------------------------------------------------------------------------------
# the schedule of csrc/nufft.hpp in numpy
# ---------------------------------------------------------------------------------------------
def width(eps: float) -> int:
    d = -math.log10(eps)
    if abs(d - round(d)) < 1e-9:
        d = round(d)
    return max(2, min(16, int(math.ceil(d)) + 1))


def grid(n: int, w: int) -> int:
    g = 8
    while g < 2 * n or g < 2 * w:
        g <<= 1
    return g


def phi(z, beta):
    z = np.asarray(z, np.float64)
    out = np.zeros_like(z)
    inside = np.abs(z) < 1
    out[inside] = np.exp(beta * (np.sqrt(1 - z[inside] ** 2) - 1))
    return out


def phi_hat(k, n_g: int, w: int, nodes: int = 32):
    """the Fourier transform of phi(2 t / w) at the grid frequencies k: Gauss-Legendre in theta, z = sin(theta)"""
    x, wt = np.polynomial.legendre.leggauss(nodes)
    th = (x + 1) * (np.pi / 4)
    f = w * (np.pi / 4) * wt * np.exp(2.30 * w * (np.cos(th) - 1)) * np.cos(th)
    return (f[None, :] * np.cos(np.outer(np.asarray(k, np.float64) * (np.pi * w / n_g), np.sin(th)))).sum(1)


def phi_hat_trapezoid(k, n_g: int, w: int, nodes: int = 4096):
    """the same integral by a `nodes`-point trapezoid sum after the tanh-sinh change of variable z = tanh(pi/2 sinh u), which
    takes the square-root ends of phi to infinity: 1 - z^2 = sech^2(pi/2 sinh u) is formed without cancellation"""
    u = np.linspace(-4.0, 4.0, nodes)
    v = (np.pi / 2) * np.sinh(u)
    z, sech = np.tanh(v), 1 / np.cosh(v)
    dz = (np.pi / 2) * np.cosh(u) * sech ** 2
    f = (w / 2) * np.exp(2.30 * w * (sech - 1)) * dz * (u[1] - u[0])
    return (f[None, :] * np.cos(np.outer(np.asarray(k, np.float64) * (np.pi * w / n_g), z))).sum(1)


def _cells(x, n_g):
    """(cell, offset) of every point, from the double the library keeps: x mod 1 cut to 53 significant bits"""
    p = np.array([_cut(v) for v in x]) * n_g
    q = np.floor(p)
    return q.astype(np.int64), p - q


def _cut(v: float) -> float:
    f = int(Fraction(float(v)) % 1 * (1 << 128))
    if f == 0:
        return 0.0
    drop = max(0, f.bit_length() - 53)
    return math.ldexp(float(f >> drop), drop - 128)


def model(t: int, x, v, n: int, eps: float, direction: int = FORWARD, dt=np.float64):
    """type t of the values v through spread / pre, numpy's FFT of n_g points and deconvolve / interpolate; `dt`: the
    arithmetic of the kernel values, the grid and the table (the FFT itself runs in double and is rounded)"""
    cd = np.complex128 if dt == np.float64 else np.complex64
    w = width(eps)
    n_g = grid(n, w)
    beta = 2.30 * w
    q, off = _cells(x, n_g)
    first = 1 - (w + 1) // 2 + ((w & 1) & (off >= 0.5))
    p = (1 / phi_hat(modes(n), n_g, w)).astype(dt)
    slot = modes(n) % n_g
    fft = (lambda a: np.fft.fft(a)) if direction == FORWARD else (lambda a: np.fft.ifft(a) * len(a))
    v = np.asarray(v).astype(cd)
    if t == 1:
        g = np.zeros(n_g, cd)
        for s in range(w):
            dq = first + s
            np.add.at(g, (q + dq) % n_g, phi((dq - off) * (2.0 / w), beta).astype(dt) * v)
        return (fft(g.astype(np.complex128)).astype(cd)[slot] * p).astype(cd)
    gh = np.zeros(n_g, cd)
    gh[slot] = v * p
    g = fft(gh.astype(np.complex128)).astype(cd)
    out = np.zeros(len(x), cd)
    for s in range(w):
        dq = first + s
        out += phi((dq - off) * (2.0 / w), beta).astype(dt) * g[(q + dq) % n_g]
    return out
