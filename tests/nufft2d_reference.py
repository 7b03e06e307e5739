"""Two-dimensional non-uniform FFTs of types 1 and 2 by the definition, in long double with exact phases, and a
numpy model of the library's schedule:

    type 1   F[m1, m2] = sum_j c_j exp(-+2 pi i (k1(m1) x_j + k2(m2) y_j))
    type 2   c_j = sum_{m1, m2} F[m1, m2] exp(-+2 pi i (k1(m1) x_j + k2(m2) y_j))

each axis in fftfreq order, (x_j, y_j) in turns, - for Forward and + for Reverse.  The CPU reference of
tests/test_gpu_nufft2d.py, tests/test_nufft2d_cpu.py and tests/golden/make_nufft2d_error_budget.py.  The direct sum shares no
code with csrc/: per axis the unit rows e1[m1, j] = exp(-2 pi i k1(m1) x_j) (N1 x M) and e2 (N2 x M) come from
tests/nufft_reference.py's limbs / unit_row, whose phases are exact mod 1, and the two are combined by matrix products in long
double:  F = (e1 * c) e2^T,   c = sum_m1 e1 * (F e2)."""
from __future__ import annotations

import numpy as np

from tests import nufft_reference as R1

LD = R1.LD
FORWARD, REVERSE = R1.FORWARD, R1.REVERSE
EPS, SEEDS, SPECIALS = R1.EPS, R1.SEEDS, R1.SPECIALS
width, grid, modes, data = R1.width, R1.grid, R1.modes, R1.data

# (N1, N2, M, kind) of the GPU tests: uniform random points in [-1, 2)^2 with the specials mixed in, or every point within 1e-7
# of (0.3, 0.7) (the long-cell-list case)
SHAPES = [(1, 1, 1, "u"), (2, 3, 5, "u"), (7, 5, 40, "u"), (16, 12, 300, "u"), (12, 40, 1000, "u"), (64, 1, 500, "u"),
          (1, 37, 200, "u"), (33, 20, 2000, "u"), (33, 20, 2000, "clump"), (130, 70, 3000, "u")]


def shape_id(s):
    return f"{s[0]}x{s[1]}x{s[2]}{'' if s[3] == 'u' else s[3]}"


def points(n1: int, n2: int, m: int, kind: str = "u"):
    """the M points of a shape as (x, y), in turns (float64); the same for every seed, eps and type.  The uniform sets start
    with SPECIALS in x and reversed SPECIALS in y, so supports wrap both ends of both axes"""
    rng = np.random.default_rng([n1, n2, m, 37])
    if kind == "clump":
        return 0.3 + 1e-7 * rng.random(m), 0.7 + 1e-7 * rng.random(m)
    x, y = rng.uniform(-1.0, 2.0, m), rng.uniform(-1.0, 2.0, m)
    k = min(m, len(SPECIALS)) if m >= 3 else 0
    x[:k] = SPECIALS[:k]
    y[:k] = SPECIALS[::-1][:k]
    return x, y


# ---------------------------------------------------------------------------------------------
# the direct sum
# ---------------------------------------------------------------------------------------------
def unit_rows(x, n: int):
    """(re, im) of e[m, j] = exp(-2 pi i k(m) x_j), (n, M) in long double"""
    hi, lo = R1.limbs(x)
    re, im = np.empty((n, len(x)), LD), np.empty((n, len(x)), LD)
    for i, k in enumerate(modes(n)):
        re[i], im[i] = R1.unit_row(int(k), hi, lo)
    return re, im


def _planes(vs, shape):
    re = np.array([np.asarray(v).real for v in vs], LD).reshape((len(vs),) + shape)
    im = np.array([np.asarray(v).imag for v in vs], LD).reshape((len(vs),) + shape)
    return re, im


def direct(x, y, n1: int, n2: int, cs=(), fs=()):
    """Forward sums of both types: cs are vectors of M point values, fs arrays of (N1, N2) mode values (or flat).  Returns
    ([F of every c], [c of every f]) as (re, im) pairs in long double, F flat in row-major order"""
    m = len(x)
    a_re, a_im = unit_rows(x, n1)      # (N1, M)
    b_re, b_im = unit_rows(y, n2)      # (N2, M)
    o1, o2 = [], []
    if len(cs):
        c_re, c_im = _planes(cs, (m,))
        for i in range(len(cs)):
            u_re, u_im = a_re * c_re[i] - a_im * c_im[i], a_re * c_im[i] + a_im * c_re[i]   # e1 * c, (N1, M)
            f_re, f_im = u_re @ b_re.T - u_im @ b_im.T, u_re @ b_im.T + u_im @ b_re.T       # (N1, N2)
            o1.append((f_re.reshape(-1), f_im.reshape(-1)))
    if len(fs):
        f_re, f_im = _planes(fs, (n1, n2))
        for i in range(len(fs)):
            v_re, v_im = f_re[i] @ b_re - f_im[i] @ b_im, f_re[i] @ b_im + f_im[i] @ b_re   # F e2, (N1, M)
            o2.append(((a_re * v_re - a_im * v_im).sum(0), (a_re * v_im + a_im * v_re).sum(0)))
    return o1, o2


def nufft2d1(x, y, c, n1: int, n2: int, direction: int = FORWARD):
    """(re, im) flat in long double; Reverse is the conjugate of Forward on the conjugate data"""
    c = np.asarray(c, np.complex128)
    (re, im), = direct(x, y, n1, n2, cs=[c if direction == FORWARD else c.conj()])[0]
    return re, (im if direction == FORWARD else -im)


def nufft2d2(x, y, f, n1: int, n2: int, direction: int = FORWARD):
    f = np.asarray(f, np.complex128)
    (re, im), = direct(x, y, n1, n2, fs=[f if direction == FORWARD else f.conj()])[1]
    return re, (im if direction == FORWARD else -im)


class Reference:
    """every reference value of one shape, from one pass: ref[(type, direction, real, seed)] = (re, im) in float64, mode-side
    values flat in row-major order.  Reverse is the conjugate of Forward on the conjugate data, and real data
    Re v = (v + conj v) / 2, so the pass carries v and conj v of every seed and nothing else."""

    def __init__(self, shape):
        n1, n2, m, kind = shape
        self.n1, self.n2, self.m = n1, n2, m
        self.x, self.y = points(n1, n2, m, kind)
        self.c = {s: data(m, s, "c") for s in SEEDS}
        self.f = {s: data(n1 * n2, s, "f") for s in SEEDS}
        cs = [v for s in SEEDS for v in (self.c[s], self.c[s].conj())]
        fs = [v for s in SEEDS for v in (self.f[s], self.f[s].conj())]
        o1, o2 = direct(self.x, self.y, n1, n2, cs, fs)
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
# the schedule of csrc/nufft_nd.hpp (D = 2) in numpy
# ---------------------------------------------------------------------------------------------
def model(t: int, x, y, v, n1: int, n2: int, eps: float, direction: int = FORWARD, dt=np.float64):
    """type t of the values v (flat) through spread / pre, numpy's 2-D FFT of the (g1, g2) grid and deconvolve / interpolate;
    `dt`: the arithmetic of the kernel values, their product, the grid and the tables (the FFT itself runs in double and is
    rounded).  Returns flat values"""
    cd = np.complex128 if dt == np.float64 else np.complex64
    w = width(eps)
    g1, g2 = grid(n1, w), grid(n2, w)
    beta = 2.30 * w
    q1, off1 = R1._cells(x, g1)
    q2, off2 = R1._cells(y, g2)
    first1 = 1 - (w + 1) // 2 + ((w & 1) & (off1 >= 0.5))
    first2 = 1 - (w + 1) // 2 + ((w & 1) & (off2 >= 0.5))
    p1 = (1 / R1.phi_hat(modes(n1), g1, w)).astype(dt)
    p2 = (1 / R1.phi_hat(modes(n2), g2, w)).astype(dt)
    slot1, slot2 = modes(n1) % g1, modes(n2) % g2
    fft = (lambda a: np.fft.fft2(a)) if direction == FORWARD else (lambda a: np.fft.ifft2(a) * a.size)
    v = np.asarray(v).astype(cd)
    k1 = [R1.phi((first1 + s - off1) * (2.0 / w), beta).astype(dt) for s in range(w)]
    k2 = [R1.phi((first2 + u - off2) * (2.0 / w), beta).astype(dt) for u in range(w)]
    if t == 1:
        g = np.zeros((g1, g2), cd)
        for s in range(w):
            for u in range(w):
                np.add.at(g, ((q1 + first1 + s) % g1, (q2 + first2 + u) % g2), (k1[s] * k2[u]).astype(dt) * v)
        gh = fft(g.astype(np.complex128)).astype(cd)
        return ((gh[np.ix_(slot1, slot2)] * p1[:, None]).astype(cd) * p2[None, :]).astype(cd).reshape(-1)
    gh = np.zeros((g1, g2), cd)
    gh[np.ix_(slot1, slot2)] = ((v.reshape(n1, n2) * p1[:, None]).astype(cd) * p2[None, :]).astype(cd)
    g = fft(gh.astype(np.complex128)).astype(cd)
    out = np.zeros(len(x), cd)
    for s in range(w):
        for u in range(w):
            out += (k1[s] * k2[u]).astype(dt) * g[(q1 + first1 + s) % g1, (q2 + first2 + u) % g2]
    return out
