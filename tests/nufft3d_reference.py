"""Three-dimensional non-uniform FFTs of types 1 and 2 by the definition, in long double with exact phases, and a
numpy model of the library's schedule:

    type 1   F[m1, m2, m3] = sum_j c_j exp(-+2 pi i (k1(m1) x_j + k2(m2) y_j + k3(m3) z_j))
    type 2   c_j = sum_m F[m1, m2, m3] exp(-+2 pi i (k1(m1) x_j + k2(m2) y_j + k3(m3) z_j))

each axis in fftfreq order, (x_j, y_j, z_j) in turns, - for Forward and + for Reverse.  The CPU reference of
tests/test_gpu_nufft3d.py, tests/test_nufft3d_cpu.py and tests/golden/make_nufft3d_error_budget.py.  The direct sum shares no
code with csrc/: per axis the unit rows e_i[m_i, j] = exp(-2 pi i k_i(m_i) coordinate_j) come from tests/nufft_reference.py's
limbs / unit_row, whose phases are exact mod 1, and the three are combined by contractions in long double:
F[a, b, c] = sum_j e1[a, j] (e2[b, j] (e3[c, j] c_j)),   c_j = sum_a e1[a, j] sum_b e2[b, j] sum_c e3[c, j] F[a, b, c]."""
from __future__ import annotations

import numpy as np

from tests import nufft_reference as R1

LD = R1.LD
FORWARD, REVERSE = R1.FORWARD, R1.REVERSE
EPS, SEEDS, SPECIALS = R1.EPS, R1.SEEDS, R1.SPECIALS
width, grid, modes, data = R1.width, R1.grid, R1.modes, R1.data

# (N1, N2, N3, M, kind) of the GPU tests: uniform random points in [-1, 2)^3 with the specials mixed in, or every point within
# 1e-7 of (0.3, 0.7, 0.55) (the long-cell-list case: one cell list that spans many LDS chunks of the spread kernel)
SHAPES = [(1, 1, 1, 1, "u"), (2, 3, 4, 5, "u"), (5, 7, 3, 40, "u"), (12, 10, 9, 300, "u"), (40, 1, 1, 200, "u"), (1, 37, 1, 200, "u"),
          (1, 1, 37, 200, "u"), (33, 20, 7, 2000, "u"), (33, 20, 7, 2000, "clump"), (70, 24, 10, 3000, "u")]


def shape_id(s):
    return f"{s[0]}x{s[1]}x{s[2]}x{s[3]}{'' if s[4] == 'u' else s[4]}"


def points(n1: int, n2: int, n3: int, m: int, kind: str = "u"):
    """the M points of a shape as (x, y, z), in turns (float64); the same for every seed, eps and type.  The uniform sets start
    with SPECIALS in x, reversed in y and rotated by two in z, so supports wrap both ends of every axis"""
    rng = np.random.default_rng([n1, n2, n3, m, 41])
    if kind == "clump":
        return 0.3 + 1e-7 * rng.random(m), 0.7 + 1e-7 * rng.random(m), 0.55 + 1e-7 * rng.random(m)
    x, y, z = rng.uniform(-1.0, 2.0, m), rng.uniform(-1.0, 2.0, m), rng.uniform(-1.0, 2.0, m)
    k = min(m, len(SPECIALS)) if m >= 3 else 0
    x[:k] = SPECIALS[:k]
    y[:k] = SPECIALS[::-1][:k]
    z[:k] = np.roll(SPECIALS, -2)[:k]
    return x, y, z


# ---------------------------------------------------------------------------------------------
# the direct sum
# ---------------------------------------------------------------------------------------------
def unit_rows(x, n: int):
    """e[m, j] = exp(-2 pi i k(m) x_j), (n, M), as a complex pair (re, im) in long double"""
    hi, lo = R1.limbs(x)
    re, im = np.empty((n, len(x)), LD), np.empty((n, len(x)), LD)
    for i, k in enumerate(modes(n)):
        re[i], im[i] = R1.unit_row(int(k), hi, lo)
    return re, im


def _mul(a, b):
    return a[0] * b[0] - a[1] * b[1], a[0] * b[1] + a[1] * b[0]


def _planes(v, shape):
    v = np.asarray(v)
    return v.real.astype(LD).reshape(shape), v.imag.astype(LD).reshape(shape)


def _contract(spec, a, b):
    """einsum of two complex pairs in long double"""
    e = lambda p, q: np.einsum(spec, p, q)
    return e(a[0], b[0]) - e(a[1], b[1]), e(a[0], b[1]) + e(a[1], b[0])


def direct(x, y, z, n1: int, n2: int, n3: int, cs=(), fs=()):
    """Forward sums of both types: cs are vectors of M point values, fs arrays of (N1, N2, N3) mode values (or flat).  Returns
    ([F of every c], [c of every f]) as (re, im) pairs in long double, F flat in row-major order"""
    m = len(x)
    e1, e2, e3 = unit_rows(x, n1), unit_rows(y, n2), unit_rows(z, n3)
    o1, o2 = [], []
    for c in cs:
        u = _mul(e3, _planes(c, (m,)))                                    # (N3, M)
        v = (e2[0][:, None, :], e2[1][:, None, :])
        v = _mul(v, (u[0][None, :, :], u[1][None, :, :]))                 # (N2, N3, M)
        f = _contract("aj,bcj->abc", e1, v)                               # (N1, N2, N3)
        o1.append((f[0].reshape(-1), f[1].reshape(-1)))
    for f in fs:
        u = _contract("abc,cj->abj", _planes(f, (n1, n2, n3)), e3)        # (N1, N2, M)
        v = _contract("abj,bj->aj", u, e2)                                # (N1, M)
        o2.append(_contract("aj,aj->j", v, e1))
    return o1, o2


def nufft3d1(x, y, z, c, n1: int, n2: int, n3: int, direction: int = FORWARD):
    """(re, im) flat in long double; Reverse is the conjugate of Forward on the conjugate data"""
    c = np.asarray(c, np.complex128)
    (re, im), = direct(x, y, z, n1, n2, n3, cs=[c if direction == FORWARD else c.conj()])[0]
    return re, (im if direction == FORWARD else -im)


def nufft3d2(x, y, z, f, n1: int, n2: int, n3: int, direction: int = FORWARD):
    f = np.asarray(f, np.complex128)
    (re, im), = direct(x, y, z, n1, n2, n3, fs=[f if direction == FORWARD else f.conj()])[1]
    return re, (im if direction == FORWARD else -im)


class Reference:
    """every reference value of one shape, from one pass: ref[(type, direction, real, seed)] = (re, im) in float64, mode-side
    values flat in row-major order.  Reverse is the conjugate of Forward on the conjugate data, and real data
    Re v = (v + conj v) / 2, so the pass carries v and conj v of every seed and nothing else."""

    def __init__(self, shape):
        n1, n2, n3, m, kind = shape
        self.n1, self.n2, self.n3, self.m = n1, n2, n3, m
        self.x, self.y, self.z = points(n1, n2, n3, m, kind)
        self.c = {s: data(m, s, "c") for s in SEEDS}
        self.f = {s: data(n1 * n2 * n3, s, "f") for s in SEEDS}
        cs = [v for s in SEEDS for v in (self.c[s], self.c[s].conj())]
        fs = [v for s in SEEDS for v in (self.f[s], self.f[s].conj())]
        o1, o2 = direct(self.x, self.y, self.z, n1, n2, n3, cs, fs)
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
# the schedule of csrc/nufft_nd.hpp (D = 3) in numpy
# ---------------------------------------------------------------------------------------------
def model(t: int, x, y, z, v, n1: int, n2: int, n3: int, eps: float, direction: int = FORWARD, dt=np.float64):
    """type t of the values v (flat) through spread / pre, numpy's 3-D FFT of the (g1, g2, g3) grid and deconvolve /
    interpolate; `dt`: the arithmetic of the kernel values, their product (k1 k2) k3, the grid and the tables (the FFT itself
    runs in double and is rounded).  Returns flat values"""
    cd = np.complex128 if dt == np.float64 else np.complex64
    w = width(eps)
    ns, gs = (n1, n2, n3), tuple(grid(n, w) for n in (n1, n2, n3))
    beta = 2.30 * w
    q, first, k, p, slot = [], [], [], [], []
    for pos, n, g in zip((x, y, z), ns, gs):
        qi, off = R1._cells(pos, g)
        fi = 1 - (w + 1) // 2 + ((w & 1) & (off >= 0.5))
        q.append(qi)
        first.append(fi)
        k.append([R1.phi((fi + s - off) * (2.0 / w), beta).astype(dt) for s in range(w)])
        p.append((1 / R1.phi_hat(modes(n), g, w)).astype(dt))
        slot.append(modes(n) % g)
    fft = (lambda a: np.fft.fftn(a)) if direction == FORWARD else (lambda a: np.fft.ifftn(a) * a.size)
    v = np.asarray(v).astype(cd)
    idx = [[(q[i] + first[i] + s) % gs[i] for s in range(w)] for i in range(3)]
    if t == 1:
        g = np.zeros(gs, cd)
        for s in range(w):
            for r in range(w):
                k12 = (k[0][s] * k[1][r]).astype(dt)
                for u in range(w):
                    np.add.at(g, (idx[0][s], idx[1][r], idx[2][u]), (k12 * k[2][u]).astype(dt) * v)
        gh = fft(g.astype(np.complex128)).astype(cd)[np.ix_(*slot)]
        gh = (gh * p[0][:, None, None]).astype(cd)
        gh = (gh * p[1][None, :, None]).astype(cd)
        return (gh * p[2][None, None, :]).astype(cd).reshape(-1)
    gh = np.zeros(gs, cd)
    f = (v.reshape(ns) * p[0][:, None, None]).astype(cd)
    f = (f * p[1][None, :, None]).astype(cd)
    gh[np.ix_(*slot)] = (f * p[2][None, None, :]).astype(cd)
    g = fft(gh.astype(np.complex128)).astype(cd)
    out = np.zeros(len(x), cd)
    for s in range(w):
        for r in range(w):
            k12 = (k[0][s] * k[1][r]).astype(dt)
            for u in range(w):
                out += (k12 * k[2][u]).astype(dt) * g[idx[0][s], idx[1][r], idx[2][u]]
    return out
