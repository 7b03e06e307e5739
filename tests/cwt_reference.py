"""The continuous wavelet transform of csrc/cwt.hpp by its definition, in numpy.longdouble: direct O(P^2) sums with the phase
k n reduced mod P in integers (P <= 512), the wavelets by Torrence & Compo's (1998) frequency-domain formulas with their
constants as exact products.  tests/test_cwt_cpu.py checks it against independent anchors (scipy.signal.hilbert, the
time-domain Morlet and Mexican hat, the peak normalisation on a sinusoid, the closed-form maxima); the GPU tests compare the
library with it.

    X[k]    = sum_n x[n] exp(-2 pi i k n / P)                    (x zero-extended from L to P points)
    w_k     = 2 pi k / P for k <= P div 2, 2 pi (k - P) / P above
    W[j, n] = 1/P sum_k X[k] conj(c_j psi0^(s_j w_k)) exp(+2 pi i k n / P),   n < L
"""
import numpy as np

LD = np.longdouble
CLD = np.clongdouble
PI = LD(2) * np.arccos(LD(0))
MAX_P = 1024  # the GPU cases stay at P <= 512; the impulse-response anchors take 1024

FAMILIES = ("morlet", "paul", "dog", "step")
NORMS = ("l2", "peak")
DEFAULTS = {"morlet": 6.0, "paul": 4.0, "dog": 2.0, "step": 0.0}


def family_const(family, param):
    """the constant in front of the family's H(x) x^m exp(..), as an exact product in long double"""
    if family == "morlet":
        return PI ** LD(-0.25)
    if family == "paul":
        m = int(param)
        fact = LD(1)
        for i in range(2, 2 * m):
            fact *= i  # (2m - 1)!
        return LD(2) ** m / np.sqrt(m * fact)
    if family == "dog":
        m = int(param)
        gam = np.sqrt(PI)  # Gamma(m + 1/2) = sqrt(pi) prod_{i < m} (i + 1/2)
        for i in range(m):
            gam *= LD(i) + LD(0.5)
        return 1 / np.sqrt(gam)
    return LD(1)


def bare(family, param, x):
    """H(x) x^m exp(..) of real long-double x, without constant and unit factor"""
    x = np.asarray(x, LD)
    if family == "morlet":
        return np.where(x > 0, np.exp(-((x - LD(param)) ** 2) / 2), LD(0))
    if family == "paul":
        m = int(param)
        xp = np.where(x > 0, x, LD(1))
        return np.where(x > 0, xp ** m * np.exp(-xp), LD(0))
    if family == "dog":
        return x ** int(param) * np.exp(-(x * x) / 2)
    raise ValueError(family)


def psi_hat(family, param, x):
    """psi0^(x) of the definition, complex long double"""
    if family == "dog":
        unit = -(CLD(1j) ** (int(param) % 4))
        return unit * (family_const(family, param) * bare(family, param, x)).astype(CLD)
    return (family_const(family, param) * bare(family, param, x)).astype(CLD)


def peak(family, param):
    """max_x |psi0^(x)| in closed form"""
    if family == "morlet":
        return family_const(family, param)
    m = LD(param)
    if family == "paul":
        return family_const(family, param) * m ** int(param) * np.exp(-m)
    if family == "dog":
        return family_const(family, param) * np.exp((m / 2) * (np.log(m) - 1))
    raise ValueError(family)


def omega(P):
    k = np.arange(P)
    kk = np.where(k <= P // 2, k, k - P)
    return 2 * PI * kk.astype(LD) / LD(P)


def step_gain(P):
    k = np.arange(P)
    g = np.where(2 * k < P, 2.0, 0.0)
    g[0] = 1.0
    if P % 2 == 0:
        g[P // 2] = 1.0
    return g.astype(LD)


def filters(P, scales, family="morlet", param=None, norm="l2"):
    """conj(c_j psi0^(s_j w_k)), shape (S, P), complex long double"""
    param = DEFAULTS[family] if param is None else param
    scales = np.asarray(scales, np.float64)
    if family == "step":
        return np.tile(step_gain(P).astype(CLD), (len(scales), 1))
    w = omega(P)
    rows = []
    for s in scales:
        s = LD(s)
        c = np.sqrt(2 * PI * s) if norm == "l2" else 2 / peak(family, param)
        rows.append(np.conj(c * psi_hat(family, param, s * w)))
    return np.array(rows, dtype=CLD)


def _twiddles(P):
    q = np.arange(P)
    ang = 2 * PI * q.astype(LD) / LD(P)
    return np.cos(ang) + CLD(1j) * np.sin(ang)


def dft(x, P, sign):
    """sum_n x[n] exp(sign 2 pi i k n / P) for k < P, x zero-extended to P points: direct sums, exact phases"""
    x = np.asarray(x, CLD)
    tw = _twiddles(P)
    if sign < 0:
        tw = np.conj(tw)
    idx = (np.arange(P)[:, None] * np.arange(len(x))[None, :]) % P
    return (tw[idx] * x[None, :]).sum(axis=1)


def cwt(x, scales, family="morlet", param=None, norm="l2", P=None):
    """W of the definition for one signal x of L points: complex long double, shape (S, L)"""
    x = np.asarray(x)
    L = len(x)
    P = L if P is None else P
    assert L <= P <= MAX_P
    X = dft(x, P, -1)
    Y = filters(P, scales, family, param, norm) * X[None, :]
    return np.array([dft(row, P, +1)[:L] / LD(P) for row in Y], dtype=CLD)


def cwt_fft(x, scales, family="morlet", param=None, norm="l2", P=None):
    """the same W in double through numpy's FFT with the long-double filters rounded once: for anchors at lengths the direct
    sums cannot reach (the FFT's own error, some 1e-15, is far below what those anchors gate)"""
    x = np.asarray(x)
    L = len(x)
    P = L if P is None else P
    F = filters(P, scales, family, param, norm).astype(np.complex128)
    return np.fft.ifft(np.fft.fft(x, P)[None, :] * F, axis=1)[:, :L]


def inner_log2(P):
    """the log2 the gates of tests/tolerances.py take: of the inner power-of-two transform of the P-point complex transform"""
    m = P if P & (P - 1) == 0 else 1 << (2 * P - 2).bit_length()
    return m.bit_length() - 1


def signal(L, seed, complex_input=False):
    """uniform [-1, 1) values that are exact in f32, so that one reference serves both types"""
    rng = np.random.default_rng(1000 * L + seed)
    x = rng.uniform(-1, 1, L).astype(np.float32).astype(np.float64)
    if complex_input:
        return x + 1j * rng.uniform(-1, 1, L).astype(np.float32).astype(np.float64)
    return x


# (L, P, S) of the GPU parity cases; scales: the dyadic ones clipped to S entries with one below 1 for L >= 7, explicit for L <= 2
SHAPES = ((1, 1, 1), (2, 2, 2), (7, 7, 3), (8, 8, 3), (100, 128, 5), (100, 131, 5), (257, 257, 9), (300, 512, 17))


def case_scales(L, S):
    if L == 1:
        return np.array([0.75])
    if L == 2:
        return np.array([0.75, 1.5])
    s0, dj = 2.0, 0.25
    J = int(np.floor(np.log2(L / s0) / dj))
    full = s0 * 2.0 ** (dj * np.arange(J + 1))
    return np.concatenate(([0.6], full[:S - 1]))
