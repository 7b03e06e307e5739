"""References for the polyphase synthesis bank (csrc/synthesizer.hpp) in long double, the cases the tests
share, the gates and a numpy model of the header's geometry.  A plain helper, not a test.

    scaled_taps     tab[j] = M g[j], the product in double, rounded once to T: what the planner keeps on the device
    rows_ref        v[m][p] = (1 / M) sum_k Y[m, k] exp(2 pi i k p / M) in long double; real output by irfft's rules
    synth_ref       s[n] = sum_m tab[n - m D] v[m][n mod M] over n < reach in long double, with A[n] = sum |tab v|, the number of
                    terms t(n) and B[n] = sum_m |tab[n - m D]| rms(v[m]) (the scales of the gates)
    definition_ref  s[n] = sum_m g[n - m D] sum_k Y[m, k] exp(2 pi i k n / M) term by term, for the small cases
                    (test_synthesizer_cpu.py holds the two together and both against scipy)
    geom            synth_geom of synthesizer.hpp
"""
import functools
import math

import numpy as np

from tests import tolerances as tol
from tests.resample_reference import LD, NDT, U, inner_m, taps  # noqa: F401  (shared generators)

CLD = np.clongdouble
PER_THREAD, TILE = 4, 1024  # the constants of csrc/synthesizer.hpp
PI = LD(np.pi) + LD(1.2246467991473532e-16)  # np.pi is a double: long double's pi is that plus the next term of its expansion

# (F, K, M, D)
SMALL_CASES = [
    (1, 1, 1, 1),
    (5, 24, 8, 8),     # critically sampled
    (7, 25, 8, 4),     # oversampled; K - 1 a multiple of M, the column rotation alternates
    (6, 21, 6, 4),     # M no power of two
    (4, 50, 7, 3),     # K > F D, prime M, D coprime to M
    (5, 5, 8, 8),      # outputs with no term at all: zeros
    (6, 32, 8, 12),    # D > M
    (9, 4, 3, 1),
]
CASES = SMALL_CASES + [
    (4, 1030, 257, 257),      # Bluestein inside, one column past 256
    (14, 2048, 256, 192),
    (6, 4100, 1024, 1024),
    (2200, 8200, 4, 4),       # 2050 terms per output
]
BATCH = 3


def case_id(c):
    return "x".join(str(v) for v in c)


def full_len(F, K, D):
    return (F - 1) * D + K


def m_lo(n, K, D):
    return max(0, -(-(n - K + 1) // D))


def m_hi(n, F, D):
    return min(F - 1, n // D)


def geom(K, M, D):
    """synth_geom: (tile, per, terms, sq, sr, sm, kq, kr)"""
    return TILE, PER_THREAD, -(-K // D), 256 // D, 256 % D, 256 % M, K // D, K % D


def windows(case):
    """(first, out_len): the whole result, and from sample 3 on (or the last legal first) one tile less one sample, one tile,
    one tile and a sample, and a window that passes full_len by two"""
    F, K, M, D = case
    full = full_len(F, K, D)
    first = min(3, full)
    out = [(0, None)] + [(first, n) for n in (TILE - 1, TILE, TILE + 1, full - first + 2) if n >= 1]
    return list(dict.fromkeys(out))


def reach(case):
    F, K, M, D = case
    full = full_len(F, K, D)
    return max(first + (n if n is not None else full - first) for first, n in windows(case))


def scaled_taps(g, M, dt):
    return (np.asarray(g, NDT[dt]).astype(np.float64) * float(M)).astype(NDT[dt])


@functools.lru_cache(maxsize=8)
def phases(M, bins):
    """W[k][p] = exp(+2 pi i k p / M) in long double, the angle from k p mod M"""
    kp = (np.arange(bins, dtype=np.int64)[:, None] * np.arange(M, dtype=np.int64)[None, :]) % M
    ang = 2 * PI * kp.astype(LD) / LD(M)
    w = np.empty(ang.shape, CLD)
    w.real, w.imag = np.cos(ang), np.sin(ang)
    return w


def rows_ref(Y, M, real):
    """v[m][p] with the 1 / M of the engine's inverse, in long double.  real: Y holds the M // 2 + 1 bins of the Hermitian half;
    the imaginary parts of bin 0 and (even M) of bin M / 2 are ignored, as irfft does"""
    Y = np.asarray(Y).astype(CLD)
    if not real:
        return (Y @ phases(M, M)) / LD(M)
    bins = M // 2 + 1
    assert Y.shape[1] == bins
    wt = np.full(bins, LD(2))
    wt[0] = 1
    Yh = Y.copy()
    Yh.imag[:, 0] = 0
    if M % 2 == 0:
        wt[-1] = 1
        Yh.imag[:, -1] = 0
    return ((Yh * wt[None, :]) @ phases(M, bins)).real / LD(M)


def synth_ref(tab, Y, M, D, real, n_out=None):
    """(s, a, t, b) on 0 <= n < n_out (default full_len; zeros at and beyond full_len) in long double from the values as given"""
    tab = np.asarray(tab).astype(LD)
    F, K = np.asarray(Y).shape[0], tab.size
    full = full_len(F, K, D)
    n_out = full if n_out is None else n_out
    size = max(full, n_out)
    v = rows_ref(Y, M, real)
    rms = np.sqrt(np.mean(np.abs(v) ** 2, axis=1)).astype(LD)
    s = np.zeros(size, LD if real else CLD)
    a, b, t = np.zeros(size, LD), np.zeros(size, LD), np.zeros(size, np.int64)
    j = np.arange(K, dtype=np.int64)
    at = np.abs(tab)
    for m in range(F):
        row = v[m][(m * D + j) % M]
        sl = slice(m * D, m * D + K)
        s[sl] += tab * row
        a[sl] += at * np.abs(row)
        b[sl] += at * rms[m]
        t[sl] += 1
    return s[:n_out], a[:n_out], t[:n_out], b[:n_out]


def hermitian_full(Y, M):
    """the M bins of a real signal's frames from its M // 2 + 1, by irfft's rules"""
    Y = np.asarray(Y).astype(CLD).copy()
    Y.imag[:, 0] = 0
    if M % 2 == 0:
        Y.imag[:, -1] = 0
    k = np.arange(M // 2 + 1, M)
    return np.concatenate([Y, np.conj(Y[:, M - k])], axis=1)


def definition_ref(g, Y, M, D):
    """s[n] for n < full_len term by term: sum_m g[n - m D] sum_k Y[m, k] exp(2 pi i k n / M), Y with all M bins"""
    g, Y = np.asarray(g).astype(LD), np.asarray(Y).astype(CLD)
    F, K = Y.shape[0], g.size
    k = np.arange(M, dtype=np.int64)
    s = np.zeros(full_len(F, K, D), CLD)
    for n in range(s.size):
        ang = 2 * PI * ((k * n) % M).astype(LD) / LD(M)
        w = np.cos(ang) + 1j * np.sin(ang)
        for m in range(F):
            if 0 <= n - m * D < K:
                s[n] += g[n - m * D] * np.sum(Y[m] * w)
    return s


def log2_inner(M):
    """the log2 the Fourier gates use: M, or the inner Bluestein length where M is no power of two"""
    return math.log2(inner_m(M)) if M > 1 else 0.0


def gates(dt, M, a, t, b):
    """(per-output gate, the two L2 terms): a chain of t products on the once-rounded scaled taps obeys |error| <= (t + 3) u A[n];
    the transform's error enters through bin_gate (rel_gate in L2) relative to the rms of a row of v, carried through
    B[n] = sum_m |tab[n - m D]| rms(v[m]).  M = 1: no transform."""
    lg = log2_inner(M)
    chain = (t + 3) * U[dt] * a.astype(np.float64)
    bw = b.astype(np.float64)
    out = chain + (tol.bin_gate(dt, lg) * bw if M > 1 else 0.0)
    l2 = float(np.sqrt(np.sum(chain ** 2))) + (tol.rel_gate(dt, lg) * float(np.sqrt(np.sum(bw ** 2))) if M > 1 else 0.0)
    return out, l2


def check(tag, dt, M, got, s, a, t, b):
    """asserts both gates for one signal's window; returns (worst output / gate, L2 error / gate).  An output without a term is
    exactly zero."""
    got = np.asarray(got)
    none = t == 0
    assert not np.any(got[none]), (tag, "outputs without a term are not 0")
    if not np.any(a):
        return 0.0, 0.0
    out, l2 = gates(dt, M, a, t, b)
    d = got.astype(CLD) - s
    err = np.maximum(np.abs(d.real), np.abs(d.imag)).astype(np.float64)
    live = out > 0
    assert not np.any(err[~live]), (tag, "an output of exact zeros is not 0")
    use = float(np.max(err[live] / out[live]))
    e2 = float(np.sqrt(np.sum(np.abs(d) ** 2)))
    print(f"{tag} {dt}: worst output {use:.3f} of its gate, L2 error {e2:.3e} of {l2:.3e}")
    assert use <= 1.0 and e2 <= l2, (tag, dt, use, e2, l2)
    return use, e2 / l2


def frames(case, dt, real, seed=0):
    """BATCH signals' worth of channel data of the case, complex (BATCH, F, bins) with parts of the type; real: the Hermitian
    half with imaginary parts in bin 0 and bin M / 2 that the planner must ignore"""
    F, K, M, D = case[:4]
    bins = M // 2 + 1 if real else M
    rng = np.random.default_rng([seed, F, M, 29])
    re = rng.uniform(-1, 1, (BATCH, F, bins)).astype(NDT[dt])
    im = rng.uniform(-1, 1, (BATCH, F, bins)).astype(NDT[dt])
    return re + 1j * im
