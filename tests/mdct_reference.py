"""References for the MDCT and its inverse (include/phastft_hip.h), sharing no code with csrc/mdct.hpp:

    (a) mdct_direct / imdct_direct   the O(N^2) definition in long double
    (b) mdct_fast / imdct_fast       fold and unfold in numpy around scipy.fft.dct(type=4) in long double

and the three perfect-reconstruction windows, the frame count, the window's TDAC defect and the gates of the GPU tests."""
from __future__ import annotations

import numpy as np
import scipy.fft as sf

from tests import tolerances as tol

LD = np.longdouble
PI = LD("3.14159265358979323846264338327950288")


def frames_of(length: int, n: int, padded: bool) -> int:
    return -(-length // n) + 1 if padded else length // n - 1


def window(name: str, n: int):
    """2N long-double values of "sine", "vorbis", "kbd" (alpha 4) or "rect" """
    t = (np.arange(2 * n, dtype=LD) + LD(0.5)) / LD(2 * n)
    if name == "sine":
        return np.sin(PI * t)
    if name == "vorbis":
        return np.sin(PI / 2 * np.sin(PI * t) ** 2)
    if name == "kbd":
        k = np.i0(np.pi * 4.0 * np.sqrt(1.0 - (2.0 * np.arange(n + 1) / n - 1.0) ** 2)).astype(LD)
        c = np.cumsum(k)
        half = np.sqrt(c[:n] / c[n])
        return np.concatenate([half, half[::-1]])
    if name == "rect":
        return np.ones(2 * n, LD)
    raise ValueError(name)


def tdac_defect(w, n: int) -> float:
    w = np.asarray(w, np.float64)
    return float(max(np.abs(w[:n] ** 2 + w[n:] ** 2 - 1).max(), np.abs(w - w[::-1]).max()))


def _framed(x, n: int, padded: bool):
    """[frames][2N]: frame t holds x[(t - padded) N + j], zero outside [0, L)"""
    x = np.asarray(x, LD)
    f = frames_of(x.size, n, padded)
    buf = np.zeros((f + 1) * n + 2 * n, LD)
    off = n if padded else 0
    take = min(x.size, buf.size - off)
    buf[off:off + take] = x[:take]
    return np.stack([buf[t * n:t * n + 2 * n] for t in range(f)]) if f else np.zeros((0, 2 * n), LD)


def _kernel(n: int):
    j = np.arange(2 * n, dtype=LD)[:, None]
    k = np.arange(n, dtype=LD)[None, :]
    return np.cos(PI / n * (j + LD(0.5) + LD(n) / 2) * (k + LD(0.5)))  # [2N][N]


def _overlap_add(y, length: int, n: int, padded: bool):
    f = y.shape[0]
    buf = np.zeros(max((f + 1) * n, length + 2 * n) + n, LD)
    for t in range(f):
        buf[t * n:t * n + 2 * n] += y[t]
    off = n if padded else 0
    return buf[off:off + length]


def mdct_direct(x, n: int, w, padded: bool = True):
    return (_framed(x, n, padded) * np.asarray(w, LD)) @ _kernel(n)


def imdct_direct(X, length: int, n: int, w, padded: bool = True):
    y = (np.asarray(X, LD) @ _kernel(n).T) * (LD(2) / n) * np.asarray(w, LD)
    return _overlap_add(y, length, n, padded)


def mdct_fast(x, n: int, w, padded: bool = True):
    h = n // 2
    fr = _framed(x, n, padded) * np.asarray(w, LD)
    a, b, c, d = fr[:, :h], fr[:, h:n], fr[:, n:n + h], fr[:, n + h:]
    u = np.concatenate([-c[:, ::-1] - d, a - b[:, ::-1]], axis=1)
    return sf.dct(u, type=4, axis=1) / 2 if u.shape[0] else u  # scipy's DCT-IV carries a factor 2


def imdct_fast(X, length: int, n: int, w, padded: bool = True):
    h = n // 2
    X = np.asarray(X, LD)
    v = sf.dct(X, type=4, axis=1) / 2 if X.shape[0] else X
    y = np.concatenate([v[:, h:], -v[:, ::-1], -v[:, :h]], axis=1) * (LD(2) / n) * np.asarray(w, LD)
    return _overlap_add(y, length, n, padded)


def inner_log2(n: int) -> int:
    """log2 of the length the inner complex transform of h = N / 2 points runs at: h, or its Bluestein length"""
    from tests.test_gpu_any_len import conv_len

    return max(1, conv_len(max(1, n // 2)).bit_length() - 1)


def mdct_gates(dt: str, n: int):
    """(rel-L2, worst coefficient / rms): the FFT gates at the inner length, times the any-length factor 2 of the DCT and
    STFT gates (two twiddle sweeps around the inner transform)"""
    lg = inner_log2(n)
    return 2 * tol.rel_gate(dt, lg), 2 * tol.bin_gate(dt, lg)


def errors(got, want):
    got, want = np.asarray(got, np.float64).ravel(), np.asarray(want, np.float64).ravel()
    den = float(np.linalg.norm(want))
    rel = float(np.linalg.norm(got - want)) / (den if den else 1.0)
    rms = float(np.sqrt(np.mean(want ** 2))) if want.size else 0.0
    worst = float(np.abs(got - want).max()) / (rms if rms else 1.0) if want.size else 0.0
    return rel, worst
