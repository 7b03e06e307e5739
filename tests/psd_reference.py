"""Welch spectral estimation in numpy long double, straight from the definitions of csrc/psd.hpp (which are scipy.signal's:
tests/test_psd_cpu.py holds this file against welch, csd and spectrogram).  The inputs are taken exactly as given (an f32
test passes its f32 values); numpy's rfft keeps long double."""
import numpy as np

LD = np.longdouble
PI = LD("3.14159265358979323846264338327950288")

# (L, P, H, F): the smallest shapes that reach each branch
SHAPES = [
    (1000, 100, 63, 128),   # zero-padded, ragged tail
    (1000, 100, 100, 100),  # no overlap, Bluestein
    (37, 37, 1, 37),        # one segment, odd F: no Nyquist bin
    (513, 64, 32, 64),      # power of two, one sample past the last segment
    (300, 7, 3, 9),         # tiny odd
    (64, 1, 1, 1),          # one bin; detrended it is exactly zero
    (50, 2, 1, 2),          # DC and Nyquist only
    (1000, 30, 23, 30),     # the shape the STFT budget found worst
    (4096, 8, 1, 8),        # 4089 frames, 5 bins: the slab path
]
MIN_SLAB = 16  # kPsdMinSlab: the Q of every planner whose S * bins stays below 2^19 * 17


def slab_shapes(q: int = MIN_SLAB):
    """P = 8, H = 8 and S in {Q - 1, Q, Q + 1, 2Q + 1}"""
    return [(8 * s, 8, 8, 8) for s in (q - 1, q, q + 1, 2 * q + 1)]


def segments(length, p, h):
    return 1 + (length - p) // h


def hann(p):
    if p == 1:
        return np.ones(1, LD)
    return LD(0.5) - LD(0.5) * np.cos(2 * PI * np.arange(p, dtype=LD) / p)


def window_of(kind, p, seed=0):
    """"hann" (None for the planner: it builds the same in long double) or "random": uniform [0.1, 1) doubles"""
    if kind == "hann":
        return None
    return np.random.default_rng(1000 + seed).uniform(0.1, 1.0, p)


def sigma(w, scaling, fs):
    w = np.asarray(w, LD)
    return 1 / (LD(fs) * np.sum(w * w)) if scaling == "density" else 1 / np.sum(w) ** 2


def onesided(f):
    c = np.full(f // 2 + 1, 2, LD)
    c[0] = 1
    if f % 2 == 0:
        c[-1] = 1
    return c


def spectra(x, p, h, f, w, detrend):
    """X_f of every segment: (S, bins) complex long double"""
    x = np.asarray(x).astype(LD)
    s = segments(x.size, p, h)
    seg = x[np.arange(s)[:, None] * h + np.arange(p)[None, :]]
    if detrend:
        seg = seg - seg.mean(axis=1, keepdims=True)
    rows = np.zeros((s, f), LD)
    rows[:, :p] = seg * w
    return np.fft.rfft(rows, axis=1)


def psd(x, p, h, f, window=None, detrend=True, scaling="density", fs=1.0, y=None, average=True):
    """auto: P_xx; with y: (P_xy complex, P_xx, P_yy).  average=False: (S, bins) per output, without the 1/S"""
    w = hann(p) if window is None else np.asarray(window).astype(LD)
    scale = sigma(w, scaling, fs) * onesided(f)
    fx = spectra(x, p, h, f, w, detrend)
    red = (lambda a: a.mean(axis=0)) if average else (lambda a: a)
    pxx = red((fx * np.conj(fx)).real) * scale
    if y is None:
        return pxx
    fy = spectra(y, p, h, f, w, detrend)
    return red(np.conj(fx) * fy) * scale, pxx, red((fy * np.conj(fy)).real) * scale
