"""The STFT and its inverse restated in numpy around scipy's long-double rfft / irfft (DESIGN.md §15's definitions, which are
torch.stft / torch.istft(length=L) with win_length = n_fft): the CPU reference of tests/test_gpu_stft.py and of
tests/golden/make_stft_error_budget.py.  It shares no code with csrc/stft.hpp: the padding is numpy.pad's, the overlap-add a
loop over frames; tests/test_stft_cpu.py checks both against torch."""
from __future__ import annotations

import numpy as np
import scipy.fft as sf

NOLA_MIN = 1e-11  # torch.istft's threshold on the window envelope
WINDOWS = ("hann", "rect", "uniform")


def window(name: str, f: int, dtype=np.float64):
    """hann: torch.hann_window(F) (periodic; w[0] = 0 for F > 1); rect: ones; uniform: uniform(0.5, 1.5), seeded by F"""
    if name == "hann":
        w = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(f) / f) if f > 1 else np.ones(1)
    elif name == "rect":
        w = np.ones(f)
    elif name == "uniform":
        w = np.random.default_rng([f, 77]).uniform(0.5, 1.5, f)
    else:
        raise ValueError(name)
    return w.astype(dtype)


def sizes(length: int, f: int, h: int, center: bool):
    """(p, frames, bins)"""
    p = f // 2 if center else 0
    return p, 1 + (length + 2 * p - f) // h, f // 2 + 1


def stft(x, w, f: int, h: int, center: bool, pad_mode: str):
    """the (frames, bins) spectrogram of x in long double (complex)"""
    p, frames, _ = sizes(len(x), f, h, center)
    xp = np.asarray(x, np.longdouble)
    if p:
        xp = np.pad(xp, (p, p), mode="reflect" if pad_mode == "reflect" else "constant")
    idx = np.arange(frames)[:, None] * h + np.arange(f)[None, :]
    return sf.rfft(xp[idx] * np.asarray(w, np.longdouble)[None, :], axis=1)


def envelope(w, length: int, f: int, h: int, center: bool):
    """(sum_f w^2 over the frames that hold output sample t, how many frames hold it), t < L, in double"""
    p, frames, _ = sizes(length, f, h, center)
    span = max((frames - 1) * h + f, length + p)
    den, cnt = np.zeros(span), np.zeros(span, np.int64)
    w2 = np.asarray(w, np.float64) ** 2
    for k in range(frames):
        den[k * h:k * h + f] += w2
        cnt[k * h:k * h + f] += 1
    return den[p:p + length], cnt[p:p + length]


def invertible(w, length: int, f: int, h: int, center: bool) -> bool:
    """torch.istft's NOLA verdict: the envelope exceeds 1e-11 wherever a frame holds the sample"""
    den, cnt = envelope(w, length, f, h, center)
    return bool(den[cnt > 0].min() > NOLA_MIN)


def istft(spec, w, length: int, f: int, h: int, center: bool):
    """the weighted overlap-add of irfft_F of the (frames, bins) spectrogram, in long double; 0 where no frame holds t"""
    p, frames, _ = sizes(length, f, h, center)
    y = sf.irfft(np.asarray(spec, np.clongdouble), n=f, axis=1) * np.asarray(w, np.longdouble)[None, :]
    span = max((frames - 1) * h + f, length + p)
    num = np.zeros(span, np.longdouble)
    for k in range(frames):
        num[k * h:k * h + f] += y[k]
    _, cnt = envelope(w, length, f, h, center)
    w2 = np.asarray(w, np.longdouble) ** 2
    den = np.zeros(span, np.longdouble)
    for k in range(frames):
        den[k * h:k * h + f] += w2
    out = np.zeros(length, np.longdouble)
    has = cnt > 0
    out[has] = num[p:p + length][has] / den[p:p + length][has]
    return out
