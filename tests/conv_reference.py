"""Convolution and correlation of real signals by the definition, in long double (DESIGN.md §16's definitions, which are
scipy.signal.convolve / correlate(x, h, mode, method="direct")): the CPU reference of tests/test_gpu_conv.py and of
tests/golden/make_conv_error_budget.py.  It shares no code with csrc/conv.hpp: the sum is numpy.convolve's on longdouble,
the modes are slices of it; tests/test_conv_cpu.py checks it against scipy."""
from __future__ import annotations

import numpy as np

MODES = ("full", "same", "valid")
TAPS = ("random", "lowpass")


def geometry(length: int, k: int, mode: str):
    """(t0, out_len): out[i] = full[t0 + i]; out_len is 0 where valid has no sample (L < K)"""
    if mode == "full":
        return 0, length + k - 1
    if mode == "same":
        return (k - 1) // 2, length
    if mode == "valid":
        return k - 1, max(length - k + 1, 0)
    raise ValueError(mode)


def taps(kind: str, k: int, dtype=np.float64, seed: int = 0):
    """random: uniform(-1, 1), seeded by (seed, K); lowpass: a Hann-windowed half-band sinc (one tap: 1)"""
    if kind == "random":
        h = np.random.default_rng([seed, k, 29]).uniform(-1, 1, k)
    elif kind == "lowpass":
        n = np.arange(k) - (k - 1) / 2
        h = 0.5 * np.sinc(0.5 * n) * np.hanning(k + 2)[1:-1] if k > 1 else np.ones(1)
    else:
        raise ValueError(kind)
    return h.astype(dtype)


def signal(length: int, dtype=np.float64, seed: int = 0):
    return np.random.default_rng([seed, length, 13]).uniform(-1, 1, length).astype(dtype)


def convolve(x, h, mode: str = "full", flip: bool = False):
    """out[i] = sum_j g[j] x[t0 + i - j] in long double; g = h, or h reversed with `flip` (correlation)"""
    g = np.asarray(h, np.longdouble)
    if flip:
        g = g[::-1]
    full = np.convolve(np.asarray(x, np.longdouble), g)
    t0, n = geometry(len(x), len(g), mode)
    return full[t0:t0 + n]
