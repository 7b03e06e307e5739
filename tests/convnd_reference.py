"""Convolution and correlation of real arrays of rank 1 .. 3 by the definition, in long double (which is
scipy.signal.convolve / correlate(x, h, mode, method="direct") of N-d arrays): the CPU reference of tests/test_gpu_convnd.py, of
tests/test_convnd_cpu.py and of tests/golden/make_convnd_error_budget.py.  It shares no code with csrc/convnd.hpp: the full sum is
one shifted add of the array per tap, the modes are slices of it; tests/test_convnd_cpu.py checks it against scipy."""
from __future__ import annotations

import functools
import itertools

import numpy as np

MODES = ("full", "same", "valid")
MODE = {"full": 0, "same": 1, "valid": 2}

# (L; K; B), B = 0: the automatic block.  DAGGER: the shapes the schedule was first tried on (even K_i and K > L included)
DAGGER = [((9, 7), (3, 4), (4, 4)), ((20, 13), (5, 3), (8, 8)),
          ((12, 10), (1, 4), (1, 8)),     # one tile axis left: the 1-D path
          ((5, 6), (7, 9), (8, 16)),      # K > L: no `valid`
          ((10, 11), (4, 5), (6, 17)),    # Bluestein axes and an odd last axis: groups straddle tile rows
          ((6, 5, 7), (2, 3, 2), (4, 4, 4))]
SHAPES = [((1, 1), (1, 1), (0, 0))] + DAGGER[:5] + [
    ((70, 300), (17, 5), (64, 32)), ((100, 130), (9, 9), (0, 0)),
    ((300, 260), (31, 31), (0, 0)),  # 128 x 128 tiles, 12 of them: the square transpose path
    DAGGER[5], ((20, 20, 20), (3, 3, 3), (8, 8, 8)), ((33, 17, 40), (5, 1, 7), (16, 1, 16)),
    ((1000,), (33,), (100,))]


def shape_id(shape) -> str:
    return ";".join(",".join(str(v) for v in part) for part in shape)


def has_mode(L, K, mode: str) -> bool:
    return mode != "valid" or all(l >= k for l, k in zip(L, K))


def geometry(L, K, mode: str):
    """(t0, out) per axis: out[i] = full[t0 + i]"""
    if mode == "full":
        return tuple(0 for _ in K), tuple(l + k - 1 for l, k in zip(L, K))
    if mode == "same":
        return tuple((k - 1) // 2 for k in K), tuple(L)
    if mode == "valid":
        return tuple(k - 1 for k in K), tuple(max(l - k + 1, 0) for l, k in zip(L, K))
    raise ValueError(mode)


def auto_block(L, K, mode: str):
    """DESIGN.md §23's rule, restated: per axis that counts (not L = K = 1; the last one if none does) the smallest power of
    two >= max(4 (K - 1), floor), floor = 1024 for one such axis and 64 for more; or the smallest power of two >= out + K - 1
    where that is smaller.  An axis that does not count: 1."""
    def pow2(v):
        return 1 << max(v - 1, 0).bit_length()

    counts = [l > 1 or k > 1 for l, k in zip(L, K)]
    if not any(counts):
        counts[-1] = True
    floor = 1024 if sum(counts) == 1 else 64
    out = geometry(L, K, mode)[1]
    return tuple(min(pow2(max(4 * (k - 1), floor)), pow2(o + k - 1)) if c else 1 for k, o, c in zip(K, out, counts))


def array(shape, dtype=np.float64, seed: int = 0):
    return np.random.default_rng([seed, 13, *shape]).uniform(-1, 1, shape).astype(dtype)


def taps(shape, dtype=np.float64, seed: int = 0):
    return np.random.default_rng([seed, 29, *shape]).uniform(-1, 1, shape).astype(dtype)


def full(x, h, flip: bool = False):
    """full[t] = sum_j g[j] x[t - j] in long double: one shifted add of x per tap; g = h, or h reversed along every axis"""
    g = np.asarray(h, np.longdouble)
    if flip:
        g = g[tuple(slice(None, None, -1) for _ in g.shape)]
    xl = np.asarray(x, np.longdouble)
    out = np.zeros(tuple(l + k - 1 for l, k in zip(xl.shape, g.shape)), np.longdouble)
    for j in itertools.product(*(range(k) for k in g.shape)):
        out[tuple(slice(a, a + l) for a, l in zip(j, xl.shape))] += g[j] * xl
    return out


def convolve(x, h, mode: str = "full", flip: bool = False):
    t0, n = geometry(x.shape, np.shape(h), mode)
    return full(x, h, flip)[tuple(slice(a, a + m) for a, m in zip(t0, n))]


@functools.lru_cache(maxsize=None)
def case(L, K, dtype_name: str, flip: bool, seed: int = 0):
    """(x, h, full) of a shape in dtype: the inputs rounded to the type first, the sum of those in long double.  Shared and
    read-only: the tests slice the modes out of `full`."""
    dt = np.dtype(dtype_name).type
    x, h = array(L, dt, seed), taps(K, dt, seed)
    f = full(x, h, flip)
    for a in (x, h, f):
        a.setflags(write=False)
    return x, h, f


def expected(L, K, dtype_name: str, mode: str, flip: bool, seed: int = 0):
    x, h, f = case(tuple(L), tuple(K), dtype_name, bool(flip), seed)
    t0, n = geometry(L, K, mode)
    return x, h, f[tuple(slice(a, a + m) for a, m in zip(t0, n))]
