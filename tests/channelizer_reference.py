"""References for the polyphase channelizer (csrc/channelizer.hpp) in long double, the cases the tests
share, the gates and a numpy model of the header's geometry.  A plain helper, not a test.

    fold_ref        u[m][p] = sum_j h[r0 + j M] x[m D - r0 - j M], r0 = (m D - p) mod M, with A[m][p] = sum |h x| (the gate's scale)
    channelize_ref  y[m][k] = sum_n h[m D - n] x[n] exp(-2 pi i k n / M): the terms of the definition grouped by n mod M (the
                    phase depends on nothing else), each group summed in long double, then the M phases applied in long double
    definition_ref  the same sum term by term, for the small cases (test_channelizer_cpu.py holds the two together and both
                    against scipy)
    geom            chan_geom of channelizer.hpp
"""
import functools
import math

import numpy as np

from tests import tolerances as tol
from tests.resample_reference import LD, NDT, U, signal, taps  # noqa: F401  (shared generators)

CLD = np.clongdouble
LDS, MAX_COLS, PER_THREAD = 4096, 256, 4  # the constants of csrc/channelizer.hpp

# (L, K, M, D)
SMALL_CASES = [
    (1, 1, 1, 1),
    (37, 24, 8, 8),    # critically sampled, T = 3
    (37, 24, 8, 4),    # 2 x oversampled: the rotation alternates
    (41, 21, 6, 4),    # K no multiple of M, M no power of two
    (30, 50, 7, 3),    # K > L, prime M, D coprime to M
    (20, 5, 8, 8),     # K < M: columns without taps
    (33, 17, 5, 5),
    (64, 32, 8, 12),   # D > M
    (9, 4, 3, 1),
]
CASES = SMALL_CASES + [
    (600, 1030, 257, 257),     # one column past a 256-column tile, Bluestein inside
    (3000, 2048, 256, 192),    # the 4/3-oversampled bank
    (5000, 4100, 1024, 1024),  # several column tiles, T = 5
    (9000, 8200, 4, 4),        # M far below a wave, T = 2050: three tap chunks
]
BATCH = 3


def case_id(c):
    return "x".join(str(v) for v in c)


def full_frames(L, K, D):
    return (L + K - 2) // D + 1


def t_of(K, M):
    return -(-K // M)


def geom(K, M, D):
    """chan_geom: (cols, fpp, per, frames, span, jc, rows)"""
    cols = min(M, MAX_COLS)
    fpp, per = 256 // cols, PER_THREAD
    max_rows = LDS // cols
    while True:
        frames = fpp * per
        span = ((frames - 1) * D + M - 1) // M + 2
        if span <= max_rows // 2 or frames == 1:
            break
        if per > 1:
            per //= 2
        else:
            fpp //= 2
    jc = min(t_of(K, M), max_rows - span + 1)
    return cols, fpp, per, frames, span, jc, span + jc - 1


def windows(case):
    """(first_frame, out_frames): the whole result, and from frame 3 on (or the last legal first_frame) one tile less one
    frame, one tile, one tile and a frame, and a window that passes full_frames by two"""
    L, K, M, D = case
    full, tile = full_frames(L, K, D), geom(K, M, D)[3]
    first = min(3, full)
    out = [(0, None)] + [(first, n) for n in (tile - 1, tile, tile + 1, full - first + 2) if n >= 1]
    return list(dict.fromkeys(out))


def fold_ref(h, x, M, D, first, frames):
    """(u, a): the fold of the frames first .. first + frames - 1 in long double from the values as given, and sum |h x| per
    element.  x real or complex; a uses |x|."""
    h, x = np.asarray(h).astype(LD), np.asarray(x)
    x = x.astype(CLD) if np.iscomplexobj(x) else x.astype(LD)
    L, K = x.size, h.size
    m = (first + np.arange(frames, dtype=np.int64))[:, None]
    p = np.arange(M, dtype=np.int64)[None, :]
    r0 = (m * D - p) % M
    top = m * D - r0
    u, a = np.zeros((frames, M), x.dtype), np.zeros((frames, M), LD)
    for j in range(t_of(K, M)):
        ti, n = r0 + j * M, top - j * M
        ok = (ti < K) & (n >= 0) & (n < L)
        term = np.where(ok, h[np.clip(ti, 0, K - 1)] * x[np.clip(n, 0, L - 1)], 0)
        u += term
        a += np.abs(term)
    return u, a


@functools.lru_cache(maxsize=8)
def phases(M, bins):
    """W[p][k] = exp(-2 pi i p k / M) in long double, the angle from p k mod M"""
    pk = (np.arange(M, dtype=np.int64)[:, None] * np.arange(bins, dtype=np.int64)[None, :]) % M
    # np.pi is a double: long double's pi is that plus the next term of its expansion
    ang = -2 * (LD(np.pi) + LD(1.2246467991473532e-16)) * pk.astype(LD) / LD(M)
    w = np.empty(ang.shape, CLD)
    w.real, w.imag = np.cos(ang), np.sin(ang)
    return w


def channelize_ref(h, x, M, D, first=0, out_frames=None):
    """(y, u, a): the frames first .. in long double, bins = M (complex x) or M // 2 + 1 (real x), with the fold and its scale"""
    x = np.asarray(x)
    if out_frames is None:
        out_frames = full_frames(x.size, len(h), D) - first
    bins = M if np.iscomplexobj(x) else M // 2 + 1
    u, a = fold_ref(h, x, M, D, first, out_frames)
    return u.astype(CLD) @ phases(M, bins), u, a


def definition_ref(h, x, M, D):
    """y[m][k] for all full_frames and all M channels, term by term: sum_n h[m D - n] x[n] exp(-2 pi i k n / M)"""
    h, x = np.asarray(h).astype(LD), np.asarray(x).astype(CLD)
    L, K = x.size, h.size
    pi = LD(np.pi) + LD(1.2246467991473532e-16)
    y = np.zeros((full_frames(L, K, D), M), CLD)
    n = np.arange(L, dtype=np.int64)
    for m in range(y.shape[0]):
        ti = m * D - n
        hx = np.where((ti >= 0) & (ti < K), h[np.clip(ti, 0, K - 1)], LD(0)) * x
        for k in range(M):
            ang = -2 * pi * ((k * n) % M).astype(LD) / LD(M)
            y[m, k] = np.sum(hx * (np.cos(ang) + 1j * np.sin(ang)))
    return y


def gates(dt, K, M, u, a):
    """(rel-L2 gate, worst-bin gate relative to the rms bin is the second plus `fold_bin` / rms): the transform's gates at
    log2 M plus the fold's bound (T + 2) u sum |h x| carried through the DFT -- (rel, bin, fold_bin).  M = 1: no transform."""
    n = t_of(K, M) + 2
    un, an = float(np.sqrt(np.sum(np.abs(u) ** 2))), float(np.sqrt(np.sum(a ** 2)))
    lg = math.log2(M)
    rel = (tol.rel_gate(dt, lg) if M > 1 else 0.0) + (n * U[dt] * an / un if un else 0.0)
    return rel, (tol.bin_gate(dt, lg) if M > 1 else 0.0), n * U[dt] * float(np.max(np.sum(a, axis=1)))


def check(tag, dt, K, M, got, y, u, a):
    """asserts both gates for one signal's window (got, y: complex (frames, bins)); returns (rel / gate, bin / gate).  A window
    without a product is exactly zero."""
    got = np.asarray(got).astype(CLD)
    if not np.any(a):
        assert not np.any(got), tag
        return 0.0, 0.0
    g_rel, g_bin, fold_bin = gates(dt, K, M, u, a)
    err = np.abs(got - y)
    if M == 1:  # per output, as upfirdn
        gate = (t_of(K, M) + 2) * U[dt] * a[:, :1].astype(np.float64)
        e = err.astype(np.float64)
        assert np.all(e <= gate), (tag, dt, float(np.max(e / np.maximum(gate, 1e-300))))
        use = float(np.max(e[gate > 0] / gate[gate > 0]))
        return use, use
    rel = float(np.sqrt(np.sum(err ** 2)) / np.sqrt(np.sum(np.abs(y) ** 2)))
    rms = float(np.sqrt(np.mean(np.abs(y) ** 2)))
    worst = float(np.max(np.maximum(np.abs((got - y).real), np.abs((got - y).imag)))) / rms
    gb = g_bin + fold_bin / rms
    print(f"{tag} {dt}: rel {rel:.3e} of {g_rel:.3e}, bin {worst:.3e} of {gb:.3e}")
    assert rel <= g_rel and worst <= gb, (tag, dt, rel, g_rel, worst, gb)
    return rel / g_rel, worst / gb


def signals(case, dt, cplx, seed=0):
    """BATCH signals of the case: values of the type, real or complex"""
    L = case[0]
    re = signal(L, dt, seed=seed, batch=BATCH)
    return re + 1j * signal(L, dt, seed=seed + 100, batch=BATCH) if cplx else re
