"""The generalised Lomb-Scargle periodogram in numpy long double, straight from the definitions of csrc/lomb.hpp (which are
scipy.signal.lombscargle's, 1.15: tests/test_lomb_cpu.py holds this file against it on centred inputs).  The three sums
A0, A2 and A1 are the direct sums of tests/nufft_t3_reference.py: every phase f_k t_j (and 2 f_k t_j: doubling a double is
exact) is formed exactly mod 1 turn, so a time origin 10^6 spans away costs nothing here.  It shares no code with the
library."""
from __future__ import annotations

import numpy as np

from tests.nufft_t3_reference import LD, direct

NORMS = ("power", "normalize", "amplitude")
EPSNEG = {"f64": float(np.finfo(np.float64).epsneg), "f32": float(np.finfo(np.float32).epsneg)}
# (M, K) of the GPU tests; (1, 1) is degenerate in normalize and amplitude (SS = 0, YY = 0), in scipy too: power only
SHAPES = [(1, 1), (5, 3), (100, 37), (1000, 257), (4096, 1000)]
# the times: uniform on [0, 50], unsorted; with duplicates; offset by 10^6 spans
KINDS = ["u", "dup", "far"]
CASES = [s + ("u",) for s in SHAPES] + [s + (k,) for s in SHAPES[2:4] for k in KINDS[1:]]
# the accuracies asked of the inner type-3 planner: both ends of the type's range and one between
EPS = {"f64": [1e-1, 1e-7, 1e-14], "f32": [1e-1, 1e-3, 1e-6]}
SEEDS = (0, 1)
SPAN = 50.0
D_MIN = 0.01  # frequencies whose clamped CCt or SSt is smaller are asserted finite only


def case_id(c):
    return f"{c[0]}x{c[1]}{c[2]}"


def points(case):
    """(t, f) of a case as float64: t uniform on [0, 50] in random order, f uniform on [0.05, 5] cycles per unit of t"""
    m, k, kind = case
    rng = np.random.default_rng([m, k, 41])
    t = rng.uniform(0.0, SPAN, m)
    f = rng.uniform(0.05, 5.0, k)
    if kind == "dup":
        t[1::7] = t[0::7][: len(t[1::7])]
    if kind == "far":
        t = t + 1e6 * SPAN
    return t, f


def signal(case, seed, offset=0.0):
    """values |y| <~ 3 that are exact in float32 (so that both types share one reference): two sinusoids and noise"""
    m = case[0]
    t, f = points(case)
    rng = np.random.default_rng([seed, m, 43])
    tc = t - t.min()
    y = 1.5 * np.sin(2 * np.pi * f[0] * tc + 0.3) + 0.8 * np.cos(2 * np.pi * 0.731 * tc) + 0.3 * rng.standard_normal(m) + offset
    return y.astype(np.float32).astype(np.float64)


def weights(case, seed=0):
    """positive weights, not normalised"""
    return np.random.default_rng([seed, case[0], 47]).uniform(0.5, 1.5, case[0])


def normalised(w, m):
    if w is None:
        return np.full(m, LD(1) / LD(m), LD)
    w = np.asarray(w).astype(LD)
    return w / w.sum()


def sums(t, f, vectors):
    """sum_j v_j exp(+2 pi i f_k t_j) of every real vector: complex long double arrays of K"""
    out = direct(np.asarray(t, np.float64), np.asarray(f, np.float64), [np.asarray(v, LD) for v in vectors])
    return [re - 1j * im for re, im in out]   # direct is the - sign; the data are real


def tables(t, f, w, floating_mean, epsneg):
    """(cos tau, sin tau, CCt, SSt) in long double, CCt and SSt clamped at epsneg"""
    t, f = np.asarray(t, np.float64), np.asarray(f, np.float64)
    a0, = sums(t, f, [w])
    a2, = sums(t, 2 * f, [w])
    return tables_of(a0, a2, floating_mean, epsneg)


def tables_of(a0, a2, floating_mean, epsneg):
    c, s, c2, s2 = a0.real, a0.imag, a2.real, a2.imag
    cc, ss, cs = (1 + c2) / 2, (1 - c2) / 2, s2 / 2
    if floating_mean:
        cc, ss, cs = cc - c * c, ss - s * s, cs - c * s
    tau = np.arctan2(2 * cs, cc - ss) / 2
    ct, st = np.cos(tau), np.sin(tau)
    cct = (1 + c2 * np.cos(2 * tau) + s2 * np.sin(2 * tau)) / 2
    sst = 1 - cct
    if floating_mean:
        cct = cct - (c * ct + s * st) ** 2
        sst = sst - (s * ct - c * st) ** 2
    return ct, st, np.maximum(cct, LD(epsneg)), np.maximum(sst, LD(epsneg))


def post(a1, tab, m, yy, norm):
    ct, st, cct, sst = tab
    yc = a1.real * ct + a1.imag * st
    ys = a1.imag * ct - a1.real * st
    a, b = yc / cct, ys / sst
    p = 2 * (a * yc + b * ys)
    if norm == "power":
        return p * LD(m) / 4
    if norm == "normalize":
        with np.errstate(divide="ignore", invalid="ignore"):
            return p * LD(0.5) / yy
    return (a + 1j * b) * (ct + 1j * st)


def lombscargle(t, y, f, weights=None, floating_mean=False, norm="power", epsneg=EPSNEG["f64"], tab=None):
    """one signal: K real values (power, normalize) or K complex values (amplitude) in long double"""
    t, f = np.asarray(t, np.float64), np.asarray(f, np.float64)
    w = normalised(weights, t.size)
    y = np.asarray(y).astype(LD)
    mean = (w * y).sum() if floating_mean else LD(0)
    r = y - mean
    a1, = sums(t, f, [w * r])
    tab = tables(t, f, w, floating_mean, epsneg) if tab is None else tab
    return post(a1, tab, t.size, (w * r * r).sum(), norm)


def smallest_d(tab, mask=None):
    """the smallest clamped CCt or SSt over the (masked) frequencies"""
    d = np.minimum(tab[2], tab[3]).astype(np.float64)
    return float(d.min() if mask is None else d[mask].min())


def gated(tab):
    """the frequencies a gate applies to: min(CCt, SSt) >= D_MIN"""
    return np.minimum(tab[2], tab[3]).astype(np.float64) >= D_MIN


def error(got, want, mask=None):
    """max_k |got - ref| / max_k |ref| over the masked frequencies; exactly zero against a zero reference counts as 0"""
    got, want = np.asarray(got), np.asarray(want)
    if mask is not None:
        got, want = got[mask], want[mask]
    if got.size == 0:
        return 0.0
    top, diff = float(np.abs(want).max()), float(np.abs(got - want.astype(np.complex128 if np.iscomplexobj(want) else np.float64)).max())
    return diff / top if top else diff
