"""The host half of the Lomb-Scargle periodogram (csrc/lomb.hpp, csrc/planner_lomb.hpp), without a GPU:

    the long double reference (tests/lomb_reference.py) against scipy.signal.lombscargle on centred inputs -- t in [0, 50],
        |y| <~ 3: elsewhere scipy's own freqs * x in double is the less exact of the two;
    lomb.hpp compiled with g++: its table and post formulas, fed the exact direct sums, against the reference for every
        M <= 64, with random weights and with none; the slab rule; the argument rule;
    the argument codes of the C ABI before the device is touched, the Python argument errors and the exports;
    a numpy model of the whole schedule around tests/test_nufft_t3_cpu.py's model of the type-3 transform, asserted against
        the reference inside the gate.

The gate of a periodogram (lomb_gate), on the metric max_k |got - ref| / max_k |ref| over the gated frequencies:
    g3 = C3 eps + KAPPA Q 2^-53 + tests/tolerances.py's rel_gate on log2 n_g      (DESIGN.md §21's, for the inner planner)
    power, normalize   C_L g3 / sqrt(d)          amplitude   C_L g3 / d
with d the smallest clamped CCt or SSt over the gated frequencies, from the reference.  The exponents: an error delta of A1
moves YC by delta and a YC by 2 delta YC / CCt <= 2 delta sqrt(YY / CCt), since YC^2 <= CCt YY; it moves a by delta / CCt.
C_L = 1/4 is the smallest round number that leaves every entry of tests/golden/lomb_error_budget.json a factor of 2
(tests/test_gpu_lomb.py: test_gates_keep_their_margin; the smallest is 2.4, at (5, 3), f32, eps 1e-3, fixed mean, d = 0.14): the
metric divides by the largest value, where g3 was fitted to an rms.  This file's model of the schedule sat 10 x below
C_L = 1 before any GPU time was spent and sits 2.4 x below the gate now."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import lomb_reference as R
from tests import nufft_t3_reference as R3
from tests import tolerances as tol
from tests.test_nufft_t3_cpu import C3, KAPPA, model as t3_model, schedule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = [f"phast_planner_lomb{s}_{w}" for s in ("64", "32")
       for w in ("new", "free", "describe", "device_bytes", "slab", "grid_len", "workspace_len", "workspace_min", "time_stages")]
NEW += [f"phast_lombscargle_{s}{suffix}" for s in ("f64", "f32") for suffix in ("", "_with_planner", "_dev")]
OK, NO_DEVICE, INVALID_ARG = 0, 15, 16
C_L = 0.25
MEANS = (False, True)


def lomb_gate(dt, n_g, eps, q, d, norm):
    """the bound on max |got - ref| / max |ref| of a periodogram whose inner planner was asked for eps, has conditioning q
    and an inner grid of n_g points, at frequencies whose clamped CCt and SSt are at least d"""
    g3 = C3[dt] * eps + KAPPA * q * 2.0 ** -53 + tol.rel_gate(dt, n_g.bit_length() - 1)
    return C_L * g3 / (d if norm == "amplitude" else np.sqrt(d))


class Reference:
    """every reference value of one case, computed once: ref[(weighted, floating_mean, norm, seed, dt)] in long double, the
    tables, the gated frequencies and d per (weighted, floating_mean, dt)"""

    def __init__(self, case, seeds=R.SEEDS, offset=0.0, means=MEANS):
        self.case = case
        m = case[0]
        self.t, self.f = R.points(case)
        self.q = R3.conditioning(self.t, self.f)
        self.w = R.weights(case)
        self.y = {sd: R.signal(case, sd, offset) for sd in seeds}
        self.tab, self.mask, self.d, self.ref = {}, {}, {}, {}
        for weighted in (False, True):
            w = R.normalised(self.w if weighted else None, m)
            res = {(fm, sd): self.y[sd].astype(R.LD) - ((w * self.y[sd].astype(R.LD)).sum() if fm else R.LD(0))
                   for fm in means for sd in seeds}
            a0, *rest = R.sums(self.t, self.f, [w] + [w * r for r in res.values()])   # one pass over the phases
            rest = dict(zip(res, rest))
            a2, = R.sums(self.t, 2 * self.f, [w])
            for fm in means:
                a1 = [rest[(fm, sd)] for sd in seeds]
                for dt in ("f64", "f32"):
                    tab = R.tables_of(a0, a2, fm, R.EPSNEG[dt])
                    key = (weighted, fm, dt)
                    self.tab[key], self.mask[key] = tab, R.gated(tab)
                    self.d[key] = R.smallest_d(tab, self.mask[key]) if self.mask[key].any() else 1.0
                    for i, sd in enumerate(seeds):
                        yy = (w * res[(fm, sd)] * res[(fm, sd)]).sum()
                        for norm in R.NORMS:
                            self.ref[(weighted, fm, norm, sd, dt)] = R.post(a1[i], tab, m, yy, norm)

    def norms(self):
        return R.NORMS[:1] if self.case[0] == 1 else R.NORMS


@functools.lru_cache(maxsize=None)
def reference(case, offset=0.0):
    """the long double reference of a case: computed once, shared, left unchanged.  With an offset: the floating mean only"""
    ref = Reference(case, offset=offset, means=MEANS if offset == 0 else (True,))
    for v in ref.ref.values():
        v.flags.writeable = False
    return ref


@pytest.fixture(scope="module")
def helpers(tmp_path_factory):
    so = tmp_path_factory.mktemp("lomb_helpers") / "liblombhelpers.so"
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-shared", "-fPIC", "-I", os.path.join(ROOT, "phastft_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "lomb_tables_test.cpp"), "-o", str(so)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    h = C.CDLL(str(so))
    u, p = C.c_ulonglong, C.c_void_p
    h.lomb_t_bad_args.argtypes = [p, u, p, u, p]
    h.lomb_t_slab_len.argtypes, h.lomb_t_slab_len.restype = [u], u
    h.lomb_t_slabs.argtypes, h.lomb_t_slabs.restype = [u], u
    h.lomb_t_epsneg.argtypes, h.lomb_t_epsneg.restype = [C.c_int], C.c_double
    h.lomb_t_weights.argtypes, h.lomb_t_weights.restype = [p, u, p], None
    h.lomb_t_tables.argtypes, h.lomb_t_tables.restype = [p, p, p, p, u, C.c_int, C.c_int, p], None
    h.lomb_t_post.argtypes, h.lomb_t_post.restype = [p, p, p, u, p], None
    return h


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def arr(v):
    return np.array(v, np.float64)


# ---------------------------------------------------------------------------------------------
# the reference against scipy
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in R.CASES if c[2] in ("u", "dup") and 1 < c[0] <= 1000], ids=R.case_id)
def test_reference_against_scipy(case):
    """centred inputs: weights or none, both mean settings, the three normalisations.  scipy works in double on phases up to
    2 pi 5 50 = 1571 rad: a phase is good to 1571 * 2^-53 = 1.7e-13, and a term divided by CCt or SSt to that over d; 1e-10 / d
    leaves both sides' rounding two orders"""
    from scipy.signal import lombscargle

    ref = reference(case)
    for weighted in (False, True):
        for fm in MEANS:
            for norm in R.NORMS:
                for sd in R.SEEDS:
                    want = ref.ref[(weighted, fm, norm, sd, "f64")]
                    got = lombscargle(ref.t, ref.y[sd], 2 * np.pi * ref.f, precenter=False, normalize=norm,
                                      weights=ref.w if weighted else None, floating_mean=fm)
                    d = R.smallest_d(ref.tab[(weighted, fm, "f64")])
                    err = R.error(got, want)
                    print(f"scipy {R.case_id(case)} w={weighted} fm={fm} {norm} seed {sd}: {err:.3e} (d = {d:.3g})")
                    assert err <= 1e-10 / d, (case, weighted, fm, norm, sd, err, d)


# ---------------------------------------------------------------------------------------------
# lomb.hpp: the slab rule, the argument rule, the formulas
# ---------------------------------------------------------------------------------------------
def test_slab_rule(helpers):
    """Q is a function of M alone, a multiple of 1024 (256 threads of 16 bytes of f32), at least 2048, and a signal has at
    most 1024 slabs"""
    for m in [1, 2, 2047, 2048, 2049, 4096, 2 ** 20, 2 ** 21, 2 ** 21 + 1, 3 * 2 ** 20 + 5, 2 ** 30 - 1, 2 ** 30]:
        q, slabs = helpers.lomb_t_slab_len(m), helpers.lomb_t_slabs(m)
        assert q % 1024 == 0 and q >= 2048 and slabs == -(-m // q) and 1 <= slabs <= 1024, (m, q, slabs)
        assert q == 2048 or (q - 1024) * 1024 < m, (m, q)   # the smallest such Q
    assert helpers.lomb_t_epsneg(0) == np.finfo(np.float64).epsneg and helpers.lomb_t_epsneg(1) == float(np.finfo(np.float32).epsneg)


def test_argument_rule(helpers):
    t, f, w = arr([0.0, 1.0, 2.5]), arr([0.1, 0.2]), arr([1.0, 0.0, 2.0])
    bad = lambda t_, m, f_, k, w_: bool(helpers.lomb_t_bad_args(ptr(t_), m, ptr(f_), k, ptr(w_)))  # noqa: E731
    assert not bad(t, 3, f, 2, None) and not bad(t, 3, f, 2, w)
    assert bad(None, 3, f, 2, None) and bad(t, 3, None, 2, None)
    assert bad(t, 0, f, 2, None) and bad(t, 3, f, 0, None) and bad(t, 2 ** 30 + 1, f, 2, None) and bad(t, 3, f, 2 ** 30 + 1, None)
    for v in (np.nan, np.inf, -np.inf):
        assert bad(arr([0.0, v, 1.0]), 3, f, 2, None) and bad(t, 3, arr([0.1, v]), 2, None) and bad(t, 3, f, 2, arr([1.0, v, 1.0]))
    assert bad(t, 3, arr([0.1, 1e308]), 2, None)         # 2 f overflows
    assert bad(t, 3, f, 2, arr([1.0, -1e-300, 1.0]))     # a negative weight
    assert bad(t, 3, f, 2, arr([0.0, 0.0, 0.0]))         # sum w = 0
    assert bad(t, 3, f, 2, arr([1e308, 1e308, 1e308]))   # sum w overflows
    out = np.zeros(3)
    helpers.lomb_t_weights(ptr(w), 3, ptr(out))
    assert np.array_equal(out, w / 3.0)
    helpers.lomb_t_weights(None, 3, ptr(out))
    assert np.array_equal(out, np.full(3, 1 / 3.0))


@pytest.mark.parametrize("weighted", [False, True])
def test_formulas_on_exact_sums(helpers, weighted):
    """lomb_table and lomb_post, fed the exact direct sums rounded to double, against the reference for every M <= 64, both
    mean settings, both clamps: at the gated frequencies within 64 eps64 / d of the largest value (the formulas are a dozen
    double operations, divided by CCt or SSt once), finite everywhere"""
    worst = 0.0
    for m in range(1, 65):
        rng = np.random.default_rng([m, 53])
        t, f = rng.uniform(0, R.SPAN, m), rng.uniform(0.05, 5.0, 5)
        y = rng.uniform(-3, 3, m)
        w = R.normalised(rng.uniform(0.5, 1.5, m) if weighted else None, m)
        for fm in MEANS:
            mean = (w * y).sum() if fm else R.LD(0)
            r = y.astype(R.LD) - mean
            a0, a1 = R.sums(t, f, [w, w * r])
            a2, = R.sums(t, 2 * f, [w])
            yy = (w * r * r).sum()
            d64 = [np.ascontiguousarray(v, np.float64) for v in (a0.real, a0.imag, a2.real, a2.imag, a1.real, a1.imag)]
            for f32 in (0, 1):
                want_tab = R.tables_of(a0, a2, fm, R.EPSNEG["f32" if f32 else "f64"])
                tab, out = np.zeros(4 * 5), np.zeros(3 * 5)
                helpers.lomb_t_tables(*(ptr(v) for v in d64[:4]), 5, int(fm), f32, ptr(tab))
                helpers.lomb_t_post(ptr(d64[4]), ptr(d64[5]), ptr(tab), 5, ptr(out))
                assert np.isfinite(tab).all() and np.isfinite(out).all(), (m, fm, f32)
                mask = R.gated(want_tab)
                if not mask.any():
                    continue
                d = R.smallest_d(want_tab, mask)
                ct, st = tab[:5], tab[5:10]
                got = {"power": out[:5] * m / 4, "normalize": out[:5] * 0.5 / float(yy) if yy else None,
                       "amplitude": (out[5:10] + 1j * out[10:]) * (ct + 1j * st)}
                for norm in R.NORMS:
                    if got[norm] is None:
                        continue
                    err = R.error(got[norm], R.post(a1, want_tab, m, yy, norm), mask)
                    worst = max(worst, err * d)
                    assert err <= 64 * tol.EPS64 / d, (m, fm, f32, norm, err, d)
    print(f"formulas weighted={weighted}: worst err * d = {worst:.3e}")


# ---------------------------------------------------------------------------------------------
# the C ABI and the Python layer without a device
# ---------------------------------------------------------------------------------------------
def test_every_bad_argument_is_refused_before_the_device():
    """PHAST_ERR_INVALID_ARG from _new and the one-shot form whether or not a GPU is there; a good call gets past the check
    (here: to the device, or to PHAST_ERR_NO_DEVICE)"""
    from phastft_amd import _lib

    lib = _lib.lib()
    t, f, w = arr([0.0, 1.0, 2.5]), arr([0.1, 0.2]), arr([1.0, 0.5, 2.0])
    wide_t, wide_f = arr([0.0, 1e9]), arr([0.0, 1e3])        # 8 S X = 4e12: no grid within the type-3 limit
    twice_t, twice_f = arr([0.0, 2.0 ** 27]), arr([0.0, 0.9])  # the grid of (t, f) fits (8 S X = 0.9 * 2^28), the one of 2 f does not
    cases = [(None, 3, f, 2, None, 0, 1e-6), (t, 3, None, 2, None, 0, 1e-6), (t, 0, f, 2, None, 0, 1e-6), (t, 3, f, 0, None, 0, 1e-6),
             (t, 2 ** 30 + 1, f, 2, None, 0, 1e-6), (t, 3, f, 2 ** 30 + 1, None, 0, 1e-6), (arr([0.0, np.nan, 1.0]), 3, f, 2, None, 0, 1e-6),
             (t, 3, arr([0.1, np.inf]), 2, None, 0, 1e-6), (t, 3, f, 2, arr([1.0, np.nan, 1.0]), 0, 1e-6),
             (t, 3, f, 2, arr([1.0, -1.0, 1.0]), 0, 1e-6), (t, 3, f, 2, arr([0.0, 0.0, 0.0]), 0, 1e-6), (t, 3, f, 2, w, 2, 1e-6),
             (t, 3, f, 2, w, 0, 0.11), (t, 3, f, 2, w, 0, 0.9e-14), (wide_t, 2, wide_f, 2, None, 0, 1e-6),
             (twice_t, 2, twice_f, 2, None, 0, 1e-6)]
    for sfx, fs, dt in (("64", "f64", np.float64), ("32", "f32", np.float32)):
        new, shot = getattr(lib, f"phast_planner_lomb{sfx}_new"), getattr(lib, f"phast_lombscargle_{fs}")
        y, o = np.zeros(8, dt), np.zeros(8, dt)
        for t_, m, f_, k, w_, fm, eps in cases + ([(t, 3, f, 2, w, 0, 0.9e-6)] if sfx == "32" else []):
            h = C.c_void_p(1)
            assert new(ptr(t_), m, ptr(f_), k, ptr(w_), fm, eps, C.byref(h)) == INVALID_ARG, (sfx, m, k, fm, eps)
            assert h.value is None
            assert shot(ptr(t_), m, ptr(f_), k, ptr(w_), fm, eps, ptr(y), ptr(o), ptr(o), 0) == INVALID_ARG
        assert new(ptr(t), 3, ptr(f), 2, ptr(w), 1, 1e-3, None) == INVALID_ARG
        h = C.c_void_p()
        rc = new(ptr(t), 3, ptr(f), 2, ptr(w), 1, 1e-3, C.byref(h))
        assert rc in (OK, NO_DEVICE)
        if rc == OK:
            getattr(lib, f"phast_planner_lomb{sfx}_free")(h)
        assert getattr(lib, f"phast_lombscargle_{fs}_with_planner")(ptr(y), 3, ptr(o), 2, ptr(o), 2, 0, None) == INVALID_ARG
        assert getattr(lib, f"phast_lombscargle_{fs}_dev")(ptr(y), ptr(o), ptr(o), 3, 1, 3, 2, 0, None, ptr(o), 8, None) == INVALID_ARG
        for name in ("slab", "grid_len", "device_bytes", "workspace_min"):
            assert getattr(lib, f"phast_planner_lomb{sfx}_{name}")(None) == 0
        assert getattr(lib, f"phast_planner_lomb{sfx}_workspace_len")(None, 3) == 0
        assert getattr(lib, f"phast_planner_lomb{sfx}_describe")(None, None, 0) == INVALID_ARG


def test_twice_the_frequencies_is_the_grid_that_decides():
    """the last pair of the cases above: the grid of (t, f) is within the type-3 limit of 2^28 at every eps, the one of
    (t, 2 f) is not -- the periodogram is refused for the tables' sake"""
    t, f = arr([0.0, 2.0 ** 27]), arr([0.0, 0.9])
    for eps in (1e-1, 1e-6, 1e-14):
        assert schedule(t, f, eps)["nf"] == 2 ** 28 and schedule(t, 2 * f, eps)["nf"] == 2 ** 29


def test_python_argument_errors():
    import phastft_amd as P

    t, f = np.linspace(0, 1, 5), np.array([0.5, 1.0])
    with pytest.raises(ValueError, match="weights"):
        P.PlannerLomb64(t, f, weights=np.ones(4))
    for bad in ("psd", 2, None):
        with pytest.raises(ValueError, match="normalize"):
            P.lombscargle_f64_with_planner(np.zeros(5), np.zeros(2), None, normalize=bad)
    with pytest.raises(TypeError):
        P.lombscargle(t, np.zeros(5), f)                  # a host array: the convenience takes device tensors
    with pytest.raises(P.PhastPanic) as e:
        P.PlannerLomb32(t, f, eps=1e-9)                   # below the f32 range
    assert e.value.code == INVALID_ARG
    with pytest.raises(P.PhastPanic) as e:
        P.PlannerLomb64(t, f, weights=-np.ones(5))
    assert e.value.code == INVALID_ARG


def test_new_symbols_are_exported_and_listed():
    from phastft_amd import _lib

    lib = _lib.lib()
    for name in NEW:
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    import phastft_amd as P

    for name in ("PlannerLomb64", "PlannerLomb32", "lombscargle_batched", "lombscargle_f64_with_planner",
                 "lombscargle_f32_with_planner", "lombscargle"):
        assert name in P.__all__ and hasattr(P, name), name
    assert "PlannerLomb64/32" in P.__doc__
    header = open(os.path.join(ROOT, "include", "phastft_hip.h")).read()
    for name, code in (("POWER", 0), ("NORMALIZE", 1), ("AMPLITUDE", 2)):
        assert f"#define PHAST_LOMB_{name} {code}\n" in header


# ---------------------------------------------------------------------------------------------
# the whole schedule in numpy
# ---------------------------------------------------------------------------------------------
def lomb_model(ref, weighted, fm, norm, seed, eps, dt):
    """planner_lomb.hpp's schedule: tables from the exact sums, rounded to T; the weights rounded to T; the mean as y_0 plus
    the weighted mean difference in double; the strengths rounded to T; tests/test_nufft_t3_cpu.py's model of the type-3
    transform (Reverse); the post formulas in double, rounded to T once"""
    nd = np.float64 if dt == "f64" else np.float32
    m = ref.case[0]
    tab = [np.asarray(v, np.float64).astype(nd).astype(np.float64) for v in ref.tab[(weighted, fm, dt)]]
    ct, st, icc, iss = tab[0], tab[1], (1 / np.asarray(ref.tab[(weighted, fm, dt)][2], np.float64)).astype(nd).astype(np.float64), \
        (1 / np.asarray(ref.tab[(weighted, fm, dt)][3], np.float64)).astype(nd).astype(np.float64)
    w = np.asarray(R.normalised(ref.w if weighted else None, m), np.float64).astype(nd).astype(np.float64)
    inv = 1.0 / w.sum()
    y = ref.y[seed]
    y0 = y[0] if fm else 0.0
    d = (w * (y - y0)).sum() * inv if fm else 0.0
    r = (y - y0) - d
    c = (w * r).astype(nd)
    yy = (w * r * r).sum() * inv
    a1 = t3_model(ref.t, ref.f, c.astype(np.float64), eps, R3.REVERSE, nd).astype(np.complex128)
    yc, ys = a1.real * ct + a1.imag * st, a1.imag * ct - a1.real * st
    a, b = yc * icc, ys * iss
    p = 2 * (a * yc + b * ys)
    if norm == "power":
        return (p * (m / 4)).astype(nd)
    if norm == "normalize":
        return (p * (0.5 / yy)).astype(nd)
    return ((a * ct - b * st).astype(nd) + 1j * (a * st + b * ct).astype(nd))


@pytest.mark.parametrize("case", [c for c in R.CASES if c[0] <= 1000], ids=R.case_id)
def test_schedule_model_against_the_reference(case):
    """the model inside the gate at every eps of both types, weights or none, both means, the three normalisations; ungated
    frequencies finite"""
    ref = reference(case)
    worst = 0.0
    for dt in ("f64", "f32"):
        for eps in R.EPS[dt]:
            n_g = 2 * schedule(ref.t, ref.f, eps)["nf"]
            for weighted in (False, True):
                for fm in MEANS:
                    key = (weighted, fm, dt)
                    for norm in ref.norms():
                        got = lomb_model(ref, weighted, fm, norm, 0, eps, dt)
                        assert np.isfinite(got).all()
                        err = R.error(got, ref.ref[(weighted, fm, norm, 0, dt)], ref.mask[key])
                        gate = lomb_gate(dt, n_g, eps, ref.q, ref.d[key], norm)
                        worst = max(worst, err / gate)
                        assert err <= gate, (case, dt, eps, weighted, fm, norm, err, gate)
    print(f"model {R.case_id(case)}: worst err / gate = {worst:.3f}")
