"""The host half of the type-3 non-uniform FFT (csrc/nufft_t3.hpp), compiled with g++ and held against Python fractions and
numpy: the grid rule and its degenerate replacements, the ranges of the rescaled points, the argument check one step either
side of every limit, the exact phases of the two tables, phi^ at a real argument -- and a numpy model of the whole schedule
against the long double direct sum of tests/nufft_t3_reference.py.

The gate of a type-3 transform (nufft_t3_gate) is C3 eps + KAPPA Q 2^-53 + tests/tolerances.py's formula on log2 n_g, with
Q = 2 pi (|C_s| + S) X the conditioning of the problem: x_j - C_x and s_k - C_s are rounded in double, and no method that
starts from the doubles can do better.  C3 and KAPPA are the smallest round numbers that leave every entry of
tests/golden/nufft_t3_error_budget.json a factor of 2 (tests/test_gpu_nufft_t3.py: test_gates_keep_their_margin)."""
import ctypes as C
import functools
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from tests import nufft_reference as R1
from tests import nufft_t3_reference as R
from tests import tolerances as tol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = [f"phast_planner_nufft_t3_{s}_{w}" for s in ("64", "32")
       for w in ("new", "free", "describe", "device_bytes", "grid_len", "width", "workspace_len", "time_stages")]
NEW += [f"phast_nufft3_{s}{suffix}" for s in ("64", "32") for suffix in ("", "_with_planner", "_dev")]
OK, NO_DEVICE, INVALID_ARG = 0, 15, 16
C3 = {"f64": 40.0, "f32": 20.0}
KAPPA = 10.0


def nufft_t3_gate(dt, n_g, eps, q):
    """(rel-L2, worst element / rms) of a type-3 transform asked for eps, of conditioning q, on an inner grid of n_g points"""
    log_g = n_g.bit_length() - 1
    base = C3[dt] * eps + KAPPA * q * 2.0 ** -53
    return base + tol.rel_gate(dt, log_g), base + tol.bin_gate(dt, log_g)


@functools.lru_cache(maxsize=None)
def reference(case):
    """the long double reference of a case: computed once, shared, left unchanged"""
    pick = None
    if case == R.BIG:
        pick = tuple(int(i) for i in np.sort(np.random.default_rng(5).choice(case[1], R.BIG_PICK, replace=False)))
    ref = R.Reference(case, pick)
    for pair in ref.ref.values():
        for a in pair:
            a.flags.writeable = False
    return ref


@pytest.fixture(scope="module")
def helpers(tmp_path_factory):
    so = tmp_path_factory.mktemp("nufft_t3_helpers") / "libnufftt3helpers.so"
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-shared", "-fPIC", "-I", os.path.join(ROOT, "phastft_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "nufft_t3_test.cpp"), "-o", str(so)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    h = C.CDLL(str(so))
    u, d, p = C.c_ulonglong, C.c_double, C.c_void_p
    h.nufft_t3_t_bad_args.argtypes = [p, u, p, u, d, C.c_int]
    h.nufft_t3_t_grid.argtypes, h.nufft_t3_t_grid.restype = [p, u, p, u, d, p, p], u
    h.nufft_t3_t_points.argtypes, h.nufft_t3_t_points.restype = [p, u, p, u, d, p, p], None
    h.nufft_t3_t_phase64.argtypes, h.nufft_t3_t_phase64.restype = [d, d, p, p], None
    h.nufft_t3_t_phase32.argtypes, h.nufft_t3_t_phase32.restype = [d, d, p, p], None
    h.nufft_t3_t_tables.argtypes, h.nufft_t3_t_tables.restype = [p, u, p, u, d, p, p, p, p, p, p], None
    h.nufft_t3_t_phi_hat.argtypes, h.nufft_t3_t_phi_hat.restype = [C.c_int, p, C.c_size_t, p], None
    return h


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def arr(v):
    return np.array(v, np.float64)


# ---------------------------------------------------------------------------------------------
# the schedule of csrc/nufft_t3.hpp in Python
# ---------------------------------------------------------------------------------------------
def schedule(x, s, eps):
    """centres, half-widths with the degenerate replacements, w, n_f and h"""
    x, s = np.asarray(x, np.float64), np.asarray(s, np.float64)
    cx, cs = 0.5 * x.min() + 0.5 * x.max(), 0.5 * s.min() + 0.5 * s.max()
    X, S = np.abs(x - cx).max(), np.abs(s - cs).max()
    if X == 0 and S == 0:
        X = S = 1.0
    elif X == 0:
        X = 1 / S
    elif S == 0:
        S = 1 / X
    w = R1.width(eps)
    nf = 8
    while nf < 8 * S * X + w or nf < 2 * w:
        nf <<= 1
    return {"cx": cx, "cs": cs, "X": X, "S": S, "w": w, "nf": nf, "h": 1 / (4 * S)}


def exact_turn(a, b):
    """a b mod 1 in [-1/2, 1/2) from the exact values of the two doubles"""
    f = Fraction(float(a)) * Fraction(float(b)) % 1
    return f - 1 if f >= Fraction(1, 2) else f


def phase(a, b):
    """exp(2 pi i a b) in double from the exact turn"""
    t = exact_turn(a, b)
    ang = float(R.TWO_PI * (R.LD(t.numerator) / R.LD(t.denominator)))   # |t| <= 1/2: the quotient is good to a long double
    return complex(math.cos(ang), math.sin(ang))


def phi_hat_real(xi, w, nodes=32):
    """phi^_outer at xi turns per cell: tests/nufft_reference.py's rule with k / n_g = xi"""
    return R1.phi_hat(np.asarray(xi, np.float64), 1, w, nodes)


def model(x, s, c, eps, direction=R.FORWARD, dt=np.float64):
    """the four stages in numpy: the outer spread with the prephase, the inner type 2 of tests/nufft_reference.py's model
    (pre, numpy's FFT, interpolate) at the rescaled targets, and the post factors; `dt`: the arithmetic of the kernel values,
    the grids and the tables"""
    cd = np.complex128 if dt == np.float64 else np.complex64
    g = schedule(x, s, eps)
    w, nf = g["w"], g["nf"]
    sign = -1 if direction == R.FORWARD else 1
    xp, sp = np.asarray(x, np.float64) - g["cx"], np.asarray(s, np.float64) - g["cs"]
    u = 4 * g["S"] * xp / nf + 0.5
    q, off = R1._cells(u, nf)
    pre = np.array([phase(g["cs"], v) for v in xp]).astype(cd)
    pre = pre if sign > 0 else pre.conj()
    v = (np.asarray(c).astype(cd) * pre).astype(cd)
    first = 1 - (w + 1) // 2 + ((w & 1) & (off >= 0.5))
    grid = np.zeros(nf, cd)
    for i in range(w):
        dq = first + i
        assert ((q + dq >= 0) & (q + dq < nf) | (R1.phi((dq - off) * (2.0 / w), 2.30 * w) == 0)).all()   # nothing wraps
        np.add.at(grid, (q + dq) % nf, R1.phi((dq - off) * (2.0 / w), 2.30 * w).astype(dt) * v)
    modes = np.roll(grid, -(nf // 2))   # mode k = l - n_f / 2 in fftfreq order
    t = sp * g["h"]
    inner = R1.model(2, t, modes, nf, eps, direction, dt)
    post = np.array([phase(sk, g["cx"]) for sk in np.asarray(s, np.float64)])
    post = (post if sign > 0 else post.conj()) / phi_hat_real(t, w)
    return (inner * post.astype(cd)).astype(cd)


# ---------------------------------------------------------------------------------------------
# the grid rule, the ranges and the argument check
# ---------------------------------------------------------------------------------------------
def c_grid(h, x, s, eps):
    x, s = arr(x), arr(s)
    out, w = np.zeros(5), C.c_int()
    nf = h.nufft_t3_t_grid(ptr(x), len(x), ptr(s), len(s), eps, ptr(out), C.byref(w))
    return {"cx": out[0], "cs": out[1], "X": out[2], "S": out[3], "h": out[4], "w": w.value, "nf": nf}


# (x, s, eps) -> (C_x, C_s, X, S, w, n_f), by hand
GRID_CASES = [
    (([-1.0, 1.0], [-2.0, 2.0], 1e-6), (0.0, 0.0, 1.0, 2.0, 7, 32)),            # 8 S X + w = 23
    (([0.0, 4.0], [10.0, 12.0], 1e-3), (2.0, 11.0, 2.0, 1.0, 4, 32)),           # 16 + 4 = 20
    (([-1.0, 1.0], [-3.0, 3.0], 1e-1), (0.0, 0.0, 1.0, 3.0, 2, 32)),            # 24 + 2 = 26
    (([-1.0, 1.0], [-3.75, 3.75], 1e-1), (0.0, 0.0, 1.0, 3.75, 2, 32)),         # 30 + 2 = 32: exactly a power of two
    (([-1.0, 1.0], [-3.875, 3.875], 1e-1), (0.0, 0.0, 1.0, 3.875, 2, 64)),      # 31 + 2 = 33
    (([5.0], [7.0], 1e-1), (5.0, 7.0, 1.0, 1.0, 2, 16)),                        # X = S = 0 -> 1, 1: 8 + 2 = 10
    (([5.0, 5.0], [-4.0, 4.0], 1e-6), (5.0, 0.0, 0.25, 4.0, 7, 16)),            # X = 0 -> 1 / S: 8 + 7 = 15
    (([-8.0, 8.0], [3.0], 1e-12), (0.0, 3.0, 8.0, 0.125, 13, 32)),              # S = 0 -> 1 / X: 8 + 13 = 21, 2 w = 26
    (([0.0, 1e-3], [0.0, 1.0], 1e-14), (5e-4, 0.5, 5e-4, 0.5, 15, 32)),         # n_f from 2 w = 30
    (([0.0, 1e-3], [0.0, 1.0], 1e-2), (5e-4, 0.5, 5e-4, 0.5, 3, 8)),            # n_f from the floor of 8
]


def test_grid_rule(helpers):
    for (x, s, eps), (cx, cs, X, S, w, nf) in GRID_CASES:
        for g in (c_grid(helpers, x, s, eps), schedule(x, s, eps)):
            assert (g["cx"], g["cs"], g["X"], g["S"], g["w"], g["nf"]) == (cx, cs, X, S, w, nf), (x, s, eps, g)
            assert g["h"] == 1 / (4 * S)


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_ranges(helpers, case):
    """every |t_k| <= 1/4, every p_j within [w / 2, n_f - w / 2], and the C schedule is the Python one"""
    x, s = R.points(case)
    for eps in (1e-1, 1e-6, 1e-14):
        g, py = c_grid(helpers, x, s, eps), schedule(x, s, eps)
        assert {k: g[k] for k in py} == py, (case, eps)
        assert 0 < g["nf"] <= 2 ** 14
        u, t = np.zeros(len(x)), np.zeros(len(s))
        helpers.nufft_t3_t_points(ptr(x), len(x), ptr(s), len(s), eps, ptr(u), ptr(t))
        assert np.abs(t).max() <= 0.25
        p = u * g["nf"]   # exact: n_f is a power of two
        assert p.min() >= g["w"] / 2 and p.max() <= g["nf"] - g["w"] / 2, (case, eps, p.min(), p.max())


def bad(h, x, s, eps, f32=False, m=None, k=None):
    xa, sa = (None if v is None else arr(v) for v in (x, s))
    return bool(h.nufft_t3_t_bad_args(None if xa is None else ptr(xa), len(x) if m is None else m,
                                      None if sa is None else ptr(sa), len(s) if k is None else k, eps, int(f32)))


def limit_pair(w, over):
    """x = +-X and s = +-1 with 8 S X + w one step below or at 2^28 (n_f = 2^28), or one step above (n_f = 2^29)"""
    X = (2 ** 28 - w) / 8
    return [-X, X * (1 + (2.0 ** -40 if over else 0))], [-1.0, 1.0]


def test_argument_rule(helpers):
    one = [0.5]
    assert not bad(helpers, one, one, 1e-6)
    # the counts, one step either side (the arrays are not read past a refused count)
    assert bad(helpers, one, one, 1e-6, m=0) and bad(helpers, one, one, 1e-6, k=0)
    assert bad(helpers, one, one, 1e-6, m=2 ** 30 + 1) and bad(helpers, one, one, 1e-6, k=2 ** 30 + 1)
    assert bad(helpers, None, one, 1e-6, m=1) and bad(helpers, one, None, 1e-6, k=1)
    # eps
    for eps, f32, want in ((1e-14, False, False), (0.9e-14, False, True), (1e-1, False, False), (0.11, False, True),
                           (1e-6, True, False), (0.9e-6, True, True), (0.9e-6, False, False), (float("nan"), False, True),
                           (0.0, False, True), (-1e-3, False, True)):
        assert bad(helpers, one, one, eps, f32) == want, (eps, f32)
    # every point finite
    for v in (float("nan"), float("inf"), -float("inf")):
        assert bad(helpers, [0.1, v], one, 1e-6) and bad(helpers, one, [v, 0.1], 1e-6)
    assert not bad(helpers, [1e300, -5.0], [1e-300], 1e-6)   # X large, S = 0 -> 1 / X
    assert bad(helpers, [1e308, -1e308], [1.0, 2.0], 1e-6)   # a half-width that is not finite
    # the fine grid, one step either side of 2^28
    for eps in (1e-1, 1e-6, 1e-14):
        w = R1.width(eps)
        x, s = limit_pair(w, False)
        assert not bad(helpers, x, s, eps) and c_grid(helpers, x, s, eps)["nf"] == 2 ** 28
        x, s = limit_pair(w, True)
        assert bad(helpers, x, s, eps) and c_grid(helpers, x, s, eps)["nf"] == 0
    # phases that no double holds
    assert bad(helpers, [1e200], [1e200], 1e-6) and not bad(helpers, [1e150], [1e150], 1e-6)


def test_every_bad_argument_is_refused_before_the_device():
    """PHAST_ERR_INVALID_ARG from _new and the one-shot form whether or not a GPU is there; a good call gets past the check
    (here: to the device, or to PHAST_ERR_NO_DEVICE)"""
    from phastft_amd import _lib

    lib = _lib.lib()
    over_x, over_s = (arr(v) for v in limit_pair(7, True))
    cases = [(None, 1, arr([0.5]), 1, 1e-6), (arr([0.5]), 1, None, 1, 1e-6), (arr([0.5]), 0, arr([0.5]), 1, 1e-6),
             (arr([0.5]), 1, arr([0.5]), 0, 1e-6), (arr([0.5]), 2 ** 30 + 1, arr([0.5]), 1, 1e-6),
             (arr([0.5]), 1, arr([0.5]), 2 ** 30 + 1, 1e-6), (arr([0.5]), 1, arr([0.5]), 1, 0.11),
             (arr([0.5]), 1, arr([0.5]), 1, 0.9e-14), (arr([0.5, np.nan]), 2, arr([0.5]), 1, 1e-6),
             (arr([0.5]), 1, arr([np.inf, 0.5]), 2, 1e-6), (over_x, 2, over_s, 2, 1e-6)]
    for sfx, dt in (("64", np.float64), ("32", np.float32)):
        new, shot = getattr(lib, f"phast_planner_nufft_t3_{sfx}_new"), getattr(lib, f"phast_nufft3_{sfx}")
        v, o = np.zeros(8, dt), np.zeros(8, dt)
        for x, m, s, k, eps in cases + ([(arr([0.5]), 1, arr([0.5]), 1, 0.9e-6)] if sfx == "32" else []):
            h = C.c_void_p(1)
            px, ps = (None if a is None else ptr(a) for a in (x, s))
            assert new(px, m, ps, k, eps, C.byref(h)) == INVALID_ARG, (sfx, m, k, eps)
            assert h.value is None
            assert shot(px, m, ps, k, ptr(v), ptr(v), ptr(o), ptr(o), eps, 1) == INVALID_ARG
        x, s = arr([0.1, 0.2]), arr([1.0, -2.0, 3.0])
        assert new(ptr(x), 2, ptr(s), 3, 1e-3, None) == INVALID_ARG
        h = C.c_void_p()
        rc = new(ptr(x), 2, ptr(s), 3, 1e-3, C.byref(h))
        assert rc in (OK, NO_DEVICE)
        if rc == OK:
            getattr(lib, f"phast_planner_nufft_t3_{sfx}_free")(h)
        assert shot(ptr(x), 2, ptr(s), 3, None, ptr(v), ptr(o), ptr(o), 1e-3, 1) == INVALID_ARG
        assert getattr(lib, f"phast_nufft3_{sfx}_with_planner")(ptr(v), ptr(v), 2, ptr(o), ptr(o), 3, 1, None) == INVALID_ARG
        assert getattr(lib, f"phast_nufft3_{sfx}_dev")(ptr(v), ptr(v), 2, ptr(o), ptr(o), 3, 1, 1, None, ptr(o), 8, None) == INVALID_ARG
        for name in ("grid_len", "width", "device_bytes"):
            assert getattr(lib, f"phast_planner_nufft_t3_{sfx}_{name}")(None) == 0
        assert getattr(lib, f"phast_planner_nufft_t3_{sfx}_workspace_len")(None, 3) == 0


def test_new_symbols_are_exported_and_listed():
    from phastft_amd import _lib

    lib = _lib.lib()
    for name in NEW:
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    import phastft_amd as P

    for name in ("PlannerNufftT3_64", "PlannerNufftT3_32", "nufft3_batched", "nufft3", "nufft3_64", "nufft3_32",
                 "nufft3_64_with_planner", "nufft3_32_with_planner"):
        assert name in P.__all__ and hasattr(P, name), name


# ---------------------------------------------------------------------------------------------
# the tables
# ---------------------------------------------------------------------------------------------
def test_phase_is_exact_mod_one_turn(helpers):
    """(cos, sin) of 2 pi a b within 1 ulp of T of the value of the exact product, at |a b| up to 1e12 and beyond"""
    rng = np.random.default_rng(11)
    pairs = [(rng.uniform(-1, 1) * 10.0 ** rng.uniform(0, 6), rng.uniform(-1, 1) * 10.0 ** rng.uniform(0, 6)) for _ in range(300)]
    pairs += [(1e6, 1e6), (-3e5 * 8.0, 1e6 * 2.0 + 0.3), (0.1, 0.1), (1e12, 1 + 2.0 ** -52), (123456.789, -98765.4321),
              (1e15 + 0.125, 1e15 + 0.375), (0.0, 5.0), (2.0 ** -600, 2.0 ** -600)]
    for dt, fn, ulp in ((np.float64, helpers.nufft_t3_t_phase64, 2.0 ** -52), (np.float32, helpers.nufft_t3_t_phase32, 2.0 ** -23)):
        worst = 0.0
        for a, b in pairs:
            c, s = np.zeros(1, dt), np.zeros(1, dt)
            fn(a, b, ptr(c), ptr(s))
            t = exact_turn(a, b)
            ang = R.TWO_PI * (R.LD(t.numerator) / R.LD(t.denominator))
            worst = max(worst, abs(float(R.LD(c[0]) - np.cos(ang))), abs(float(R.LD(s[0]) - np.sin(ang))))
        assert worst <= ulp, (dt, worst)


@pytest.mark.parametrize("case", [c for c in R.CASES if c[4] in ("off", "far")] + [(50, 20, 1.0, 4.0, "huge")], ids=R.case_id)
def test_phase_tables(helpers, case):
    """the prephase table (sorted order) and the phase of the post table against the exact fractions, to 1 ulp; the sorted
    positions are the binned fractions of the outer grid"""
    if case[4] == "huge":   # |C_s x'| and |s C_x| near 1e12
        x, s = R.points(case[:4] + ("u",))
        x, s = x + 1.0, s - 1e12
    else:
        x, s = R.points(case)
    eps = 1e-9
    g = c_grid(helpers, x, s, eps)
    m, k, nf = len(x), len(s), g["nf"]
    xs, perm, cell = np.zeros(m), np.zeros(m, np.uint32), np.zeros(nf + 1, np.uint32)
    pre, d_re, d_im = np.zeros(2 * m), np.zeros(k), np.zeros(k)
    helpers.nufft_t3_t_tables(ptr(x), m, ptr(s), k, eps, ptr(xs), ptr(perm), ptr(cell), ptr(pre), ptr(d_re), ptr(d_im))
    assert sorted(perm.tolist()) == list(range(m)) and cell[0] == 0 and cell[nf] == m and (np.diff(cell.astype(np.int64)) >= 0).all()
    u = 4 * g["S"] * (x - g["cx"]) / nf + 0.5
    assert np.array_equal(xs, u[perm]) and (np.diff(np.floor(xs * nf)) >= 0).all()
    for q in range(nf):
        assert (np.floor(xs[cell[q]:cell[q + 1]] * nf) == q).all()
    want = np.array([phase(g["cs"], x[j] - g["cx"]) for j in perm])
    assert np.abs(pre[0::2] - want.real).max() <= 2.0 ** -52 and np.abs(pre[1::2] - want.imag).max() <= 2.0 ** -52
    hat = np.zeros(k)
    t = (s - g["cs"]) * g["h"]
    helpers.nufft_t3_t_phi_hat(g["w"], ptr(t), k, ptr(hat))
    want = np.array([phase(sk, g["cx"]) for sk in s]).conj()
    got = (d_re + 1j * d_im) * hat
    # the table's rounding and the product's, half an ulp each
    assert np.abs(got.real - want.real).max() <= 2.0 ** -52 and np.abs(got.imag - want.imag).max() <= 2.0 ** -52


def test_phi_hat_at_a_real_argument(helpers):
    """the 32-node rule at |xi| <= 1/4 against the tanh-sinh trapezoid sum, to 1e-13 of phi^(0), for every width"""
    xi = np.concatenate([np.linspace(-0.25, 0.25, 201), np.random.default_rng(3).uniform(-0.25, 0.25, 100)])
    for w in range(2, 17):
        got = np.zeros(len(xi))
        helpers.nufft_t3_t_phi_hat(w, ptr(xi), len(xi), ptr(got))
        want = R1.phi_hat_trapezoid(xi, 1, w)
        assert np.abs(got - want).max() <= 1e-13 * want.max(), w
        assert np.abs(got - phi_hat_real(xi, w)).max() <= 1e-14 * want.max(), w   # the model's rule is the same rule


# ---------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in R.CASES if c[0] <= 1000], ids=R.case_id)
def test_schedule_model_against_the_reference(case):
    """the numpy model of the four stages meets the gate against the direct sum, both dtypes, both directions, real data too"""
    ref = reference(case)
    for dt, ndt in (("f64", np.float64), ("f32", np.float32)):
        for eps in (R.EPS[dt][0], R.EPS[dt][-1]):
            n_g = 2 * schedule(ref.x, ref.s, eps)["nf"]
            g_rel, g_bin = nufft_t3_gate(dt, n_g, eps, ref.q)
            for d, real in ((R.FORWARD, False), (R.REVERSE, True)):
                got = model(ref.x, ref.s, ref.inp(real, 0), eps, d, ndt)
                want = ref.ref[(d, real, 0)]
                rel, worst = tol.rel_l2(got.real, got.imag, *want), tol.max_bin_err(got.real, got.imag, *want)
                assert rel <= g_rel and worst <= g_bin, (case, dt, eps, d, real, rel, g_rel, worst, g_bin)


def test_reference_against_python_fractions():
    """the vectorised integers of the reference against Fraction arithmetic, element by element"""
    rng = np.random.default_rng(2)
    x = np.concatenate([rng.uniform(-5, 5, 20) * 10.0 ** rng.integers(-3, 9, 20), [0.0, 1.0, -3.0, 2.0 ** -40]])
    for sk in (0.0, 1.0, -2.5, 1e6 + 0.1, -3.3e-7, 2.0 ** 30):
        got = R.turns(x, sk)
        for j, v in enumerate(x):
            t = exact_turn(v, sk)
            assert abs(float(got[j] - R.LD(t.numerator) / R.LD(t.denominator))) <= 2.0 ** -63, (v, sk)
