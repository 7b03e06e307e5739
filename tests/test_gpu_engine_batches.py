"""The power-of-two engine of the composite planners at the batch sizes only they give it.

Every composite planner (any-length complex and real transforms, DCT / DST, STFT, convolution, CZT, NUFFT, MDCT, Welch, resample)
runs its M-point transforms through ConvCore::engine (csrc/planner_any.hpp): the plan of ONE transform -- choose(kC2C, 1, 1) on
route_small(1) -- forced on exec_in for the c transforms of a chunk, "so the bits of a transform do not depend on what it is
batched with".  A direct call never does that: Planner::plan_for leaves the multi-pass twin of 4096 / 8192 points above 128
transforms, the wave / four-wave single plans above 4 transforms (or 2^19 points in flight), and a wisdom line of bucket 0 above
one.  What changes with c inside those kernels is index arithmetic (tiles_total = c * tiles_per_xform in locate, the XCD remap
when the tile or workgroup count is a multiple of 8, the rounded grid, the quad kernel's tile loop, the wave kernels' stagger
above 1024 tiles, the scratch planes at cap * stride), and this file holds it to four assertions per case of ROWS:

    1. every transform of the batch has the bits of the same transform run alone on the same planner;
    2. transforms 0, c // 2, c - 1 and both sides of every chunk boundary of exec_in's own loop pass the any-length module's
       gates (any_gates of tests/test_gpu_any_len.py; real_gates of tests/test_gpu_any_real.py) against numpy's long-double FFT;
    3. the gaps between the transforms (dist = n + 3) and the margins of the planes (which start at buf[1:]) keep their sentinel;
    4. the plan is the one the row names: describe_call(1) of a PlannerDit of M points made beside the planner -- the library's
       own answer for choose(kC2C, 1, 1) on route_small(1), which is the engine's rule -- and, for the static wave / four-wave
       plans, the marks tests/test_gpu_parity.py asserts on (" w16 ", " q16 "; f32: " w32 ") in the inner planner's describe().

The rows run with the built-in wisdom as the library ships it, and under the static rules of plan.hpp as well wherever the two
differ (BUILTIN).  The same kernels are also reached directly (set_plan on PlannerDit64/32 at batch 5, 8, 65), through R2C / C2R
of any length, and through an STFT of 71 frames of 10 000 samples.  The scratches carry guard bands for the whole module;
check_guards is asserted wherever the Python surface has it (PlannerDit*: the direct cases and the probe of assertion 4).

Plans that ran on the MI355X (printed per case as "engine_batches ..."; tests/golden/engine_batch_error_budget.json keeps them):

    type  M      c            rules     describe_call(1)
    f64   2^12   5, 130       both      single [64x16A p8][64x16 p8]                        (the twin, past 128)
    f32   2^12   5, 130       both      single [64x16A p8][64x16 p8]
    f64   2^13   9, 130       built-in  tuned [128x8A p8][64x16 p8]                         (f64 c2c 13 0 on the twin)
    f64   2^13   9, 130       static    single [64x16A w16][128x16 p8]
    f32   2^13   9, 130       built-in  tuned [64x16A p8][128x8 p8]
    f32   2^13   9, 130       static    latency [128x32A p8][64x64 p8]
    f64   2^14   33, 64, 65   built-in  tuned [128x8A p8][128x8 p8]                         (f64 c2c 14 0)
    f64   2^14   33, 64, 65   static    single [64x16A w16][256x16 q16]
    f32   2^14   33           built-in  tuned [64x16A p8][256x8 p8]
    f32   2^14   33           static    single [128x16A p8][128x16 p8]
    f64   2^15   17, 24, 5    both      single [128x8A p8][256x16 q16]                      (c = 5: the scratch of 2 transforms)
    f32   2^15   17           both      single [256x16A p8][128x16 p8]
    f64   2^18   5            built-in  tuned [64x16A p8][64x16 p8][64x16 p8]               (f64 c2c 18 0)
    f64   2^19   5, 8         both      single [64x16A w16][128x16 p8][64x16 w16]
    f32   2^19   5, 8         both      single [64x32A w32][128x32 p8][64x32 w32]
    f64   2^20   5            both      single [64x16A w16][256x16 q16][64x16 w16]
    f32   2^20   5, 8         both      single [64x32A w32][256x32 q16][64x32 w32]
    f64   2^21   5            both      single [64x16A w16][256x16 q16][128x32 p8]
    f32   2^22   5            built-in  tuned [128x64A p16][256x32 q16][128x32 p16]         (f32 c2c 22 0)
    f32   2^22   5            static    single [64x32A w32][256x32 q16][256x32 q16]
    ("both": no line of bucket 0 at this length -- one plan under either rule, run once with the wisdom on.)  The real cases and
    the STFT run the M = 2^14 built-in plans; the direct cases run "forced" with the static tiles of 2^20 (both types) and 2^14.

Gates: the existing ones, unchanged.  The measured use (error / gate, worst of rel-L2 and worst bin over the transforms of
assertion 2) is in tests/golden/engine_batch_error_budget.json, written on the MI355X by
tests/golden/make_engine_batch_error_budget.py; test_gates_keep_their_margin holds every entry to use <= 0.5.
Measured on an MI355X: worst use 0.123 (f32, N = 1 200 000, built-in line), f64 at most 0.045; every transform of every
case bit-identical to its single run.  The whole file: 46 tests in 7.2 s with the built-in wisdom on, 6.9 s under
PHAST_BUILTIN_WISDOM=0; the slowest case takes 0.9 s (the direct 2^20 batches: 52 reference FFTs on the host).

Teeth, checked once on a scratch build that is not committed: with TileBody::locate, WaveBody::locate_tile and QuadBody::locate
taking `xform = 0` for every tile beyond the first transform's (tile >= tiles_per_xform), assertion 1 fails at the first case.
It did: "f64 N=2000 c=5 builtin [single [64x16A p8][64x16 p8]]: transform 1 differs from the same transform run alone, first
at element 0".
"""
import functools
import importlib.util
import json
import os
import re as regex   # (`re` is a real plane throughout the tests)
import time

import numpy as np
import pytest

from tests import test_gpu_stft as S
from tests import tolerances as tol
from tests.test_gpu_any_len import _check, _dev_fft, _input, _planner, _ref, any_gates, conv_len
from tests.test_gpu_any_real import _check_c2r, _check_r2c, _dev_c2r, _dev_r2c, _ref_c2r, _ref_r2c, _signal, _spectrum, real_gates
from tests.test_gpu_any_real import _planner as _real_planner

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = os.path.join(ROOT, "tests", "golden", "engine_batch_error_budget.json")

_spec = importlib.util.spec_from_file_location("make_plan_space", os.path.join(ROOT, "tests", "golden", "make_plan_space.py"))
mps = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mps)

# (types, N, batches, built-in run only, what the row reaches); M = conv_len(N): the smallest N that reaches each plan
ROWS = [
    (("f64", "f32"), 2000, (5, 130), False, "M = 2^12: the multi-pass twin past kTwinMaxBatch = 128"),
    (("f64", "f32"), 3000, (9, 130), False, "M = 2^13: the twin (f64 static: wave tiles; built-in: 7,6@10,10) past 128"),
    (("f64",), 5000, (33, 64, 65), False, "M = 2^14: the wave plan past 2^19 points in flight; 1024 and 1040 tiles: the stagger on and "
                                          "off; 64: a workgroup count that is a multiple of 8, 33 and 65: not"),
    (("f64",), 12_000, (17, 24), False, "M = 2^15: the four-wave last pass past 2^19 points in flight, ragged and a multiple of 8"),
    (("f32",), 5000, (33,), False, "M = 2^14: the f32 static single plan (generic tiles); the built-in line f32 c2c 14 0"),
    (("f32",), 12_000, (17,), False, "M = 2^15: the f32 static single plan (generic tiles)"),
    (("f64",), 200_000, (5, 8), False, "M = 2^19: the three-pass wave plan past 4 transforms"),
    (("f64",), 300_000, (5,), False, "M = 2^20: the four-wave middle pass with more tiles than workgroups (the t += gridDim.x loop)"),
    (("f64",), 600_000, (5,), False, "M = 2^21: the {21, 6, 8, 7} wave plan"),
    (("f32",), 200_000, (5, 8), False, "M = 2^19: the f32 wave plan on float2 column pairs"),
    (("f32",), 300_000, (5, 8), False, "M = 2^20: the f32 wave / four-wave plan on float2 column pairs"),
    (("f32",), 1_200_000, (5,), False, "M = 2^22: {22, 6, 8, 8}; the built-in line f32 c2c 22 0"),
    (("f64",), 100_000, (5,), True, "M = 2^18: the built-in line f64 c2c 18 0 6,6,6@10,10,10 (built-in run only)"),
    # (the issue that asked for this file names N = 150 000 for the row above; 2 N - 1 > 2^18 there, so it is a second length of
    #  the three-pass wave plan: kept as it was asked for, with N = 100 000 beside it for the line it was meant to reach)
    (("f64",), 150_000, (5,), True, "M = 2^19: the three-pass wave plan at a second length"),
]

# the plan of ONE transform, in the notation of plan.hpp's PlanSpec and the wisdom text, per (type, log2 M):
# STATIC: plan.hpp -- single_plan's table, or (f32 2^13, which has no entry) the latency plan of heuristic_plan
STATIC = {
    ("f64", 12): ("single", "6,6@10,10:p8"), ("f64", 13): ("single", "6,7@10,11:p8w"), ("f64", 14): ("single", "6,8@10,12:p16w"),
    ("f64", 15): ("single", "7,8@10,12:p8w"), ("f64", 19): ("single", "6,7,6@10,11,10:p8w"), ("f64", 20): ("single", "6,8,6@10,12,10:p8w"),
    ("f64", 21): ("single", "6,8,7@10,12,12:p8w"),
    ("f32", 12): ("single", "6,6@10,10:p8"), ("f32", 13): ("latency", "7,6@12,12:p8"), ("f32", 14): ("single", "7,7@11,11:p8"),
    ("f32", 15): ("single", "8,7@12,11:p8"), ("f32", 19): ("single", "6,7,6@11,12,11:p8w"), ("f32", 20): ("single", "6,8,6@11,13,11:p8w"),
    ("f32", 22): ("single", "6,8,8@11,13,13:p8w"),
}
# BUILTIN: the lines of bucket 0 of csrc/builtin_wisdom.inc at these lengths; a length without one runs its static plan under
# both rules and is kept once, with the wisdom on (a line added later then fails assertion 4 here instead of running untested)
BUILTIN = {
    ("f64", 13): ("tuned", "7,6@10,10:p8"), ("f64", 14): ("tuned", "7,7@10,10:p8"), ("f64", 18): ("tuned", "6,6,6@10,10,10:p8"),
    ("f32", 13): ("tuned", "6,7@10,10:p8"), ("f32", 14): ("tuned", "6,8@10,11:p8"), ("f32", 22): ("tuned", "7,8,7@13,13,12:p16w"),
}
SENTINEL = 7.0
TAIL = 5   # sentinel elements behind the last transform (in front: the one element the planes skip)


def _log_m(n):
    return conv_len(n).bit_length() - 1


def cases():
    """(type, N, c, rules) of every run of the table"""
    out = []
    for dts, n, cs, builtin_only, _ in ROWS:
        for dt in dts:
            for c in cs:
                out.append((dt, n, c, "builtin"))
                if (dt, _log_m(n)) in BUILTIN and not builtin_only:
                    out.append((dt, n, c, "static"))
    return out


def expected_plan(dt, log_m, rules):
    return BUILTIN[(dt, log_m)] if rules == "builtin" and (dt, log_m) in BUILTIN else STATIC[(dt, log_m)]


class rules_of:
    """planners made inside see the built-in wisdom ("builtin": also where the suite runs under PHAST_BUILTIN_WISDOM=0) or the
    static rules alone ("static": what the static_rules fixture does); what was set before comes back"""

    def __init__(self, P, rules):
        self.P, self.on = P, rules == "builtin"

    def __enter__(self):
        self.was = self.P.wisdom_builtin(self.on)

    def __exit__(self, *exc):
        self.P.wisdom_builtin(self.was)


@pytest.fixture(scope="module")
def guarded(gpu):
    """guard bands around every scratch allocated while the module runs (as tests/test_gpu_plan_space.py's fixture)"""
    gpu.debug_set_guard_bytes(1 << 20)
    try:
        yield gpu
    finally:
        gpu.debug_set_guard_bytes(0)


@functools.lru_cache(maxsize=12)
def _reference(dt, n, b):
    """the long-double forward FFT of transform b of a case's batch, as float64 planes: computed once, shared by the rules"""
    re, im = _input(n, dt, seed=10 + b)
    ref = _ref(re, im, 1)
    out = np.asarray(ref.real, np.float64), np.asarray(ref.imag, np.float64)
    for v in out:
        v.flags.writeable = False
    return out


def check_plan(P, dt, pl, rules):
    """assertion 4; returns the describe_call text"""
    log_m = pl.m.bit_length() - 1
    which, spec = expected_plan(dt, log_m, rules)
    probe = (P.PlannerDit64 if dt == "f64" else P.PlannerDit32)(pl.m)
    call = probe.describe_call(1, 0)
    tiles = "".join(mps.tile_strings(spec, dt))
    assert call == f"{which} {tiles}", (dt, pl.m, rules, call, which, tiles)
    desc = pl.describe()
    assert f"M={pl.m} (Bluestein)" in desc, desc
    if which == "single":   # the composite's own inner planner lists the same tiles as its single= plan
        single = regex.search(r" single=\d+p((?:\[[^\]]*\])+)", desc).group(1)
        assert [t[:-1] for t in mps.tile_strings(spec, dt)] == regex.findall(r"(\[[^\]]*?) lds=", single), (spec, desc)
        if spec.endswith("w"):   # the marks tests/test_gpu_parity.py asserts on, and their f32 equivalents
            marks = {"wave": " w16 " if dt == "f64" else " w32 ", "quad": " q16 "}
            kinds = [k for _, k, _, _ in mps.pass_classes(spec, dt) if k in marks]
            assert kinds and all(single.count(marks[k]) == kinds.count(k) for k in set(kinds)), (kinds, desc)
    elif which == "tuned" and log_m > 13:   # (4096 / 8192 points: the twin carries the line, the one-pass planner's text does not)
        assert " tuned:c2c/b0=" in desc, desc
    assert probe.check_guards() == 0
    return call


def ref_set(c, cap=None):
    """the transforms of assertion 2: the ends, the middle, and both sides of every chunk boundary of a scratch of `cap`"""
    s = {0, c // 2, c - 1}
    if cap:
        for b0 in range(cap, c, cap):
            s |= {b0 - 1, b0}
    return sorted(s)


def run_case(P, dt, n, c, rules, cap=None, planner=None):
    """One fft_any_batched call of c transforms, assertions 1 - 4.  `cap`: the transforms exec_in's scratch holds (None: all).
    Returns the measurement of assertion 2 and the bits."""
    import torch

    with rules_of(P, rules):
        pl = planner or _planner(P, dt, n)
        call = check_plan(P, dt, pl, rules)
    assert pl.m == conv_len(n)
    ndt = np.float64 if dt == "f64" else np.float32
    dist = n + 3
    span = (c - 1) * dist + n
    buf_re = np.full(1 + span + TAIL, SENTINEL, ndt)
    buf_im = np.full_like(buf_re, -SENTINEL)
    mask = np.ones(len(buf_re), bool)
    for b in range(c):
        s = slice(1 + b * dist, 1 + b * dist + n)
        buf_re[s], buf_im[s] = _input(n, dt, seed=10 + b)
        mask[s] = False
    d_re, d_im = torch.from_numpy(buf_re).cuda(), torch.from_numpy(buf_im).cuda()
    work = torch.empty(pl.workspace_len(c), dtype=d_re.dtype, device="cuda")   # one engine call of c transforms
    P.fft_any_batched(d_re[1:1 + span], d_im[1:1 + span], n, P.Direction.Forward, pl, dist=dist, workspace=work)
    g_re, g_im = d_re.cpu().numpy(), d_im.cpu().numpy()
    bytes_after = pl.device_bytes()
    # 3. gaps and margins
    assert np.all(g_re[mask] == SENTINEL) and np.all(g_im[mask] == -SENTINEL), (dt, n, c, rules, "gaps or margins written")
    # 1. the bits of every transform run alone
    for b in range(c):
        s = slice(1 + b * dist, 1 + b * dist + n)
        a_re, a_im = _dev_fft(P, dt, buf_re[s], buf_im[s], 1, pl)
        if not (np.array_equal(g_re[s], a_re) and np.array_equal(g_im[s], a_im)):
            bad = int(np.flatnonzero((g_re[s] != a_re) | (g_im[s] != a_im))[0])
            raise AssertionError(f"{dt} N={n} c={c} {rules} [{call}]: transform {b} differs from the same transform run alone, "
                                 f"first at element {bad}")
    # 2. the reference
    g_rel, g_bin = any_gates(dt, n)
    worst_rel = worst_bin = 0.0
    for b in ref_set(c, cap):
        s = slice(1 + b * dist, 1 + b * dist + n)
        r_re, r_im = _reference(dt, n, b)
        rel, worst = tol.rel_l2(g_re[s], g_im[s], r_re, r_im), tol.max_bin_err(g_re[s], g_im[s], r_re, r_im)
        worst_rel, worst_bin = max(worst_rel, rel), max(worst_bin, worst)
        print(f"engine_batches {dt} N={n} M=2^{_log_m(n)} c={c} {rules} b={b}: rel {rel:.3e} / {g_rel:.3e}, bin {worst:.3e} / {g_bin:.3e}")
        _check(f"engine:{n}x{c}:{rules}:{b}", dt, n, g_re[s], g_im[s], r_re + 1j * r_im)
    print(f"engine_batches {dt} N={n} M=2^{_log_m(n)} c={c} {rules}: plan [{call}]")
    return {"dt": dt, "n": n, "m": pl.m, "c": c, "rules": rules, "plan": call, "rel": worst_rel, "bin": worst_bin, "gate_rel": g_rel,
            "gate_bin": g_bin, "use": max(worst_rel / g_rel, worst_bin / g_bin), "bits": (g_re, g_im), "bytes": bytes_after}


@pytest.mark.parametrize("dt,n,c,rules", cases(), ids=lambda v: str(v))
def test_engine_batch(guarded, dt, n, c, rules):
    t0 = time.perf_counter()
    run_case(guarded, dt, n, c, rules)
    print(f"engine_batches {dt} N={n} c={c} {rules}: {time.perf_counter() - t0:.2f} s")


def run_scratch_chunks(P):
    """exec_in's own chunk loop under the forced choice, inside ONE chunk of the composite: a fresh f64 planner of N = 12 000
    (M = 2^15), PHAST_SCRATCH_MB=1 around the call: the scratch holds 2 transforms, 5 run as 2 + 2 + 1"""
    dt, n, c = "f64", 12_000, 5
    with rules_of(P, "builtin"):
        small, whole = _planner(P, dt, n), _planner(P, dt, n)
    old = os.environ.get("PHAST_SCRATCH_MB")
    os.environ["PHAST_SCRATCH_MB"] = "1"
    try:
        # (the transforms run alone come after the batch, on the same planner: its scratch of 2 transforms serves them)
        got = run_case(P, dt, n, c, "builtin", cap=2, planner=small)
    finally:
        if old is None:
            del os.environ["PHAST_SCRATCH_MB"]
        else:
            os.environ["PHAST_SCRATCH_MB"] = old
    want = run_case(P, dt, n, c, "builtin", planner=whole)
    assert np.array_equal(got["bits"][0], want["bits"][0]) and np.array_equal(got["bits"][1], want["bits"][1])
    # the loop did run: the second planner's scratch holds 5 transforms, the first one's 2.  A transform takes two planes of M
    # elements, and up to a quarter more for the padded rows of the widest plan installed (plan.hpp: at M = 2^15 the throughput
    # plan's 256 + 48 elements per row, 19 %) -- 2 or 4 transforms' difference lie outside these bounds
    per = 2 * small.m * 8
    assert 3 * per <= want["bytes"] - got["bytes"] < 1.25 * 3 * per, (got["bytes"], want["bytes"], per)
    got["rules"] = "builtin scratch=1MiB"
    return got


def test_engine_chunks_inside_one_composite_chunk(guarded):
    run_scratch_chunks(guarded)


REAL_CASES = [(dt, n, 33) for n in (10_000, 5001) for dt in ("f64", "f32")]   # even: H = 5000 -> M = 2^14; odd: N -> M = 2^14


@functools.lru_cache(maxsize=8)
def _real_reference(dt, n, b):
    x = _signal(n, dt, seed=10 + b)
    re, im = _spectrum(n, dt, seed=20 + b)
    return x, _ref_r2c(x), (re, im), np.asarray(_ref_c2r(re, im, n), np.float64)


def run_real_case(P, dt, n, c):
    """r2c_any_batched and c2r_any_batched of c transforms at odd distances, planes at buf[1:], one engine call: assertions 1 - 3
    through the any-real module's gates.  Returns the measurement."""
    import torch

    with rules_of(P, "builtin"):
        pl = _real_planner(P, dt, n)
        # assertion 4: the real planner's engine is the same rule on its inner AnyPlanner (csrc/planner_any_real.hpp)
        which, spec = expected_plan(dt, 14, "builtin")
        call = (P.PlannerDit64 if dt == "f64" else P.PlannerDit32)(1 << 14).describe_call(1, 0)
    assert pl.m == 1 << 14 and call == which + " " + "".join(mps.tile_strings(spec, dt)), (call, pl.describe())
    ndt = np.float64 if dt == "f64" else np.float32
    h1 = n // 2 + 1
    work = torch.empty(pl.workspace_len(c), dtype=torch.float64 if dt == "f64" else torch.float32, device="cuda")
    g_rel, g_bin = real_gates(dt, n)
    use = {"rel": 0.0, "bin": 0.0}

    def measure(got_re, got_im, ref_re, ref_im):
        r, i = np.asarray(ref_re, np.float64), np.asarray(ref_im, np.float64)
        use["rel"] = max(use["rel"], tol.rel_l2(got_re, got_im, r, i))
        use["bin"] = max(use["bin"], tol.max_bin_err(got_re, got_im, r, i))

    # R2C
    in_dist, out_dist = n + 3, h1 + 2
    buf = np.full(1 + (c - 1) * in_dist + n + TAIL, SENTINEL, ndt)
    for b in range(c):
        buf[1 + b * in_dist:1 + b * in_dist + n] = _signal(n, dt, seed=10 + b)
    d_in = torch.from_numpy(buf).cuda()
    o_re = torch.full((1 + (c - 1) * out_dist + h1 + TAIL,), -SENTINEL, dtype=d_in.dtype, device="cuda")
    o_im = o_re.clone()
    P.r2c_any_batched(d_in[1:], o_re[1:], o_im[1:], pl, c, in_dist=in_dist, out_dist=out_dist, workspace=work)
    g_re, g_im = o_re.cpu().numpy(), o_im.cpu().numpy()
    assert np.array_equal(d_in.cpu().numpy(), buf)
    mask = np.ones(len(g_re), bool)
    for b in range(c):
        s = slice(1 + b * out_dist, 1 + b * out_dist + h1)
        mask[s] = False
        a_re, a_im = _dev_r2c(P, dt, _signal(n, dt, seed=10 + b), pl)
        assert np.array_equal(g_re[s], a_re) and np.array_equal(g_im[s], a_im), (dt, n, "r2c", b)
    assert np.all(g_re[mask] == -SENTINEL) and np.all(g_im[mask] == -SENTINEL)
    for b in ref_set(c):
        s = slice(1 + b * out_dist, 1 + b * out_dist + h1)
        x, ref, _, _ = _real_reference(dt, n, b)
        measure(g_re[s], g_im[s], ref.real, ref.imag)
        _check_r2c(dt, n, (g_re[s], g_im[s]), x)
    # C2R
    c_in_dist, c_out_dist = h1 + 2, n + 3
    b_re = np.full(1 + (c - 1) * c_in_dist + h1 + TAIL, SENTINEL, ndt)
    b_im = b_re.copy()
    for b in range(c):
        s = slice(1 + b * c_in_dist, 1 + b * c_in_dist + h1)
        b_re[s], b_im[s] = _spectrum(n, dt, seed=20 + b)
    d_re, d_im = torch.from_numpy(b_re).cuda(), torch.from_numpy(b_im).cuda()
    out = torch.full((1 + (c - 1) * c_out_dist + n + TAIL,), -SENTINEL, dtype=d_re.dtype, device="cuda")
    P.c2r_any_batched(d_re[1:], d_im[1:], out[1:], pl, c, in_dist=c_in_dist, out_dist=c_out_dist, workspace=work)
    g = out.cpu().numpy()
    assert np.array_equal(d_re.cpu().numpy(), b_re) and np.array_equal(d_im.cpu().numpy(), b_im)
    mask = np.ones(len(g), bool)
    for b in range(c):
        s = slice(1 + b * c_out_dist, 1 + b * c_out_dist + n)
        mask[s] = False
        i = slice(1 + b * c_in_dist, 1 + b * c_in_dist + h1)
        assert np.array_equal(g[s], _dev_c2r(P, dt, b_re[i], b_im[i], n, pl)), (dt, n, "c2r", b)
    assert np.all(g[mask] == -SENTINEL)
    for b in ref_set(c):
        s = slice(1 + b * c_out_dist, 1 + b * c_out_dist + n)
        _, _, (re, im), ref = _real_reference(dt, n, b)
        measure(g[s], np.zeros(n), ref, np.zeros(n))
        _check_c2r(dt, n, g[s], re, im)
    print(f"engine_batches real {dt} N={n} M=2^14 c={c}: rel {use['rel']:.3e} / {g_rel:.3e}, bin {use['bin']:.3e} / {g_bin:.3e}, plan [{call}]")
    return {"dt": dt, "n": n, "m": pl.m, "c": c, "rules": "builtin real", "plan": call, "rel": use["rel"], "bin": use["bin"],
            "gate_rel": g_rel, "gate_bin": g_bin, "use": max(use["rel"] / g_rel, use["bin"] / g_bin)}


@pytest.mark.parametrize("dt,n,c", REAL_CASES, ids=lambda v: str(v))
def test_real_transforms_at_batch_33(guarded, dt, n, c):
    run_real_case(guarded, dt, n, c)


# ---- the same kernels reached directly: the static single plans forced on a PlannerDit, run at batches plan_for never gives them
DIRECT = [("f64", 20, (6, 8, 6), (10, 12, 10), 3 | 0x10, "6,8,6@10,12,10:p8w", (5, 8)),
          ("f32", 20, (6, 8, 6), (11, 13, 11), 3 | 0x10, "6,8,6@11,13,11:p8w", (5, 8)),
          ("f64", 14, (6, 8), (10, 12), 4 | 0x10, "6,8@10,12:p16w", (65,))]


@pytest.mark.parametrize("dt,L,lrs,tls,lp,spec,batches", DIRECT, ids=lambda v: str(v))
def test_single_plans_forced_on_direct_batches(guarded, dt, L, lrs, tls, lp, spec, batches):
    """fft_dit_batched forward and reverse at dist = n + 8 on the forced plan: np.fft.fft / ifft in double through tol.check_c
    (as tests/test_gpu_fuzz.py), the gaps untouched, and the bits of every transform those of the same data run at batch 1"""
    import torch

    P = guarded
    n, dist = 1 << L, (1 << L) + 8
    ndt, tdt = (np.float64, torch.float64) if dt == "f64" else (np.float32, torch.float32)
    planner = (P.PlannerDit64 if dt == "f64" else P.PlannerDit32)(n)
    planner.set_plan(lrs, tls, lp)
    tiles = "".join(mps.tile_strings(spec, dt))
    rng = np.random.default_rng([0xE9, L, 8 if dt == "f64" else 4])
    for batch in batches:
        assert planner.describe_call(batch, 0) == f"forced {tiles}", planner.describe_call(batch, 0)
        span = (batch - 1) * dist + n
        h_re, h_im = np.full(span, SENTINEL, ndt), np.full(span, -SENTINEL, ndt)
        mask = np.ones(span, bool)
        for b in range(batch):
            h_re[b * dist:b * dist + n], h_im[b * dist:b * dist + n] = rng.uniform(-1, 1, n).astype(ndt), rng.uniform(-1, 1, n).astype(ndt)
            mask[b * dist:b * dist + n] = False
        for direction in (P.Direction.Forward, P.Direction.Reverse):
            d_re, d_im = torch.from_numpy(h_re).cuda(), torch.from_numpy(h_im).cuda()
            P.fft_dit_batched(d_re, d_im, n, direction, planner, dist=dist)
            g_re, g_im = d_re.cpu().numpy(), d_im.cpu().numpy()
            assert np.all(g_re[mask] == SENTINEL) and np.all(g_im[mask] == -SENTINEL), (dt, L, batch, "gaps written")
            for b in range(batch):
                s = slice(b * dist, b * dist + n)
                z = h_re[s].astype(np.float64) + 1j * h_im[s].astype(np.float64)
                ref = np.fft.fft(z) if direction == P.Direction.Forward else np.fft.ifft(z)
                tol.check_c(f"engine_direct:{dt}:{L}:{batch}:{b}", dt, L, g_re[s].astype(np.float64) + 1j * g_im[s].astype(np.float64), ref)
                a_re, a_im = torch.from_numpy(h_re[s].copy()).cuda(), torch.from_numpy(h_im[s].copy()).cuda()
                P.fft_dit_batched(a_re, a_im, n, direction, planner)
                assert np.array_equal(a_re.cpu().numpy(), g_re[s]) and np.array_equal(a_im.cpu().numpy(), g_im[s]), (dt, L, batch, b)
        assert planner.check_guards() == 0, planner.describe()
    print(f"engine_batches direct {dt} 2^{L} batches {batches}: {planner.describe_call(batches[0], 0)}")


# ---- one consumer with a naturally large c: 71 frames of 10 000 samples (H = 5000 -> M = 2^14) in one engine chunk
STFT_SHAPE = (175_000, 10_000, 2500)


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_stft_of_71_long_frames_in_one_chunk(guarded, dt):
    import torch

    P = guarded
    length, f, h = STFT_SHAPE
    w, spec, *_ = S.reference(dt, length, f, h, True, "reflect", "hann")
    with rules_of(P, "builtin"):
        pl = S.planner(P, dt, length, f, h, w, True, "reflect")
    assert (pl.frames, pl.bins) == spec.shape and pl.frames >= 70
    work = torch.empty(pl.workspace_len(1), dtype=S._tdt(dt), device="cuda")   # every frame of the signal in one chunk
    re, im = S.forward(P, pl, S._signal(length, dt), workspace=work)
    S.check_forward(f"engine_stft:{STFT_SHAPE}", dt, f, re, im, spec)
    # ... and frame by frame (a frame in another frame's place moves the whole-spectrogram rel-L2 by 1 / sqrt(frames) only)
    g_rel, g_bin = S.stft_gates(dt, f)
    want_re, want_im = np.asarray(spec.real, np.float64), np.asarray(spec.imag, np.float64)
    re, im = re.reshape(spec.shape), im.reshape(spec.shape)
    for k in range(pl.frames):
        rel, worst = tol.rel_l2(re[k], im[k], want_re[k], want_im[k]), tol.max_bin_err(re[k], im[k], want_re[k], want_im[k])
        assert rel <= g_rel and worst <= g_bin, (dt, k, rel, g_rel, worst, g_bin)
    print(f"engine_batches stft {dt} {STFT_SHAPE}: {pl.frames} frames in one chunk of {len(work)} elements")


def test_gates_keep_their_margin():
    """every case of this file is in the budget file, measured on the MI355X, and uses at most half of its gates"""
    budget = json.load(open(BUDGET))
    have = {(e["dt"], e["n"], e["c"], e["rules"]): e for e in budget["entries"]}
    want = cases() + [("f64", 12_000, 5, "builtin scratch=1MiB")] + [(dt, n, c, "builtin real") for dt, n, c in REAL_CASES]
    assert sorted(have) == sorted(want), (sorted(set(want) - set(have)), sorted(set(have) - set(want)))
    for key, e in have.items():
        real = e["rules"] == "builtin real"
        g_rel, g_bin = real_gates(e["dt"], e["n"]) if real else any_gates(e["dt"], e["n"])
        assert e["rel"] <= 0.5 * g_rel and e["bin"] <= 0.5 * g_bin and e["use"] <= 0.5, e
        which, spec = expected_plan(e["dt"], e["m"].bit_length() - 1, "static" if e["rules"] == "static" else "builtin")
        assert e["plan"] == which + " " + "".join(mps.tile_strings(spec, e["dt"])), e
