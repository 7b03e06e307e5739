"""Every plan a tuning run, a wisdom file or a regenerated builtin_wisdom.inc can install, run on the device against numpy's
pocketfft in double precision.

The list is tests/golden/plan_space.json (written by tests/golden/make_plan_space.py from csrc/plan.hpp: enumerate_plans, kept
current by tests/test_emulator.py): per type every plan of the inner lengths 2^13 .. 2^19 over the whole tile range, and for
2^20 .. 2^25 a cover of every pass class (role, kind, rows, cols) that the shorter lengths do not reach, plus the built-in wisdom's
plans of those lengths.  One case per (type, call kind, inner length):

    L = 13 .. 17     every plan, every kind: C2C planar, C2C interleaved, R2C with and without the fused untangle, C2R
    L = 18, 19       every plan, C2C planar
    cover set        C2C planar; its plans of L <= 21 also as R2C and C2R           (real kinds: real length 2^(L + 1))

A plan is installed the way a tuner's result reaches a planner: one imported wisdom line for (type, kind, log2 length, bucket 0)
-- bucket 2 as well where a batch of three runs -- and a fresh planner, whose describe_call must say `tuned` and name the plan's
tiles.  A plan the list marks as refused by the planner's build step must not be installed; every other one must be.

Gates: tests/tolerances.py against the float64 reference ("f64ref"), rel-L2 and worst bin, nothing else.  From L = 18 on the
two error numbers are formed on the device in float64 against the reference uploaded once.  Forward for every plan; for L <= 16
also reverse (C2C kinds) and a batch of three transforms n + 8 apart whose gaps must stay untouched.  The caller's arrays sit
between canary margins that must be bit-exact afterwards; the scratches carry guard bands, checked after every plan
(check_guards of PlannerDit* and PlannerR2c*: the real transforms run in the inner planner's scratches).

Measured on an MI355X (the whole file: 84 cases, 23 s): a wisdom import plus a fresh planner costs 0.15 .. 0.6 ms, so every kind
takes the wisdom route; the slowest case is the f64 cover of 2^25 points at 1.2 s (its reference FFT on the host), the
exhaustive cases take 0.1 .. 0.7 s.  5116 plans run (f64: 915 C2C, 393 interleaved, 418 R2C, 300 R2C fused, 418 C2R; f32: 994,
415, 445, 373, 445), one f64 plan of 2^25 points is refused on the device as the list says.  Worst use of a gate: 0.09 (f64),
0.31 (f32).
"""
import importlib.util
import os
import time

import numpy as np
import pytest

from tests import tolerances as tol

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("make_plan_space", os.path.join(os.path.dirname(__file__), "golden", "make_plan_space.py"))
mps = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mps)
SPACE = mps.load()

CANARY = 1234.5
PAD = 1 << 14       # elements of margin on either side of every caller's array
GAP = 8             # batch of three: transforms n + GAP apart
HEADER = "phastft-hip-wisdom 1\n"   # no cus= / arch= / lib=: applied on whatever device runs the test (csrc/wisdom.hpp)
KINDS = {"c2c": 0, "c2ci": 1, "r2c": 2, "r2cf": 2, "c2r": 3}   # PHAST_TUNE_* ("r2cf": R2C with fuse=1)


def _entries(dt, group, L):
    return [tuple(e.split(" ")) for e in SPACE[dt][group][str(L)]]


def _cases():
    out = []
    for dt in ("f64", "f32"):
        for L in range(13, 20):
            for kind in (("c2c", "c2ci", "r2c", "r2cf", "c2r") if L <= 17 else ("c2c",)):
                out.append((dt, kind, "exhaustive", L))
        for L in range(20, 26):
            for kind in (("c2c", "r2c", "r2cf", "c2r") if L <= 21 else ("c2c",)):
                out.append((dt, kind, "cover", L))
    return out


@pytest.fixture(scope="module")
def space_env(gpu):
    """Guard bands on, built-in wisdom off, an empty store.  Afterwards the built-in switch is what it was and the store holds the
    entries it held -- as far as the public surface can put them back: the exported text is imported again, so entries read from a
    PHAST_WISDOM file or measured by this process return as imported ones (the same plans apply, from layer 2); and the guard
    bands are switched off, there being no query for their previous size (0 unless another module left them on)."""
    gpu.debug_set_guard_bytes(1 << 20)
    was = gpu.wisdom_builtin(False)
    kept = gpu.wisdom_export()
    gpu.wisdom_forget()
    try:
        yield gpu
    finally:
        gpu.wisdom_forget()
        gpu.wisdom_import(kept)
        gpu.wisdom_builtin(was)
        gpu.debug_set_guard_bytes(0)


def _data(dt, kind, L, nb, seed=0):
    """(inputs, references) of `nb` transforms: uniform [-1, 1) in the type under test, the reference from those values in float64"""
    np_t = np.float64 if dt == "f64" else np.float32
    real = kind in ("r2c", "r2cf", "c2r")
    n = 1 << (L + 1 if real else L)
    rng = np.random.default_rng([0x9A5, seed, L, KINDS[kind], 8 if dt == "f64" else 4])
    ins, refs = [], []
    for _ in range(nb):
        if kind == "c2r":
            half = n // 2 + 1
            s_re, s_im = rng.uniform(-1, 1, half).astype(np_t), rng.uniform(-1, 1, half).astype(np_t)
            s_im[0] = s_im[-1] = 0   # irfft ignores Im(DC) and Im(Nyquist): keep the comparison Hermitian (tests/test_gpu_fuzz.py)
            ins.append((s_re, s_im))
            refs.append({1: np.fft.irfft(s_re.astype(np.float64) + 1j * s_im.astype(np.float64), n)})
        elif real:
            x = rng.uniform(-1, 1, n).astype(np_t)
            ins.append((x,))
            refs.append({1: np.fft.rfft(x.astype(np.float64))})
        else:
            re, im = rng.uniform(-1, 1, n).astype(np_t), rng.uniform(-1, 1, n).astype(np_t)
            z = re.astype(np.float64) + 1j * im.astype(np.float64)
            ins.append((re, im))
            refs.append({1: np.fft.fft(z), -1: np.fft.ifft(z) if L <= 16 else None})
    return ins, refs


class _Arrays:
    """the caller's arrays of one case, each between canary margins: `planes` arrays of (nb - 1) * dist + per elements"""

    def __init__(self, torch, t_t, pers, nb, gap=GAP):
        self.torch, self.nb = torch, nb
        self.dists = [per + (gap if nb > 1 else 0) for per in pers]
        self.counts = [(nb - 1) * d + per for d, per in zip(self.dists, pers)]
        self.pers = pers
        self.whole = [torch.full((c + 2 * PAD,), CANARY, dtype=t_t, device="cuda") for c in self.counts]
        self.view = [w[PAD:PAD + c] for w, c in zip(self.whole, self.counts)]
        self.canary = torch.full((PAD,), CANARY, dtype=t_t, device="cuda")

    def load(self, k, host_parts):
        """array k <- the transforms' data, the gaps between them <- the canary"""
        self.view[k].fill_(CANARY)
        for b, part in enumerate(host_parts):
            self.view[k][b * self.dists[k]:b * self.dists[k] + self.pers[k]].copy_(part)

    def intact(self):
        """margins of every array and the gaps between the transforms still hold the canary"""
        t = self.torch
        for w, v, c, d, per in zip(self.whole, self.view, self.counts, self.dists, self.pers):
            if not (t.equal(w[:PAD], self.canary) and t.equal(w[PAD + c:], self.canary)):
                return False
            for b in range(self.nb - 1):
                if not bool((v[b * d + per:(b + 1) * d] == CANARY).all()):
                    return False
        return True

    def part(self, k, b):
        return self.view[k][b * self.dists[k]:b * self.dists[k] + self.pers[k]]


def _errors_dev(torch, got_re, got_im, ref_re, ref_im):
    """rel-L2 and worst bin / rms bin as tests/tolerances.py forms them, on the device in float64"""
    d_re = got_re.to(torch.float64) - ref_re
    num = d_re.square().sum()
    e = d_re.abs()
    den = ref_re.square().sum()
    if got_im is not None:
        d_im = got_im.to(torch.float64) - ref_im
        num = num + d_im.square().sum()
        e = torch.maximum(e, d_im.abs())
        den = den + ref_im.square().sum()
    rms = torch.sqrt(den / ref_re.numel())
    out = torch.stack([torch.sqrt(num / den), e.max() / rms]).cpu()
    return float(out[0]), float(out[1])


def _wisdom_line(dt, kind, log2n, bucket, spec):
    name = "r2c" if kind == "r2cf" else kind
    return f"{dt} {name} {log2n} {bucket} {spec} fuse={1 if kind == 'r2cf' else 0} us=1.00 heur=2.00\n"


def _run_case(gpu, dt, kind, group, L, entries, refs_override=None, report=None):
    """Runs every entry of the case; returns the number of plans run.  `refs_override`: references to compare with instead of
    the case's own (the negative check)."""
    import torch

    P = gpu
    f64 = dt == "f64"
    t_t = torch.float64 if f64 else torch.float32
    real = kind in ("r2c", "r2cf", "c2r")
    log2n = L + 1 if real else L
    n, half = 1 << log2n, (1 << log2n) // 2 + 1
    nb = 3 if L <= 16 else 1
    on_dev = L >= 18
    ins, refs = _data(dt, kind, L, nb)
    if refs_override is not None:
        refs = refs_override
    d_ins = [[torch.from_numpy(a).cuda() for a in parts] for parts in ins]
    d_refs = None
    if on_dev:
        d_refs = [{d: (torch.from_numpy(np.ascontiguousarray(r.real)).cuda(), torch.from_numpy(np.ascontiguousarray(r.imag)).cuda() if np.iscomplexobj(r) else None)
                   for d, r in ref.items() if r is not None} for ref in refs]
    sfx = "64" if f64 else "32"
    fs = "f64" if f64 else "f32"
    Planner = (P.PlannerR2c64 if f64 else P.PlannerR2c32) if real else (P.PlannerDit64 if f64 else P.PlannerDit32)
    # the arrays of a single transform and of the batch of three: C2C in place, the real kinds out of place
    pers = {"c2c": [n, n], "c2ci": [2 * n], "r2c": [n, half, half], "r2cf": [n, half, half], "c2r": [half, half, n]}[kind]
    single = _Arrays(torch, t_t, pers, 1)
    triple = _Arrays(torch, t_t, pers, 3, 2 * GAP if kind == "c2ci" else GAP) if nb == 3 else None   # (c2ci: GAP complex elements)
    n_in = {"c2c": 2, "c2ci": 1, "r2c": 1, "r2cf": 1, "c2r": 2}[kind]
    stream = P._stream

    def load(arr, count):
        if kind == "c2ci":
            arr.load(0, [torch.stack([d_ins[b][0], d_ins[b][1]], dim=1).reshape(-1) for b in range(count)])
        else:
            for k in range(n_in):
                arr.load(k, [d_ins[b][k] for b in range(count)])
        for k in range(n_in, len(pers)):
            arr.view[k].fill_(CANARY)

    def launch(arr, count, direction, planner):
        v, d = arr.view, arr.dists
        if kind == "c2c":
            rc = P._call(f"phast_fft_{sfx}_dit_dev", v[0].data_ptr(), v[1].data_ptr(), n, count, d[0], direction, planner._h, stream())
        elif kind == "c2ci":
            rc = P._call(f"phast_fft_{sfx}_interleaved_dev", v[0].data_ptr(), n, count, d[0] // 2, direction, planner._h, stream())
        elif kind == "c2r":
            rc = P._call(f"phast_c2r_fft_{fs}_dev", v[0].data_ptr(), v[1].data_ptr(), v[2].data_ptr(), count, d[0], d[2], planner._h, stream())
        else:
            rc = P._call(f"phast_r2c_fft_{fs}_dev", v[0].data_ptr(), v[1].data_ptr(), v[2].data_ptr(), count, d[0], d[1], planner._h, stream())
        P._check(rc)   # a launch the device refuses raises here, with the HIP error's text

    def result(arr, b):
        if kind == "c2c":
            return arr.part(0, b), arr.part(1, b)
        if kind == "c2ci":
            z = arr.part(0, b).view(n, 2)
            return z[:, 0], z[:, 1]
        if kind == "c2r":
            return arr.part(2, b), None
        return arr.part(1, b), arr.part(2, b)

    def compare(tag, arr, b, direction):
        g_re, g_im = result(arr, b)
        if on_dev:
            r_re, r_im = d_refs[b][direction]
            rel, worst = _errors_dev(torch, g_re, g_im, r_re, r_im)
            g_rel, g_bin = tol.gates(dt, log2n)
            tol.record(tag, log2n, rel, worst, g_rel, g_bin)
            assert rel <= g_rel and worst <= g_bin, (tag, dt, log2n, rel, g_rel, worst, g_bin)
        elif g_im is None:
            rel, worst = tol.check_real(tag, dt, log2n, g_re.cpu().numpy(), refs[b][direction])
        else:
            rel, worst = tol.check_c(tag, dt, log2n, g_re.cpu().numpy().astype(np.float64) + 1j * g_im.cpu().numpy().astype(np.float64),
                                     refs[b][direction])
        if report is not None:
            g_rel, g_bin = tol.gates(dt, log2n)
            report["worst"] = max(report.get("worst", 0.0), rel / g_rel, worst / g_bin)

    ran = refused = 0
    for spec, flags in entries:
        if kind == "r2cf" and "r" not in flags:
            continue   # the last pass has no fused form: the plan runs as "r2c" only
        tag = f"plan_space {dt} {kind} L={L} {spec}"
        P.wisdom_forget()
        P.wisdom_import(HEADER + _wisdom_line(dt, kind, log2n, 0, spec) + (_wisdom_line(dt, kind, log2n, 2, spec) if nb == 3 else ""))
        t0 = time.perf_counter()
        planner = Planner(n)
        if report is not None:
            report["install_s"] = report.get("install_s", 0.0) + time.perf_counter() - t0
        try:
            descs = [planner.describe_call(1, KINDS[kind])] + ([planner.describe_call(3, KINDS[kind])] if nb == 3 else [])
            if "x" in flags:   # refused by the build step: the line must be skipped, the static rules serve
                assert not any(d.startswith("tuned") for d in descs), (tag, descs)
                refused += 1
                continue
            for desc in descs:
                assert desc.startswith("tuned "), (tag, desc)
                assert desc.split(" ", 1)[1].startswith("".join(mps.tile_strings(spec, dt))), (tag, desc)
                assert ("untangle-fused" in desc) == (kind == "r2cf"), (tag, desc)
                assert ("preprocess-fused" in desc) == (kind == "c2r" and "c" in flags), (tag, desc)
            for direction in ((1, -1) if (not real and L <= 16) else (1,)):
                load(single, 1)
                launch(single, 1, direction, planner)
                compare(f"{tag} dir={direction}", single, 0, direction)
                assert single.intact(), tag
                if kind in ("r2c", "r2cf"):
                    assert torch.equal(single.view[0], d_ins[0][0]), f"{tag}: R2C must not modify its input"
            if nb == 3:
                load(triple, 3)
                launch(triple, 3, 1, planner)
                for b in range(3):
                    compare(f"{tag} batch=3 b={b}", triple, b, 1)
                assert triple.intact(), f"{tag}: margins or the gaps between the transforms of a batch were written"
            assert planner.check_guards() == 0, (tag, planner.describe())   # (the real planners: the inner planner's scratches)
            ran += 1
        except P.PhastHipError as e:   # any HIP error is a failure that names the plan
            raise AssertionError(f"{tag}: {e}") from e
        finally:
            del planner
    return ran, refused


@pytest.mark.parametrize("dt,kind,group,L", _cases(), ids=lambda v: str(v))
def test_every_installable_plan_against_pocketfft(space_env, dt, kind, group, L):
    entries = _entries(dt, group, L)
    report = {}
    t0 = time.perf_counter()
    ran, refused = _run_case(space_env, dt, kind, group, L, entries, report=report)
    secs = time.perf_counter() - t0
    # coverage: every plan of the list for this key ran (R2C with the fused untangle: every plan whose last pass has the form)
    want = [e for e in entries if kind != "r2cf" or "r" in e[1]]
    assert refused == sum("x" in f for _, f in want) and ran == len(want) - refused, (ran, refused, len(want))
    assert ran > 0, "nothing ran"
    print(f"plan_space {dt} {kind} {group} L={L}: {ran} plans run, {refused} refused, {secs:.2f} s, "
          f"{1e3 * report['install_s'] / max(1, ran + refused):.2f} ms per wisdom import + planner, worst gate fraction {report.get('worst', 0):.3f}")


@pytest.mark.parametrize("dt,kind,L", [("f64", "c2c", 14), ("f32", "r2cf", 13), ("f64", "c2r", 13), ("f32", "c2c", 18)])
def test_the_gates_notice_the_reference_of_another_seed(space_env, dt, kind, L):
    """teeth: the same plans, the same code path, against the reference of inputs drawn from another seed -- the case must fail"""
    entries = [e for e in _entries(dt, "exhaustive", L) if "x" not in e[1] and (kind != "r2cf" or "r" in e[1])][:3]
    assert entries
    _, other = _data(dt, kind, L, 3 if L <= 16 else 1, seed=1)
    # the failure must be the GATES' -- their message is (tag, type, log2 n, ...) -- not a describe_call mismatch or a HIP error
    with pytest.raises(AssertionError, match=r"^\('plan_space [^']+', 'f(64|32)', \d+, "):
        _run_case(space_env, dt, kind, "exhaustive", L, entries, refs_override=other)
    ran, _ = _run_case(space_env, dt, kind, "exhaustive", L, entries)   # ... and passes against its own
    assert ran == len(entries)


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_every_pass_class_is_seen_on_the_device(space_env, dt):
    """Every (role, kind, rows, cols) a buildable plan of L <= 25 contains is in the file (tests/test_emulator.py shows that from
    the odometer) -- and the device agrees: the tile strings describe_call prints for the cover plans and for one exhaustive
    plan per class name every class."""
    import re

    P = space_env
    f64 = dt == "f64"
    seen, want, have = set(), set(SPACE[dt]["classes"]), set()
    picked = []
    for L in range(13, 20):
        for spec, flags in _entries(dt, "exhaustive", L):
            cls = set(mps.pass_classes(spec, dt))
            if "x" not in flags and not cls <= have:
                picked.append((L, spec))
                have |= cls
    for L in range(20, 26):
        picked += [(L, spec) for spec, flags in _entries(dt, "cover", L) if "x" not in flags]
    for L, spec in picked:
        P.wisdom_forget()
        P.wisdom_import(HEADER + _wisdom_line(dt, "c2c", L, 0, spec))
        planner = (P.PlannerDit64 if f64 else P.PlannerDit32)(1 << L)
        desc = planner.describe_call(1, 0)
        del planner
        assert desc.startswith("tuned "), (L, spec, desc)
        tiles = re.findall(r"\[(\d+)x(\d+)(A?) ([pwq])(\d+)\]", desc)
        for i, (rows, cols, a, k, pts) in enumerate(tiles):
            role = "first" if i == 0 else "last" if i + 1 == len(tiles) else "middle"
            assert (a == "A") == (i == 0), desc
            kind = "wave" if k == "w" else "quad" if k == "q" else f"p{pts}"
            seen.add(mps.class_name((role, kind, int(rows).bit_length() - 1, int(cols).bit_length() - 1)))
    assert seen == want, (sorted(want - seen), sorted(seen - want))
