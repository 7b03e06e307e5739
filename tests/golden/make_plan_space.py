"""Writes tests/golden/plan_space.json: the plans a tuning run, a wisdom file or a regenerated builtin_wisdom.inc can install
(csrc/plan.hpp: enumerate_plans), as the list tests/test_gpu_plan_space.py runs on the device.  Needs no GPU: the list comes
from the CPU emulator (tests/emu/emu.hip: phast_emu_list_plans), which calls enumerate_plans itself and restates the planner's
build step (make_passes, the 160 KiB LDS refusal, which passes have the fused R2C / C2R form).

    python tests/golden/make_plan_space.py          # rewrites the file, prints the sizes

An entry is "<spec> <flags>": the spec in the wisdom's text form ("6,8,6@10,12,10:p8w"), flags `x` = refused by the build
step, `r` = the last pass has the fused R2C form, `c` = the first pass has the fused C2R form, `-` = none.  Per type:

    exhaustive  every plan of the inner lengths L = 13 .. 19 with every pass's tile size in 10 .. 14 (f64) / 10 .. 15 (f32): a
                superset of what tune_tile_range gives any tuning run, whatever its batch
    classes     every pass class "<role> <kind> <log2 rows> <log2 cols>" of a buildable plan of L = 13 .. 25
    cover       L = 20 .. 25: a greedy cover of the pass CLASSES -- (role first / middle / last, kind p8 / p16 / p32 / wave /
                quad, log2 rows, log2 cols) -- that occur in a buildable plan of L <= 25 and in no exhaustive plan, the shortest L
                first; plus the first refused plan per class of last pass (the refusal is checked on the device too) and every
                plan of csrc/builtin_wisdom.inc with an inner length of 20 .. 23

tests/test_emulator.py checks that the committed file is what this script writes, that the tuner's candidates are in it, and
that the cover is complete.
"""
from __future__ import annotations

import ctypes as C
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PATH = os.path.join(HERE, "plan_space.json")
WISDOM = os.path.join(ROOT, "phastft_amd", "csrc", "builtin_wisdom.inc")

TYPES = {"f64": 8, "f32": 4}
TILE_RANGE = {"f64": (10, 14), "f32": (10, 15)}
EXHAUSTIVE_L = range(13, 20)
COVER_L = range(20, 26)
WISDOM_MAX_L = 23


def parse_spec(spec: str):
    """'6,8,6@10,12,10:p8w' -> ((6, 8, 6), (10, 12, 10), 3, True): log2 rows, log2 tile points, log2 points per thread, w"""
    m = re.fullmatch(r"([\d,]+)@([\d,]+):p(8|16|32)(w?)", spec)
    lrs, tls = tuple(map(int, m.group(1).split(","))), tuple(map(int, m.group(2).split(",")))
    assert len(lrs) == len(tls) and 2 <= len(lrs) <= 3, spec
    return lrs, tls, {8: 3, 16: 4, 32: 5}[int(m.group(3))], m.group(4) == "w"


def pass_classes(spec: str, dt: str):
    """the (role, kind, log2 rows, log2 cols) of every pass of a plan -- plan.hpp: make_passes' rule for which passes of a `w`
    plan run as one-wave tiles (64 rows x 128 bytes) and which as the four-wave kernel (256 rows x 128 bytes, not first)"""
    lrs, tls, lp, w = parse_spec(spec)
    wave_tl, quad_tl = (10, 12) if dt == "f64" else (11, 13)
    out = []
    for i, (lr, tl) in enumerate(zip(lrs, tls)):
        role = "first" if i == 0 else "last" if i + 1 == len(lrs) else "middle"
        kind = "wave" if w and lr == 6 and tl == wave_tl else "quad" if w and lr == 8 and tl == quad_tl and i > 0 else f"p{1 << lp}"
        out.append((role, kind, lr, tl - lr))
    return out


def class_name(c) -> str:
    return "%s %s %d %d" % c


def tile_strings(spec: str, dt: str):
    """the "[rows x cols ...]" groups Planner::describe_call prints for the plan"""
    out = []
    for role, kind, lr, lc in pass_classes(spec, dt):
        pts = (16 if dt == "f64" else 32) if kind == "wave" else 16 if kind == "quad" else int(kind[1:])
        out.append(f"[{1 << lr}x{1 << lc}{'A' if role == 'first' else ''} {'w' if kind == 'wave' else 'q' if kind == 'quad' else 'p'}{pts}]")
    return out


def list_plans(emu, L: int, dt: str, tl_lo: int, tl_hi: int):
    """[(spec, flags)] of enumerate_plans(L, ...) in its own order"""
    emu.phast_emu_list_plans.argtypes = [C.c_uint, C.c_size_t, C.c_uint, C.c_uint, C.c_char_p, C.c_size_t]
    emu.phast_emu_list_plans.restype = C.c_size_t
    need = emu.phast_emu_list_plans(L, TYPES[dt], tl_lo, tl_hi, None, 0)
    buf = C.create_string_buffer(need)
    assert emu.phast_emu_list_plans(L, TYPES[dt], tl_lo, tl_hi, buf, need) == need
    return [tuple(ln.split(" ")) for ln in buf.value.decode().splitlines()]


def classes_of(entries, dt: str):
    """the classes of the entries' buildable plans"""
    out = set()
    for e in entries:
        spec, flags = e.split(" ") if isinstance(e, str) else e
        if "x" not in flags:
            out.update(pass_classes(spec, dt))
    return out


def wisdom_specs(dt: str):
    """{inner L: [spec ...]} of builtin_wisdom.inc, in file order, without repeats"""
    out: dict = {}
    for m in re.finditer(r'^"(f64|f32) (c2c|c2ci|r2c|c2r) (\d+) (\d+) (\S+) fuse=', open(WISDOM).read(), re.M):
        if m.group(1) != dt or m.group(5) == "heuristic":
            continue
        inner = int(m.group(3)) - (1 if m.group(2) in ("r2c", "c2r") else 0)
        if m.group(5) not in out.setdefault(inner, []):
            out[inner].append(m.group(5))
    return out


def generate(emu, log=None) -> str:
    doc = {"format": 1, "tile_range": {dt: list(TILE_RANGE[dt]) for dt in TYPES}}
    for dt in TYPES:
        lo, hi = TILE_RANGE[dt]
        full = {L: list_plans(emu, L, dt, lo, hi) for L in range(EXHAUSTIVE_L[0], COVER_L[-1] + 1)}
        exhaustive = {L: full[L] for L in EXHAUSTIVE_L}
        covered = set()
        for L in EXHAUSTIVE_L:
            covered |= classes_of(full[L], dt)
        universe = set()
        for L in full:
            universe |= classes_of(full[L], dt)
        cover = {L: [] for L in COVER_L}
        for L in COVER_L:  # the shortest length first; at each length the plan that adds the most classes, the first of equals
            plans = [(s, f, set(pass_classes(s, dt))) for s, f in full[L] if "x" not in f]
            while True:
                best = max(plans, key=lambda p: len(p[2] - covered), default=None)
                if best is None or not (best[2] - covered):
                    break
                cover[L].append((best[0], best[1]))
                covered |= best[2]
        assert covered == universe, sorted(universe - covered)
        n_greedy = sum(len(v) for v in cover.values())
        # plans the build step refuses (a pass whose tile and twiddle tables do not fit one CU's LDS: f64 from L = 25 on): the
        # first one per class of the last pass, so that the device is asked about the refusal too
        n_refused, last_seen = 0, set()
        for L in COVER_L:
            for s, f in full[L]:
                last = pass_classes(s, dt)[-1]
                if "x" in f and last not in last_seen:
                    last_seen.add(last)
                    cover[L].append((s, f))
                    n_refused += 1
        n_wisdom = 0
        for L, specs in sorted(wisdom_specs(dt).items()):
            if L not in cover or L > WISDOM_MAX_L:
                continue
            flags = dict(full[L])
            for s in specs:
                assert s in flags, (dt, L, s)  # tests/test_emulator.py: every built-in line is a candidate
                if (s, flags[s]) not in cover[L]:
                    cover[L].append((s, flags[s]))
                    n_wisdom += 1
        doc[dt] = {"classes": sorted(class_name(c) for c in universe),
                   "exhaustive": {str(L): [f"{s} {f}" for s, f in exhaustive[L]] for L in EXHAUSTIVE_L},
                   "cover": {str(L): [f"{s} {f}" for s, f in cover[L]] for L in COVER_L}}
        if log:
            n_ex = sum(len(v) for v in exhaustive.values())
            n_x = sum(1 for v in exhaustive.values() for _, f in v if "x" in f)
            log(f"{dt}: exhaustive {n_ex} plans ({', '.join(f'L={L}: {len(exhaustive[L])}' for L in EXHAUSTIVE_L)}), {n_x} refused; "
                f"{len(universe)} pass classes up to L = {COVER_L[-1]}; cover {n_greedy} plans + {n_refused} refused + {n_wisdom} built-in wisdom plans "
                f"({', '.join(f'L={L}: {len(cover[L])}' for L in COVER_L)})")
    # one list per line: small, and a regenerated file shows as a readable diff
    text = json.dumps(doc, indent=1, sort_keys=True)
    text = re.sub(r"\[\s+([^\[\]]*?)\s+\]", lambda m: "[" + re.sub(r",\s+", ", ", m.group(1)) + "]", text)
    return text + "\n"


def load(path: str = PATH) -> dict:
    return json.load(open(path))


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    from tests.emu import build_emulator

    text = generate(C.CDLL(build_emulator()), log=print)
    with open(PATH, "w") as f:
        f.write(text)
    print(f"{PATH}: {len(text)} bytes")
