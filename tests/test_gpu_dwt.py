"""The discrete wavelet transform on the MI355X (csrc/dwt.hip, csrc/planner_dwt.hpp) against tests/dwt_reference.py, the
definitions in long double over the same T-rounded taps and values.

Gates -- nothing is fitted.  A sum of n products through an FMA chain obeys |got - ref| <= (n + 2) u sum |h x|.
A coefficient of level l has passed l such stages of F products, so
    wavedec   |got - ref| <= l (F + 2) u Abs_l[i]          Abs: the cascade of |taps| on |values| (abs_wavedec)
    waverec   |got - ref| <= J (F + 2) u AbsS[r]           the synthesis cascade of |taps| on |coefficients| (abs_waverec)
    round trip |got - x|  <= 2 J (F + 2) u AbsS(AbsA(|x|)) + the reference's own long double round-trip defect (the built-in
              taps are rounded)
with u = 2^-53 / 2^-24.  The worst use of every gate is in tests/golden/dwt_error_budget.json, written on the MI355X by
tests/golden/make_dwt_error_budget.py; test_gates_keep_their_margin keeps every entry 2 x inside."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

from tests import dwt_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTS = ["f64", "f32"]
NDT = {"f64": np.float64, "f32": np.float32}
U = {"f64": 2.0 ** -53, "f32": 2.0 ** -24}
BUDGET = os.path.join(ROOT, "tests", "golden", "dwt_error_budget.json")
BATCH = 3
TILE = 1024
# (L, F, J); L < 0: the length whose first level has -L coefficients (2 n_1 - F + 2, in periodization 2 n_1)
CASES = [(1, 2, 1), (2, 2, 1), (3, 4, 1), (5, 8, 1), (17, 4, 3), (9, 4, 4), (40, 6, 2), (-(TILE - 1), 6, 1), (-TILE, 6, 1), (-(TILE + 1), 6, 1),
         (-(2 * TILE + 3), 6, 2), (4100, 20, 5), (3000, 256, 2)]
ROUND_TRIPS = [("haar", 1, 1), ("db2", 17, 3), ("db4", 9, 4), ("db3", 2 * TILE + 5, 2), ("db10", 4100, 5)]


def _tdt(dt):
    import torch

    return torch.float64 if dt == "f64" else torch.float32


def case_id(c):
    return "x".join(str(v) for v in c).replace("-", "n1=")


def case_len(case, mode):
    L, f, _ = case
    return L if L > 0 else (-2 * L if mode == "periodization" else -2 * L - f + 2)


def signal(n, dt, seed, batch=BATCH):
    return [np.random.default_rng(1000 * seed + b).standard_normal(n).astype(NDT[dt]) for b in range(batch)]


@functools.lru_cache(maxsize=None)
def bank_of(case, dt):
    """the four filters of a case as values of the type: the built-in bank of its length, the LeGall 5/3 pair for (40, 6, 2),
    256 random taps for the longest filter"""
    import phastft_amd as P

    L, f, J = case
    if case == (40, 6, 2):
        bank = R.legall53()
    elif f <= 20:
        bank = P.wavelet_filters(f"db{f // 2}")
    else:
        rng = np.random.default_rng(f)
        bank = tuple(rng.standard_normal(f) / np.sqrt(f) for _ in range(4))
    return tuple(np.asarray(b, dtype=NDT[dt]) for b in bank)


@functools.lru_cache(maxsize=None)
def reference(case, dt, mode):
    """BATCH signals and BATCH packed rows of random coefficients (values of the type) with, per row, the long double result
    and its gate in both directions"""
    _, f, J = case
    L, bank, u = case_len(case, mode), bank_of(case, dt), U[dt]
    lens = R.level_lens(L, f, J, mode)
    level_of = np.concatenate([np.full(lens[J], J)] + [np.full(lens[l], l) for l in range(J, 0, -1)])   # the level of a packed element
    xs = signal(L, dt, seed=L + f)
    cs = signal(level_of.size, dt, seed=L + f + 7)
    fwd, inv = [], []
    for x in xs:
        ref = R.pack(R.wavedec(x, bank, J, mode))
        gate = level_of * (f + 2) * u * R.pack(R.abs_wavedec(x, bank, J, mode))
        fwd.append((ref, gate.astype(np.float64)))
    for c in cs:
        parts = R.unpack(c, L, f, J, mode)
        ref = R.waverec(parts, bank, mode, L)
        gate = J * (f + 2) * u * R.abs_waverec(parts, bank, mode, L)
        inv.append((ref, gate.astype(np.float64)))
    return xs, cs, fwd, inv


@functools.lru_cache(maxsize=None)
def planner(P, dt, case, mode):
    _, f, J = case
    return (P.PlannerDwt64 if dt == "f64" else P.PlannerDwt32)(case_len(case, mode), bank_of(case, dt), J, mode)


def batched(P, inverse, pl, rows, dt, in_dist, out_dist, off=1, work=None, stream=None):
    """`rows` through wavedec_batched / waverec_batched at the distances, from `off` elements past a 16-byte boundary: the
    outputs; the inputs, the gaps and what lies around the outputs are not written"""
    import torch

    fn = P.waverec_batched if inverse else P.wavedec_batched
    n, m = (pl.coeff_len, pl.signal_len) if inverse else (pl.signal_len, pl.coeff_len)
    b = len(rows)
    buf = torch.full((off + b * in_dist + 4,), 9.0, dtype=_tdt(dt), device="cuda")
    x = torch.as_strided(buf, (b, n), (in_dist, 1), off)
    for i, r in enumerate(rows):
        x[i] = torch.from_numpy(np.ascontiguousarray(r, dtype=NDT[dt]))
    keep = buf.clone()
    obuf = torch.full((off + b * out_dist + 4,), 9.0, dtype=_tdt(dt), device="cuda")
    out = torch.as_strided(obuf, (b, m), (out_dist, 1), off)
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    fn(x if b > 1 else x[0], pl, out=out if b > 1 else out[0], work=work, stream=stream)
    torch.cuda.synchronize()
    assert torch.equal(buf, keep)
    got = obuf.cpu().numpy()
    assert (got[:off] == 9.0).all() and (got[off + (b - 1) * out_dist + m:] == 9.0).all()
    for i in range(b - 1):
        assert (got[off + i * out_dist + m:off + (i + 1) * out_dist] == 9.0).all()
    return [got[off + i * out_dist:off + i * out_dist + m].copy() for i in range(b)]


def _use(got, ref, gate, where):
    err = np.abs(got.astype(np.longdouble) - ref).astype(np.float64)
    print(f"{where}: worst {float(np.max(err / np.maximum(gate, 1e-300))):.3f} of the gate")
    assert np.all(err <= gate), (where, float(np.max(err / np.maximum(gate, 1e-300))))
    live = gate > 0
    assert not got[~live].any(), where   # no product: exactly zero
    return float(np.max(err[live] / gate[live])) if live.any() else 0.0


def measure(P, dt, case, mode):
    """(worst use forward, worst use inverse) over the batch; asserts the bits of batch 1 and of chunks of one signal"""
    import torch

    xs, cs, fwd, inv = reference(case, dt, mode)
    pl = planner(P, dt, case, mode)
    L, nc, f, J = case_len(case, mode), fwd[0][0].size, case[1], case[2]
    assert pl.signal_len == L and pl.coeff_len == nc == sum(P.dwt_coeff_lens(L, f, J, mode)) and pl.tile == TILE
    assert pl.level_lens == R.level_lens(L, f, J, mode)
    assert [n for _, n in pl.bands()] == P.dwt_coeff_lens(L, f, J, mode) and [o for o, _ in pl.bands()] == list(np.cumsum([0] + P.dwt_coeff_lens(L, f, J, mode))[:-1])
    per = pl.workspace_min()
    assert per == (0 if J == 1 else max(pl.level_lens[1:J:2]) + max(pl.level_lens[2:J:2], default=0)) and pl.workspace_len(BATCH) == BATCH * per
    use = []
    for inverse, rows, refs in ((False, xs, fwd), (True, cs, inv)):
        n, m = (nc, L) if inverse else (L, nc)
        got = batched(P, inverse, pl, rows, dt, (n + 5) | 1, (m + 3) | 1)
        alone = batched(P, inverse, pl, rows[2:], dt, n, m, off=0)[0]
        small = torch.empty(per + 1, dtype=_tdt(dt), device="cuda")
        chunks = batched(P, inverse, pl, rows, dt, (n + 7) | 1, (m + 9) | 1, off=3 if dt == "f32" else 1, work=small[1:] if per else None)
        assert np.array_equal(alone, got[2]) and all(np.array_equal(a, b) for a, b in zip(chunks, got)), (case, dt, mode, inverse)
        use.append(max(_use(g, ref, gate, f"{'waverec' if inverse else 'wavedec'} {case_id(case)} {mode} {dt} signal {i}")
                       for i, (g, (ref, gate)) in enumerate(zip(got, refs))))
    return tuple(use)


@pytest.mark.parametrize("case", CASES, ids=case_id)
@pytest.mark.parametrize("dt", DTS)
def test_parity(gpu, dt, case):
    """forward, and inverse on random coefficients, in all six modes: batch 3 at odd distances one element off a 16-byte
    boundary, batch 1, and the batch in chunks of one signal in a workspace of workspace_min()"""
    for mode in R.MODES:
        fwd, inv = measure(gpu, dt, case, mode)
        print(f"dwt {case_id(case)} {mode} {dt}: wavedec {fwd:.3f}, waverec {inv:.3f} of the gates")


# ---- round trip ----
@functools.lru_cache(maxsize=None)
def round_trip_reference(name, L, J, dt, mode):
    import phastft_amd as P

    bank = tuple(np.asarray(b, dtype=NDT[dt]) for b in P.wavelet_filters(name))
    f = bank[0].size
    x = signal(L, dt, seed=L + J, batch=1)[0]
    defect = np.abs(R.waverec(R.wavedec(x, bank, J, mode), bank, mode, L) - x.astype(np.longdouble))
    scale = R.abs_waverec(R.abs_wavedec(x, bank, J, mode), bank, mode, L)
    return x, (2 * J * (f + 2) * U[dt] * scale + defect).astype(np.float64)


def measure_round_trip(P, dt, name, L, J, mode):
    import torch

    x, gate = round_trip_reference(name, L, J, dt, mode)
    d_x = torch.from_numpy(x).cuda().reshape(1, 1, L)
    coeffs = P.wavedec(d_x, name, mode, J)
    assert [c.shape[-1] for c in coeffs] == P.dwt_coeff_lens(L, name, J, mode) and coeffs[0].shape[:2] == (1, 1)
    back = P.waverec(coeffs, name, mode)
    # the list fixes the length up to one sample: the longer signal comes back, its first L samples are x
    assert back.shape[-1] in (L, L + 1)
    return _use(back[0, 0, :L].cpu().numpy(), x.astype(np.longdouble), gate, f"round trip {name} L={L} J={J} {mode} {dt}")


@pytest.mark.parametrize("dt", DTS)
def test_round_trip(gpu, dt):
    """waverec(wavedec(x)) against x through the conveniences, the built-in banks, all six modes"""
    for name, L, J in ROUND_TRIPS:
        for mode in R.MODES:
            measure_round_trip(gpu, dt, name, L, J, mode)


# ---- the conveniences ----
@pytest.mark.parametrize("dt", DTS)
def test_conveniences_against_the_reference(gpu, dt):
    """dwt, idwt, wavedec and waverec on device tensors with leading axes; a wavelet by name and as four arrays"""
    import torch

    P, u = gpu, U[dt]
    L = 45
    rows = signal(L, dt, seed=77, batch=4)
    dev = torch.from_numpy(np.stack(rows).reshape(2, 2, L)).cuda()
    for wavelet, mode in (("db3", "symmetric"), ("haar", "periodization"), (R.legall53(), "reflect"), ("db2", "zero")):
        bank = tuple(np.asarray(b, dtype=NDT[dt]) for b in (P.wavelet_filters(wavelet) if isinstance(wavelet, str) else wavelet))
        f = bank[0].size
        cA, cD = P.dwt(dev, wavelet, mode)
        assert cA.shape == cD.shape == (2, 2, R.level_len(L, f, mode))
        rec = P.idwt(cA, cD, wavelet, mode)
        assert rec.shape == (2, 2, R.synth_len(cA.shape[-1], f, mode))
        coeffs = P.wavedec(dev, wavelet, mode, 3)
        back = P.waverec(coeffs, wavelet, mode)
        for i, x in enumerate(rows):
            ra, rd = R.analysis_level(x, bank[0], bank[1], mode)
            ga, gd = R.analysis_level(np.abs(x), np.abs(bank[0]), np.abs(bank[1]), mode)
            where = f"dwt {mode} {dt} row {i}"
            _use(cA[i // 2, i % 2].cpu().numpy(), ra, ((f + 2) * u * ga).astype(np.float64), where)
            _use(cD[i // 2, i % 2].cpu().numpy(), rd, ((f + 2) * u * gd).astype(np.float64), where)
            a, d = cA[i // 2, i % 2].cpu().numpy(), cD[i // 2, i % 2].cpu().numpy()
            _use(rec[i // 2, i % 2].cpu().numpy(), R.synthesis_level(a, d, bank[2], bank[3], mode),
                 ((f + 2) * u * R.synthesis_level(np.abs(a), np.abs(d), np.abs(bank[2]), np.abs(bank[3]), mode)).astype(np.float64), "i" + where)
            ref = R.wavedec(x, bank, 3, mode)
            scale = R.abs_wavedec(x, bank, 3, mode)
            assert len(coeffs) == 4
            for j, (c, r, s) in enumerate(zip(coeffs, ref, scale)):
                level = 3 if j == 0 else 4 - j
                _use(c[i // 2, i % 2].cpu().numpy(), r, (level * (f + 2) * u * s).astype(np.float64), f"wavedec band {j} " + where)
            parts = [c[i // 2, i % 2].cpu().numpy() for c in coeffs]
            n = back.shape[-1]
            assert n in (L, L + 1)
            _use(back[i // 2, i % 2].cpu().numpy()[:L], R.waverec(parts, bank, mode, L),
                 (3 * (f + 2) * u * R.abs_waverec(parts, bank, mode, L)).astype(np.float64), "waverec " + where)
    with pytest.raises(ValueError):
        P.waverec([coeffs[0], coeffs[1][..., :-1]], "db2")
    with pytest.raises(ValueError):
        P.idwt(cA, None, "db2")
    with pytest.raises(TypeError):
        P.dwt(dev.to(torch.complex64), "db2")


# ---- bits ----
@pytest.mark.parametrize("dt", DTS)
def test_bit_identity(gpu, dt):
    """the same input returns the same bits alone and inside a batch, through buf[1:] and buf[3:] views (one and three elements
    off a 16-byte boundary), on a side stream, in one captured graph replayed on new data, and through the host form -- both
    directions"""
    import torch

    P = gpu
    for case, mode in (((17, 4, 3), "symmetric"), ((4100, 20, 5), "periodization"), ((-(2 * TILE + 3), 6, 2), "reflect"), ((5, 8, 1), "periodic")):
        pl = planner(P, dt, case, mode)
        L, nc = pl.signal_len, pl.coeff_len
        for inverse in (False, True):
            n, m = (nc, L) if inverse else (L, nc)
            fn = P.waverec_batched if inverse else P.wavedec_batched
            rows = signal(n, dt, seed=11 + inverse)
            alone = [batched(P, inverse, pl, [r], dt, n, m, off=0)[0] for r in rows]
            for off in (1, 3):
                got = batched(P, inverse, pl, rows, dt, (n + 5 + off) | 1, (m + 3 + off) | 1, off=off)
                assert all(np.array_equal(a, g) for a, g in zip(alone, got)), (case, mode, inverse, off)
            side = torch.cuda.Stream()
            assert np.array_equal(batched(P, inverse, pl, [rows[1]], dt, n, m, off=1, stream=side)[0], alone[1]), (case, mode, inverse, "side stream")
            # graph replay on new data
            d_x = torch.zeros(n, dtype=_tdt(dt), device="cuda")
            out = torch.zeros(m, dtype=_tdt(dt), device="cuda")
            work = torch.empty(max(1, pl.workspace_len(1)), dtype=_tdt(dt), device="cuda")
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):  # warm-up on the capture stream
                fn(d_x, pl, out=out, work=work)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                fn(d_x, pl, out=out, work=work)
            for i in (0, 2):
                d_x.copy_(torch.from_numpy(np.ascontiguousarray(rows[i], dtype=NDT[dt])))
                out.zero_()
                g.replay()
                torch.cuda.synchronize()
                assert np.array_equal(out.cpu().numpy(), alone[i]), (case, mode, inverse, "graph", i)
            host = getattr(P, f"{'waverec' if inverse else 'wavedec'}_{dt[1:]}_with_planner")
            h_out = np.zeros(m, NDT[dt])
            host(np.ascontiguousarray(rows[2], dtype=NDT[dt]), h_out, pl)
            assert np.array_equal(h_out, alone[2]), (case, mode, inverse, "host")


# ---- the guarded arena ----
@pytest.mark.parametrize("case,mode", [((17, 4, 3), "symmetric"), ((4100, 20, 5), "periodization"), ((9, 4, 4), "zero")], ids=lambda v: v if isinstance(v, str) else case_id(v))
@pytest.mark.parametrize("inverse", [False, True], ids=["wavedec", "waverec"])
@pytest.mark.parametrize("dt", DTS)
def test_arena(gpu, dt, inverse, case, mode):
    """a _dev call in the poisoned, guarded arena: workspace lengths workspace_min(), that plus 1, chunks of two plus 1 and
    workspace_len(3) at three bases -- bands whole, inputs kept, the bits of a zero-filled workspace, gaps keep their sentinel,
    one element below workspace_min() is refused with nothing written; and an output declared one short is seen"""
    import torch

    from tests import test_gpu_workspace_guard as G

    P = gpu
    pl = planner(P, dt, case, mode)
    xs, cs, fwd, inv = reference(case, dt, mode)
    L, nc = pl.signal_len, pl.coeff_len
    n, m = (nc, L) if inverse else (L, nc)
    in_dist, out_dist = (n + 5) | 1, (m + 3) | 1
    fn = P.waverec_batched if inverse else P.wavedec_batched

    def call(t, work):
        fn(torch.as_strided(t["x"], (G.BATCH, n), (in_dist, 1)), pl, out=torch.as_strided(t["out"], (G.BATCH, m), (out_dist, 1)), work=work)

    def gate(got):
        for i, (ref, bound) in enumerate(inv if inverse else fwd):
            _use(got["out"][i], ref, bound, f"arena {case_id(case)} {mode} {dt} {inverse}")

    planes = [G.Plane("x", "in", n, in_dist, [r.astype(NDT[dt]) for r in (cs if inverse else xs)]), G.Plane("out", "out", m, out_dist)]
    c = G.Case(f"dwt:{case}:{mode}:{inverse}", dt, 0, planes, G._lengths(pl.workspace_min(), pl.workspace_len(2) + 1, pl.workspace_len(G.BATCH)), call, gate)
    G.drive(P, c)
    G.overrun(P, c, "out")


@pytest.mark.parametrize("dt", DTS)
def test_one_level_does_not_read_the_workspace(gpu, dt):
    """J = 1: workspace_len is 0 and a d_work of NaN between guard bands is neither read nor written -- the bits of a call
    without one"""
    import torch

    from tests import test_gpu_workspace_guard as G

    P = gpu
    for case, mode in (((3, 4, 1), "periodization"), ((-(TILE + 1), 6, 1), "symmetric")):
        pl = planner(P, dt, case, mode)
        assert pl.workspace_len(BATCH) == pl.workspace_min() == 0
        xs, cs, fwd, inv = reference(case, dt, mode)
        for inverse in (False, True):
            n, m = (pl.coeff_len, pl.signal_len) if inverse else (pl.signal_len, pl.coeff_len)
            in_dist, out_dist = (n + 5) | 1, (m + 3) | 1
            fn = P.waverec_batched if inverse else P.wavedec_batched

            def call(t, work):
                fn(torch.as_strided(t["x"], (G.BATCH, n), (in_dist, 1)), pl, out=torch.as_strided(t["out"], (G.BATCH, m), (out_dist, 1)), work=work)

            planes = [G.Plane("x", "in", n, in_dist, [r.astype(NDT[dt]) for r in (cs if inverse else xs)]), G.Plane("out", "out", m, out_dist)]
            c = G.Case(f"dwt1:{case}:{mode}:{inverse}", dt, 0, planes, [("poisoned", 64)], call, None)
            for off in (0, 1, 16 // np.dtype(NDT[dt]).itemsize - 1):
                a, before = G._run(c, 64, off, "poison")
                nan_bits = a.bytes_of("work").clone()
                assert a.check() == [], (c.tag, off)
                for name, kept in before.items():
                    assert torch.equal(a.bytes_of(name), kept), (c.tag, name)
                assert torch.equal(a.bytes_of("work"), nan_bits) and bool(torch.isnan(a["work"]).all()), c.tag
                plain = G._packed(c, 64, off, "poison")
                call({p.name: plain[p.name] for p in planes}, None)
                assert torch.equal(a.bytes_of("out"), plain.bytes_of("out")), c.tag
                G._gaps_keep_the_sentinel(c, a, c.tag)
                for g, (ref, bound) in zip(G._rows(c, a)["out"], inv if inverse else fwd):
                    _use(g, ref, bound, c.tag)


# ---- status codes ----
@pytest.mark.parametrize("dt", DTS)
def test_codes_describe_and_stages(gpu, dt):
    """a wrong length, null pointers, short distances, a null or short workspace and identical pointers come back with their
    codes and write nothing; describe names the parts; the stage timers leave the results behind"""
    import torch

    from phastft_amd import _lib

    P, n_ = gpu, C.c_size_t
    lib = _lib.lib()
    case, mode = (17, 4, 3), "symmetric"
    pl, p1 = planner(P, dt, case, mode), planner(P, dt, (3, 4, 1), "zero")
    L, nc, w = pl.signal_len, pl.coeff_len, pl.workspace_len(2)
    assert (L, nc, pl.workspace_min(), w) == (17, 24, 16, 32) and pl.level_offsets == [0, 14, 8, 4]
    big = torch.zeros(4096, dtype=_tdt(dt), device="cuda")
    at = lambda off: C.c_void_p(big.data_ptr() + off * big.element_size())  # noqa: E731
    px, pc, pw = at(0), at(1000), at(2000)
    for name in ("wavedec", "waverec"):
        dev = getattr(lib, f"phast_{name}_{dt}_dev")
        a, b, da, db = (px, pc, L, nc) if name == "wavedec" else (pc, px, nc, L)
        ok = (n_(L), n_(2), n_(da), n_(db), pl._h, pw, n_(w), None)
        assert dev(None, b, *ok) == 16 and dev(a, None, *ok) == 16 and dev(a, a, *ok) == 16
        assert dev(a, b, n_(L - 1), n_(1), n_(da), n_(db), pl._h, pw, n_(w), None) == 3          # PHAST_ERR_PLANNER_SIZE
        assert dev(a, b, n_(L), n_(2), n_(da - 1), n_(db), pl._h, pw, n_(w), None) == 16         # a distance below the row
        assert dev(a, b, n_(L), n_(2), n_(da), n_(db - 1), pl._h, pw, n_(w), None) == 16
        assert dev(a, b, n_(L), n_(1), n_(da), n_(db), pl._h, None, n_(w), None) == 16           # a null workspace
        assert dev(a, b, n_(L), n_(1), n_(da), n_(db), pl._h, pw, n_(pl.workspace_min() - 1), None) == 16
        assert dev(a, b, n_(L), n_(0), n_(da), n_(db), pl._h, None, n_(0), None) == 0            # an empty batch
        assert dev(a, b, n_(L), n_(1), n_(da), n_(db), None, pw, n_(w), None) == 16
    torch.cuda.synchronize()
    assert not bool(big.any())  # none of the refused calls ran
    kind = P.PlannerDwt64 if dt == "f64" else P.PlannerDwt32
    for bad in (lambda: kind(0, "db2"), lambda: kind(16, "db2", 0), lambda: kind(16, "db2", 33), lambda: kind((1 << 29) + 1, "haar")):
        with pytest.raises(P.PhastPanic) as e:
            bad()
        assert e.value.code == 16
    assert pl.describe() == "dwt L=17 F=4 J=3 mode=symmetric coeffs=24 tile=1024 levels 10,6,4 work=16"
    assert p1.describe() == "dwt L=3 F=4 J=1 mode=zero coeffs=6 tile=1024 levels 3 work=0"
    assert pl.device_bytes() == 16 * np.dtype(NDT[dt]).itemsize
    x = signal(L, dt, seed=5, batch=1)[0]
    for name, n, m in (("wavedec", L, nc), ("waverec", nc, L)):
        host = getattr(P, f"{name}_{dt[1:]}_with_planner")
        with pytest.raises(P.PhastPanic) as e:
            host(np.zeros(n - 1, NDT[dt]), np.zeros(m, NDT[dt]), pl)
        assert e.value.code == (3 if name == "wavedec" else 2)
        with pytest.raises(P.PhastPanic) as e:
            host(np.zeros(n, NDT[dt]), np.zeros(m - 1, NDT[dt]), pl)
        assert e.value.code == (2 if name == "wavedec" else 3)     # PHAST_ERR_LEN_MISMATCH: the packed row; 3: the signal
    want = batched(P, False, pl, [x], dt, L, nc, off=0)[0]
    back = batched(P, True, pl, [want], dt, nc, L, off=0)[0]
    d_x, d_c = torch.from_numpy(x).cuda(), torch.zeros(nc, dtype=_tdt(dt), device="cuda")
    st = pl.time_stages(d_x, d_c, 1, reps=1)
    assert len(st) == 2 and all(v >= 0 for v in st)
    assert np.array_equal(d_c.cpu().numpy(), want) and np.array_equal(d_x.cpu().numpy(), back)


# ---- the budget ----
def budget_keys():
    keys = {(dt, "cascade", case_id(c), mode) for dt in DTS for c in CASES for mode in R.MODES}
    return keys | {(dt, "round trip", f"{name}x{L}x{J}", mode) for dt in DTS for name, L, J in ROUND_TRIPS for mode in R.MODES}


def test_gates_keep_their_margin():
    """every gate sits >= 2 x over its worst use measured on the MI355X, and no case, mode or type is missing"""
    budget = json.load(open(BUDGET))
    have = {(e["dt"], e["what"], e["case"], e["mode"]) for e in budget["entries"]}
    assert have == budget_keys() and len(budget["entries"]) == len(have)
    for e in budget["entries"]:
        assert 0 <= e["use"] <= 0.5, e
