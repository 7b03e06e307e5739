"""Sample-rate conversion on the MI355X (csrc/resample.hip, csrc/planner_resample.hpp) against tests/resample_reference.py, the
definitions in long double.

Polyphase path: an output is a sum of n = Kp products, so |got - ref| <= (n + 2) u sum |h x| whatever the order (u = 2^-53 /
2^-24; ref: the long double sum over the same T-rounded taps and samples; sum |h x| formed per output).  Fourier path (its
signals are f32 values for both types, so one reference serves both): tests/tolerances.py's check_real at the log2 of the
larger inner transform (tests/resample_reference.py: fourier_log2).  The worst use of every gate is in
tests/golden/resample_error_budget.json, written on the MI355X by tests/golden/make_resample_error_budget.py;
test_gates_keep_their_margin keeps every entry 2 x inside."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

from tests import resample_reference as R
from tests import tolerances as tol
from tests.test_resample_cpu import _windows

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTS = ["f64", "f32"]
BUDGET = os.path.join(ROOT, "tests", "golden", "resample_error_budget.json")
BATCH = 3


def _tdt(dt):
    import torch

    return torch.float64 if dt == "f64" else torch.float32


def case_id(c):
    return "x".join(str(v) for v in c)


def _pow2(n):
    return n >= 4 and n & (n - 1) == 0


def _dist(n, extra):
    """a distance above the row: odd, but even where the power-of-two real transforms need it"""
    return n + extra + (n + extra) % 2 if _pow2(n) else (n + extra) | 1


# ---- polyphase ----
@functools.lru_cache(maxsize=None)
def poly_reference(case, dt):
    """taps, BATCH signals (values of the type) and, per signal, the long double outputs 0 .. the furthest any window reaches
    with their sum |h x|"""
    L, K, up, down = case
    h, xs = R.taps(K, dt), R.signal(L, dt, batch=BATCH)
    reach = max(first + (n if n is not None else R.full_len(L, K, up, down) - first) for first, n in _windows(L, K, up, down))
    return h, xs, [R.upfirdn_ref(h, x, up, down, 0, reach) for x in xs]


@functools.lru_cache(maxsize=None)
def up_planner(P, dt, case, first, out_len):
    L, K, up, down = case
    return (P.PlannerUpfirdn64 if dt == "f64" else P.PlannerUpfirdn32)(L, R.taps(K, dt), up, down, first, out_len)


def batched(P, fn, pl, rows, dt, sig_dist, out_dist, off=1, work=None, stream=None):
    """`rows` through fn (upfirdn_batched / resample_batched) at the distances, from `off` elements past a 16-byte boundary:
    the outputs; the inputs, the gaps and what lies around the outputs are not written"""
    import torch

    b, n, m = len(rows), pl.signal_len, pl.out_len
    buf = torch.full((off + b * sig_dist + 4,), 9.0, dtype=_tdt(dt), device="cuda")
    x = torch.as_strided(buf, (b, n), (sig_dist, 1), off)
    for i, r in enumerate(rows):
        x[i] = torch.from_numpy(np.ascontiguousarray(r, dtype=R.NDT[dt]))
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


def measure_poly(P, dt, case):
    """the worst |got - ref| / gate over the windows of the case and the signals of the batch; asserts the bits of batch 1"""
    L, K, up, down = case
    h, xs, refs = poly_reference(case, dt)
    worst = 0.0
    for first, out_len in _windows(L, K, up, down):
        pl = up_planner(P, dt, case, first, out_len)
        m = pl.out_len
        assert pl.full_len == R.full_len(L, K, up, down) and m == (out_len or pl.full_len - first)
        assert (pl.tile, pl.chunk) == (R.geom(K, up, down)[3], R.geom(K, up, down)[1]) and pl.workspace_len(BATCH) == 0
        got = batched(P, P.upfirdn_batched, pl, xs, dt, (L + 5) | 1, (m + 3) | 1)
        alone = batched(P, P.upfirdn_batched, pl, xs[2:], dt, L, m, off=0)[0]
        assert np.array_equal(alone, got[2]), (case, dt, first, out_len)
        for g, (ref, scale) in zip(got, refs):
            err = np.abs(g.astype(np.longdouble) - ref[first:first + m]).astype(np.float64)
            gate = R.poly_gate(dt, K, up, scale[first:first + m])
            assert np.all(err <= gate), (case, dt, first, out_len, float(np.max(err / np.maximum(gate, 1e-300))))
            live = gate > 0
            assert not g[~live].any()   # no product: exactly zero
            if live.any():
                worst = max(worst, float(np.max(err[live] / gate[live])))
    return worst


@pytest.mark.parametrize("case", R.UPFIRDN_CASES, ids=case_id)
@pytest.mark.parametrize("dt", DTS)
def test_upfirdn_parity(gpu, dt, case):
    """the whole result, and windows of one tile - 1, one tile, one tile + 1 and two tiles + 3 outputs from first = 3 on, past
    full_len where the result is shorter: batch 3 at odd distances one element off a 16-byte boundary, and batch 1"""
    worst = measure_poly(gpu, dt, case)
    print(f"upfirdn {case_id(case)} {dt}: worst {worst:.3f} of the gate")


# ---- Fourier ----
@functools.lru_cache(maxsize=None)
def fourier_reference(case):
    L, num = case
    xs = R.signal(L, "f32", batch=BATCH)
    return xs, [np.asarray(R.resample_ref(x, num), np.float64) for x in xs]


@functools.lru_cache(maxsize=None)
def rs_planner(P, dt, case):
    return (P.PlannerResample64 if dt == "f64" else P.PlannerResample32)(*case)


def measure_fourier(P, dt, case):
    """(worst rel / gate, worst bin / gate) over the signals of the batch; asserts the bits of batch 1 and of chunks"""
    import torch

    L, num = case
    xs, refs = fourier_reference(case)
    pl = rs_planner(P, dt, case)
    got = batched(P, P.resample_batched, pl, xs, dt, _dist(L, 5), _dist(num, 3))
    alone = batched(P, P.resample_batched, pl, xs[2:], dt, L, num, off=0)[0]
    small = torch.empty(pl.workspace_min() + 1, dtype=_tdt(dt), device="cuda")
    chunks = batched(P, P.resample_batched, pl, xs, dt, _dist(L, 7), _dist(num, 9), off=3 if dt == "f32" else 1, work=small[1:])
    assert np.array_equal(alone, got[2]) and all(np.array_equal(a, b) for a, b in zip(chunks, got)), (case, dt)
    lg = R.fourier_log2(L, num)
    g_rel, g_bin = tol.gates(dt, lg)
    use = [0.0, 0.0]
    for i, (g, ref) in enumerate(zip(got, refs)):
        rel, worst = tol.check_real(f"resample:{L}:{num}:{i}", dt, lg, g, ref)
        use = [max(use[0], rel / g_rel), max(use[1], worst / g_bin)]
    return use


@pytest.mark.parametrize("case", R.FOURIER_CASES, ids=case_id)
@pytest.mark.parametrize("dt", DTS)
def test_resample_parity(gpu, dt, case):
    """batch 3 at distances above the rows, batch 1, and the batch in chunks of one signal in a workspace of workspace_min()"""
    rel, worst = measure_fourier(gpu, dt, case)
    print(f"resample {case_id(case)} {dt}: rel {rel:.3f}, bin {worst:.3f} of the gates")


# ---- against scipy ----
@pytest.mark.parametrize("dt", DTS)
def test_conveniences_against_scipy(gpu, dt):
    """upfirdn, resample_poly, decimate and resample on device tensors with leading axes, against scipy on the host in double
    from the same T-rounded signal.  Polyphase bound: scipy's own sum and the device's each stay inside (Kp + 2) u sum |h x|
    (scipy filters an f32 signal in f32), and the taps as rounded to T differ from scipy's by up to 2 u each: (2 (Kp + 2) + 4) u
    sum |h x| in all.  Fourier: check_real against scipy in double."""
    import torch
    from scipy import signal as S

    P = gpu
    u = R.U[dt]
    x = R.signal(300, dt, seed=3, batch=2).reshape(2, 1, 300)
    dev = torch.from_numpy(x).cuda()
    x64 = x.astype(np.float64)

    def poly_check(got, want, h, up, down, first, tag):
        assert got.shape == want.shape, tag
        kp = R.kp_of(len(h), up)
        for i in range(2):
            scale = R.upfirdn_ref(np.abs(h), np.abs(x64[i, 0]), up, down, first, want.shape[-1])[0].astype(np.float64)
            err = np.abs(got[i, 0].astype(np.float64) - want[i, 0])
            assert np.all(err <= (2 * (kp + 2) + 4) * u * scale + 1e-300), (tag, dt, float(np.max(err / (u * scale + 1e-300))))

    h = R.taps(33, dt)
    got = P.upfirdn(h, dev, 2, 3)
    poly_check(got.cpu().numpy(), S.upfirdn(h.astype(np.float64), x64, 2, 3, axis=-1), h.astype(np.float64), 2, 3, 0, "upfirdn")
    for up, down in ((160, 147), (147, 160), (3, 2), (1, 4), (4, 1), (6, 4)):
        got = P.resample_poly(dev, up, down).cpu().numpy()
        hp, u_, d_, first, _ = R.resample_poly_plan(300, up, down)
        poly_check(got, S.resample_poly(x64, up, down, axis=-1), np.asarray(hp, np.float64), u_, d_, first, f"resample_poly {up}/{down}")
    assert torch.equal(P.resample_poly(dev, 5, 5), dev)
    b = R.taps(9, dt).astype(np.float64)
    hp, u_, d_, first, _ = R.resample_poly_plan(300, 3, 2, taps=b)
    poly_check(P.resample_poly(dev, 3, 2, window=b).cpu().numpy(), S.resample_poly(x64, 3, 2, axis=-1, window=b), np.asarray(hp, np.float64),
               u_, d_, first, "resample_poly taps")
    for q, n in ((4, None), (3, None), (2, 10)):
        got = P.decimate(dev, q, n).cpu().numpy()
        taps = R.firwin_ref((20 * q if n is None else n) + 1, 1.0 / q, "hamming")
        hp, u_, d_, first, _ = R.resample_poly_plan(300, 1, q, taps=taps)
        poly_check(got, S.decimate(x64, q, n, ftype="fir", axis=-1), np.asarray(hp, np.float64), u_, d_, first, f"decimate {q}")
    for num in (441, 300, 128, 601):
        got = P.resample(dev, num).cpu().numpy()
        want = S.resample(x64, num, axis=-1)
        assert got.shape == want.shape == (2, 1, num)
        for i in range(2):
            tol.check_real(f"resample_vs_scipy:{num}", dt, R.fourier_log2(300, num), got[i, 0], want[i, 0])


# ---- bits ----
@pytest.mark.parametrize("dt", DTS)
def test_bit_identity(gpu, dt):
    """the same signal returns the same bits alone and inside a batch, through buf[1:] and buf[3:] views (one and three
    elements off a 16-byte boundary), on a side stream and in a replayed graph -- both methods"""
    import torch

    P = gpu
    jobs = [(P.upfirdn_batched, up_planner(P, dt, c, 3, None), c[0]) for c in ((17, 7, 3, 2), (300, 3201, 160, 147), (20, 6000, 300, 7))]
    jobs += [(P.resample_batched, rs_planner(P, dt, c), c[0]) for c in ((8, 12), (1000, 441), (9, 6))]
    for fn, pl, L in jobs:
        rows = R.signal(L, "f32", seed=11, batch=BATCH)
        m = pl.out_len
        alone = [batched(P, fn, pl, [r], dt, L, m, off=0)[0] for r in rows]
        for off in (1, 3):
            got = batched(P, fn, pl, rows, dt, _dist(L, 5 + off), _dist(m, 3 + off), off=off)
            assert all(np.array_equal(a, g) for a, g in zip(alone, got)), (fn.__name__, L, m, off)
        side = torch.cuda.Stream()
        assert np.array_equal(batched(P, fn, pl, [rows[1]], dt, L, m, off=1, stream=side)[0], alone[1]), (fn.__name__, "side stream")
        # graph replay on new data
        d_x = torch.zeros(L, dtype=_tdt(dt), device="cuda")
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
            d_x.copy_(torch.from_numpy(np.ascontiguousarray(rows[i], dtype=R.NDT[dt])))
            out.zero_()
            g.replay()
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy(), alone[i]), (fn.__name__, "graph", i)
        # the host form
        host = getattr(P, f"{'upfirdn' if fn is P.upfirdn_batched else 'resample'}_{dt[1:]}_with_planner")
        h_out = np.zeros(m, R.NDT[dt])
        host(np.ascontiguousarray(rows[2], dtype=R.NDT[dt]), h_out, pl)
        assert np.array_equal(h_out, alone[2]), (fn.__name__, "host")


# ---- the guarded arena ----
def _rs_case(P, dt, case):
    from tests import test_gpu_workspace_guard as G

    L, num = case
    pl = rs_planner(P, dt, case)
    xs, refs = fourier_reference(case)
    sig_dist, out_dist = _dist(L, 5), _dist(num, 3)

    def call(t, work):
        import torch

        P.resample_batched(torch.as_strided(t["x"], (G.BATCH, L), (sig_dist, 1)), pl,
                           out=torch.as_strided(t["out"], (G.BATCH, num), (out_dist, 1)), work=work)

    def gate(got):
        for i in range(G.BATCH):
            tol.check_real(f"guard:resample:{case}", dt, R.fourier_log2(L, num), got["out"][i], refs[i])

    planes = [G.Plane("x", "in", L, sig_dist, [x.astype(R.NDT[dt]) for x in xs]), G.Plane("out", "out", num, out_dist)]
    lengths = G._lengths(pl.workspace_min(), pl.workspace_len(2) + 1, pl.workspace_len(G.BATCH))
    m = max(0 if n & (n - 1) == 0 else R.inner_m(n) for n in case)
    return G.Case(f"resample:{case}", dt, m, planes, lengths, call, gate)


@pytest.mark.parametrize("case", [(1000, 441), (8, 13)], ids=case_id)
@pytest.mark.parametrize("dt", DTS)
def test_arena_resample(gpu, dt, case):
    """the Fourier _dev call in the poisoned, guarded arena: workspace lengths workspace_min(), that plus 1, chunks of two plus 1
    and workspace_len(3) at three bases -- bands whole, inputs kept, the bits of a zero-filled workspace, gaps keep their
    sentinel, one element below workspace_min() is refused with nothing written; and an output declared one short is seen"""
    from tests import test_gpu_workspace_guard as G

    c = _rs_case(gpu, dt, case)
    G.drive(gpu, c)
    G.overrun(gpu, c, "out")


@pytest.mark.parametrize("case", [(17, 7, 3, 2), (300, 3201, 160, 147), (20, 6000, 300, 7)], ids=case_id)
@pytest.mark.parametrize("dt", DTS)
def test_arena_upfirdn(gpu, dt, case):
    """the polyphase _dev call between guard bands with a poisoned workspace it must not read: bands whole, inputs kept, the
    workspace still NaN, the bits of a call without one, the gaps keep their sentinel, inside the gate"""
    import torch

    from tests import test_gpu_workspace_guard as G

    P = gpu
    L, K, up, down = case
    h, xs, refs = poly_reference(case, dt)
    pl = up_planner(P, dt, case, 3, None)
    m = pl.out_len
    sig_dist, out_dist = (L + 5) | 1, (m + 3) | 1

    def call(t, work):
        P.upfirdn_batched(torch.as_strided(t["x"], (G.BATCH, L), (sig_dist, 1)), pl,
                          out=torch.as_strided(t["out"], (G.BATCH, m), (out_dist, 1)), work=work)

    planes = [G.Plane("x", "in", L, sig_dist, [x.astype(R.NDT[dt]) for x in xs]), G.Plane("out", "out", m, out_dist)]
    c = G.Case(f"upfirdn:{case}", dt, 0, planes, [("poisoned", 64)], call, None)
    for off in (0, 1, 16 // np.dtype(R.NDT[dt]).itemsize - 1):
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
        for g, (ref, scale) in zip(G._rows(c, a)["out"], refs):
            err = np.abs(g.astype(np.longdouble) - ref[3:3 + m]).astype(np.float64)
            assert np.all(err <= R.poly_gate(dt, K, up, scale[3:3 + m])), (c.tag, off)
    G.overrun(P, c, "out")


# ---- status codes ----
@pytest.mark.parametrize("dt", DTS)
def test_codes_describe_and_stages(gpu, dt):
    """a wrong length, null pointers, short distances, a null or short workspace and illegal arguments come back with their codes
    and write nothing; describe names the parts; the stage timers leave the result behind"""
    import torch

    from phastft_amd import _lib

    P, n_ = gpu, C.c_size_t
    lib = _lib.lib()
    L, K, up, down = case = (40, 33, 2, 3)
    pu, pr = up_planner(P, dt, case, 0, None), rs_planner(P, dt, (1000, 441))
    big = torch.zeros(4096 + pr.workspace_len(2), dtype=_tdt(dt), device="cuda")
    at = lambda off: C.c_void_p(big.data_ptr() + off * big.element_size())  # noqa: E731
    px, po, pw = at(0), at(1100), at(2200)
    dev = getattr(lib, f"phast_upfirdn_{dt}_dev")
    m = pu.out_len
    assert dev(None, po, n_(L), n_(1), n_(L), n_(m), pu._h, None, n_(0), None) == 16
    assert dev(px, None, n_(L), n_(1), n_(L), n_(m), pu._h, None, n_(0), None) == 16
    assert dev(px, po, n_(L - 1), n_(1), n_(L), n_(m), pu._h, None, n_(0), None) == 3     # PHAST_ERR_PLANNER_SIZE
    assert dev(px, po, n_(L), n_(2), n_(L - 1), n_(m), pu._h, None, n_(0), None) == 16    # sig_dist below the row
    assert dev(px, po, n_(L), n_(2), n_(L), n_(m - 1), pu._h, None, n_(0), None) == 16    # out_dist below the row
    assert dev(px, po, n_(L), n_(0), n_(L), n_(m), pu._h, None, n_(0), None) == 0         # an empty batch
    dev = getattr(lib, f"phast_resample_{dt}_dev")
    size = n_(pr.workspace_len(1))
    assert dev(None, po, n_(1000), n_(1), n_(1000), n_(441), pr._h, pw, size, None) == 16
    assert dev(px, None, n_(1000), n_(1), n_(1000), n_(441), pr._h, pw, size, None) == 16
    assert dev(px, po, n_(999), n_(1), n_(1000), n_(441), pr._h, pw, size, None) == 3
    assert dev(px, po, n_(1000), n_(2), n_(999), n_(441), pr._h, pw, size, None) == 16
    assert dev(px, po, n_(1000), n_(2), n_(1000), n_(440), pr._h, pw, size, None) == 16
    assert dev(px, po, n_(1000), n_(1), n_(1000), n_(441), pr._h, None, size, None) == 16
    assert dev(px, po, n_(1000), n_(1), n_(1000), n_(441), pr._h, pw, n_(pr.workspace_min() - 1), None) == 16
    assert dev(px, po, n_(1000), n_(0), n_(1000), n_(441), pr._h, None, n_(0), None) == 0
    p8 = rs_planner(P, dt, (8, 12))   # powers of two move the real side in pairs: an odd distance in a batch is refused
    assert dev(px, po, n_(8), n_(2), n_(9), n_(12), p8._h, pw, size, None) == 16
    torch.cuda.synchronize()
    assert not bool(big.any())  # none of the refused calls ran
    for bad in ((0, 2), (2, 0), ((1 << 20) + 1, 1)):
        with pytest.raises(P.PhastPanic) as e:
            (P.PlannerUpfirdn64 if dt == "f64" else P.PlannerUpfirdn32)(L, np.ones(3), *bad)
        assert e.value.code == 16
    with pytest.raises(P.PhastPanic) as e:
        (P.PlannerResample64 if dt == "f64" else P.PlannerResample32)(8, 0)
    assert e.value.code == 16
    g = R.geom(K, up, down)
    assert pu.describe() == (f"upfirdn L={L} K={K} up={up} down={down} first=0 out={m} of {m}: Kp={R.kp_of(K, up)} tile={g[3]} "
                             f"chunk={g[1]} x {g[0]} phase rows")
    assert pr.describe().startswith("resample L=1000 num=441 bins=221: real any N=1000")
    assert pu.device_bytes() == up * (R.kp_of(K, up) | 1) * np.dtype(R.NDT[dt]).itemsize and pr.device_bytes() > 0
    assert rs_planner(P, dt, (8, 8)).describe().endswith("(both ways)")
    for fn, pl, name in ((P.upfirdn_batched, pu, "upfirdn"), (P.resample_batched, pr, "resample")):
        host = getattr(P, f"{name}_{dt[1:]}_with_planner")
        x = R.signal(pl.signal_len, dt, seed=5)
        with pytest.raises(P.PhastPanic) as e:
            host(x[:-1].copy(), np.zeros(pl.out_len, R.NDT[dt]), pl)
        assert e.value.code == 3
        with pytest.raises(P.PhastPanic) as e:
            host(x, np.zeros(pl.out_len - 1, R.NDT[dt]), pl)
        assert e.value.code == 2  # PHAST_ERR_LEN_MISMATCH
        want = batched(P, fn, pl, [x], dt, pl.signal_len, pl.out_len, off=0)[0]
        d_x, d_o = torch.from_numpy(x).cuda(), torch.zeros(pl.out_len, dtype=_tdt(dt), device="cuda")
        st = pl.time_stages(d_x, d_o, 1, reps=1)
        assert len(st) == (1 if name == "upfirdn" else 3) and all(v >= 0 for v in st)
        assert np.array_equal(d_o.cpu().numpy(), want)


# ---- the budget ----
def budget_keys():
    return {(dt, "upfirdn", case_id(c)) for dt in DTS for c in R.UPFIRDN_CASES} | {(dt, "resample", case_id(c)) for dt in DTS for c in R.FOURIER_CASES}


def test_gates_keep_their_margin():
    """every gate sits >= 2 x over its worst use measured on the MI355X, and no case or type is missing"""
    budget = json.load(open(BUDGET))
    have = {(e["dt"], e["method"], e["case"]) for e in budget["entries"]}
    assert have == budget_keys() and len(budget["entries"]) == len(have)
    for e in budget["entries"]:
        assert 0 <= e["use"] <= 0.5, e
