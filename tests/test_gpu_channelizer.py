"""The polyphase channelizer on the MI355X (csrc/channelizer.hip, csrc/planner_channelizer.hpp) against
tests/channelizer_reference.py, the definition in long double on the T-rounded taps and samples.

Gates (nothing fitted): a fold element is a chain of T products, |error| <= (T + 2) u A with A = sum |h x| (u = 2^-53 / 2^-24),
and the DFT carries a relative L2 error through unchanged: rel-L2 <= tolerances.rel_gate(dt, log2 M) + (T + 2) u |A|_2 / |U|_2,
and the worst bin relative to the rms bin <= tolerances.bin_gate(dt, log2 M) + (T + 2) u max_m sum_p A[m][p] / rms.  M = 1 has no
transform: per output, as upfirdn.  The worst use of every gate is in tests/golden/channelizer_error_budget.json, written on
the MI355X by tests/golden/make_channelizer_error_budget.py."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

from tests import channelizer_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = os.path.join(ROOT, "tests", "golden", "channelizer_error_budget.json")
DTS = ["f64", "f32"]
KINDS = ["real", "complex"]
BATCH = R.BATCH


def _tdt(dt):
    import torch

    return torch.float64 if dt == "f64" else torch.float32


@functools.lru_cache(maxsize=None)
def reference(case, dt, cplx):
    """taps, BATCH signals (values of the type) and, per signal, (y, u, a) for the frames 0 .. the furthest any window reaches"""
    L, K, M, D = case
    h, xs = R.taps(K, dt), R.signals(case, dt, cplx)
    full = R.full_frames(L, K, D)
    reach = max(first + (n if n is not None else full - first) for first, n in R.windows(case))
    return h, xs, [R.channelize_ref(h, x, M, D, 0, reach) for x in xs]


@functools.lru_cache(maxsize=None)
def planner(P, dt, case, first, out_frames, cplx):
    L, K, M, D = case
    return (P.PlannerChannelizer64 if dt == "f64" else P.PlannerChannelizer32)(L, R.taps(K, dt), M, D, first, out_frames, cplx)


def batched(P, pl, rows, dt, sig_dist, off=1, work=None, stream=None):
    """`rows` (real or complex host signals) through channelize_batched at distance sig_dist, every plane `off` elements past a
    16-byte boundary: per signal the complex (out_frames, bins) result; the inputs and what lies around the outputs are not
    written"""
    import torch

    b, n, pts = len(rows), pl.signal_len, pl.out_frames * pl.bins
    planes, keeps = [], []
    for part in ("real", "imag") if pl.complex_input else ("real",):
        buf = torch.full((off + b * sig_dist + 4,), 9.0, dtype=_tdt(dt), device="cuda")
        x = torch.as_strided(buf, (b, n), (sig_dist, 1), off)
        for i, r in enumerate(rows):
            x[i] = torch.from_numpy(np.ascontiguousarray(getattr(np.asarray(r), part), dtype=R.NDT[dt]))
        planes.append(x if b > 1 else x[0])
        keeps.append((buf, buf.clone()))
    obuf = torch.full((2, off + b * pts + 4), 9.0, dtype=_tdt(dt), device="cuda")
    out = (obuf[0, off:off + b * pts], obuf[1, off:off + b * pts])
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    P.channelize_batched(tuple(planes) if pl.complex_input else planes[0], pl, out=out, work=work, stream=stream)
    torch.cuda.synchronize()
    assert all(torch.equal(buf, keep) for buf, keep in keeps)
    got = obuf.cpu().numpy()
    assert (got[:, :off] == 9.0).all() and (got[:, off + b * pts:] == 9.0).all()
    z = (got[0, off:off + b * pts] + 1j * got[1, off:off + b * pts]).reshape(b, pl.out_frames, pl.bins)
    return [z[i].copy() for i in range(b)]


def measure(P, dt, case, cplx):
    """the worst use of (rel, bin) gates over the windows of the case and the signals of the batch; asserts the bits of batch 1"""
    L, K, M, D = case
    h, xs, refs = reference(case, dt, cplx)
    use = [0.0, 0.0]
    for first, out_frames in R.windows(case):
        pl = planner(P, dt, case, first, out_frames, cplx)
        n = pl.out_frames
        g = R.geom(K, M, D)
        assert pl.full_frames == R.full_frames(L, K, D) and n == (out_frames or pl.full_frames - first)
        assert pl.bins == (M if cplx else M // 2 + 1)
        assert (pl.tile_cols, pl.tile_frames, pl.chunk, pl.periods) == (g[0], g[3], g[5], g[6])
        got = batched(P, pl, xs, dt, (L + 5) | 1)
        alone = batched(P, pl, xs[2:], dt, L, off=0)[0]
        assert np.array_equal(alone, got[2]), (case, dt, cplx, first, out_frames)
        for i, (z, (y, u, a)) in enumerate(zip(got, refs)):
            rel, worst = R.check(f"channelize:{R.case_id(case)}:{'c' if cplx else 'r'}:{first}+{n}:{i}", dt, K, M, z,
                                 y[first:first + n, :pl.bins], u[first:first + n], a[first:first + n])
            use = [max(use[0], rel), max(use[1], worst)]
    return use


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dt", DTS)
def test_parity(gpu, dt, kind, case):
    """the whole result, and windows of one tile - 1, one tile, one tile + 1 frames and past full_frames from frame 3 on: batch 3
    at an odd distance one element off a 16-byte boundary, and batch 1 to the same bits"""
    rel, worst = measure(gpu, dt, case, kind == "complex")
    print(f"channelize {R.case_id(case)} {kind} {dt}: rel {rel:.3f}, bin {worst:.3f} of the gates")


BIT_CASES = [(37, 24, 8, 4), (30, 50, 7, 3), (600, 1030, 257, 257), (3000, 2048, 256, 192)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dt", DTS)
def test_bit_identity(gpu, dt, kind):
    """the same signal returns the same bits alone and inside a batch, through buf[1:] and buf[3:] views, on a side stream, in a
    replayed graph, chunked to workspace_min() and through the host form"""
    import torch

    P, cplx = gpu, kind == "complex"
    for case in BIT_CASES:
        L = case[0]
        pl = planner(P, dt, case, 3, None, cplx)
        rows = R.signals(case, dt, cplx, seed=11)
        pts = pl.out_frames * pl.bins
        alone = [batched(P, pl, [r], dt, L, off=0)[0] for r in rows]
        for off in (1, 3):
            got = batched(P, pl, rows, dt, (L + 5 + off) | 1, off=off)
            assert all(np.array_equal(a, g) for a, g in zip(alone, got)), (case, off)
        side = torch.cuda.Stream()
        assert np.array_equal(batched(P, pl, [rows[1]], dt, L, off=1, stream=side)[0], alone[1]), (case, "side stream")
        if pl.workspace_min():
            small = torch.full((pl.workspace_min() + 1,), float("nan"), dtype=_tdt(dt), device="cuda")
            got = batched(P, pl, rows, dt, (L + 7) | 1, off=1, work=small[1:])
            assert all(np.array_equal(a, g) for a, g in zip(alone, got)), (case, "chunks")
        # graph replay on new data
        d_x = [torch.zeros(L, dtype=_tdt(dt), device="cuda") for _ in range(2 if cplx else 1)]
        out = torch.zeros((2, pts), dtype=_tdt(dt), device="cuda")
        work = torch.empty(max(1, pl.workspace_len(1)), dtype=_tdt(dt), device="cuda")
        arg = tuple(d_x) if cplx else d_x[0]
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):  # warm-up on the capture stream
            P.channelize_batched(arg, pl, out=(out[0], out[1]), work=work)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            P.channelize_batched(arg, pl, out=(out[0], out[1]), work=work)
        for i in (0, 2):
            d_x[0].copy_(torch.from_numpy(np.ascontiguousarray(rows[i].real, dtype=R.NDT[dt])))
            if cplx:
                d_x[1].copy_(torch.from_numpy(np.ascontiguousarray(rows[i].imag, dtype=R.NDT[dt])))
            out.zero_()
            g.replay()
            torch.cuda.synchronize()
            o = out.cpu().numpy()
            assert np.array_equal((o[0] + 1j * o[1]).reshape(alone[i].shape), alone[i]), (case, "graph", i)
        # the host form
        host = getattr(P, f"channelize_{dt[1:]}_with_planner")
        h_re, h_im = np.zeros(pts, R.NDT[dt]), np.zeros(pts, R.NDT[dt])
        x = rows[2]
        host(np.ascontiguousarray(x.real, dtype=R.NDT[dt]), h_re, h_im, pl,
             signal_im=np.ascontiguousarray(x.imag, dtype=R.NDT[dt]) if cplx else None)
        assert np.array_equal((h_re + 1j * h_im).reshape(alone[2].shape), alone[2]), (case, "host")


# ---- the guarded arena ----
@pytest.mark.parametrize("case", [(30, 50, 7, 3), (600, 1030, 257, 257), (3000, 2048, 256, 192)], ids=R.case_id)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dt", DTS)
def test_arena(gpu, dt, kind, case):
    """the _dev call in the poisoned (NaN), guarded arena: workspace lengths workspace_min(), that plus 1, chunks of two plus 1
    and workspace_len(3) at three bases -- bands whole, inputs kept, the bits of a zero-filled workspace, one element below
    workspace_min() refused with nothing written; and an output declared one short is seen.  Without a workspace (complex, a
    power-of-two M): a poisoned one is left alone."""
    import torch

    from tests import test_gpu_workspace_guard as G

    P, cplx = gpu, kind == "complex"
    L, K, M, D = case
    pl = planner(P, dt, case, 3, None, cplx)
    h, xs, refs = reference(case, dt, cplx)
    n, pts, dist = pl.out_frames, pl.out_frames * pl.bins, (L + 5) | 1

    def call(t, work):
        x = torch.as_strided(t["x"], (G.BATCH, L), (dist, 1))
        if cplx:
            x = (x, torch.as_strided(t["xi"], (G.BATCH, L), (dist, 1)))
        P.channelize_batched(x, pl, out=(t["re"], t["im"]), work=work)

    def gate(got):
        for b in range(G.BATCH):
            y, u, a = refs[b]
            z = (got["re"][b] + 1j * got["im"][b]).reshape(n, pl.bins)
            R.check(f"guard:channelize:{case}", dt, K, M, z, y[3:3 + n, :pl.bins], u[3:3 + n], a[3:3 + n])

    planes = [G.Plane("x", "in", L, dist, [np.asarray(x.real, R.NDT[dt]) for x in xs])]
    if cplx:
        planes.append(G.Plane("xi", "in", L, dist, [np.asarray(x.imag, R.NDT[dt]) for x in xs]))
    planes += [G.Plane("re", "out", pts, pts), G.Plane("im", "out", pts, pts)]
    vec = G._vec(dt)
    if pl.workspace_min():
        per = pl.workspace_min() - (vec - 1)
        lengths = G._lengths(pl.workspace_min(), 2 * per + vec, pl.workspace_len(G.BATCH))
        m = 1 << (2 * (M if cplx or M % 2 else M // 2) - 2).bit_length()
    else:
        lengths, m = [("poisoned", 64)], 0
    c = G.Case(f"channelize:{case}:{kind}", dt, m, planes, lengths, call, gate)
    G.drive(P, c, gate_at=(lengths[0][0], 1))
    G.overrun(P, c, "re")


# ---- status codes ----
@pytest.mark.parametrize("dt", DTS)
def test_codes_describe_and_stages(gpu, dt):
    """a wrong length, null pointers, the wrong imaginary plane, short distances, identical pointers, a null or short workspace
    and illegal arguments come back with their codes and write nothing; describe names the parts; the stage timers leave the
    result behind"""
    import torch

    from phastft_amd import _lib

    P, n_ = gpu, C.c_size_t
    lib = _lib.lib()
    case = L, K, M, D = (30, 50, 7, 3)
    pr, pc = planner(P, dt, case, 0, None, False), planner(P, dt, case, 0, None, True)
    big = torch.zeros(8192 + pc.workspace_len(2), dtype=_tdt(dt), device="cuda")
    at = lambda off: C.c_void_p(big.data_ptr() + off * big.element_size())  # noqa: E731
    px, pxi, pre, pim, pw = at(0), at(100), at(200), at(1200), at(2200)
    dev = getattr(lib, f"phast_channelize_{dt}_dev")
    for pl, xi in ((pr, None), (pc, pxi)):
        size = n_(pl.workspace_len(1))
        assert dev(None, xi, pre, pim, n_(L), n_(1), n_(L), pl._h, pw, size, None) == 16
        assert dev(px, xi, None, pim, n_(L), n_(1), n_(L), pl._h, pw, size, None) == 16
        assert dev(px, xi, pre, None, n_(L), n_(1), n_(L), pl._h, pw, size, None) == 16
        assert dev(px, pxi if xi is None else None, pre, pim, n_(L), n_(1), n_(L), pl._h, pw, size, None) == 16  # the wrong planes
        assert dev(px, xi, pre, pim, n_(L - 1), n_(1), n_(L), pl._h, pw, size, None) == 3      # PHAST_ERR_PLANNER_SIZE
        assert dev(px, xi, pre, pim, n_(L), n_(2), n_(L - 1), pl._h, pw, size, None) == 16     # sig_dist below the row
        assert dev(px, xi, px, pim, n_(L), n_(1), n_(L), pl._h, pw, size, None) == 16          # output on the input
        assert dev(px, xi, pre, pre, n_(L), n_(1), n_(L), pl._h, pw, size, None) == 16         # one output plane
        assert dev(px, xi, pre, pim, n_(L), n_(1), n_(L), pl._h, None, size, None) == 16       # no workspace
        assert dev(px, xi, pre, pim, n_(L), n_(1), n_(L), pl._h, pw, n_(pl.workspace_min() - 1), None) == 16
        assert dev(px, xi, pre, pim, n_(L), n_(0), n_(L), pl._h, None, n_(0), None) == 0       # an empty batch
    torch.cuda.synchronize()
    assert not bool(big.any())  # none of the refused calls ran
    cls = P.PlannerChannelizer64 if dt == "f64" else P.PlannerChannelizer32
    big_n = (1 << 29) + 1
    for bad in ((0, np.ones(3), 4, 4), (big_n, np.ones(3), 4, 4), (8, np.ones(3), 0, 1), (8, np.ones(3), 4, 0),
                (8, np.ones(3), big_n, 4), (8, np.ones(3), 4, big_n), (8, np.ones(0), 4, 4),
                (8, np.ones(3), 4, 4, 4),                    # first_frame > full_frames = 3
                (8, np.ones(3), 4, 4, 3, None),              # no frame left
                (8, np.ones(3), 1 << 20, 4, 0, 1025)):       # out_frames M > 2^30
        with pytest.raises(P.PhastPanic) as e:
            cls(*bad)
        assert e.value.code == 16, bad
    host = getattr(P, f"channelize_{dt[1:]}_with_planner")
    pts = pr.out_frames * pr.bins
    x = R.signal(L, dt, seed=5)
    with pytest.raises(P.PhastPanic) as e:
        host(x[:-1].copy(), np.zeros(pts, R.NDT[dt]), np.zeros(pts, R.NDT[dt]), pr)
    assert e.value.code == 3
    with pytest.raises(P.PhastPanic) as e:
        host(x, np.zeros(pts - 1, R.NDT[dt]), np.zeros(pts - 1, R.NDT[dt]), pr)
    assert e.value.code == 2  # PHAST_ERR_LEN_MISMATCH
    with pytest.raises(P.PhastPanic) as e:
        host(x, np.zeros(pts, R.NDT[dt]), np.zeros(pts, R.NDT[dt]), pr, signal_im=x.copy())
    assert e.value.code == 16
    g = R.geom(K, M, D)
    full = R.full_frames(L, K, D)
    assert pr.describe().startswith(f"channelizer real L={L} K={K} M={M} D={D} first=0 frames={full} of {full}: T={R.t_of(K, M)} "
                                    f"tile={g[3]} x {g[0]} chunk={g[5]} periods={g[6]} around real any N=7")
    assert "around any N=7" in pc.describe()
    assert ("(taps held)" in planner(P, dt, (37, 24, 8, 8), 0, None, True).describe()) == (dt == "f64")   # D mod M = 0, f64 only
    assert pr.device_bytes() > R.t_of(K, M) * M * np.dtype(R.NDT[dt]).itemsize
    assert planner(P, dt, (37, 24, 8, 8), 0, None, True).workspace_len(5) == 0
    for pl, cplx in ((pr, False), (pc, True)):
        xs = R.signals(case, dt, cplx, seed=5)[:1]
        want = batched(P, pl, xs, dt, L, off=0)[0]
        d_re = torch.from_numpy(np.ascontiguousarray(xs[0].real, dtype=R.NDT[dt])).cuda()
        d_im = torch.from_numpy(np.ascontiguousarray(xs[0].imag, dtype=R.NDT[dt])).cuda() if cplx else None
        out = torch.zeros((2, pl.out_frames * pl.bins), dtype=_tdt(dt), device="cuda")
        st = pl.time_stages(d_re, d_im, out[0], out[1], 1, reps=1)
        assert len(st) == 2 and all(v >= 0 for v in st)
        o = out.cpu().numpy()
        assert np.array_equal((o[0] + 1j * o[1]).reshape(want.shape), want)


# ---- the conveniences ----
@pytest.mark.parametrize("dt", DTS)
def test_channelize_poly_against_scipy(gpu, dt):
    """channelize_poly on device tensors with a leading axis against the scipy expression on the host in double from the same
    T-rounded signal and taps, real and complex, a pfb_prototype and an oversampled hop.  The gates of the parity test with the
    fold's term doubled.  The host side is exact next to the f32 gate; in f64 its own sums of K products and its phases stay
    within (K + 16) u sum |h x| per bin (tests/test_channelizer_cpu.py), 80 u sum |h x| for K = 64: with sum |h x| a few times
    the rms bin that is under half the transform's worst-bin gate of 64 eps 4 alone, and far less in rel-L2."""
    import torch
    from scipy import signal as S

    P = gpu
    for (L, M, T, D), cplx in (((300, 16, 4, 16), True), ((257, 12, 3, 9), False)):
        h = P.pfb_prototype(M, T).astype(R.NDT[dt])
        x = R.signals((L,), dt, cplx, seed=3)[:2]
        dev = torch.from_numpy(np.ascontiguousarray(x).astype(np.complex128 if dt == "f64" else np.complex64) if cplx
                               else np.ascontiguousarray(x, dtype=R.NDT[dt])).cuda().reshape(2, 1, L)
        got = P.channelize_poly(dev, h, M, D).cpu().numpy()
        n = np.arange(L)
        bins = M if cplx else M // 2 + 1
        for i in range(2):
            want = np.stack([S.upfirdn(h.astype(np.float64), x[i] * np.exp(-2j * np.pi * ((k * n) % M) / M), 1, D) for k in range(bins)], 1)
            assert got[i, 0].shape == want.shape
            y, u, a = R.channelize_ref(h, x[i], M, D)
            R.check(f"poly:{L}:{M}:{D}:{i}", dt, len(h), M, got[i, 0], want, u, 2 * a)


# ---- the budget ----
def test_gates_keep_their_margin():
    """every gate sits >= 2 x over its worst use measured on the MI355X, and no case, kind or type is missing"""
    budget = json.load(open(BUDGET))
    have = {(e["dt"], e["kind"], e["case"]) for e in budget["entries"]}
    assert have == {(dt, kind, R.case_id(c)) for dt in DTS for kind in KINDS for c in R.CASES} and len(budget["entries"]) == len(have)
    for e in budget["entries"]:
        assert 0 <= e["use"] <= 0.5, e
