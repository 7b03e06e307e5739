"""The polyphase synthesis bank on the MI355X (csrc/synthesizer.hip, csrc/planner_synthesizer.hpp) against
tests/synthesizer_reference.py, the definition in long double on the T-rounded channel data and on the planner's T-rounded
scaled taps.

Gates (nothing fitted): an output is a chain of t(n) products on taps rounded once more (M g[j]), |error|
<= (t + 3) u A[n] with A = sum_m |tab v| (u = 2^-53 / 2^-24); the transform's error enters through tolerances.bin_gate(dt, log2 M)
relative to the rms of a row of v -- the inner Bluestein length's log2 where M is no power of two --, carried through
B[n] = sum_m |tab[n - m D]| rms(v[m]).  Per output: (t + 3) u A[n] + bin_gate B[n]; in L2: |(t + 3) u A|_2 + rel_gate |B|_2.  An
output without a term is exactly 0.  M = 1 has no transform.  The worst use of every gate is in
tests/golden/synthesizer_error_budget.json, written on the MI355X by tests/golden/make_synthesizer_error_budget.py.

Round trip and adjoint: the sum of the two planners' gates on the same data, the channelizer's worst-bin bound (its gate times
the rms bin plus its fold's term, tests/channelizer_reference.py) carried through the synthesis by the triangle inequality."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

from tests import channelizer_reference as A
from tests import synthesizer_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = os.path.join(ROOT, "tests", "golden", "synthesizer_error_budget.json")
DTS = ["f64", "f32"]
KINDS = ["real", "complex"]
BATCH = R.BATCH
CLD = R.CLD


def _tdt(dt):
    import torch

    return torch.float64 if dt == "f64" else torch.float32


@functools.lru_cache(maxsize=None)
def reference(case, dt, real):
    """taps, BATCH signals' channel data (values of the type) and, per signal, (s, a, t, b) on 0 .. the furthest any window reaches"""
    F, K, M, D = case
    g, ys = R.taps(K, dt), R.frames(case, dt, real)
    tab = R.scaled_taps(g, M, dt)
    return g, ys, [R.synth_ref(tab, y, M, D, real, R.reach(case)) for y in ys]


@functools.lru_cache(maxsize=None)
def planner(P, dt, case, first, out_len, real):
    F, K, M, D = case
    return (P.PlannerSynthesizer64 if dt == "f64" else P.PlannerSynthesizer32)(F, R.taps(K, dt), M, D, first, out_len, not real)


def batched(P, pl, ys, dt, out_dist, off=1, work=None, stream=None):
    """the channel data `ys` (complex (F, bins) each) through synthesize_batched into signals out_dist apart, every plane `off`
    elements past a 16-byte boundary: per signal the (out_len,) result, complex for a complex planner; the inputs and what
    lies around and between the outputs are not written"""
    import torch

    b, n, pts = len(ys), pl.out_len, pl.frames * pl.bins
    ibuf = torch.full((2, off + b * pts + 4), 9.0, dtype=_tdt(dt), device="cuda")
    for i, y in enumerate(ys):
        y = np.asarray(y)
        ibuf[0, off + i * pts:off + (i + 1) * pts] = torch.from_numpy(np.ascontiguousarray(y.real, dtype=R.NDT[dt]).reshape(-1))
        ibuf[1, off + i * pts:off + (i + 1) * pts] = torch.from_numpy(np.ascontiguousarray(y.imag, dtype=R.NDT[dt]).reshape(-1))
    keep = ibuf.clone()
    shape = (b, pl.frames, pl.bins) if b > 1 else (pl.frames, pl.bins)
    planes = tuple(ibuf[p, off:off + b * pts].reshape(shape) for p in range(2))
    np_ = 2 if pl.complex_output else 1
    span = (b - 1) * out_dist + n
    obuf = torch.full((np_, off + span + 4), 9.0, dtype=_tdt(dt), device="cuda")
    outs = tuple(torch.as_strided(obuf[p, off:], (b, n), (out_dist, 1)) if b > 1 else obuf[p, off:off + n] for p in range(np_))
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    P.synthesize_batched(planes, pl, out=outs if pl.complex_output else outs[0], work=work, stream=stream)
    torch.cuda.synchronize()
    assert torch.equal(ibuf, keep)
    got = obuf.cpu().numpy()
    mask = np.ones(got.shape[1], bool)
    for i in range(b):
        mask[off + i * out_dist:off + i * out_dist + n] = False
    assert (got[:, mask] == 9.0).all()
    rows = [got[:, off + i * out_dist:off + i * out_dist + n] for i in range(b)]
    return [(r[0] + 1j * r[1]) if pl.complex_output else r[0].copy() for r in rows]


def measure(P, dt, case, real):
    """the worst use of (per-output, L2) gates over the windows of the case and the signals of the batch; asserts the bits of
    batch 1"""
    F, K, M, D = case
    g, ys, refs = reference(case, dt, real)
    use = [0.0, 0.0]
    for first, out_len in R.windows(case):
        pl = planner(P, dt, case, first, out_len, real)
        n = pl.out_len
        assert pl.full_len == R.full_len(F, K, D) and n == (out_len or pl.full_len - first)
        assert pl.bins == (M // 2 + 1 if real else M)
        assert (pl.tile_samples, pl.per_thread, pl.max_terms) == R.geom(K, M, D)[:3]
        got = batched(P, pl, ys, dt, (n + 5) | 1)
        alone = batched(P, pl, ys[2:], dt, n, off=0)[0]
        assert np.array_equal(alone, got[2]), (case, dt, real, first, out_len)
        for i, (z, (s, a, t, b)) in enumerate(zip(got, refs)):
            w = slice(first, first + n)
            out, l2 = R.check(f"synthesize:{R.case_id(case)}:{'r' if real else 'c'}:{first}+{n}:{i}", dt, M, z, s[w], a[w], t[w], b[w])
            use = [max(use[0], out), max(use[1], l2)]
    return use


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dt", DTS)
def test_parity(gpu, dt, kind, case):
    """the whole result, and windows of one tile - 1, one tile, one tile + 1 samples and past full_len from sample 3 on: batch 3
    at an odd distance one element off a 16-byte boundary, and batch 1 to the same bits"""
    out, l2 = measure(gpu, dt, case, kind == "real")
    print(f"synthesize {R.case_id(case)} {kind} {dt}: output {out:.3f}, L2 {l2:.3f} of the gates")


BIT_CASES = [(7, 25, 8, 4), (4, 50, 7, 3), (4, 1030, 257, 257), (14, 2048, 256, 192)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dt", DTS)
def test_bit_identity(gpu, dt, kind):
    """the same channel data returns the same bits alone and inside a batch, through buf[1:] and buf[3:] views, on a side
    stream, in a replayed graph on new data, chunked to workspace_min() and through the host form"""
    import torch

    P, real = gpu, kind == "real"
    for case in BIT_CASES:
        pl = planner(P, dt, case, 3, None, real)
        n, pts = pl.out_len, pl.frames * pl.bins
        ys = R.frames(case, dt, real, seed=11)
        alone = [batched(P, pl, [y], dt, n, off=0)[0] for y in ys]
        for off in (1, 3):
            got = batched(P, pl, ys, dt, (n + 5 + off) | 1, off=off)
            assert all(np.array_equal(a, g) for a, g in zip(alone, got)), (case, off)
        side = torch.cuda.Stream()
        assert np.array_equal(batched(P, pl, [ys[1]], dt, n, off=1, stream=side)[0], alone[1]), (case, "side stream")
        assert pl.workspace_min() > 0
        small = torch.full((pl.workspace_min() + 1,), float("nan"), dtype=_tdt(dt), device="cuda")
        got = batched(P, pl, ys, dt, (n + 7) | 1, off=1, work=small[1:])
        assert all(np.array_equal(a, g) for a, g in zip(alone, got)), (case, "chunks")
        # graph replay on new data
        d_y = tuple(torch.zeros((pl.frames, pl.bins), dtype=_tdt(dt), device="cuda") for _ in range(2))
        out = torch.zeros((2, n), dtype=_tdt(dt), device="cuda")
        work = torch.empty(max(1, pl.workspace_len(1)), dtype=_tdt(dt), device="cuda")
        o_arg = out[0] if real else (out[0], out[1])
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):  # warm-up on the capture stream
            P.synthesize_batched(d_y, pl, out=o_arg, work=work)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            P.synthesize_batched(d_y, pl, out=o_arg, work=work)
        for i in (0, 2):
            d_y[0].copy_(torch.from_numpy(np.ascontiguousarray(ys[i].real, dtype=R.NDT[dt])))
            d_y[1].copy_(torch.from_numpy(np.ascontiguousarray(ys[i].imag, dtype=R.NDT[dt])))
            out.zero_()
            g.replay()
            torch.cuda.synchronize()
            o = out.cpu().numpy()
            assert np.array_equal(o[0] if real else o[0] + 1j * o[1], alone[i]), (case, "graph", i)
        # the host form
        host = getattr(P, f"synthesize_{dt[1:]}_with_planner")
        h_re, h_im = np.zeros(n, R.NDT[dt]), np.zeros(n, R.NDT[dt])
        y = ys[2]
        host(np.ascontiguousarray(y.real, dtype=R.NDT[dt]).reshape(-1), np.ascontiguousarray(y.imag, dtype=R.NDT[dt]).reshape(-1), h_re, pl,
             out_im=None if real else h_im)
        assert np.array_equal(h_re if real else h_re + 1j * h_im, alone[2]), (case, "host")


# ---- the guarded arena ----
@pytest.mark.parametrize("case", [(4, 50, 7, 3), (4, 1030, 257, 257), (14, 2048, 256, 192)], ids=R.case_id)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dt", DTS)
def test_arena(gpu, dt, kind, case):
    """the _dev call in the poisoned (NaN), guarded arena: workspace lengths workspace_min() (one signal), that plus 1, two
    signals plus 1 and workspace_len(3) at three bases -- bands whole, inputs kept, the bits of a zero-filled workspace, one
    element below workspace_min() refused with nothing written; and an output declared one short is seen"""
    import torch

    from tests import test_gpu_workspace_guard as G

    P, real = gpu, kind == "real"
    F, K, M, D = case
    pl = planner(P, dt, case, 3, None, real)
    g, ys, refs = reference(case, dt, real)
    n, pts, dist = pl.out_len, pl.frames * pl.bins, (pl.out_len + 5) | 1

    def call(t, work):
        y = tuple(t[k].reshape(G.BATCH, F, pl.bins) for k in ("re", "im"))
        outs = tuple(torch.as_strided(t[k], (G.BATCH, n), (dist, 1)) for k in (("x",) if real else ("x", "xi")))
        P.synthesize_batched(y, pl, out=outs[0] if real else outs, work=work)

    def gate(got):
        for b in range(G.BATCH):
            s, a, t, bb = refs[b]
            z = got["x"][b] if real else got["x"][b] + 1j * got["xi"][b]
            R.check(f"guard:synthesize:{case}", dt, M, z, s[3:3 + n], a[3:3 + n], t[3:3 + n], bb[3:3 + n])

    planes = [G.Plane("re", "in", pts, pts, [np.asarray(y.real, R.NDT[dt]).reshape(-1) for y in ys]),
              G.Plane("im", "in", pts, pts, [np.asarray(y.imag, R.NDT[dt]).reshape(-1) for y in ys]),
              G.Plane("x", "out", n, dist)]
    if not real:
        planes.append(G.Plane("xi", "out", n, dist))
    vec = G._vec(dt)
    per = pl.workspace_min() - (vec - 1)
    lengths = G._lengths(pl.workspace_min(), 2 * per + vec, pl.workspace_len(G.BATCH))
    m = 0 if M & (M - 1) == 0 else R.inner_m(M)
    c = G.Case(f"synthesize:{case}:{kind}", dt, m, planes, lengths, call, gate)
    G.drive(P, c, gate_at=(lengths[0][0], 1))
    G.overrun(P, c, "x")


# ---- status codes ----
@pytest.mark.parametrize("dt", DTS)
def test_codes(gpu, dt):
    """a wrong frame count, null pointers, the wrong imaginary plane, short distances, identical pointers, a null or short
    workspace and illegal arguments come back with their codes and write nothing; describe names the parts; the stage timers
    leave the result behind"""
    import torch

    from phastft_amd import _lib

    P, n_ = gpu, C.c_size_t
    lib = _lib.lib()
    case = F, K, M, D = (4, 50, 7, 3)
    pr, pc = planner(P, dt, case, 0, None, True), planner(P, dt, case, 0, None, False)
    big = torch.zeros(8192 + pc.workspace_len(2), dtype=_tdt(dt), device="cuda")
    at = lambda off: C.c_void_p(big.data_ptr() + off * big.element_size())  # noqa: E731
    pyr, pyi, pre, pim, pw = at(0), at(100), at(200), at(1200), at(2200)
    dev = getattr(lib, f"phast_synthesize_{dt}_dev")
    for pl, oi in ((pr, None), (pc, pim)):
        size, n = n_(pl.workspace_len(1)), pl.out_len
        assert dev(None, pyi, pre, oi, n_(F), n_(1), n_(n), pl._h, pw, size, None) == 16
        assert dev(pyr, None, pre, oi, n_(F), n_(1), n_(n), pl._h, pw, size, None) == 16
        assert dev(pyr, pyi, None, oi, n_(F), n_(1), n_(n), pl._h, pw, size, None) == 16
        assert dev(pyr, pyi, pre, pim if oi is None else None, n_(F), n_(1), n_(n), pl._h, pw, size, None) == 16  # the wrong planes
        assert dev(pyr, pyi, pre, oi, n_(F - 1), n_(1), n_(n), pl._h, pw, size, None) == 3     # PHAST_ERR_PLANNER_SIZE
        assert dev(pyr, pyi, pre, oi, n_(F), n_(2), n_(n - 1), pl._h, pw, size, None) == 16    # out_dist below the signal
        assert dev(pyr, pyi, pyr, oi, n_(F), n_(1), n_(n), pl._h, pw, size, None) == 16        # output on the input
        assert dev(pyr, pyr, pre, oi, n_(F), n_(1), n_(n), pl._h, pw, size, None) == 16        # one input plane
        assert dev(pyr, pyi, pre, oi, n_(F), n_(1), n_(n), pl._h, None, size, None) == 16      # no workspace
        assert dev(pyr, pyi, pre, oi, n_(F), n_(1), n_(n), pl._h, pw, n_(pl.workspace_min() - 1), None) == 16
        assert dev(pyr, pyi, pre, oi, n_(F), n_(0), n_(n), pl._h, None, n_(0), None) == 0      # an empty batch
    assert dev(pyr, pyi, pre, pre, n_(F), n_(1), n_(pc.out_len), pc._h, pw, n_(pc.workspace_len(1)), None) == 16  # one output plane
    torch.cuda.synchronize()
    assert not bool(big.any())  # none of the refused calls ran
    cls = P.PlannerSynthesizer64 if dt == "f64" else P.PlannerSynthesizer32
    big_n = (1 << 29) + 1
    for bad in ((0, np.ones(3), 4, 4), (big_n, np.ones(3), 1, 4), (8, np.ones(3), 0, 1), (8, np.ones(3), 4, 0),
                (8, np.ones(3), big_n, 4), (8, np.ones(3), 4, big_n), (8, np.ones(0), 4, 4),
                (8, np.ones(3), 4, 4, 32),                   # first > full_len = 31
                (8, np.ones(3), 4, 4, 31, None),             # no sample left
                (2048, np.ones(3), 1 << 20, 4),              # F M > 2^30
                (8, np.ones(3), 4, 4, 0, (1 << 30) + 1)):    # out_len > 2^30
        with pytest.raises(P.PhastPanic) as e:
            cls(*bad)
        assert e.value.code == 16, bad
    host = getattr(P, f"synthesize_{dt[1:]}_with_planner")
    pts = pr.frames * pr.bins
    z = lambda k: np.zeros(k, R.NDT[dt])  # noqa: E731
    with pytest.raises(P.PhastPanic) as e:
        host(z(pts - 1), z(pts - 1), z(pr.out_len), pr)
    assert e.value.code == 3
    with pytest.raises(P.PhastPanic) as e:
        host(z(pts), z(pts), z(pr.out_len - 1), pr)
    assert e.value.code == 2  # PHAST_ERR_LEN_MISMATCH
    with pytest.raises(P.PhastPanic) as e:
        host(z(pts), z(pts), z(pr.out_len), pr, out_im=z(pr.out_len))
    assert e.value.code == 16
    full = R.full_len(F, K, D)
    assert pr.describe().startswith(f"synthesizer real F={F} K={K} M={M} D={D} first=0 samples={full} of {full}: terms<={-(-K // D)} "
                                    f"tile={R.TILE} ({R.PER_THREAD} per thread, no LDS) behind real any N=7")
    assert "behind any N=7" in pc.describe()
    assert pr.device_bytes() > K * np.dtype(R.NDT[dt]).itemsize
    one = planner(P, dt, (1, 1, 1, 1), 0, None, False)
    assert one.workspace_len(5) == 0 and one.workspace_min() == 0 and "one point" in one.describe()
    for pl, real in ((pr, True), (pc, False)):
        ys = R.frames(case, dt, real, seed=5)[:1]
        want = batched(P, pl, ys, dt, pl.out_len, off=0)[0]
        d_re = torch.from_numpy(np.ascontiguousarray(ys[0].real, dtype=R.NDT[dt])).cuda().reshape(-1)
        d_im = torch.from_numpy(np.ascontiguousarray(ys[0].imag, dtype=R.NDT[dt])).cuda().reshape(-1)
        out = torch.zeros((2, pl.out_len), dtype=_tdt(dt), device="cuda")
        st = pl.time_stages(d_re, d_im, out[0], None if real else out[1], 1, reps=1)
        assert len(st) == 2 and all(v >= 0 for v in st)
        o = out.cpu().numpy()
        assert np.array_equal(o[0] if real else o[0] + 1j * o[1], want)


# ---- the pair: analysis, then synthesis ----
def _chan_bin_bound(dt, K, M, y, u, a):
    """what one real or imaginary part of a channelizer bin may be off by: its worst-bin gate times the rms bin plus its fold's
    term (tests/channelizer_reference.py); M = 1: the fold's bound alone"""
    if not np.any(a):
        return 0.0
    g_rel, g_bin, fold_bin = A.gates(dt, K, M, u, a)
    y_rms = float(np.sqrt(np.mean(np.abs(y) ** 2)))
    return g_bin * y_rms + fold_bin


def _sine_pair(M, dt):
    h = np.sin(np.pi * (np.arange(M) + 0.5) / M).astype(R.NDT[dt])
    g = (np.concatenate(([0.0], h[::-1].astype(np.float64))) / M).astype(R.NDT[dt])
    return h, g


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dt", DTS)
def test_round_trip(gpu, dt, kind):
    """synthesize_poly(channelize_poly(x, h, M, M / 2), g, M, M / 2) with h[j] = sin(pi (j + 1/2) / M) and g = (0, h reversed) / M
    is x delayed by M.  Three terms bound the difference: the synthesis gate on the reference's frames; the channelizer's
    worst-bin bound e, which reaches an output as at most sqrt(2) e M sum_m |g[n - m D]| (M bins of modulus <= sqrt(2) e per frame);
    and the identity's own error from the rounded taps: s[n] = sum_m sum_{n' = n mod M} tab[n - m D] h[m D - n'] x[n'] exactly, each
    product with three roundings in its factors (h, g, M g), so 4 u E[n] with E the same sum of absolute values."""
    import torch

    P, real = gpu, kind == "real"
    for M, D in ((8, 4), (6, 3), (512, 256)):
        L = 5 * M + 3
        h, g = _sine_pair(M, dt)
        tab = R.scaled_taps(g, M, dt)
        x = A.signals((L,), dt, not real, seed=7)[0]
        xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
        y = P.channelize_poly(xd, h, M, D)
        got = P.synthesize_poly(y, g, M, D, real=real).cpu().numpy()
        y_ref, u, a = A.channelize_ref(h, x, M, D)
        F = y_ref.shape[0]
        assert tuple(y.shape) == y_ref.shape and got.shape == (R.full_len(F, M + 1, D),) and np.iscomplexobj(got) == (not real)
        s, sa, st, sb = R.synth_ref(tab, y_ref, M, D, real)
        gate_s = R.gates(dt, M, sa, st, sb)[0]
        e_bin = _chan_bin_bound(dt, M, M, y_ref, u, a)
        at, ah, ax = np.abs(tab.astype(np.float64)), np.abs(h.astype(np.float64)), np.abs(np.asarray(x))
        carried, ident = np.zeros(got.size), np.zeros(got.size)
        j = np.arange(M + 1)
        for m in range(F):
            n = m * D + j
            carried[n] += np.sqrt(2.0) * e_bin * at          # tab = M g
            src = m * D - ((m * D - n) % M)                    # the one n' = n mod M under frame m's M taps
            ok = (src >= 0) & (src < L)
            ident[n] += np.where(ok, at * ah[np.clip(m * D - src, 0, M - 1)] * ax[np.clip(src, 0, L - 1)], 0.0)
        gate = gate_s + carried + 4 * R.U[dt] * ident
        want = np.zeros(got.size, np.complex128)
        want[M:M + L] = x
        d = got - want
        err = np.maximum(np.abs(d.real), np.abs(d.imag))
        live = gate > 0   # the leading zero tap alone reaches sample 0: an exact zero
        assert not np.any(err[~live]), (M, D, kind, dt)
        use = float(np.max(err[live] / gate[live]))
        print(f"round trip M={M} D={D} {kind} {dt}: worst output {use:.3f} of its gate, largest error {err.max():.3e}")
        assert use <= 1.0, (M, D, kind, dt, use)


@pytest.mark.parametrize("dt", DTS)
def test_adjoint(gpu, dt):
    """<Y, A x> = <(S Y)[K : K + L], x> through both planners, g = (0, h reversed) (M a power of two: M g is exact).  The sum of
    the two planners' gates: sum |Y| sqrt(2) e for the channelizer's worst-bin bound e, and sum |x| sqrt(2) gate[n] for the
    synthesis' per-output gate"""
    import torch

    P = gpu
    for L, K, M, D in ((37, 24, 8, 4), (3000, 2048, 256, 192)):
        h = A.taps(K, dt)
        g = np.concatenate(([0.0], h[::-1])).astype(R.NDT[dt])
        x = A.signals((L,), dt, True, seed=9)[0]
        ax = P.channelize_poly(torch.from_numpy(np.ascontiguousarray(x)).cuda(), h, M, D).cpu().numpy()
        F = ax.shape[0]
        Y = R.frames((F, K + 1, M, D), dt, False, seed=9)[0]
        sy = P.synthesize_poly(torch.from_numpy(np.ascontiguousarray(Y)).cuda(), g, M, D, 0, K + L).cpu().numpy()
        lhs = np.sum(np.conj(Y.astype(CLD)) * ax.astype(CLD))
        rhs = np.sum(np.conj(sy[K:K + L].astype(CLD)) * x.astype(CLD))
        y_ref, u, a = A.channelize_ref(h, x, M, D)
        s, sa, st, sb = R.synth_ref(R.scaled_taps(g, M, dt), Y, M, D, False, K + L)
        gate_s = R.gates(dt, M, sa, st, sb)[0]
        gate = np.sqrt(2.0) * (float(np.sum(np.abs(Y))) * _chan_bin_bound(dt, K, M, y_ref, u, a) + float(np.sum(np.abs(x) * gate_s[K:K + L])))
        print(f"adjoint L={L} K={K} M={M} D={D} {dt}: |lhs - rhs| {abs(lhs - rhs):.3e} of {gate:.3e} (|lhs| {abs(lhs):.3e})")
        assert abs(lhs - rhs) <= gate, (L, K, M, D, dt)


# ---- the conveniences ----
@pytest.mark.parametrize("dt", DTS)
def test_synthesize_poly_against_scipy(gpu, dt):
    """synthesize_poly on device tensors with a leading axis against the scipy expression on the host in double from the same
    T-rounded channel data and taps, real and complex, a pfb_prototype and an oversampled hop.  The gates of the parity test with
    the chain's term doubled: the host side's own sums and phases stay within (ceil(K / D) + M + 16) u sum |g| sum_k |Y| per output
    (tests/test_synthesizer_cpu.py), exact next to the f32 gate and, in f64, under the transform's term of 64 eps 4 B[n]."""
    import torch
    from scipy import signal as S

    P = gpu
    for (F, M, T, D), real in (((20, 16, 4, 16), False), ((23, 12, 3, 9), True)):
        g = P.pfb_prototype(M, T).astype(R.NDT[dt])
        ys = R.frames((F, len(g), M, D), dt, real, seed=3)[:2]
        dev = torch.from_numpy(np.ascontiguousarray(ys)).cuda().reshape(2, 1, F, ys.shape[-1])
        got = P.synthesize_poly(dev, g, M, D, real=real).cpu().numpy()
        full = R.full_len(F, len(g), D)
        n = np.arange(full)
        assert got.shape == (2, 1, full)
        for i in range(2):
            Yf = (R.hermitian_full(ys[i], M) if real else ys[i]).astype(np.complex128)
            want = sum(np.exp(2j * np.pi * ((k * n) % M) / M) * S.upfirdn(g.astype(np.float64), Yf[:, k], D, 1) for k in range(M))
            s, a, t, b = R.synth_ref(R.scaled_taps(g, M, dt), ys[i], M, D, real)
            R.check(f"poly:{F}:{M}:{D}:{i}", dt, M, got[i, 0], want.real if real else want, 2 * a, t, b)


# ---- the budget ----
def test_gates_keep_their_margin():
    """every gate sits >= 2 x over its worst use measured on the MI355X, and no case, kind or type is missing"""
    budget = json.load(open(BUDGET))
    have = {(e["dt"], e["kind"], e["case"]) for e in budget["entries"]}
    assert have == {(dt, kind, R.case_id(c)) for dt in DTS for kind in KINDS for c in R.CASES} and len(budget["entries"]) == len(have)
    for e in budget["entries"]:
        assert 0 <= e["use"] <= 0.5, e
