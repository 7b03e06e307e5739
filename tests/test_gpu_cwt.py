"""The continuous wavelet transform and the analytic signal on the MI355X (csrc/cwt.hip, csrc/planner_cwt.hpp) against
tests/cwt_reference.py, the definition in long double by direct sums.

Gates: tests/tolerances.py's `check`, unchanged, per row (signal, scale), at the log2 of the inner power-of-two transform of the
P-point complex transform (tests/cwt_reference.py: inner_log2), as the Fourier method of section 27 is gated.  The signals are
uniform [-1, 1) values that are exact in f32, so one reference serves both types.  A reference row that is identically zero
(P = 1: the only bin is k = 0, where every family but STEP is 0) must be matched exactly.  The worst use of every gate is in
tests/golden/cwt_error_budget.json, written on the MI355X by tests/golden/make_cwt_error_budget.py."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import scipy.signal

from tests import cwt_reference as R
from tests import tolerances as tol

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = os.path.join(ROOT, "tests", "golden", "cwt_error_budget.json")
DTS = ["f64", "f32"]
KINDS = ["real", "complex"]
NDT = {"f64": np.float64, "f32": np.float32}
BATCH = 3


def shape_id(shape):
    return "x".join(map(str, shape))


def _tdt(dt):
    import torch

    return torch.float64 if dt == "f64" else torch.float32


def signals(L, real, seed=0):
    return [R.signal(L, seed + i, not real) for i in range(BATCH)]


@functools.lru_cache(maxsize=None)
def reference(shape, family, norm, real, seed=0):
    """per signal of the batch, W (S, L) in complex long double"""
    L, P, S = shape
    return [R.cwt(x, R.case_scales(L, S), family, None, norm, P) for x in signals(L, real, seed)]


@functools.lru_cache(maxsize=None)
def planner(P, dt, shape, family, norm, real):
    L, Pn, S = shape
    return (P.PlannerCwt64 if dt == "f64" else P.PlannerCwt32)(L, R.case_scales(L, S), family, None, norm, Pn, real)


def needs_even_dist(pl):
    """the engine's batched power-of-two R2C reads (even, odd) pairs: a real planner with P = L = 2^k >= 4"""
    p = pl.pad_len
    return pl.real_input and p == pl.signal_len and p >= 4 and p & (p - 1) == 0


def batched(P, pl, xs, dt, sig_dist, out_dist, off=1, work=None, stream=None):
    """the signals `xs` through cwt_batched from planes sig_dist apart into planes out_dist apart, every plane `off` elements
    past a 16-byte boundary: per signal the complex (S, L) result; the inputs and what lies around and between the outputs are
    not written"""
    import torch

    b, L, S = len(xs), pl.signal_len, pl.num_scales
    n = S * L
    np_in = 1 if pl.real_input else 2
    ibuf = torch.full((np_in, off + (b - 1) * sig_dist + L + 4), 9.0, dtype=_tdt(dt), device="cuda")
    for i, x in enumerate(xs):
        x = np.asarray(x)
        ibuf[0, off + i * sig_dist:off + i * sig_dist + L] = torch.from_numpy(np.ascontiguousarray(x.real, dtype=NDT[dt]))
        if not pl.real_input:
            ibuf[1, off + i * sig_dist:off + i * sig_dist + L] = torch.from_numpy(np.ascontiguousarray(x.imag, dtype=NDT[dt]))
    keep = ibuf.clone()
    ins = tuple(torch.as_strided(ibuf[p, off:], (b, L), (sig_dist, 1)) if b > 1 else ibuf[p, off:off + L] for p in range(np_in))
    obuf = torch.full((2, off + (b - 1) * out_dist + n + 4), 9.0, dtype=_tdt(dt), device="cuda")
    outs = tuple(torch.as_strided(obuf[p, off:], (b, S, L), (out_dist, L, 1)) if b > 1 else obuf[p, off:off + n].reshape(S, L)
                 for p in range(2))
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    P.cwt_batched(ins[0] if pl.real_input else ins, pl, out=outs, work=work, stream=stream)
    torch.cuda.synchronize()
    assert torch.equal(ibuf, keep)
    got = obuf.cpu().numpy()
    mask = np.ones(got.shape[1], bool)
    for i in range(b):
        mask[off + i * out_dist:off + i * out_dist + n] = False
    assert (got[:, mask] == 9.0).all()
    return [(got[0, off + i * out_dist:off + i * out_dist + n] + 1j * got[1, off + i * out_dist:off + i * out_dist + n]).reshape(S, L)
            for i in range(b)]


def odd_dists(pl):
    """(sig_dist, out_dist) of the batched runs: odd, above the rows -- the signal distance even where the engine demands it"""
    sd = (pl.signal_len + 5) | 1
    return sd + (1 if needs_even_dist(pl) else 0), (pl.num_scales * pl.signal_len + 5) | 1


def measure(P, dt, shape, family, norm, real):
    """the worst use of (rel-L2, per-bin) gates over the rows and the signals of the batch; asserts the bits of batch 1 and of
    chunks of one row"""
    import torch

    L, Pn, S = shape
    pl = planner(P, dt, shape, family, norm, real)
    assert (pl.pad_len, pl.num_scales, pl.signal_len) == (Pn, S, L)
    xs, refs = signals(L, real), reference(shape, family, norm, real)
    sd, od = odd_dists(pl)
    got = batched(P, pl, xs, dt, sd, od)
    alone = batched(P, pl, xs[2:], dt, L, S * L, off=0)[0]
    assert np.array_equal(alone, got[2]), (shape, dt, family, norm, real)
    small = torch.full((pl.workspace_min() + 1,), float("nan"), dtype=_tdt(dt), device="cuda")
    chunked = batched(P, pl, xs, dt, sd, od, work=small[1:])
    assert all(np.array_equal(a, g) for a, g in zip(chunked, got)), (shape, dt, family, norm, real, "chunks of one row")
    lg = R.inner_log2(Pn)
    g_rel, g_bin = tol.gates(dt, lg)
    use = [0.0, 0.0]
    for i, (w, ref) in enumerate(zip(got, refs)):
        for j in range(S):
            want = ref[j]
            if not np.any(want):
                assert not np.any(w[j]), (shape, dt, family, i, j)   # an exact zero
                continue
            rel, worst = tol.check(f"cwt:{shape_id(shape)}:{family}:{norm}:{'r' if real else 'c'}:{i}:{j}", dt, lg, w[j].real, w[j].imag,
                                   want.real.astype(np.float64), want.imag.astype(np.float64))
            use = [max(use[0], rel / g_rel), max(use[1], worst / g_bin)]
    return use


@pytest.mark.parametrize("shape", R.SHAPES, ids=shape_id)
@pytest.mark.parametrize("norm", R.NORMS)
@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dt", DTS)
def test_parity(gpu, dt, kind, family, norm, shape):
    """every row against the long-double definition: batch 3 at odd distances one element off a 16-byte boundary, batch 1 and
    chunks of one row (a workspace of workspace_min()) to the same bits"""
    rel, worst = measure(gpu, dt, shape, family, norm, kind == "real")
    print(f"cwt {shape_id(shape)} {family} {norm} {kind} {dt}: rel-L2 {rel:.3f}, worst bin {worst:.3f} of the gates")


def test_the_engines_even_distance_is_inherited(gpu):
    """a real planner with P = L = 8 and batch 3 at an odd signal distance is refused before anything runs; P > L is not"""
    import torch

    P = gpu
    pl = planner(P, "f64", (8, 8, 3), "morlet", "l2", True)
    assert needs_even_dist(pl)
    x = torch.zeros(40, dtype=torch.float64, device="cuda")
    out = tuple(torch.zeros((3, 3, 8), dtype=torch.float64, device="cuda") for _ in range(2))
    with pytest.raises(P.PhastPanic) as e:
        P.cwt_batched(torch.as_strided(x, (3, 8), (9, 1)), pl, out=out)
    assert e.value.code == 16
    torch.cuda.synchronize()
    assert not bool(out[0].any()) and not bool(out[1].any())
    P.cwt_batched(torch.as_strided(x, (3, 8), (10, 1)), pl, out=out)
    padded = planner(P, "f64", (100, 128, 5), "morlet", "l2", True)
    assert not needs_even_dist(padded)


BIT_SHAPES = [(7, 7, 3), (8, 8, 3), (100, 131, 5), (300, 512, 17)]


@pytest.mark.parametrize("family", ["morlet", "dog"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dt", DTS)
def test_bit_identity(gpu, dt, kind, family):
    """the same signal returns the same bits alone and inside a batch, through buf[1:] and buf[3:] views, on a side stream, in a
    replayed graph on new data and through the host form"""
    import torch

    P, real = gpu, kind == "real"
    for shape in BIT_SHAPES:
        L, Pn, S = shape
        pl = planner(P, dt, shape, family, "l2", real)
        xs = signals(L, real, seed=11)
        alone = [batched(P, pl, [x], dt, L, S * L, off=0)[0] for x in xs]
        sd, od = odd_dists(pl)
        for off in (1, 3):
            got = batched(P, pl, xs, dt, sd + 2 * (off // 2), od + 2 * (off // 2), off=off)
            assert all(np.array_equal(a, g) for a, g in zip(alone, got)), (shape, off)
        side = torch.cuda.Stream()
        assert np.array_equal(batched(P, pl, [xs[1]], dt, L, S * L, off=1, stream=side)[0], alone[1]), (shape, "side stream")
        # graph replay on new data
        d_x = tuple(torch.zeros(L, dtype=_tdt(dt), device="cuda") for _ in range(1 if real else 2))
        out = torch.zeros((2, S, L), dtype=_tdt(dt), device="cuda")
        work = torch.empty(max(1, pl.workspace_len(1)), dtype=_tdt(dt), device="cuda")
        x_arg = d_x[0] if real else d_x
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):  # warm-up on the capture stream
            P.cwt_batched(x_arg, pl, out=(out[0], out[1]), work=work)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            P.cwt_batched(x_arg, pl, out=(out[0], out[1]), work=work)
        for i in (0, 2):
            d_x[0].copy_(torch.from_numpy(np.ascontiguousarray(np.asarray(xs[i]).real, dtype=NDT[dt])))
            if not real:
                d_x[1].copy_(torch.from_numpy(np.ascontiguousarray(xs[i].imag, dtype=NDT[dt])))
            out.zero_()
            g.replay()
            torch.cuda.synchronize()
            o = out.cpu().numpy()
            assert np.array_equal(o[0] + 1j * o[1], alone[i]), (shape, "graph", i)
        # the host form
        host = getattr(P, f"cwt_{dt[1:]}_with_planner")
        h_re, h_im = np.zeros(S * L, NDT[dt]), np.zeros(S * L, NDT[dt])
        x = np.asarray(xs[2])
        host(np.ascontiguousarray(x.real, dtype=NDT[dt]), h_re, h_im, pl, x_im=None if real else np.ascontiguousarray(x.imag, dtype=NDT[dt]))
        assert np.array_equal((h_re + 1j * h_im).reshape(S, L), alone[2]), (shape, "host")


# ---- the guarded arena ----
@pytest.mark.parametrize("shape", [(257, 257, 9), (100, 131, 5), (300, 512, 17)], ids=shape_id)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dt", DTS)
def test_arena(gpu, dt, kind, shape):
    """the _dev call in the poisoned (NaN), guarded arena, P = L and P > L: workspace lengths workspace_min() (one row), that
    plus 1, one in between and workspace_len(3) at three bases -- bands whole, inputs kept, the bits of a zero-filled
    workspace, one element below workspace_min() refused with nothing written; and an output declared one short is seen"""
    import torch

    from tests import test_gpu_workspace_guard as G

    P, real = gpu, kind == "real"
    L, Pn, S = shape
    pl = planner(P, dt, shape, "dog", "l2", real)
    xs, refs = signals(L, real), reference(shape, "dog", "l2", real)
    sd, od = odd_dists(pl)
    n = S * L

    def call(t, work):
        ins = tuple(torch.as_strided(t[k], (G.BATCH, L), (sd, 1)) for k in (("x",) if real else ("x", "xi")))
        outs = tuple(torch.as_strided(t[k], (G.BATCH, S, L), (od, L, 1)) for k in ("w", "wi"))
        P.cwt_batched(ins[0] if real else ins, pl, out=outs, work=work)

    def gate(got):
        for b in range(G.BATCH):
            w = (got["w"][b] + 1j * got["wi"][b]).reshape(S, L)
            for j in range(S):
                tol.check(f"guard:cwt:{shape_id(shape)}", dt, R.inner_log2(Pn), w[j].real, w[j].imag, refs[b][j].real.astype(np.float64),
                          refs[b][j].imag.astype(np.float64))

    planes = [G.Plane("x", "in", L, sd, [np.asarray(np.asarray(x).real, NDT[dt]) for x in xs])]
    if not real:
        planes.append(G.Plane("xi", "in", L, sd, [np.asarray(x.imag, NDT[dt]) for x in xs]))
    planes += [G.Plane("w", "out", n, od), G.Plane("wi", "out", n, od)]
    lo, hi = pl.workspace_min(), pl.workspace_len(G.BATCH)
    lengths = G._lengths(lo, (lo + hi) // 2 + 1, hi)
    m = 0 if Pn & (Pn - 1) == 0 else 1 << (2 * Pn - 2).bit_length()
    c = G.Case(f"cwt:{shape_id(shape)}:{kind}", dt, m, planes, lengths, call, gate)
    G.drive(P, c, gate_at=(lengths[0][0], 1))
    G.overrun(P, c, "w")


# ---- status codes ----
@pytest.mark.parametrize("dt", DTS)
def test_codes(gpu, dt):
    """a wrong length, null pointers, the wrong imaginary plane, short distances, identical pointers, a null or short workspace
    and illegal arguments come back with their codes and write nothing; describe names the family, P and the chunking; the
    stage timers leave the result behind"""
    import torch

    from phastft_amd import _lib

    P, n_ = gpu, C.c_size_t
    lib = _lib.lib()
    shape = L, Pn, S = (100, 131, 5)
    pr, pc = planner(P, dt, shape, "paul", "peak", True), planner(P, dt, shape, "paul", "peak", False)
    big = torch.zeros(8192 + pc.workspace_len(2), dtype=_tdt(dt), device="cuda")
    at = lambda off: C.c_void_p(big.data_ptr() + off * big.element_size())  # noqa: E731
    pxr, pxi, pre, pim, pw = at(0), at(300), at(1000), at(3000), at(5000)
    dev = getattr(lib, f"phast_cwt_{dt[1:]}_dev")
    n = S * L
    for pl, xi in ((pr, None), (pc, pxi)):
        size = n_(pl.workspace_len(1))
        ok = (n_(L), n_(1), n_(L), n_(n), pl._h, pw, size, None)
        assert dev(None, xi, pre, pim, *ok) == 16
        assert dev(pxr, xi, None, pim, *ok) == 16
        assert dev(pxr, xi, pre, None, *ok) == 16
        assert dev(pxr, pxi if xi is None else None, pre, pim, *ok) == 16                          # the wrong planes
        assert dev(pxr, xi, pre, pim, n_(L - 1), n_(1), n_(L), n_(n), pl._h, pw, size, None) == 3   # PHAST_ERR_PLANNER_SIZE
        assert dev(pxr, xi, pre, pim, n_(L), n_(2), n_(L - 1), n_(n), pl._h, pw, size, None) == 16  # sig_dist below the signal
        assert dev(pxr, xi, pre, pim, n_(L), n_(2), n_(L), n_(n - 1), pl._h, pw, size, None) == 16  # out_dist below the rows
        assert dev(pxr, xi, pxr, pim, *ok) == 16                                                   # output on the input
        assert dev(pxr, xi, pre, pre, *ok) == 16                                                   # one output plane
        assert dev(pxr, xi, pre, pim, n_(L), n_(1), n_(L), n_(n), pl._h, None, size, None) == 16    # no workspace
        assert dev(pxr, xi, pre, pim, n_(L), n_(1), n_(L), n_(n), pl._h, pw, n_(pl.workspace_min() - 1), None) == 16
        assert dev(pxr, xi, pre, pim, n_(L), n_(0), n_(L), n_(n), pl._h, None, n_(0), None) == 0    # an empty batch
    assert dev(pxr, pxr, pre, pim, n_(L), n_(1), n_(L), n_(n), pc._h, pw, n_(pc.workspace_len(1)), None) == 16   # one input plane
    torch.cuda.synchronize()
    assert not bool(big.any())  # none of the refused calls ran
    cls = P.PlannerCwt64 if dt == "f64" else P.PlannerCwt32
    for bad in ((0, [1.0]), (8, []), (8, [1.0, 0.0]), (8, [-1.0]), (8, [float("nan")]), (8, [float("inf")]),
                (8, [1.0], "morlet", 0.0), (8, [1.0], "paul", 2.5), (8, [1.0], "paul", 86), (8, [1.0], "dog", 0), (8, [1.0], "dog", 171),
                (8, [1.0], "morlet", None, "l2", 7), (8, [1.0], "morlet", None, "l2", (1 << 29) + 1)):
        with pytest.raises(P.PhastPanic) as e:
            cls(*bad)
        assert e.value.code == 16, bad
    host = getattr(P, f"cwt_{dt[1:]}_with_planner")
    z = lambda k: np.zeros(k, NDT[dt])  # noqa: E731
    with pytest.raises(P.PhastPanic) as e:
        host(z(L - 1), z(n), z(n), pr)
    assert e.value.code == 3
    with pytest.raises(P.PhastPanic) as e:
        host(z(L), z(n - 1), z(n - 1), pr)
    assert e.value.code == 2  # PHAST_ERR_LEN_MISMATCH
    with pytest.raises(P.PhastPanic) as e:
        host(z(L), z(n), z(n), pr, x_im=z(L))
    assert e.value.code == 16
    d = pr.describe()
    assert d.startswith(f"cwt paul(m=4) peak real L={L} P={Pn} S={S}: bank tile={pr.tile_bins} bins x {pr.scale_group} scales (no LDS), "
                        f"rows in the workspace, cropped, chunks of whole rows ({S} per signal; one row at workspace_min={pr.workspace_min()}")
    assert "forward real any N=131" in d and "inverse any N=131" in d
    assert "complex" in pc.describe() and "forward any N=131" in pc.describe()
    whole = planner(P, dt, (8, 8, 3), "morlet", "l2", True)
    assert "cwt morlet(w0=6" in whole.describe() and " l2 real L=8 P=8 S=3" in whole.describe() and "rows in the output planes" in whole.describe()
    assert "cwt step real" in planner(P, dt, (8, 8, 3), "step", "l2", True).describe()
    assert (pr.tile_bins, pr.scale_group) == (256 * (2 if dt == "f64" else 4), 8)
    assert pr.device_bytes() >= 2 * S * 8
    # a power-of-two P = L works in the spectra alone: 2 planes of P / 2 + 1 (real) or P (complex) bins, rounded up to 16 bytes
    v = 2 if dt == "f64" else 4
    for real, bins in ((True, 5), (False, 8)):
        p8 = planner(P, dt, (8, 8, 3), "morlet", "l2", real)
        xd = -(-bins // v) * v
        assert p8.workspace_min() == 2 * xd + v - 1 and p8.workspace_len(3) == 3 * 2 * xd + v - 1
    for pl, real in ((pr, True), (pc, False)):
        x = signals(L, real, seed=5)[0]
        want = batched(P, pl, [x], dt, L, n, off=0)[0]
        d_re = torch.from_numpy(np.ascontiguousarray(np.asarray(x).real, dtype=NDT[dt])).cuda()
        d_im = None if real else torch.from_numpy(np.ascontiguousarray(x.imag, dtype=NDT[dt])).cuda()
        out = torch.zeros((2, n), dtype=_tdt(dt), device="cuda")
        st = pl.time_stages(d_re, d_im, out[0], out[1], 1, reps=1)
        assert len(st) == 4 and all(v >= 0 for v in st)
        o = out.cpu().numpy()
        assert np.array_equal((o[0] + 1j * o[1]).reshape(S, L), want)


# ---- the conveniences ----
@pytest.mark.parametrize("L", [7, 8, 1000])
@pytest.mark.parametrize("dt", DTS)
def test_hilbert_against_scipy(gpu, dt, L):
    """hilbert(x) against scipy.signal.hilbert in double on the same T-exact signal, through the gates of the type at the inner
    log2 of L; a padded length and a complex signal too"""
    import torch

    P = gpu
    x = R.signal(L, 21)
    got = P.hilbert(torch.from_numpy(x.astype(NDT[dt])).cuda()).cpu().numpy()
    assert got.shape == (L,) and got.dtype == (np.complex128 if dt == "f64" else np.complex64)
    tol.check_c(f"hilbert:{L}", dt, R.inner_log2(L), got, scipy.signal.hilbert(x))
    pad = L + 5
    got = P.hilbert(torch.from_numpy(x.astype(NDT[dt])).cuda(), pad_len=pad).cpu().numpy()
    tol.check_c(f"hilbert:{L}:{pad}", dt, R.inner_log2(pad), got, scipy.signal.hilbert(x, N=pad)[:L])
    z = R.signal(L, 22, True)
    got = P.hilbert(torch.from_numpy(z.astype(np.complex128 if dt == "f64" else np.complex64)).cuda()).cpu().numpy()
    want = scipy.signal.hilbert(z.real) + 1j * scipy.signal.hilbert(z.imag)   # the filter is linear
    tol.check_c(f"hilbert:c:{L}", dt, R.inner_log2(L), got, want)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dt", DTS)
def test_cwt_convenience_is_the_planner_call(gpu, dt, kind):
    """cwt on tensors of shape (3, L) and (2, 3, L): the bits of cwt_batched through a planner of the same arguments"""
    import torch

    P, real = gpu, kind == "real"
    L, pad = 100, 131
    sc = P.cwt_scales(L)[:6]
    xs = np.array(signals(L, real, seed=31))
    ct = (np.float64 if real else np.complex128) if dt == "f64" else (np.float32 if real else np.complex64)
    d = torch.from_numpy(np.ascontiguousarray(xs.astype(ct))).cuda()
    for wavelet, param, norm in (("morlet", None, "l2"), ("paul", 3, "peak"), ("dog", 1, "l2")):
        got = P.cwt(d, sc, wavelet, param, norm, pad)
        assert tuple(got.shape) == (3, len(sc), L) and got.dtype == (torch.complex128 if dt == "f64" else torch.complex64)
        pl = (P.PlannerCwt64 if dt == "f64" else P.PlannerCwt32)(L, sc, wavelet, param, norm, pad, real)
        want = P.cwt_batched(d, pl)
        torch.cuda.synchronize()
        assert torch.equal(got, want), (wavelet, dt, kind)
        again = P.cwt(torch.stack((d, d)), sc, wavelet, param, norm, pad)
        assert tuple(again.shape) == (2, 3, len(sc), L) and torch.equal(again[1], want)
    assert tuple(P.cwt(d[:0], sc).shape) == (0, len(sc), L)
    with pytest.raises(TypeError):
        P.cwt(d.cpu(), sc)


# ---- the budget ----
def test_gates_keep_their_margin():
    """every gate sits >= 2 x over its worst use measured on the MI355X, and no case is missing"""
    budget = json.load(open(BUDGET))
    have = {(e["dt"], e["kind"], e["family"], e["norm"], e["shape"]) for e in budget["entries"]}
    want = {(dt, kind, f, n, shape_id(s)) for dt in DTS for kind in KINDS for f in R.FAMILIES for n in R.NORMS for s in R.SHAPES}
    assert have == want and len(budget["entries"]) == len(have)
    for e in budget["entries"]:
        assert 0 <= e["use"] <= 0.5, e
