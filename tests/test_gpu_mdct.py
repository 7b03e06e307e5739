"""The MDCT and its inverse on the MI355X (csrc/mdct.hip, csrc/planner_mdct.hpp) against tests/mdct_reference.py in long
double: reference (b), fold and unfold around scipy's DCT-IV, and the O(N^2) definition (a) as well up to N = 64.

Gates (mdct_reference.mdct_gates): tests/tolerances.py's formulas on log2 of the length the inner complex transform of N / 2
points runs at (its Bluestein length where N / 2 is no power of two), times the any-length factor 2 of the DCT and STFT gates:
a frame is one complex transform between two twiddle sweeps.  The forward result is gated as rel-L2 and worst coefficient over
all frames, the inverse as rel-L2 and worst sample over the signal.  The round trip through a window that reconstructs
perfectly is held to tolerances.ROUNDTRIP_ABS on inputs in [-1, 1).  The measured worst over seeds 0-3 is in
tests/golden/mdct_error_budget.json (tests/golden/make_mdct_error_budget.py)."""
import functools
import json
import os

import numpy as np
import pytest

from tests import mdct_reference as R
from tests import tolerances as tol

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = [(n, ln) for n in (2, 4, 6, 30) for ln in (1, n + 1, 3 * n + 5)]
LARGE = [(960, 48_000), (1024, 1 << 20), (2050, 10_000), (1 << 16, 5 * (1 << 16) + 7)]
SHAPES = SMALL + LARGE
IDS = lambda s: "x".join(map(str, s))  # noqa: E731
WINDOWS = ("sine", "vorbis", "kbd")


def framings(n, length):
    return [True, False] if length >= 2 * n else [True]


def _ndt(dt):
    return np.float64 if dt == "f64" else np.float32


def _tdt(dt):
    import torch

    return torch.float64 if dt == "f64" else torch.float32


@functools.lru_cache(maxsize=None)
def _signal(length: int, dt: str, seed: int = 0):
    x = np.random.default_rng([seed, length, 24]).uniform(-1, 1, length).astype(_ndt(dt))
    x.flags.writeable = False
    return x


@functools.lru_cache(maxsize=None)
def _window(n: int, dt: str, name: str = "uniform"):
    if name == "uniform":
        w = np.random.default_rng([n, 25]).uniform(-1, 1, 2 * n).astype(_ndt(dt))
    else:
        w = R.window(name, n).astype(_ndt(dt))
    w.flags.writeable = False
    return w


@functools.lru_cache(maxsize=None)
def reference(dt, n, length, padded, seed=0):
    """(window, long-double coefficients, their rounding to dt, the reference inverse of the rounded ones), computed once"""
    x, w = _signal(length, dt, seed), _window(n, dt)
    X = R.mdct_fast(x, n, w, padded)
    Xr = np.ascontiguousarray(X, _ndt(dt)).reshape(-1)
    back = R.imdct_fast(Xr.reshape(X.shape), length, n, w, padded)
    for v in (X, Xr, back):
        v.flags.writeable = False
    return w, X, Xr, back


def planner(P, dt, length, n, w, padded):
    return (P.PlannerMdct64 if dt == "f64" else P.PlannerMdct32)(length, n, window=w, padded=padded)


def forward(P, pl, x, workspace=None, offset=0):
    import torch

    d_x = torch.full((x.size + offset,), 7.0, dtype=_tdt(P_dt(pl)), device="cuda")
    d_x[offset:] = torch.from_numpy(np.array(x))
    pts = pl.frames * pl.n
    out = torch.full((offset + pts + 3,), 7.0, dtype=d_x.dtype, device="cuda")
    P.mdct_batched(d_x[offset:], out[offset:], pl, 1, workspace=workspace)
    assert np.array_equal(d_x[offset:].cpu().numpy(), x)  # the signal is never written
    out = out.cpu().numpy()
    assert (out[:offset] == 7.0).all() and (out[offset + pts:] == 7.0).all()
    return out[offset:offset + pts]


def inverse(P, pl, coefs, workspace=None, offset=0):
    import torch

    d_c = torch.full((coefs.size + offset,), 7.0, dtype=_tdt(P_dt(pl)), device="cuda")
    d_c[offset:] = torch.from_numpy(np.array(coefs))
    out = torch.full((offset + pl.signal_len + 3,), 7.0, dtype=d_c.dtype, device="cuda")
    P.imdct_batched(d_c[offset:], out[offset:], pl, 1, workspace=workspace)
    assert np.array_equal(d_c[offset:].cpu().numpy(), coefs)  # the coefficients are never written
    out = out.cpu().numpy()
    assert (out[:offset] == 7.0).all() and (out[offset + pl.signal_len:] == 7.0).all()
    return out[offset:offset + pl.signal_len]


def P_dt(pl):
    return "f64" if pl._dtype == np.float64 else "f32"


def check(tag, dt, n, got, want):
    rel, worst = R.errors(got, want)
    g_rel, g_bin = R.mdct_gates(dt, n)
    tol.record(tag, R.inner_log2(n), rel, worst, g_rel, g_bin)
    print(f"{tag} {dt}: rel {rel:.3e} / {g_rel:.3e}, worst {worst:.3e} / {g_bin:.3e}")
    assert rel <= g_rel and worst <= g_bin, (tag, dt, rel, g_rel, worst, g_bin)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_forward_and_inverse_parity(gpu, dt, shape):
    """random uniform windows (analysis only: nothing reconstructs), both framings"""
    n, length = shape
    for padded in framings(n, length):
        w, X, Xr, back = reference(dt, n, length, padded)
        pl = planner(gpu, dt, length, n, w, padded)
        assert pl.frames == X.shape[0] == R.frames_of(length, n, padded)
        assert abs(pl.tdac_defect - R.tdac_defect(w, n)) <= 1e-15
        x = _signal(length, dt)
        got = forward(gpu, pl, x)
        check(f"mdct:{shape}:{int(padded)}", dt, n, got, X)
        got_back = inverse(gpu, pl, Xr)
        check(f"imdct:{shape}:{int(padded)}", dt, n, got_back, back)
        if n <= 64:  # the definition itself
            check(f"mdct-def:{shape}:{int(padded)}", dt, n, got, R.mdct_direct(x, n, w, padded))
            check(f"imdct-def:{shape}:{int(padded)}", dt, n, got_back, R.imdct_direct(Xr.reshape(X.shape), length, n, w, padded))


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_round_trip(gpu, dt, shape):
    """imdct(mdct(x)) = x on [0, L) (padded) or [N, F N) (unpadded) with the three windows; outside that, the one-frame
    term or 0, which the parity test holds against the reference"""
    n, length = shape
    x = _signal(length, dt, seed=5)
    for name in WINDOWS:
        w = _window(n, dt, name)
        for padded in framings(n, length):
            pl = planner(gpu, dt, length, n, w, padded)
            assert pl.tdac_defect <= (1e-15 if dt == "f64" else 2.5e-7), (name, pl.tdac_defect)  # f32: the rounded window's
            back = inverse(gpu, pl, forward(gpu, pl, x))
            lo, hi = (0, length) if padded else (n, pl.frames * n)
            err = float(np.abs(back[lo:hi].astype(np.float64) - x[lo:hi]).max())
            print(f"round:{shape}:{name}:{int(padded)} {dt}: {err:.3e} / {tol.ROUNDTRIP_ABS[dt]:.1e}")
            assert err <= tol.ROUNDTRIP_ABS[dt], (name, padded, err)
            if not padded:
                assert (back[pl.frames * n + n:] == 0).all()  # no frame holds the tail


def test_default_window_and_convenience_pair(gpu):
    import torch

    n, length = 30, 95
    for dt in ("f64", "f32"):
        x = _signal(length, dt, seed=6)
        pl = planner(gpu, dt, length, n, None, True)
        assert pl.tdac_defect < 1e-15
        assert np.array_equal(forward(gpu, pl, x), forward(gpu, planner(gpu, dt, length, n, _window(n, dt, "sine"), True), x))
        d_x = torch.from_numpy(np.array(x)).cuda()
        X = gpu.mdct(d_x, n)
        named = planner(gpu, dt, length, n, gpu.mdct_window("sine", n, _ndt(dt)), True)
        assert X.shape == (pl.frames, n) and np.array_equal(X.cpu().numpy().reshape(-1), forward(gpu, named, x))
        back = gpu.imdct(X, length)
        assert float((back - d_x).abs().max()) <= tol.ROUNDTRIP_ABS[dt]
        Xk = gpu.mdct(d_x, n, window="kbd", padded=False)
        assert Xk.shape == (length // n - 1, n)
        with pytest.raises(ValueError):
            gpu.imdct(X, length + n)  # another frame count


def _guard():
    from tests import test_gpu_workspace_guard as G

    return G


def mdct_case(P, dt, shape, inv):
    """a batch of 3 at sig_dist = L + 5 for tests/test_gpu_workspace_guard.py's drive()"""
    G = _guard()
    n, length = shape
    refs = [reference(dt, n, length, True, seed=20 + b) for b in range(G.BATCH)]
    pl = planner(P, dt, length, n, refs[0][0], True)
    h = n // 2
    m = 0 if h & (h - 1) == 0 else 1 << R.inner_log2(n)
    pts, dist, vec = pl.frames * n, length + 5, G._vec(dt)
    per = pl.workspace_min() - (vec - 1)
    assert pl.workspace_len(G.BATCH) == G.BATCH * pl.frames * per + vec - 1 and pl.workspace_min(True) == pl.frames * per + vec - 1
    assert per == 2 * (-(-h // vec) * vec) + -(-n // vec) * vec + 2 * m
    if not inv:
        xs = [_signal(length, dt, seed=20 + b) for b in range(G.BATCH)]

        def call(t, work):
            P.mdct_batched(t["x"], t["X"], pl, G.BATCH, sig_dist=dist, workspace=work)

        def gate(got):
            for b in range(G.BATCH):
                check(f"guard:mdct:{shape}", dt, n, got["X"][b], refs[b][1])

        planes = [G.Plane("x", "in", length, dist, xs), G.Plane("X", "out", pts, pts)]
        return G.Case(f"mdct:{shape}", dt, m, planes, G._lengths(pl.workspace_min(), 2 * per + vec, pl.workspace_len(G.BATCH)),
                      call, gate)

    def call(t, work):
        P.imdct_batched(t["X"], t["x"], pl, G.BATCH, sig_dist=dist, workspace=work)

    def gate(got):
        for b in range(G.BATCH):
            check(f"guard:imdct:{shape}", dt, n, got["x"][b], refs[b][3])

    planes = [G.Plane("X", "in", pts, pts, [r[2] for r in refs]), G.Plane("x", "out", length, dist)]
    return G.Case(f"imdct:{shape}", dt, m, planes,
                  G._lengths(pl.workspace_min(True), 2 * pl.frames * per + vec, pl.workspace_len(G.BATCH)), call, gate)


@pytest.mark.parametrize("inv", [False, True], ids=["mdct", "imdct"])
@pytest.mark.parametrize("shape", [(6, 23), (30, 95), (64, 300), (2050, 10_000)], ids=IDS)
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_workspace_contract(gpu, dt, shape, inv):
    """batch 3 at a signal distance above L in a guarded arena with a NaN-poisoned workspace, at workspace_min (forward: one
    frame per chunk, gated), one more, chunks of two, workspace_len(batch), each on three bases: bands intact, inputs
    unmodified, the bits of a zero-filled workspace, the gaps untouched; one element below the minimum is code 16 with nothing
    written"""
    G = _guard()
    G.drive(gpu, mdct_case(gpu, dt, shape, inv))
    G.overrun(gpu, mdct_case(gpu, dt, shape, inv), "x" if inv else "X")


@pytest.mark.parametrize("shape", [(30, 95), (960, 5000), (1024, 5000)], ids=IDS)
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_same_bits_unaligned_graph_and_host(gpu, dt, shape):
    """pointers one element off a 16-byte boundary, a replay of the call captured in a graph, and the host-slice form all
    give the bits of the aligned direct device call"""
    import torch

    n, length = shape
    w = _window(n, dt)
    pl = planner(gpu, dt, length, n, w, True)
    x = _signal(length, dt, seed=7)
    X = forward(gpu, pl, x)
    back = inverse(gpu, pl, X)
    assert np.array_equal(forward(gpu, pl, x, offset=1), X) and np.array_equal(inverse(gpu, pl, X, offset=1), back)
    hX, hb = np.zeros(X.size, _ndt(dt)), np.zeros(length, _ndt(dt))
    getattr(gpu, f"mdct_{dt}_with_planner")(np.array(x), hX, pl)
    getattr(gpu, f"imdct_{dt}_with_planner")(hX, hb, pl)
    assert np.array_equal(hX, X) and np.array_equal(hb, back)
    with pytest.raises(gpu.PhastPanic) as e:
        getattr(gpu, f"mdct_{dt}_with_planner")(np.array(x[:-1]), hX, pl)
    assert e.value.code == 3  # PHAST_ERR_PLANNER_SIZE
    with pytest.raises(gpu.PhastPanic) as e:
        getattr(gpu, f"imdct_{dt}_with_planner")(hX[:-1].copy(), hb, pl)
    assert e.value.code == 2  # PHAST_ERR_LEN_MISMATCH
    assert f"mdct L={length} N={n}" in pl.describe() and pl.device_bytes() >= (2 * n + 2 * n) * np.dtype(_ndt(dt)).itemsize
    d_x = torch.from_numpy(np.array(x)).cuda()
    d_X = torch.zeros(X.size, dtype=_tdt(dt), device="cuda")
    d_b = torch.zeros(length, dtype=_tdt(dt), device="cuda")
    work = torch.empty(pl.workspace_len(1), dtype=_tdt(dt), device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on the capture stream
        gpu.mdct_batched(d_x, d_X, pl, 1, workspace=work)
        gpu.imdct_batched(d_X, d_b, pl, 1, workspace=work)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        gpu.mdct_batched(d_x, d_X, pl, 1, workspace=work)
        gpu.imdct_batched(d_X, d_b, pl, 1, workspace=work)
    d_X.zero_()
    d_b.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(d_X.cpu().numpy(), X) and np.array_equal(d_b.cpu().numpy(), back)


def test_gates_keep_their_margin():
    """the gates above sit >= 3 x over the worst error measured on the MI355X over seeds 0-3, as the DCT suite demands"""
    budget = json.load(open(os.path.join(ROOT, "tests", "golden", "mdct_error_budget.json")))
    assert budget["entries"]
    for e in budget["entries"]:
        g_rel, g_bin = R.mdct_gates(e["dt"], e["n"])
        assert g_rel >= 3 * e["rel"] and g_bin >= 3 * e["bin"], e
