"""Welch spectral estimation on the MI355X (csrc/psd.hip, csrc/planner_psd.hpp) against tests/psd_reference.py in long double
(which tests/test_psd_cpu.py holds against scipy.signal.welch, csd and spectrogram).

Gate: 4 x tolerances.rel_gate(dt, log2 M), twice the STFT's: a squared magnitude doubles a relative error and the sums,
carried in double, add none.  M is the inner length of the real transform of F: its Bluestein length, or the packed length
F / 2 of a power of two.  The error is |got - ref|_2 / |ref|_2; for the cross planes it is taken over |sqrt(P_xx P_yy)|_2,
because incoherent signals average towards 0.  A reference that is exactly zero (P = 1, detrended) is compared absolutely.
The measured worst over seeds 0-3 is in tests/golden/psd_error_budget.json (tests/golden/make_psd_error_budget.py)."""
import functools

import numpy as np
import pytest

from tests import psd_reference as R
from tests import tolerances as tol
from tests.test_gpu_any_real import inner_m

pytestmark = pytest.mark.gpu

SHAPES = R.SHAPES + R.slab_shapes()
IDS = lambda s: "x".join(map(str, s))  # noqa: E731
CONFIGS = [(det, sc, win) for det in (True, False) for sc in ("density", "spectrum") for win in ("hann", "random")]
FS = 2.5
BIT_SHAPES = [(1000, 100, 63, 128), (4096, 8, 1, 8)]


def psd_log2m(f: int) -> int:
    m = max(f // 2, 1) if f & (f - 1) == 0 else inner_m(f)
    return m.bit_length() - 1


def psd_gate(dt: str, f: int) -> float:
    return 4.0 * tol.rel_gate(dt, psd_log2m(f))


def _ndt(dt):
    return np.float64 if dt == "f64" else np.float32


def _tdt(dt):
    import torch

    return torch.float64 if dt == "f64" else torch.float32


@functools.lru_cache(maxsize=None)
def _signal(length: int, dt: str, seed: int = 0, offset: float = 0.0):
    x = (np.random.default_rng([seed, length, 25]).uniform(-1, 1, length) + offset).astype(_ndt(dt))
    x.flags.writeable = False
    return x


@functools.lru_cache(maxsize=None)
def reference(dt, shape, det, sc, win, seed=0, average=True, offset=0.0):
    """(P_xy, P_xx, P_yy) in long double of the signals of seeds `seed` and `seed + 100`, computed once"""
    length, p, h, f = shape
    out = R.psd(_signal(length, dt, seed, offset), p, h, f, R.window_of(win, p), det, sc, FS, y=_signal(length, dt, seed + 100, offset),
                average=average)
    for v in out:
        v.flags.writeable = False
    return out


def planner(P, dt, shape, det=True, sc="density", win="hann"):
    length, p, h, f = shape
    pl = (P.PlannerPsd64 if dt == "f64" else P.PlannerPsd32)(length, p, h, f, R.window_of(win, p), "constant" if det else "none", sc, FS)
    assert pl.segments == R.segments(length, p, h) and pl.bins == f // 2 + 1
    assert pl.slab == max(R.MIN_SLAB, pl.segments * pl.bins >> 19)
    return pl


def dev(x, dt, lead=0):
    """a device copy of x behind `lead` elements (lead = 1: an element-aligned view)"""
    import torch

    t = torch.full((lead + x.size,), 7.0, dtype=_tdt(dt), device="cuda")
    t[lead:] = torch.from_numpy(np.array(x))
    return t[lead:]


def run_auto(P, pl, dt, x, average=True, workspace=None, lead=0):
    import torch

    pts = pl.bins * (1 if average else pl.segments)
    d_x = dev(x, dt, lead)
    out = torch.full((lead + pts + 3,), 7.0, dtype=_tdt(dt), device="cuda")
    P.psd_batched(d_x, out[lead:lead + pts], pl, 1, average=average, workspace=workspace)
    assert np.array_equal(d_x.cpu().numpy(), x)  # the signal is never written
    out = out.cpu().numpy()
    assert (out[:lead] == 7.0).all() and (out[lead + pts:] == 7.0).all()
    return out[lead:lead + pts]


def run_cross(P, pl, dt, x, y, average=True, workspace=None, lead=0, autos=True):
    import torch

    pts = pl.bins * (1 if average else pl.segments)
    d_x, d_y = dev(x, dt, lead), dev(y, dt, lead)
    outs = [torch.full((lead + pts + 3,), 7.0, dtype=_tdt(dt), device="cuda") for _ in range(4 if autos else 2)]
    views = [o[lead:lead + pts] for o in outs]
    P.csd_batched(d_x, d_y, views[0], views[1], pl, 1, *views[2:], average=average, workspace=workspace)
    assert np.array_equal(d_x.cpu().numpy(), x) and np.array_equal(d_y.cpu().numpy(), y)
    res = []
    for o in outs:
        o = o.cpu().numpy()
        assert (o[:lead] == 7.0).all() and (o[lead + pts:] == 7.0).all()
        res.append(o[lead:lead + pts])
    return res


def _norm(v):
    return float(np.sqrt(np.sum(np.abs(np.asarray(v, np.complex128)) ** 2)))


def check(tag, dt, f, got, want, den=None):
    """|got - want|_2 over `den` (default |want|_2) against the gate; a zero denominator: got must be exactly zero"""
    want = np.asarray(want).reshape(-1)
    den = _norm(want) if den is None else den
    gate = psd_gate(dt, f)
    if den == 0:
        assert not np.any(got), (tag, dt)
        return 0.0
    err = _norm(np.asarray(got, np.complex128) - want.astype(np.complex128)) / den
    tol.record(tag, psd_log2m(f), err, 0.0, gate, 0.0)
    print(f"{tag} {dt}: rel {err:.3e} / {gate:.3e}")
    assert err <= gate, (tag, dt, err, gate)
    return err


def check_all(tag, dt, shape, cfg, P, pl, seed=0, offset=0.0, **kw):
    """auto, cross with P_xx and P_yy returned, and average = False of one configuration"""
    length, p, h, f = shape
    x, y = _signal(length, dt, seed, offset), _signal(length, dt, seed + 100, offset)
    errs = []
    for average in (True, False):
        pxy, pxx, pyy = reference(dt, shape, *cfg, seed=seed, average=average, offset=offset)
        errs.append(check(f"psd:{tag}:avg{int(average)}", dt, f, run_auto(P, pl, dt, x, average, **kw), pxx))
        if average or length <= 1000:
            re, im, gxx, gyy = run_cross(P, pl, dt, x, y, average, **kw)
            den = _norm(np.sqrt((pxx * pyy).astype(np.float64)))
            errs.append(check(f"csd:{tag}:avg{int(average)}", dt, f, re.astype(np.float64) + 1j * im, pxy, den))
            errs.append(check(f"csd-xx:{tag}:avg{int(average)}", dt, f, gxx, pxx))
            errs.append(check(f"csd-yy:{tag}:avg{int(average)}", dt, f, gyy, pyy))
    return max(errs)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_parity(gpu, dt, shape):
    """both detrends, both scalings, fs = 2.5, a random window in [0.1, 1) and Hann"""
    for cfg in CONFIGS:
        check_all(f"{shape}:{cfg}", dt, shape, cfg, gpu, planner(gpu, dt, shape, *cfg))


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_offset_signal(gpu, dt):
    """x = uniform(-1, 1) + 1000, P = 256, H = 128, Hann: on the CPU the f32 estimate is wrong by 5.5e-8 with the segment mean in
    double and by 1.1e-5 with the mean in float, so a mean kept in T fails the gate (4.2e-6)"""
    shape = (8192, 256, 128, 256)
    assert dt == "f64" or abs(psd_gate(dt, 256) - 4.2e-6) < 1e-12
    check_all("offset", dt, shape, (True, "density", "hann"), gpu, planner(gpu, dt, shape), seed=3, offset=1000.0)


def _batch_case(gpu, dt, shape, cross, lead=0):
    """three signals at sig_dist = L + 5 and the planner; returns a function (workspace) -> list of output arrays"""
    import torch

    length = shape[0]
    pl = planner(gpu, dt, shape, True, "density", "random")
    dist, nb = length + 5, pl.bins
    xs = [_signal(length, dt, 50 + b) for b in range(3)]
    ys = [_signal(length, dt, 60 + b) for b in range(3)]

    def pack(vs):
        t = torch.full((lead + 2 * dist + length,), 7.0, dtype=_tdt(dt), device="cuda")
        for b, v in enumerate(vs):
            t[lead + b * dist:lead + b * dist + length] = torch.from_numpy(np.array(v))
        return t[lead:]

    d_x, d_y = pack(xs), pack(ys)

    def call(workspace=None):
        outs = [torch.full((lead + 3 * nb,), 7.0, dtype=_tdt(dt), device="cuda")[lead:] for _ in range(4 if cross else 1)]
        if cross:
            gpu.csd_batched(d_x, d_y, outs[0], outs[1], pl, 3, outs[2], outs[3], sig_dist=dist, workspace=workspace)
        else:
            gpu.psd_batched(d_x, outs[0], pl, 3, sig_dist=dist, workspace=workspace)
        return [o.cpu().numpy() for o in outs]

    return pl, xs, ys, call


@pytest.mark.parametrize("cross", [False, True], ids=["auto", "cross"])
@pytest.mark.parametrize("shape", BIT_SHAPES, ids=IDS)
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_bits_do_not_depend_on_batch_or_workspace(gpu, dt, shape, cross):
    import torch

    pl, xs, ys, call = _batch_case(gpu, dt, shape, cross)
    nb = pl.bins
    whole = call()
    for b in range(3):
        single = run_cross(gpu, pl, dt, xs[b], ys[b]) if cross else [run_auto(gpu, pl, dt, xs[b])]
        for got, want in zip(whole, single):
            assert np.array_equal(got[b * nb:(b + 1) * nb], want), (b,)
    lens = {pl.workspace_min(cross), pl.workspace_min(cross) + 1, 2 * pl.workspace_min(cross) + 3, pl.workspace_len(2, cross),
            pl.workspace_len(3, cross) - 1}
    for n in sorted(lens):
        small = call(torch.full((n,), float("nan"), dtype=_tdt(dt), device="cuda"))
        for got, want in zip(small, whole):
            assert np.array_equal(got, want), (n,)
    with pytest.raises(gpu.PhastPanic):
        call(torch.empty(pl.workspace_min(cross) - 1, dtype=_tdt(dt), device="cuda"))


@pytest.mark.parametrize("shape", BIT_SHAPES, ids=IDS)
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_bits_on_a_side_stream_and_in_a_graph_replay(gpu, dt, shape):
    import torch

    length = shape[0]
    pl = planner(gpu, dt, shape)
    d_x = dev(_signal(length, dt, 70), dt)
    out = torch.zeros(pl.bins, dtype=_tdt(dt), device="cuda")
    work = torch.empty(pl.workspace_len(1), dtype=_tdt(dt), device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        gpu.psd_batched(d_x, out, pl, 1, workspace=work)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), run_auto(gpu, pl, dt, _signal(length, dt, 70)))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        gpu.psd_batched(d_x, out, pl, 1, workspace=work)
    for seed in (71, 72):
        x = _signal(length, dt, seed)
        want = run_auto(gpu, pl, dt, x)
        d_x.copy_(torch.from_numpy(np.array(x)))
        out.zero_()
        work.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), want), seed


@pytest.mark.parametrize("cross", [False, True], ids=["auto", "cross"])
@pytest.mark.parametrize("shape", [(1000, 100, 63, 128), (1000, 30, 23, 30), (4096, 8, 1, 8)], ids=IDS)
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_guarded_workspace(gpu, dt, shape, cross):
    """batch 3 in a guarded arena with a NaN-poisoned workspace at workspace_min(): bands intact, inputs untouched, no NaN in
    the output, and the bits of a call in a full workspace"""
    from tests.arena import Arena, Region

    length, p, h, f = shape
    pl, xs, ys, call = _batch_case(gpu, dt, shape, cross)
    want = call()
    dist, nb = length + 5, pl.bins
    pack = lambda vs: np.concatenate([np.concatenate([v, np.full(5, 3.0, _ndt(dt))]) for v in vs])[:2 * dist + length]  # noqa: E731
    names = ["re", "im", "pxx", "pyy"] if cross else ["out"]
    for off in (0, 1):
        regions = [Region("x", 2 * dist + length, off, "data", pack(xs)), Region("y", 2 * dist + length, off, "data", pack(ys))]
        regions += [Region(n, 3 * nb, off, "sentinel") for n in names]
        regions += [Region("work", pl.workspace_min(cross), off, "poison")]
        m = 0 if f & (f - 1) == 0 or f < 3 else inner_m(f)
        a = Arena(_tdt(dt), regions, m=m, device="cuda")
        before = {n: a[n].clone() for n in ("x", "y")}
        if cross:
            gpu.csd_batched(a["x"], a["y"], a["re"], a["im"], pl, 3, a["pxx"], a["pyy"], sig_dist=dist, workspace=a["work"])
        else:
            gpu.psd_batched(a["x"], a["out"], pl, 3, sig_dist=dist, workspace=a["work"])
        import torch

        torch.cuda.synchronize()
        assert a.check() == [], (off, a.check())
        for n in ("x", "y"):
            assert torch.equal(a[n], before[n]), n
        for n, w in zip(names, want):
            got = a[n].cpu().numpy()
            assert not np.isnan(got).any(), n
            assert np.array_equal(got, w), (n, off)


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_element_aligned_views(gpu, dt):
    """buf[1:] views for the signals, the outputs and the workspace: the bits of the aligned call"""
    import torch

    for shape in [(1000, 100, 63, 128), (300, 7, 3, 9), (4096, 8, 1, 8)]:
        length = shape[0]
        pl = planner(gpu, dt, shape, True, "spectrum", "random")
        x, y = _signal(length, dt, 80), _signal(length, dt, 81)
        for cross in (False, True):
            for average in (True, False):
                run = (lambda **kw: run_cross(gpu, pl, dt, x, y, average, **kw)) if cross else (lambda **kw: [run_auto(gpu, pl, dt, x, average, **kw)])
                want = run()
                work = torch.full((pl.workspace_len(1, cross) + 1,), float("nan"), dtype=_tdt(dt), device="cuda")[1:]
                for got, w in zip(run(workspace=work, lead=1), want):
                    assert np.array_equal(got, w), (shape, cross, average)


def test_host_forms_are_the_device_forms(gpu):
    for dt in ("f64", "f32"):
        for shape in [(1000, 100, 63, 128), (300, 7, 3, 9)]:
            length = shape[0]
            pl = planner(gpu, dt, shape)
            x, y = np.array(_signal(length, dt, 90)), np.array(_signal(length, dt, 91))
            for average in (True, False):
                pts = pl.bins * (1 if average else pl.segments)
                out = np.zeros(pts, _ndt(dt))
                getattr(gpu, f"psd_{dt}_with_planner")(x, out, pl, average=average)
                assert np.array_equal(out, run_auto(gpu, pl, dt, x, average))
                outs = [np.zeros(pts, _ndt(dt)) for _ in range(4)]
                getattr(gpu, f"csd_{dt}_with_planner")(x, y, outs[0], outs[1], pl, outs[2], outs[3], average=average)
                for got, want in zip(outs, run_cross(gpu, pl, dt, x, y, average)):
                    assert np.array_equal(got, want)
                two = [np.zeros(pts, _ndt(dt)) for _ in range(2)]
                getattr(gpu, f"csd_{dt}_with_planner")(x, y, two[0], two[1], pl, average=average)   # without the auto spectra
                assert np.array_equal(two[0], outs[0]) and np.array_equal(two[1], outs[1])
            with pytest.raises(gpu.PhastPanic):
                getattr(gpu, f"psd_{dt}_with_planner")(x, np.zeros(pl.bins + 1, _ndt(dt)), pl)
            with pytest.raises(gpu.PhastPanic):
                getattr(gpu, f"psd_{dt}_with_planner")(x[:-1], np.zeros(pl.bins, _ndt(dt)), pl)


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_conveniences_against_scipy(gpu, dt):
    """welch, csd, spectrogram, periodogram and coherence on a [2, 3, 1000] tensor: shapes and values"""
    import warnings

    import scipy.signal as ss
    import torch

    rng = np.random.default_rng(11)
    x = rng.uniform(-1, 1, (2, 3, 1000)).astype(_ndt(dt))
    y = (0.5 * x + rng.uniform(-1, 1, x.shape)).astype(_ndt(dt))
    d_x, d_y = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    xd, yd = x.astype(np.float64), y.astype(np.float64)
    eps = float(np.finfo(_ndt(dt)).eps)

    def same(tag, got, want, f, den=None):
        got = got.cpu().numpy()
        assert got.shape == want.shape, (tag, got.shape, want.shape)
        check(f"conv:{tag}", dt, f, got.reshape(-1), want.reshape(-1), den)

    for kw in (dict(nperseg=100, noverlap=37, nfft=128, fs=FS), dict(nperseg=256), dict(nperseg=64, scaling="spectrum", detrend=False,
                                                                                         window=rng.uniform(0.1, 1, 64))):
        f = kw.get("nfft", kw["nperseg"])
        fr, want = ss.welch(xd, **kw)
        gf, got = gpu.welch(d_x, **kw)
        assert np.allclose(gf.cpu().numpy(), fr, rtol=4 * eps, atol=0)
        same("welch", got, want, f)
        _, wxy = ss.csd(xd, yd, **kw)
        _, wyy = ss.welch(yd, **kw)
        gf, got = gpu.csd(d_x, d_y, **kw)
        assert got.is_complex()
        same("csd", got, wxy, f, _norm(np.sqrt(want * wyy)))
        fr, tt, wsp = ss.spectrogram(xd, mode="psd", **{"window": "hann", **kw})
        gf, gt, got = gpu.spectrogram(d_x, **kw)
        assert np.allclose(gt.cpu().numpy(), tt, rtol=4 * eps, atol=0)
        same("spectrogram", got, wsp, f)
        if "scaling" not in kw:
            _, wco = ss.coherence(xd, yd, **kw)
            _, got = gpu.coherence(d_x, d_y, **kw)
            same("coherence", got, wco, f)
    _, want = ss.periodogram(xd, fs=FS)
    _, got = gpu.periodogram(d_x, fs=FS)
    same("periodogram", got, want, 1000)
    _, one = gpu.coherence(d_x, d_x, nperseg=100)
    assert float((one - 1).abs().max()) <= 10 * eps     # |P_xx|^2 / (P_xx P_xx)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        _, got = gpu.welch(d_x[0, 0, :50], nperseg=256)   # clamped to the length, as scipy does, with a warning
    assert any("nperseg" in str(w.message) for w in caught)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, want = ss.welch(xd[0, 0, :50], nperseg=256)
    same("clamped", got, want, 50)
