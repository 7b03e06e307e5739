"""The STFT and its inverse on the MI355X (csrc/stft.hip, csrc/planner_stft.hpp) against tests/stft_reference.py in long double
(which tests/test_stft_cpu.py holds against torch.stft / torch.istft).

Gates: tests/tolerances.py's formulas on log2 of the inner length of the real transform of F (inner_m of
tests/test_gpu_any_real.py), times the any-length factor 2, as for the real transforms and the DCT: a frame is one R2C or C2R
of F between a sweep that multiplies once and one that adds F / H products and divides.  The forward result is gated as
rel-L2 and worst bin over the whole spectrogram, the inverse and the round trip as rel-L2 over the signal.  The measured worst
over seeds 0-3 is in tests/golden/stft_error_budget.json (tests/golden/make_stft_error_budget.py).

The inverse runs wherever the reference itself inverts: every window with center, rectangular and uniform(0.5, 1.5) without.
Where it does not -- Hann without center (w[0] = 0 is sample 0's only tap) and Hann with H = F, whose zero lands on an
interior sample even with center -- the planner must refuse, and the test asserts that instead."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import stft_reference as R
from tests import tolerances as tol
from tests.test_gpu_any_real import inner_m

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANY_FACTOR = 2.0
SHAPES = [(37, 1, 1), (64, 2, 1), (101, 7, 3), (1000, 16, 16), (1000, 30, 23), (4099, 64, 16), (5000, 1000, 250),
          (5000, 1024, 256)]
MODES = [(c, pad) for c in (True, False) for pad in ("reflect", "zero")]


def stft_gates(dt: str, f: int):
    lm = inner_m(f).bit_length() - 1
    return ANY_FACTOR * tol.rel_gate(dt, lm), ANY_FACTOR * tol.bin_gate(dt, lm)


def _ndt(dt):
    return np.float64 if dt == "f64" else np.float32


def _tdt(dt):
    import torch

    return torch.float64 if dt == "f64" else torch.float32


@functools.lru_cache(maxsize=None)
def _signal(length: int, dt: str, seed: int = 0):
    x = np.random.default_rng([seed, length, 13]).uniform(-1, 1, length).astype(_ndt(dt))
    x.flags.writeable = False
    return x


@functools.lru_cache(maxsize=None)
def reference(dt, length, f, h, center, pad, win, seed=0):
    """(window, long-double spectrogram, its rounding to dt as two planes, the reference inverse of those planes or None)"""
    x, w = _signal(length, dt, seed), R.window(win, f, _ndt(dt))
    spec = R.stft(x, w, f, h, center, pad)
    re, im = (np.ascontiguousarray(v, _ndt(dt)).reshape(-1) for v in (spec.real, spec.imag))
    back = None
    if R.invertible(w, length, f, h, center):
        frames, bins = spec.shape
        back = R.istft(re.reshape(frames, bins).astype(np.longdouble) + 1j * im.reshape(frames, bins).astype(np.longdouble),
                       w, length, f, h, center)
    for v in (w, re, im):
        v.flags.writeable = False
    return w, spec, re, im, back


def planner(P, dt, length, f, h, w, center, pad):
    return (P.PlannerStft64 if dt == "f64" else P.PlannerStft32)(length, f, h, window=w, center=center, pad_mode=pad)


def forward(P, pl, x, workspace=None):
    import torch

    d_x = torch.from_numpy(np.array(x)).cuda()
    pts = pl.frames * pl.bins
    re = torch.full((pts + 3,), 7.0, dtype=d_x.dtype, device="cuda")
    im = torch.full((pts + 3,), 7.0, dtype=d_x.dtype, device="cuda")
    P.stft_batched(d_x, re, im, pl, 1, workspace=workspace)
    assert np.array_equal(d_x.cpu().numpy(), x)  # the signal is never written
    re, im = re.cpu().numpy(), im.cpu().numpy()
    assert (re[pts:] == 7.0).all() and (im[pts:] == 7.0).all()
    return re[:pts], im[:pts]


def inverse(P, pl, re, im, workspace=None):
    import torch

    d_re, d_im = torch.from_numpy(np.array(re)).cuda(), torch.from_numpy(np.array(im)).cuda()
    out = torch.full((pl.signal_len + 3,), 7.0, dtype=d_re.dtype, device="cuda")
    P.istft_batched(d_re, d_im, out, pl, 1, workspace=workspace)
    assert np.array_equal(d_re.cpu().numpy(), re) and np.array_equal(d_im.cpu().numpy(), im)
    out = out.cpu().numpy()
    assert (out[pl.signal_len:] == 7.0).all()
    return out[:pl.signal_len]


def rel_l2(got, want):
    want = np.asarray(want, np.longdouble)
    den = np.sqrt(np.sum(want * want))
    return float(np.sqrt(np.sum((np.asarray(got, np.longdouble) - want) ** 2)) / (den if den else 1))


def check_forward(tag, dt, f, re, im, spec):
    want_re, want_im = (np.asarray(v, np.float64).reshape(-1) for v in (spec.real, spec.imag))
    rel, worst = tol.rel_l2(re, im, want_re, want_im), tol.max_bin_err(re, im, want_re, want_im)
    g_rel, g_bin = stft_gates(dt, f)
    tol.record(tag, inner_m(f).bit_length() - 1, rel, worst, g_rel, g_bin)
    print(f"{tag} {dt}: rel {rel:.3e} / {g_rel:.3e}, bin {worst:.3e} / {g_bin:.3e}")
    assert rel <= g_rel and worst <= g_bin, (tag, dt, rel, g_rel, worst, g_bin)


def check_signal(tag, dt, f, got, want):
    rel = rel_l2(got, want)
    g_rel, _ = stft_gates(dt, f)
    tol.record(tag, inner_m(f).bit_length() - 1, rel, 0.0, g_rel, 0.0)
    print(f"{tag} {dt}: rel {rel:.3e} / {g_rel:.3e}")
    assert rel <= g_rel, (tag, dt, rel, g_rel)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_forward_parity(gpu, dt, shape):
    length, f, h = shape
    for center, pad in MODES:
        for win in R.WINDOWS:
            w, spec, *_ = reference(dt, length, f, h, center, pad, win)
            pl = planner(gpu, dt, length, f, h, w, center, pad)
            assert (pl.frames, pl.bins) == spec.shape
            re, im = forward(gpu, pl, _signal(length, dt))
            check_forward(f"stft:{shape}:{center}:{pad}:{win}", dt, f, re, im, spec)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_inverse_parity_and_round_trip(gpu, dt, shape):
    """the inverse of the reference's (rounded) spectrogram against the reference inverse of the same planes, and
    istft(stft(x)) on the device against x (0 where no frame holds the sample); a window the reference cannot invert is
    refused"""
    import torch

    length, f, h = shape
    inverted = 0
    for center, pad in MODES:
        for win in R.WINDOWS:
            w, spec, re, im, back = reference(dt, length, f, h, center, pad, win)
            pl = planner(gpu, dt, length, f, h, w, center, pad)
            den, cnt = R.envelope(w, length, f, h, center)
            assert abs(pl.envelope_min - den[cnt > 0].min()) <= 1e-12 * max(1.0, pl.envelope_min)
            assert (back is None) == (win == "hann" and f > 1 and (not center or h == f)), (shape, center, win)
            if back is None:  # the cases the docstring names
                with pytest.raises(gpu.PhastPanic) as e:
                    gpu.istft_batched(torch.from_numpy(np.array(re)).cuda(), torch.from_numpy(np.array(im)).cuda(),
                                      torch.zeros(length, dtype=_tdt(dt), device="cuda"), pl, 1)
                assert e.value.code == 16
                continue
            inverted += 1
            tag = f"{shape}:{center}:{pad}:{win}"
            check_signal("istft:" + tag, dt, f, inverse(gpu, pl, re, im), back)
            x = _signal(length, dt)
            g_re, g_im = forward(gpu, pl, x)
            want = np.where(cnt > 0, x.astype(np.float64), 0.0)
            check_signal("round:" + tag, dt, f, inverse(gpu, pl, g_re, g_im), want)
    assert inverted >= 8


@pytest.mark.parametrize("shape", [(1000, 30, 23), (4099, 64, 16), (5000, 1000, 250)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_batch_properties(gpu, dt, shape):
    """batch 3 at sig_dist = L + 5 on a base offset by one element: the sentinel in the gaps and past the end stays; the bits
    do not depend on the workspace (1 frame, 2 frames + 1 element, everything; 1 signal per chunk or all) or on the batch"""
    import torch

    length, f, h = shape
    batch, dist = 3, length + 5
    w = R.window("hann", f, _ndt(dt))
    pl = planner(gpu, dt, length, f, h, w, True, "reflect")
    pts = pl.frames * pl.bins
    xs = [_signal(length, dt, seed=20 + b) for b in range(batch)]
    alone = [forward(gpu, pl, x) for x in xs]
    buf = torch.full((1 + batch * dist + 4,), 9.0, dtype=_tdt(dt), device="cuda")
    sig = buf[1:]
    for b in range(batch):
        sig[b * dist:b * dist + length] = torch.from_numpy(np.array(xs[b]))
    keep = buf.cpu().numpy()
    vec = 16 // np.dtype(_ndt(dt)).itemsize
    per = pl.workspace_min() - (vec - 1)
    assert pl.workspace_len(batch) == batch * pl.frames * per + vec - 1 and pl.workspace_min(True) == pl.frames * per + vec - 1
    spaces = {"one frame": pl.workspace_min(), "two frames + 1": 2 * per + vec, "everything": pl.workspace_len(batch)}
    planes = None
    for name, size in spaces.items():
        ws = torch.empty(size, dtype=_tdt(dt), device="cuda")
        re = torch.full((1 + batch * pts + 4,), 9.0, dtype=_tdt(dt), device="cuda")
        im = torch.full((1 + batch * pts + 4,), 9.0, dtype=_tdt(dt), device="cuda")
        gpu.stft_batched(sig, re[1:], im[1:], pl, batch, sig_dist=dist, workspace=ws)
        assert np.array_equal(buf.cpu().numpy(), keep), name  # the signals and their gaps are not written
        got_re, got_im = re.cpu().numpy(), im.cpu().numpy()
        for v in (got_re, got_im):
            assert v[0] == 9.0 and (v[1 + batch * pts:] == 9.0).all(), name
        for b in range(batch):
            assert np.array_equal(got_re[1 + b * pts:1 + (b + 1) * pts], alone[b][0]), (name, b)
            assert np.array_equal(got_im[1 + b * pts:1 + (b + 1) * pts], alone[b][1]), (name, b)
        planes = (re, im)
    re, im = planes
    back_alone = [inverse(gpu, pl, *alone[b]) for b in range(batch)]
    for name, size in {"one signal": pl.workspace_min(True), "everything": pl.workspace_len(batch)}.items():
        ws = torch.empty(size + 1, dtype=_tdt(dt), device="cuda")[1:]  # an unaligned workspace base
        out = torch.full((1 + batch * dist + 4,), 9.0, dtype=_tdt(dt), device="cuda")
        gpu.istft_batched(re[1:], im[1:], out[1:], pl, batch, sig_dist=dist, workspace=ws)
        got = out.cpu().numpy()
        assert got[0] == 9.0 and (got[1 + (batch - 1) * dist + length:] == 9.0).all(), name
        for b in range(batch):
            at = 1 + b * dist
            assert np.array_equal(got[at:at + length], back_alone[b]), (name, b)
            if b + 1 < batch:
                assert (got[at + length:at + dist] == 9.0).all(), (name, b)
    with pytest.raises(gpu.PhastPanic):  # less than one signal's frames: refused, not run
        gpu.istft_batched(re[1:], im[1:], sig, pl, batch, sig_dist=dist,
                          workspace=torch.empty(pl.workspace_min(True) - 1, dtype=_tdt(dt), device="cuda"))


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_two_streams_share_one_planner(gpu, dt):
    """two streams, each with its own workspace and outputs, interleaved on one planner: the single-stream bits"""
    import torch

    length, f, h = 5000, 1000, 250
    pl = planner(gpu, dt, length, f, h, R.window("hann", f, _ndt(dt)), True, "reflect")
    xs = [_signal(length, dt, seed=30 + i) for i in range(2)]
    want = [forward(gpu, pl, x) for x in xs]
    want_back = [inverse(gpu, pl, *v) for v in want]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in range(2)]
    d_x = [torch.from_numpy(np.array(x)).cuda() for x in xs]
    pts = pl.frames * pl.bins
    bufs = [[torch.zeros(pts, dtype=_tdt(dt), device="cuda") for _ in range(2)] + [torch.zeros(length, dtype=_tdt(dt), device="cuda")]
            for _ in range(2)]
    work = [torch.empty(pl.workspace_len(1), dtype=_tdt(dt), device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    for _ in range(3):
        for i, s in enumerate(streams):
            with torch.cuda.stream(s):
                gpu.stft_batched(d_x[i], bufs[i][0], bufs[i][1], pl, 1, workspace=work[i])
                gpu.istft_batched(bufs[i][0], bufs[i][1], bufs[i][2], pl, 1, workspace=work[i])
    torch.cuda.synchronize()
    for i in range(2):
        assert np.array_equal(bufs[i][0].cpu().numpy(), want[i][0]) and np.array_equal(bufs[i][1].cpu().numpy(), want[i][1])
        assert np.array_equal(bufs[i][2].cpu().numpy(), want_back[i])


@pytest.mark.parametrize("shape", [(5000, 1000, 250), (5000, 1024, 256)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_graph_capture(gpu, dt, shape):
    """a forward + inverse pair captured on a side stream and replayed on new data: the eager results of that data"""
    import torch

    length, f, h = shape
    pl = planner(gpu, dt, length, f, h, R.window("uniform", f, _ndt(dt)), True, "reflect")
    pts = pl.frames * pl.bins
    d_x = torch.from_numpy(np.array(_signal(length, dt, seed=40))).cuda()
    re, im = (torch.zeros(pts, dtype=_tdt(dt), device="cuda") for _ in range(2))
    out = torch.zeros(length, dtype=_tdt(dt), device="cuda")
    work = torch.empty(pl.workspace_len(1), dtype=_tdt(dt), device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on the capture stream
        gpu.stft_batched(d_x, re, im, pl, 1, workspace=work)
        gpu.istft_batched(re, im, out, pl, 1, workspace=work)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        gpu.stft_batched(d_x, re, im, pl, 1, workspace=work)
        gpu.istft_batched(re, im, out, pl, 1, workspace=work)
    for seed in (41, 42):
        x = _signal(length, dt, seed=seed)
        want = forward(gpu, pl, x)
        want_back = inverse(gpu, pl, *want)
        d_x.copy_(torch.from_numpy(np.array(x)))
        for v in (re, im, out):
            v.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(re.cpu().numpy(), want[0]) and np.array_equal(im.cpu().numpy(), want[1])
        assert np.array_equal(out.cpu().numpy(), want_back)


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_host_forms_and_lengths(gpu, dt):
    """host slices give the _dev bits; wrong lengths come back as codes"""
    length, f, h = 1000, 30, 23
    w = R.window("uniform", f, _ndt(dt))
    pl = planner(gpu, dt, length, f, h, w, True, "zero")
    x = np.array(_signal(length, dt, seed=50))
    want = forward(gpu, pl, x)
    pts = pl.frames * pl.bins
    re, im = np.zeros(pts, _ndt(dt)), np.zeros(pts, _ndt(dt))
    getattr(gpu, f"stft_{dt}_with_planner")(x, re, im, pl)
    assert np.array_equal(re, want[0]) and np.array_equal(im, want[1])
    back = np.zeros(length, _ndt(dt))
    getattr(gpu, f"istft_{dt}_with_planner")(re, im, back, pl)
    assert np.array_equal(back, inverse(gpu, pl, re, im))
    with pytest.raises(gpu.PhastPanic) as e:
        getattr(gpu, f"stft_{dt}_with_planner")(x[:-1].copy(), re, im, pl)
    assert e.value.code == 3  # PHAST_ERR_PLANNER_SIZE
    with pytest.raises(gpu.PhastPanic) as e:
        getattr(gpu, f"istft_{dt}_with_planner")(re[:-1].copy(), im, back, pl)
    assert e.value.code == 2  # PHAST_ERR_LEN_MISMATCH
    assert "stft L=1000 F=30 H=23" in pl.describe() and pl.device_bytes() > 0


def test_short_window_is_centred(gpu):
    """win_length < n_fft in the Python wrapper: the window zero-padded on both sides, as torch.stft does"""
    import torch

    length, f, h = 400, 32, 8
    x = np.array(_signal(length, "f64", seed=60))
    w = R.window("hann", 20)
    pl = gpu.PlannerStft64(length, f, h, window=w)
    re, im = forward(gpu, pl, x)
    want = torch.stft(torch.from_numpy(x), f, h, win_length=20, window=torch.from_numpy(w), return_complex=True).numpy().T
    assert np.abs(re.reshape(want.shape) - want.real).max() < 1e-12 and np.abs(im.reshape(want.shape) - want.imag).max() < 1e-12


def test_cpp_mirror(gpu, tmp_path):
    from phastft_amd import build

    lib = build.build()
    exe = str(tmp_path / "stft_test")
    libdir = os.path.dirname(lib)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "stft_test.cpp"), "-o", exe, "-L", libdir, "-lphastft_hip",
                        f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, "gpu"], capture_output=True, text=True)
    sys.stdout.write(r.stdout)
    assert r.returncode == 0 and "stft: ok" in r.stdout, r.stdout + r.stderr


def test_gates_keep_their_margin():
    """the gates above sit >= 2 x over the worst error measured on the MI355X over seeds 0-3"""
    budget = json.load(open(os.path.join(ROOT, "tests", "golden", "stft_error_budget.json")))
    assert budget["entries"]
    for e in budget["entries"]:
        g_rel, g_bin = stft_gates(e["dt"], e["f"])
        assert g_rel >= 2 * e["rel"] and g_bin >= 2 * e["bin"], e
