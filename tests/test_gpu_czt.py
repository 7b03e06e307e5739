"""The chirp-Z transform on the MI355X (csrc/czt.hip, csrc/planner_czt.hpp) against tests/czt_reference.py, the direct sum in long
double with exact phases (which tests/test_czt_cpu.py holds against scipy.signal.czt / zoom_fft), on the rounded inputs.

The gate: tests/tolerances.py's rel-L2 and per-bin formulas on log2 L, L the convolution length, times the any-length factor 2,
as for the any-length transforms, the STFT and the convolution: the schedule is Bluestein's, two L-point
transforms around a multiply by a table built in double.  A numpy model of the schedule in double on the library's phases uses
at most 0.19 of the f64 gate (tests/test_czt_cpu.py prints it); the measured worst on the device over seeds 0-3 is in
tests/golden/czt_error_budget.json (tests/golden/make_czt_error_budget.py).

The shapes (N, M, step, start) are the smallest that reach the degenerate lengths, ragged groups, M > N and M < N, N + M - 1 on
and one past a power of two, the DFT's parameters, and phases of ~1.6e9 turns at large n and large k."""
import functools
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from tests import czt_reference as R
from tests import tolerances as tol
from tests.test_czt_cpu import SHAPES, START, conv_len, czt_gate, step_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def shape_id(s):
    return "x".join(str(v) for v in s[:2]) + ("" if s[2] is None else f"-step{s[2]:.4g}") + (f"-start{s[3]:.3g}" if s[3] != START else "")


def _ndt(dt):
    return np.float64 if dt == "f64" else np.float32


def _tdt(dt):
    import torch

    return torch.float64 if dt == "f64" else torch.float32


@functools.lru_cache(maxsize=None)
def _signal(n: int, dt: str, seed: int = 0):
    re, im = R.signal(n, _ndt(dt), seed)
    re.flags.writeable = im.flags.writeable = False
    return re, im


@functools.lru_cache(maxsize=None)
def reference(dt, n, m, step, start, seed=0, real=False):
    """the M bins of the rounded input in long double; computed once per case and left unchanged"""
    re, im = _signal(n, dt, seed)
    out = R.czt(re if real else re.astype(np.complex128) + 1j * im, m, step, start)
    for a in out:
        a.flags.writeable = False
    return out


def planner(P, dt, n, m, step, start=0.0):
    return (P.PlannerCzt64 if dt == "f64" else P.PlannerCzt32)(n, m, step, start)


def run(P, pl, re, im, work=None):
    """one signal through czt_batched: the input is never written, nothing is written past M"""
    import torch

    d_re = torch.from_numpy(np.array(re)).cuda()
    d_im = None if im is None else torch.from_numpy(np.array(im)).cuda()
    o_re = torch.full((pl.m + 3,), 7.0, dtype=d_re.dtype, device="cuda")
    o_im = torch.full((pl.m + 3,), 7.0, dtype=d_re.dtype, device="cuda")
    got = P.czt_batched(d_re, d_im, pl, out=(o_re[:pl.m], o_im[:pl.m]), work=work)
    assert got[0].data_ptr() == o_re.data_ptr()
    assert np.array_equal(d_re.cpu().numpy(), re) and (im is None or np.array_equal(d_im.cpu().numpy(), im))
    o_re, o_im = o_re.cpu().numpy(), o_im.cpu().numpy()
    assert (o_re[pl.m:] == 7.0).all() and (o_im[pl.m:] == 7.0).all()
    return o_re[:pl.m], o_im[:pl.m]


def errors(got_re, got_im, ref_re, ref_im):
    """(rel-L2, worst bin / rms bin) in long double"""
    e_re, e_im = got_re.astype(R.LD) - ref_re, got_im.astype(R.LD) - ref_im
    den = np.sqrt(np.sum(ref_re ** 2 + ref_im ** 2))
    rms = np.sqrt(np.mean(ref_re ** 2 + ref_im ** 2))
    return (float(np.sqrt(np.sum(e_re ** 2 + e_im ** 2)) / (den if den else 1)),
            float(np.maximum(np.abs(e_re), np.abs(e_im)).max() / (rms if rms else 1)))


def check(tag, dt, n, m, got, want):
    rel, worst = errors(*got, *want)
    g_rel, g_bin = czt_gate(dt, n, m)
    tol.record(tag, conv_len(n, m).bit_length() - 1, rel, worst, g_rel, g_bin)
    print(f"{tag} {dt}: rel {rel:.3e} / {g_rel:.3e}, bin {worst:.3e} / {g_bin:.3e}")
    assert rel <= g_rel and worst <= g_bin, (tag, dt, rel, g_rel, worst, g_bin)


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_parity(gpu, dt, shape):
    n, m, _, start = shape
    step = step_of(shape)
    pl = planner(gpu, dt, n, m, step, start)
    assert pl.conv_len == conv_len(n, m) and pl.workspace_len(3) == 6 * pl.conv_len
    re, im = _signal(n, dt)
    got = run(gpu, pl, re, im)
    check(f"czt:{shape_id(shape)}", dt, n, m, got, reference(dt, n, m, step, start))
    if (n, m, step, start) == (64, 64, 1 / 64, 0.0):  # the DFT's parameters: the any-length transform's result, within the gate
        f_re, f_im = np.array(re), np.array(im)
        (gpu.fft_64_any if dt == "f64" else gpu.fft_32_any)(f_re, f_im, gpu.Direction.Forward)
        check("czt:64x64:vs fft_any", dt, n, m, got, (f_re.astype(R.LD), f_im.astype(R.LD)))


@pytest.mark.parametrize("shape", [(37, 101), (100, 29), (4099, 513)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_real_signal(gpu, dt, shape):
    """a null imaginary plane: the bits of the same signal with a zero imaginary plane, and the reference of the real signal"""
    n, m = shape
    step = 0.37 / n
    pl = planner(gpu, dt, n, m, step, START)
    re, _ = _signal(n, dt, seed=5)
    got = run(gpu, pl, re, None)
    zero = run(gpu, pl, re, np.zeros(n, _ndt(dt)))
    assert np.array_equal(got[0], zero[0]) and np.array_equal(got[1], zero[1])
    check(f"czt-real:{shape}", dt, n, m, got, reference(dt, n, m, step, START, seed=5, real=True))


@pytest.mark.parametrize("shape", [(37, 101), (101, 37), (100, 30), (4099, 513)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_batch_properties(gpu, dt, shape):
    """batch 3 at in_dist > N and out_dist > M on planes one element past a 16-byte boundary (the element-access kernels), with
    workspaces that force chunks of 1 and of 2 and one that holds everything: the input and the gaps of the output are not
    written, and every row has the bits of the same row transformed alone on aligned planes"""
    import torch

    n, m = shape
    batch = 3
    pl = planner(gpu, dt, n, m, 0.37 / n, START)
    ell = pl.conv_len
    in_dist, out_dist = (n + 5) | 1, (m + 3) | 1
    rows = [_signal(n, dt, seed=20 + i) for i in range(batch)]
    alone = [run(gpu, pl, re, im) for re, im in rows]
    bufs = [torch.full((1 + batch * in_dist + 4,), 9.0, dtype=_tdt(dt), device="cuda") for _ in range(2)]
    assert bufs[0][1:].data_ptr() % 16 == np.dtype(_ndt(dt)).itemsize
    x = [b[1:1 + batch * in_dist].view(batch, in_dist)[:, :n] for b in bufs]
    for i in range(batch):
        x[0][i] = torch.from_numpy(np.array(rows[i][0]))
        x[1][i] = torch.from_numpy(np.array(rows[i][1]))
    keep = [b.cpu().numpy() for b in bufs]
    assert pl.workspace_len(1) == 2 * ell and pl.workspace_len(batch) == 2 * ell * batch
    for name, size in {"chunks of 1": 2 * ell, "chunks of 2": 4 * ell + 1, "one chunk": pl.workspace_len(batch)}.items():
        outs = [torch.full((1 + batch * out_dist + 4,), 9.0, dtype=_tdt(dt), device="cuda") for _ in range(2)]
        o = tuple(b[1:1 + batch * out_dist].view(batch, out_dist)[:, :m] for b in outs)
        gpu.czt_batched(x[0], x[1], pl, out=o, work=torch.empty(size, dtype=_tdt(dt), device="cuda"))
        for b, k in zip(bufs, keep):
            assert np.array_equal(b.cpu().numpy(), k), name  # the input and its gaps are not written
        for plane in range(2):
            got = outs[plane].cpu().numpy()
            assert got[0] == 9.0 and (got[1 + (batch - 1) * out_dist + m:] == 9.0).all(), name
            for i in range(batch):
                at = 1 + i * out_dist
                assert np.array_equal(got[at:at + m], alone[i][plane]), (name, plane, i)
                if i + 1 < batch:
                    assert (got[at + m:at + out_dist] == 9.0).all(), (name, plane, i)
    with pytest.raises(gpu.PhastPanic) as e:  # less than one transform's workspace: refused, not run
        gpu.czt_batched(x[0], x[1], pl, work=torch.empty(2 * ell - 1, dtype=_tdt(dt), device="cuda"))
    assert e.value.code == 16


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_host_forms_and_codes(gpu, dt):
    """host slices give the _dev bits, with and without a planner, complex and real; a wrong length, a null plane, a short
    workspace and an output on top of the input come back as codes and run nothing"""
    import ctypes as C

    import torch

    from phastft_amd import _lib

    n, m, step, start = 1000, 333, 0.37 / 1000, START
    sfx = "64" if dt == "f64" else "32"
    pl = planner(gpu, dt, n, m, step, start)
    re, im = (np.array(a) for a in _signal(n, dt, seed=50))
    shot, host = getattr(gpu, f"czt_{sfx}"), getattr(gpu, f"czt_{sfx}_with_planner")
    for x_im in (im, None):
        want = run(gpu, pl, re, x_im)
        for call in (lambda o_re, o_im: host(re, x_im, o_re, o_im, pl), lambda o_re, o_im: shot(re, x_im, o_re, o_im, step, start)):
            o_re, o_im = np.zeros(m, _ndt(dt)), np.zeros(m, _ndt(dt))
            call(o_re, o_im)
            assert np.array_equal(o_re, want[0]) and np.array_equal(o_im, want[1])
    o_re, o_im = np.zeros(m, _ndt(dt)), np.zeros(m, _ndt(dt))
    with pytest.raises(gpu.PhastPanic) as e:
        host(re[:-1].copy(), im[:-1].copy(), o_re, o_im, pl)
    assert e.value.code == 3  # PHAST_ERR_PLANNER_SIZE
    with pytest.raises(gpu.PhastPanic) as e:
        host(re, im, o_re[:-1].copy(), o_im[:-1].copy(), pl)
    assert e.value.code == 3
    with pytest.raises(gpu.PhastPanic) as e:
        host(re, im[:-1].copy(), o_re, o_im, pl)
    assert e.value.code == 2  # PHAST_ERR_LEN_MISMATCH
    lib, n_ = _lib.lib(), C.c_size_t
    d_re, d_im = torch.from_numpy(re).cuda(), torch.from_numpy(im).cuda()
    d_or, d_oi = (torch.zeros(m, dtype=_tdt(dt), device="cuda") for _ in range(2))
    ws = torch.empty(pl.workspace_len(1), dtype=_tdt(dt), device="cuda")
    dev = getattr(lib, f"phast_czt_{sfx}_dev")
    px, py, por, poi, pw = (C.c_void_p(t.data_ptr()) for t in (d_re, d_im, d_or, d_oi, ws))
    size = n_(ws.numel())
    assert dev(None, py, n_(n), por, poi, n_(m), n_(1), pl._h, pw, size, None) == 16
    assert dev(px, py, n_(n), None, poi, n_(m), n_(1), pl._h, pw, size, None) == 16
    assert dev(px, py, n_(n), por, None, n_(m), n_(1), pl._h, pw, size, None) == 16
    assert dev(px, py, n_(n), por, poi, n_(m), n_(1), pl._h, None, size, None) == 16
    assert dev(px, py, n_(n), por, poi, n_(m), n_(1), pl._h, pw, n_(2 * pl.conv_len - 1), None) == 16   # a short workspace
    assert dev(px, py, n_(n - 1), por, poi, n_(m), n_(2), pl._h, pw, size, None) == 16                   # in_dist < N
    assert dev(px, py, n_(n), por, poi, n_(m - 1), n_(2), pl._h, pw, size, None) == 16                   # out_dist < M
    assert dev(px, py, n_(n), px, poi, n_(m), n_(1), pl._h, pw, size, None) == 16                        # the output on the input
    assert dev(px, py, n_(n), por, pw, n_(m), n_(1), pl._h, pw, size, None) == 16                        # ... on the workspace
    assert dev(px, py, n_(n), por, por, n_(m), n_(1), pl._h, pw, size, None) == 16                       # ... on its other plane
    assert dev(px, py, n_(n), por, poi, n_(m), n_(0), pl._h, None, n_(0), None) == 0                     # an empty batch
    wp = getattr(lib, f"phast_czt_{sfx}_with_planner")
    hp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert wp(None, hp(im), n_(n), hp(o_re), hp(o_im), n_(m), pl._h) == 16
    assert wp(hp(re), hp(im), n_(n), None, hp(o_im), n_(m), pl._h) == 16
    torch.cuda.synchronize()
    assert (d_or.cpu().numpy() == 0).all() and (d_oi.cpu().numpy() == 0).all()  # none of the refused calls ran
    text = pl.describe()
    assert text.startswith(f"czt N={n} M={m} L={pl.conv_len} ") and pl.device_bytes() > 0
    want = run(gpu, pl, re, im)
    st = pl.time_stages(d_re, d_im, d_or, d_oi, 1, ws, reps=1)
    assert len(st) == 5 and all(v >= 0 for v in st)
    assert np.array_equal(d_or.cpu().numpy(), want[0]) and np.array_equal(d_oi.cpu().numpy(), want[1])


def test_two_threads_two_streams_one_planner(gpu):
    import torch

    n, m = 100003, 4001
    pl = planner(gpu, "f64", n, m, 0.37 / n, START)
    inputs = [_signal(n, "f64", seed=30 + t) for t in range(2)]
    want = [run(gpu, pl, re, im) for re, im in inputs]
    torch.cuda.synchronize()
    errs = []

    def worker(t):
        try:
            s = torch.cuda.Stream()
            work = torch.empty(pl.workspace_len(1), dtype=torch.float64, device="cuda")
            with torch.cuda.stream(s):
                d_re, d_im = (torch.from_numpy(np.array(a)).cuda() for a in inputs[t])
                for _ in range(4):
                    o_re, o_im = gpu.czt_batched(d_re, d_im, pl, work=work, stream=s)
                    s.synchronize()
                    if not (np.array_equal(o_re.cpu().numpy(), want[t][0]) and np.array_equal(o_im.cpu().numpy(), want[t][1])):
                        errs.append(t)
        except Exception as e:  # noqa: BLE001
            errs.append(repr(e))

    th = [threading.Thread(target=worker, args=(t,)) for t in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_graph_capture(gpu, dt):
    """one _dev call captured on a side stream (a single-stream linear capture), replayed three times on new data: the eager
    results of that data"""
    import torch

    n, m = 100003, 513
    pl = planner(gpu, dt, n, m, 0.37 / n, START)
    re, im = _signal(n, dt, seed=40)
    d_re, d_im = torch.from_numpy(np.array(re)).cuda(), torch.from_numpy(np.array(im)).cuda()
    out = tuple(torch.zeros(m, dtype=_tdt(dt), device="cuda") for _ in range(2))
    work = torch.empty(pl.workspace_len(1), dtype=_tdt(dt), device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on the capture stream
        gpu.czt_batched(d_re, d_im, pl, out=out, work=work)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        gpu.czt_batched(d_re, d_im, pl, out=out, work=work)
    for seed in (41, 42, 43):
        re, im = _signal(n, dt, seed=seed)
        want = run(gpu, pl, re, im)
        d_re.copy_(torch.from_numpy(np.array(re)))
        d_im.copy_(torch.from_numpy(np.array(im)))
        out[0].zero_()
        out[1].zero_()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out[0].cpu().numpy(), want[0]) and np.array_equal(out[1].cpu().numpy(), want[1])


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_conveniences(gpu, dt):
    """czt and zoom_fft on device tensors, complex and real, one row and several: against the reference of their parameters"""
    import torch

    n = 1000
    re, im = _signal(n, dt, seed=60)
    x = torch.from_numpy(np.array(re) + 1j * np.array(im)).cuda()
    assert x.dtype == (torch.complex128 if dt == "f64" else torch.complex64)
    got = gpu.czt(x)  # m = n, step = 1 / n: the DFT
    assert got.dtype == x.dtype and got.shape == (n,)
    check("czt():dft", dt, n, n, (got.real.cpu().numpy(), got.imag.cpu().numpy()), reference(dt, n, n, 1.0 / n, 0.0, seed=60))
    for fn, m, fs, endpoint in (([0.1, 0.3], 257, 2.0, False), ([0.1, 0.3], 257, 2.0, True), (0.5, 64, 2.0, False),
                                ([100.0, 180.0], 500, 1000.0, True)):
        start, step = R.zoom_params(fn, m, fs, endpoint)
        got = gpu.zoom_fft(x, fn, m, fs=fs, endpoint=endpoint)
        assert got.shape == (m,)
        check(f"zoom_fft:{fn}:{m}:{endpoint}", dt, n, m, (got.real.cpu().numpy(), got.imag.cpu().numpy()),
              reference(dt, n, m, step, start, seed=60))
    start, step = R.zoom_params([0.1, 0.3], 257, 2.0, True)
    real = torch.from_numpy(np.array(re)).cuda()
    got = gpu.zoom_fft(real, [0.1, 0.3], 257, endpoint=True)
    assert got.dtype == x.dtype
    check("zoom_fft:real", dt, n, 257, (got.real.cpu().numpy(), got.imag.cpu().numpy()),
          reference(dt, n, 257, step, start, seed=60, real=True))
    rows = torch.stack([x, x.flip(0), 2 * x]).reshape(3, 1, n)  # leading axes are batches
    got = gpu.czt(rows, 257, step, start)
    assert got.shape == (3, 1, 257)
    pl = planner(gpu, dt, n, 257, step, start)
    for i in range(3):
        r = rows[i, 0]
        want = run(gpu, pl, r.real.cpu().numpy(), r.imag.cpu().numpy())
        assert np.array_equal(got[i, 0].real.cpu().numpy(), want[0]) and np.array_equal(got[i, 0].imag.cpu().numpy(), want[1])


def test_cpp_mirror(gpu, tmp_path):
    from phastft_amd import build

    lib = build.build()
    exe = str(tmp_path / "czt_test")
    libdir = os.path.dirname(lib)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "czt_test.cpp"), "-o", exe, "-L", libdir, "-lphastft_hip",
                        f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, "gpu"], capture_output=True, text=True)
    sys.stdout.write(r.stdout)
    assert r.returncode == 0 and "czt: ok" in r.stdout, r.stdout + r.stderr


def test_gates_keep_their_margin():
    """the gates above sit >= 2 x over the worst errors measured on the MI355X over seeds 0-3"""
    budget = json.load(open(os.path.join(ROOT, "tests", "golden", "czt_error_budget.json")))
    assert len(budget["entries"]) == 2 * len(SHAPES)
    for e in budget["entries"]:
        g_rel, g_bin = czt_gate(e["dt"], e["n"], e["m"])
        assert g_rel >= 2 * e["rel"] and g_bin >= 2 * e["bin"], e
