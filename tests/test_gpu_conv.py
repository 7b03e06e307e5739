"""Overlap-save convolution and correlation on the MI355X (csrc/conv.hip, csrc/planner_conv.hpp) against tests/conv_reference.py,
the direct sum in long double (which tests/test_conv_cpu.py holds against scipy.signal.convolve / correlate).

The gate: tests/tolerances.py's rel-L2 formula on log2 of the inner length of the real transform of B (inner_m of
tests/test_gpu_any_real.py), times the any-length factor 2, as for the STFT: a segment is one R2C, one complex multiply and one
C2R of B, which is the STFT's round trip; the filter's spectrum is built in double.  The result is gated as rel-L2 over the
whole output.  A pocketfft emulation of the schedule in the working precision uses at most 0.034 of this gate in f64 and 0.10
in f32; the measured worst on the device over seeds 0-3 is in tests/golden/conv_error_budget.json
(tests/golden/make_conv_error_budget.py).

The shapes (L, K, B) are the smallest that reach S = 1, K = 1, K > L, a Bluestein block, a ragged last segment, rows that
start 8 bytes off a 16-byte boundary, and one-kernel power-of-two rows; B = 0 is the automatic block."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import conv_reference as R
from tests import tolerances as tol
from tests.test_gpu_any_real import inner_m

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANY_FACTOR = 2.0
SHAPES = [(1, 1, 1), (37, 1, 8), (64, 5, 8), (100, 17, 17), (101, 7, 16), (10, 30, 64), (1000, 30, 64), (1000, 33, 100),
          (4099, 64, 256), (5000, 251, 1000), (5000, 1000, 4096), (5000, 1000, 1024), (5000, 251, 0)]
AUTO = {(5000, 251): 1024}  # what B = 0 resolves to
CASES = [(mode, flip) for mode in R.MODES for flip in (False, True)]


def block_of(shape):
    length, k, b = shape
    return b or AUTO[(length, k)]


def conv_gate(dt: str, b: int) -> float:
    return ANY_FACTOR * tol.rel_gate(dt, inner_m(b).bit_length() - 1)


def _ndt(dt):
    return np.float64 if dt == "f64" else np.float32


def _tdt(dt):
    import torch

    return torch.float64 if dt == "f64" else torch.float32


@functools.lru_cache(maxsize=None)
def _signal(length: int, dt: str, seed: int = 0):
    x = R.signal(length, _ndt(dt), seed)
    x.flags.writeable = False
    return x


@functools.lru_cache(maxsize=None)
def _taps(kind: str, k: int, dt: str, seed: int = 0):
    h = R.taps(kind, k, _ndt(dt), seed)
    h.flags.writeable = False
    return h


@functools.lru_cache(maxsize=None)
def _full(dt, length, k, kind, flip, seed=0):
    """the full convolution of the rounded signal and taps in long double: every mode is a slice of it"""
    full = R.convolve(_signal(length, dt, seed), _taps(kind, k, dt, seed), "full", flip)
    full.flags.writeable = False
    return full


def reference(dt, length, k, kind, mode, flip, seed=0):
    t0, n = R.geometry(length, k, mode)
    return _full(dt, length, k, kind, flip, seed)[t0:t0 + n]


def planner(P, dt, length, taps, mode, flip, block):
    return (P.PlannerConv64 if dt == "f64" else P.PlannerConv32)(length, taps, mode=mode, correlate=flip, block=block)


def run(P, pl, x, workspace=None):
    """one signal through conv_batched: the signal is never written, nothing is written past out_len"""
    import torch

    d_x = torch.from_numpy(np.array(x)).cuda()
    out = torch.full((pl.out_len + 3,), 7.0, dtype=d_x.dtype, device="cuda")
    P.conv_batched(d_x, out, pl, 1, workspace=workspace)
    assert np.array_equal(d_x.cpu().numpy(), x)
    out = out.cpu().numpy()
    assert (out[pl.out_len:] == 7.0).all()
    return out[:pl.out_len]


def rel_l2(got, want):
    want = np.asarray(want, np.longdouble)
    den = np.sqrt(np.sum(want * want))
    return float(np.sqrt(np.sum((np.asarray(got, np.longdouble) - want) ** 2)) / (den if den else 1))


def check(tag, dt, b, got, want):
    rel, gate = rel_l2(got, want), conv_gate(dt, b)
    tol.record(tag, inner_m(b).bit_length() - 1, rel, 0.0, gate, 0.0)
    print(f"{tag} {dt}: rel {rel:.3e} / {gate:.3e}")
    assert rel <= gate, (tag, dt, rel, gate)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_parity(gpu, dt, shape):
    length, k, block = shape
    b = block_of(shape)
    for kind in R.TAPS:
        for mode, flip in CASES:
            if mode == "valid" and length < k:
                with pytest.raises(gpu.PhastPanic) as e:
                    planner(gpu, dt, length, _taps(kind, k, dt), mode, flip, block)
                assert e.value.code == 16
                continue
            pl = planner(gpu, dt, length, _taps(kind, k, dt), mode, flip, block)
            want = reference(dt, length, k, kind, mode, flip)
            s = b - k + 1
            assert (pl.out_len, pl.block, pl.segments) == (len(want), b, -(-len(want) // s)), (shape, mode)
            check(f"conv:{shape}:{kind}:{mode}:{int(flip)}", dt, b, run(gpu, pl, _signal(length, dt)), want)


@pytest.mark.parametrize("shape", [(100, 17, 17), (1000, 33, 100), (4099, 64, 256), (5000, 1000, 1024)],
                         ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_batch_properties(gpu, dt, shape):
    """batch 3 at odd sig_dist and out_dist on bases one element past a 16-byte boundary: the sentinel in the gaps and past
    the end stays, the signals are not written; the bits do not depend on the batch, on the workspace (1 segment, 2 segments
    + 1 element on an unaligned base, everything) or on the alignment of the pointers"""
    import torch

    length, k, block = shape
    batch = 3
    for mode, flip in (("full", False), ("same", True), ("valid", False)):
        pl = planner(gpu, dt, length, _taps("random", k, dt), mode, flip, block)
        n = pl.out_len
        sig_dist, out_dist = (length + 5) | 1, (n + 3) | 1
        xs = [_signal(length, dt, seed=20 + i) for i in range(batch)]
        alone = [run(gpu, pl, x) for x in xs]
        buf = torch.full((1 + batch * sig_dist + 4,), 9.0, dtype=_tdt(dt), device="cuda")
        sig = buf[1:]
        assert sig.data_ptr() % 16 == np.dtype(_ndt(dt)).itemsize
        for i in range(batch):
            sig[i * sig_dist:i * sig_dist + length] = torch.from_numpy(np.array(xs[i]))
        keep = buf.cpu().numpy()
        vec = 16 // np.dtype(_ndt(dt)).itemsize
        per = pl.workspace_min() - (vec - 1)
        assert pl.workspace_len(batch) == batch * pl.segments * per + vec - 1 and pl.workspace_len(1) == pl.segments * per + vec - 1
        spaces = {"one segment": pl.workspace_min(), "two segments + 1": 2 * per + vec, "everything": pl.workspace_len(batch)}
        for name, size in spaces.items():
            ws = torch.empty(size + 1, dtype=_tdt(dt), device="cuda")[1:] if name == "two segments + 1" else \
                torch.empty(size, dtype=_tdt(dt), device="cuda")
            out = torch.full((1 + batch * out_dist + 4,), 9.0, dtype=_tdt(dt), device="cuda")
            gpu.conv_batched(sig, out[1:], pl, batch, sig_dist=sig_dist, out_dist=out_dist, workspace=ws)
            assert np.array_equal(buf.cpu().numpy(), keep), name  # the signals and their gaps are not written
            got = out.cpu().numpy()
            assert got[0] == 9.0 and (got[1 + (batch - 1) * out_dist + n:] == 9.0).all(), name
            for i in range(batch):
                at = 1 + i * out_dist
                assert np.array_equal(got[at:at + n], alone[i]), (mode, name, i)
                if i + 1 < batch:
                    assert (got[at + n:at + out_dist] == 9.0).all(), (mode, name, i)
        with pytest.raises(gpu.PhastPanic) as e:  # less than one segment: refused, not run
            gpu.conv_batched(sig, torch.empty(batch * out_dist, dtype=_tdt(dt), device="cuda"), pl, batch, sig_dist=sig_dist,
                             out_dist=out_dist, workspace=torch.empty(pl.workspace_min() - 1, dtype=_tdt(dt), device="cuda"))
        assert e.value.code == 16


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_two_streams_share_one_planner(gpu, dt):
    """two streams, each with its own workspace and output, interleaved on one planner: the single-stream bits"""
    import torch

    length, k, block = 5000, 251, 1000
    pl = planner(gpu, dt, length, _taps("lowpass", k, dt), "same", False, block)
    xs = [_signal(length, dt, seed=30 + i) for i in range(2)]
    want = [run(gpu, pl, x) for x in xs]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in range(2)]
    d_x = [torch.from_numpy(np.array(x)).cuda() for x in xs]
    outs = [torch.zeros(pl.out_len, dtype=_tdt(dt), device="cuda") for _ in range(2)]
    work = [torch.empty(pl.workspace_len(1), dtype=_tdt(dt), device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    for _ in range(3):
        for i, s in enumerate(streams):
            with torch.cuda.stream(s):
                gpu.conv_batched(d_x[i], outs[i], pl, 1, workspace=work[i])
    torch.cuda.synchronize()
    for i in range(2):
        assert np.array_equal(outs[i].cpu().numpy(), want[i])


@pytest.mark.parametrize("shape", [(5000, 251, 1000), (5000, 1000, 4096)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_graph_capture(gpu, dt, shape):
    """a call captured on a side stream and replayed on new data: the eager results of that data"""
    import torch

    length, k, block = shape
    pl = planner(gpu, dt, length, _taps("random", k, dt), "full", True, block)
    d_x = torch.from_numpy(np.array(_signal(length, dt, seed=40))).cuda()
    out = torch.zeros(pl.out_len, dtype=_tdt(dt), device="cuda")
    work = torch.empty(pl.workspace_len(1), dtype=_tdt(dt), device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on the capture stream
        gpu.conv_batched(d_x, out, pl, 1, workspace=work)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        gpu.conv_batched(d_x, out, pl, 1, workspace=work)
    for seed in (41, 42):
        x = _signal(length, dt, seed=seed)
        want = run(gpu, pl, x)
        d_x.copy_(torch.from_numpy(np.array(x)))
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), want)


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_host_forms_and_codes(gpu, dt):
    """host slices give the _dev bits; a wrong length, a null pointer and a too-small workspace come back as codes"""
    import ctypes as C

    import torch

    from phastft_amd import _lib

    length, k, block = 1000, 33, 100
    pl = planner(gpu, dt, length, _taps("random", k, dt), "same", True, block)
    x = np.array(_signal(length, dt, seed=50))
    want = run(gpu, pl, x)
    out = np.zeros(pl.out_len, _ndt(dt))
    host = getattr(gpu, f"conv_{dt}_with_planner")
    host(x, out, pl)
    assert np.array_equal(out, want)
    with pytest.raises(gpu.PhastPanic) as e:
        host(x[:-1].copy(), out, pl)
    assert e.value.code == 3  # PHAST_ERR_PLANNER_SIZE
    with pytest.raises(gpu.PhastPanic) as e:
        host(x, out[:-1].copy(), pl)
    assert e.value.code == 2  # PHAST_ERR_LEN_MISMATCH
    lib, n = _lib.lib(), C.c_size_t
    assert getattr(lib, f"phast_conv_{dt}_with_planner")(None, n(length), out.ctypes.data_as(C.c_void_p), n(out.size), pl._h) == 16
    assert getattr(lib, f"phast_conv_{dt}_with_planner")(x.ctypes.data_as(C.c_void_p), n(length), None, n(out.size), pl._h) == 16
    d_x, d_out = torch.from_numpy(x).cuda(), torch.zeros(pl.out_len, dtype=_tdt(dt), device="cuda")
    ws = torch.empty(pl.workspace_len(1), dtype=_tdt(dt), device="cuda")
    dev = getattr(lib, f"phast_conv_{dt}_dev")
    px, po, pw = (C.c_void_p(t.data_ptr()) for t in (d_x, d_out, ws))
    assert dev(None, po, n(length), n(1), n(length), n(pl.out_len), pl._h, pw, n(ws.numel()), None) == 16
    assert dev(px, None, n(length), n(1), n(length), n(pl.out_len), pl._h, pw, n(ws.numel()), None) == 16
    assert dev(px, po, n(length), n(1), n(length), n(pl.out_len), pl._h, None, n(ws.numel()), None) == 16
    assert dev(px, po, n(length), n(1), n(length), n(pl.out_len), pl._h, pw, n(pl.workspace_min() - 1), None) == 16
    assert dev(px, po, n(length - 1), n(1), n(length), n(pl.out_len), pl._h, pw, n(ws.numel()), None) == 3
    assert dev(px, po, n(length), n(2), n(length - 1), n(pl.out_len), pl._h, pw, n(ws.numel()), None) == 16  # sig_dist < L
    assert dev(px, po, n(length), n(2), n(length), n(pl.out_len - 1), pl._h, pw, n(ws.numel()), None) == 16  # out_dist < out_len
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == 0).all()  # none of the refused calls ran
    assert "L=1000 K=33 same out=1000 B=100 S=68" in pl.describe() and pl.describe().startswith("correlate")
    assert pl.device_bytes() > 0
    st = pl.time_stages(d_x, d_out, 1, ws, reps=1)
    assert len(st) == 5 and all(v >= 0 for v in st) and np.array_equal(d_out.cpu().numpy(), want)


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_conveniences(gpu, dt):
    """fftconvolve and correlate on one device tensor: the bits of a planner with the automatic block, for every mode"""
    import torch

    length, k = 5000, 251
    x, h = _signal(length, dt, seed=60), _taps("random", k, dt)
    d_x = torch.from_numpy(np.array(x)).cuda()
    for mode in R.MODES:
        for flip, fn in ((False, gpu.fftconvolve), (True, gpu.correlate)):
            got = fn(d_x, h, mode)
            pl = planner(gpu, dt, length, h, mode, flip, 0)
            assert got.dtype == _tdt(dt) and got.shape == (pl.out_len,) and pl.block == AUTO[(length, k)]
            assert np.array_equal(got.cpu().numpy(), run(gpu, pl, x)), (mode, flip)
    got = gpu.fftconvolve(d_x, torch.from_numpy(np.array(h)).cuda(), "same")  # taps as a device tensor
    assert np.array_equal(got.cpu().numpy(), run(gpu, planner(gpu, dt, length, h, "same", False, 0), x))


def test_cpp_mirror(gpu, tmp_path):
    from phastft_amd import build

    lib = build.build()
    exe = str(tmp_path / "conv_test")
    libdir = os.path.dirname(lib)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "conv_test.cpp"), "-o", exe, "-L", libdir, "-lphastft_hip",
                        f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, "gpu"], capture_output=True, text=True)
    sys.stdout.write(r.stdout)
    assert r.returncode == 0 and "conv: ok" in r.stdout, r.stdout + r.stderr


def test_gates_keep_their_margin():
    """the gate above sits >= 2 x over the worst error measured on the MI355X over seeds 0-3"""
    budget = json.load(open(os.path.join(ROOT, "tests", "golden", "conv_error_budget.json")))
    assert len(budget["entries"]) == 2 * len(SHAPES)
    for e in budget["entries"]:
        assert conv_gate(e["dt"], e["block"]) >= 2 * e["rel"], e
