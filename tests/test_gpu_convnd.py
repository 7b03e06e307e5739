"""N-d overlap-save convolution and correlation on the MI355X (csrc/convnd.hip, csrc/planner_convnd.hpp) against
tests/convnd_reference.py, the direct sum in long double (which tests/test_convnd_cpu.py holds against scipy.signal.convolve /
correlate).

The gate is tests/test_gpu_conv.py's with tests/test_gpu_real_nd.py's substitution: 2 x tolerances.rel_gate(dt, sum_i log2 M_i)
over the tile's axes, M_i the Bluestein length of an axis that is no power of two and the packed inner length of the real (last)
axis; a tile is one N-d R2C, one complex multiply and one N-d C2R, the filter's spectrum is built in double.  The result is gated
as rel-L2 over the whole output.  A pocketfft emulation of the schedule in the working precision (tests/test_convnd_cpu.py) stays
16 x (f64) and 9.6 x (f32) under it at the small shapes; the measured worst on the device over seeds 0-3 (at least 14 x under
it in f64, 11 x in f32) is in tests/golden/convnd_error_budget.json (tests/golden/make_convnd_error_budget.py).

The shapes (L; K; B) are tests/convnd_reference.py's: the smallest that reach one tile axis (the 1-D path), K > L, Bluestein axes
with an odd last axis (groups straddle tile rows), ragged last tiles on every axis, 128 x 128 tiles on the square transpose
path, rank 3 and rank 1; B = 0 is the automatic block."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import convnd_reference as R
from tests import tolerances as tol
from tests.arena import Arena, Region
from tests.test_gpu_nd import conv_len, log2_m_sum
from tests.test_gpu_real_nd import real_inner_m

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANY_FACTOR = 2.0
CASES = [(mode, flip) for mode in R.MODES for flip in (False, True)]
BITS = [((20, 13), (5, 3), (8, 8)), ((300, 260), (31, 31), (0, 0)), ((20, 20, 20), (3, 3, 3), (8, 8, 8))]


def convnd_gate(dt: str, block) -> float:
    ms = [conv_len(b) for b in block[:-1] if b > 1] + [real_inner_m(block[-1])]
    return ANY_FACTOR * tol.rel_gate(dt, log2_m_sum(ms))


def _ndt(dt):
    return np.float64 if dt == "f64" else np.float32


def _tdt(dt):
    import torch

    return torch.float64 if dt == "f64" else torch.float32


def planner(P, dt, L, taps, mode, flip, block):
    return (P.PlannerConvNd64 if dt == "f64" else P.PlannerConvNd32)(L, taps, mode=mode, correlate=flip,
                                                                     block=None if not any(block) else block)


def run(P, pl, x, workspace=None):
    """one array through convnd_batched: the array is never written, nothing is written past out_len"""
    import torch

    d_x = torch.from_numpy(np.array(x)).cuda()
    out = torch.full((pl.out_len + 3,), 7.0, dtype=d_x.dtype, device="cuda")
    P.convnd_batched(d_x, out, pl, 1, workspace=workspace)
    assert np.array_equal(d_x.cpu().numpy(), x)
    out = out.cpu().numpy()
    assert (out[pl.out_len:] == 7.0).all()
    return out[:pl.out_len].reshape(pl.out_shape)


def rel_l2(got, want):
    want = np.asarray(want, np.longdouble)
    den = np.sqrt(np.sum(want * want))
    return float(np.sqrt(np.sum((np.asarray(got, np.longdouble) - want) ** 2)) / (den if den else 1))


def check(tag, dt, block, got, want):
    rel, gate = rel_l2(got, want), convnd_gate(dt, block)
    tol.record(tag, 0, rel, 0.0, gate, 0.0)
    print(f"{tag} {dt}: rel {rel:.3e} / {gate:.3e}")
    assert rel <= gate, (tag, dt, rel, gate)


@pytest.mark.parametrize("shape", R.SHAPES, ids=R.shape_id)
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_parity(gpu, dt, shape):
    L, K, B = shape
    for mode, flip in CASES:
        if not R.has_mode(L, K, mode):
            with pytest.raises(gpu.PhastPanic) as e:
                planner(gpu, dt, L, R.taps(K, _ndt(dt)), mode, flip, B)
            assert e.value.code == 16
            continue
        x, h, want = R.expected(L, K, np.dtype(_ndt(dt)).name, mode, flip)
        pl = planner(gpu, dt, L, h, mode, flip, B)
        block = tuple(b or a for b, a in zip(B, R.auto_block(L, K, mode)))
        tiles = int(np.prod([-(-o // (b - k + 1)) for o, b, k in zip(want.shape, block, K)]))
        assert (pl.out_shape, pl.out_len, pl.block, pl.tiles) == (want.shape, want.size, block, tiles), (shape, mode)
        check(f"convnd:{R.shape_id(shape)}:{mode}:{int(flip)}", dt, block, run(gpu, pl, x), want)


@pytest.mark.parametrize("shape", BITS, ids=R.shape_id)
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_bits_do_not_depend_on_how_a_call_is_made(gpu, dt, shape):
    """batch 3 at padded distances on bases one element past a 16-byte boundary, in the smallest workspace, one of two tiles and
    one element on an unaligned base, and the full one; on a second stream; captured in a graph and replayed after the planner
    has served another call: the bits of the array alone.  The sentinel in the gaps and past the end stays, the arrays are not
    written."""
    import torch

    L, K, B = shape
    batch = 3
    for mode, flip in (("full", False), ("same", True), ("valid", False)):
        pl = planner(gpu, dt, L, R.taps(K, _ndt(dt)), mode, flip, B)
        n, length = pl.out_len, pl.signal_len
        sig_dist, out_dist = (length + 5) | 1, (n + 3) | 1
        xs = [R.array(L, _ndt(dt), seed=20 + i) for i in range(batch)]
        alone = [run(gpu, pl, x).reshape(-1) for x in xs]
        buf = torch.full((1 + batch * sig_dist + 4,), 9.0, dtype=_tdt(dt), device="cuda")
        sig = buf[1:]
        assert sig.data_ptr() % 16 == np.dtype(_ndt(dt)).itemsize
        for i in range(batch):
            sig[i * sig_dist:i * sig_dist + length] = torch.from_numpy(xs[i].reshape(-1))
        keep = buf.cpu().numpy()
        vec = 16 // np.dtype(_ndt(dt)).itemsize
        per = pl.workspace_min() - (vec - 1)
        assert pl.workspace_len(batch) == batch * pl.tiles * per + vec - 1 and pl.workspace_len(1) == pl.tiles * per + vec - 1
        side = torch.cuda.Stream()
        for name, size in {"one tile": pl.workspace_min(), "two tiles + 1": 2 * per + vec, "everything": pl.workspace_len(batch),
                           "second stream": pl.workspace_len(batch)}.items():
            ws = torch.empty(size + 1, dtype=_tdt(dt), device="cuda")[1:] if name == "two tiles + 1" else \
                torch.empty(size, dtype=_tdt(dt), device="cuda")
            out = torch.full((1 + batch * out_dist + 4,), 9.0, dtype=_tdt(dt), device="cuda")
            torch.cuda.synchronize()
            with torch.cuda.stream(side if name == "second stream" else torch.cuda.current_stream()):
                gpu.convnd_batched(sig, out[1:], pl, batch, sig_dist=sig_dist, out_dist=out_dist, workspace=ws)
            torch.cuda.synchronize()
            assert np.array_equal(buf.cpu().numpy(), keep), name  # the arrays and their gaps are not written
            got = out.cpu().numpy()
            assert got[0] == 9.0 and (got[1 + (batch - 1) * out_dist + n:] == 9.0).all(), name
            for i in range(batch):
                at = 1 + i * out_dist
                assert np.array_equal(got[at:at + n], alone[i]), (mode, name, i)
                if i + 1 < batch:
                    assert (got[at + n:at + out_dist] == 9.0).all(), (mode, name, i)
        with pytest.raises(gpu.PhastPanic) as e:  # less than one tile: refused, not run
            gpu.convnd_batched(sig, torch.empty(batch * out_dist, dtype=_tdt(dt), device="cuda"), pl, batch, sig_dist=sig_dist,
                               out_dist=out_dist, workspace=torch.empty(pl.workspace_min() - 1, dtype=_tdt(dt), device="cuda"))
        assert e.value.code == 16
        # a call captured on the side stream, replayed on new data after the planner has served another call
        d_x = torch.from_numpy(xs[0].reshape(-1)).cuda()
        out = torch.zeros(n, dtype=_tdt(dt), device="cuda")
        work = torch.empty(pl.workspace_len(1), dtype=_tdt(dt), device="cuda")
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):  # warm-up on the capture stream
            gpu.convnd_batched(d_x, out, pl, 1, workspace=work)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            gpu.convnd_batched(d_x, out, pl, 1, workspace=work)
        for i in (1, 2):
            assert np.array_equal(run(gpu, pl, xs[i]).reshape(-1), alone[i])  # the other call
            d_x.copy_(torch.from_numpy(xs[i].reshape(-1)))
            out.zero_()
            g.replay()
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy(), alone[i]), (mode, "graph", i)


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_two_streams_share_one_planner(gpu, dt):
    """two streams, each with its own workspace and output, interleaved on one planner: the single-stream bits"""
    import torch

    L, K, B = (300, 260), (31, 31), (0, 0)
    pl = planner(gpu, dt, L, R.taps(K, _ndt(dt)), "same", False, B)
    xs = [R.array(L, _ndt(dt), seed=30 + i) for i in range(2)]
    want = [run(gpu, pl, x).reshape(-1) for x in xs]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in range(2)]
    d_x = [torch.from_numpy(x.reshape(-1)).cuda() for x in xs]
    outs = [torch.zeros(pl.out_len, dtype=_tdt(dt), device="cuda") for _ in range(2)]
    work = [torch.empty(pl.workspace_len(1), dtype=_tdt(dt), device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    for _ in range(3):
        for i, s in enumerate(streams):
            with torch.cuda.stream(s):
                gpu.convnd_batched(d_x[i], outs[i], pl, 1, workspace=work[i])
    torch.cuda.synchronize()
    for i in range(2):
        assert np.array_equal(outs[i].cpu().numpy(), want[i])


@pytest.mark.parametrize("shape", [((10, 11), (4, 5), (6, 17)), ((300, 260), (31, 31), (0, 0)), ((20, 20, 20), (3, 3, 3), (8, 8, 8))],
                         ids=R.shape_id)
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_guarded_poisoned_workspace(gpu, dt, shape):
    """array, output and workspace packed in one guarded arena, the workspace NaN-poisoned, at workspace_min() and at the full
    length: no band changes, the array keeps its bytes, no NaN reaches the output, the bits are those of a plain call"""
    import torch

    L, K, B = shape
    x = R.array(L, _ndt(dt), seed=70)
    pl = planner(gpu, dt, L, R.taps(K, _ndt(dt)), "full", True, B)
    want = run(gpu, pl, x).reshape(-1)
    m = max(conv_len(b) for b in pl.block)
    for size in (pl.workspace_min(), pl.workspace_len(1)):
        for off in (0, 1):
            arena = Arena(_tdt(dt), [Region("signal", pl.signal_len, off, "data", x), Region("out", pl.out_len, off, "sentinel"),
                                     Region("work", size, off, "poison")], m=m, device="cuda")
            before = arena.bytes_of("signal").clone()
            gpu.convnd_batched(arena["signal"], arena["out"], pl, 1, workspace=arena["work"])
            torch.cuda.synchronize()
            assert arena.check() == [], (size, off, arena.check())
            assert bool((arena.bytes_of("signal") == before).all())
            assert np.array_equal(arena["out"].cpu().numpy(), want), (size, off)


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_host_forms_and_codes(gpu, dt):
    """host slices give the _dev bits; a wrong length, a null pointer and a too-small workspace come back as codes"""
    import ctypes as C

    import torch

    from phastft_amd import _lib

    L, K, B = (20, 13), (5, 3), (8, 8)
    length = 260
    pl = planner(gpu, dt, L, R.taps(K, _ndt(dt)), "same", True, B)
    x = R.array(L, _ndt(dt), seed=50)
    want = run(gpu, pl, x)
    out = np.zeros(pl.out_shape, _ndt(dt))
    host = getattr(gpu, f"convnd_{dt}_with_planner")
    host(x, out, pl)
    assert np.array_equal(out, want)
    flat, oflat = x.reshape(-1), out.reshape(-1)
    with pytest.raises(gpu.PhastPanic) as e:
        host(flat[:-1].copy(), oflat, pl)
    assert e.value.code == 3  # PHAST_ERR_PLANNER_SIZE
    with pytest.raises(gpu.PhastPanic) as e:
        host(flat, oflat[:-1].copy(), pl)
    assert e.value.code == 2  # PHAST_ERR_LEN_MISMATCH
    lib, n = _lib.lib(), C.c_size_t
    assert getattr(lib, f"phast_convnd_{dt}_with_planner")(None, n(length), oflat.ctypes.data_as(C.c_void_p), n(out.size), pl._h) == 16
    assert getattr(lib, f"phast_convnd_{dt}_with_planner")(flat.ctypes.data_as(C.c_void_p), n(length), None, n(out.size), pl._h) == 16
    d_x, d_out = torch.from_numpy(flat).cuda(), torch.zeros(pl.out_len, dtype=_tdt(dt), device="cuda")
    ws = torch.empty(pl.workspace_len(1), dtype=_tdt(dt), device="cuda")
    dev = getattr(lib, f"phast_convnd_{dt}_dev")
    px, po, pw = (C.c_void_p(t.data_ptr()) for t in (d_x, d_out, ws))
    assert dev(None, po, n(length), n(1), n(length), n(pl.out_len), pl._h, pw, n(ws.numel()), None) == 16
    assert dev(px, None, n(length), n(1), n(length), n(pl.out_len), pl._h, pw, n(ws.numel()), None) == 16
    assert dev(px, po, n(length), n(1), n(length), n(pl.out_len), pl._h, None, n(ws.numel()), None) == 16
    assert dev(px, po, n(length), n(1), n(length), n(pl.out_len), pl._h, pw, n(pl.workspace_min() - 1), None) == 16
    assert dev(px, po, n(length - 1), n(1), n(length), n(pl.out_len), pl._h, pw, n(ws.numel()), None) == 3
    assert dev(px, po, n(length), n(2), n(length - 1), n(pl.out_len), pl._h, pw, n(ws.numel()), None) == 16  # sig_dist < prod L
    assert dev(px, po, n(length), n(2), n(length), n(pl.out_len - 1), pl._h, pw, n(ws.numel()), None) == 16  # out_dist < prod out
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == 0).all()  # none of the refused calls ran
    text = pl.describe()
    assert text.startswith("correlate nd L=[20x13] K=[5x3] same out=[20x13] B=[8x8] S=[4x6] tiles=[5x3]"), text
    assert pl.device_bytes() > 0
    dims = (C.c_size_t * 3)()
    assert getattr(lib, f"phast_planner_convnd{dt[1:]}_out_dims")(pl._h, dims, n(3)) == 16  # the planner's rank is 2
    st = pl.time_stages(d_x, d_out, 1, ws, reps=1)
    assert len(st) == 5 and all(v >= 0 for v in st) and np.array_equal(d_out.cpu().numpy(), want.reshape(-1))


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_conveniences(gpu, dt):
    """fftconvolve_nd and correlate_nd on one device tensor: a new tensor of the output's shape with the bits of a planner with
    the automatic block, and scipy.signal.fftconvolve / correlate of the same data in double within the gate (scipy's own
    error in double, a few 1e-16, is far below either gate)"""
    import scipy.signal as ss
    import torch

    for L, K in (((100, 130), (9, 9)), ((33, 17, 40), (5, 1, 7)), ((1000,), (33,))):
        x, h = R.array(L, _ndt(dt), seed=60), R.taps(K, _ndt(dt))
        d_x = torch.from_numpy(x).cuda()
        for mode in R.MODES:
            for flip, fn, ref in ((False, gpu.fftconvolve_nd, ss.fftconvolve), (True, gpu.correlate_nd, ss.correlate)):
                got = fn(d_x, h, mode)
                pl = planner(gpu, dt, L, h, mode, flip, (0,) * len(L))
                assert got.dtype == _tdt(dt) and tuple(got.shape) == pl.out_shape and pl.block == R.auto_block(L, K, mode)
                assert np.array_equal(got.cpu().numpy(), run(gpu, pl, x)), (L, mode, flip)
                want = ref(x.astype(np.float64), h.astype(np.float64), mode=mode)
                check(f"convnd:scipy:{L}:{mode}:{int(flip)}", dt, pl.block, got.cpu().numpy(), want)
    got = gpu.fftconvolve_nd(d_x, torch.from_numpy(h).cuda(), "same")  # taps as a device tensor
    assert np.array_equal(got.cpu().numpy(), run(gpu, planner(gpu, dt, L, h, "same", False, (0,)), x))
    y = torch.from_numpy(R.array((6, 4), _ndt(dt))).cuda()
    assert tuple(gpu.fftconvolve(y, np.ones(3, _ndt(dt))).shape) == (26,)  # the 1-D convenience still flattens


def test_gates_keep_their_margin():
    """the gate above sits >= 2 x over the worst error measured on the MI355X over seeds 0-3"""
    budget = json.load(open(os.path.join(ROOT, "tests", "golden", "convnd_error_budget.json")))
    assert [(e["dt"], e["shape"]) for e in budget["entries"]] == [(dt, R.shape_id(s)) for dt in ("f64", "f32") for s in R.SHAPES]
    for e in budget["entries"]:
        assert convnd_gate(e["dt"], tuple(e["block"])) >= 2 * e["rel"], e


def test_cpp_mirror(gpu, tmp_path):
    from phastft_amd import build

    lib = build.build()
    exe = str(tmp_path / "convnd_test")
    libdir = os.path.dirname(lib)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "convnd_test.cpp"), "-o", exe, "-L", libdir, "-lphastft_hip",
                        f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, "gpu"], capture_output=True, text=True)
    sys.stdout.write(r.stdout)
    assert r.returncode == 0 and "convnd: ok" in r.stdout, r.stdout + r.stderr
