"""Multi-dimensional complex transforms on the MI355X (csrc/nd.hip, csrc/planner_nd.hpp): every axis of a row-major array,
against numpy's fftn / ifftn in long double (complex128 for the arrays of 2^21 points and more).

Gates: tests/tolerances.py's formulas with log2 N replaced by the sum of log2 M_i over the transformed axes (M_i = n_i for a
power of two, the Bluestein convolution length otherwise), times the any-length factor 2.  The measured worst over seeds 0-3
(tests/golden/nd_error_budget.json, written on the MI355X by tests/golden/make_nd_error_budget.py) sits at least 3.7 x below
them (test_gates_keep_their_margin)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import tolerances as tol

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ND_FACTOR = 2.0
SHAPES = [(64, 64), (1000, 1000), (1009, 17), (3, 5, 7), (2, 3, 4, 5), (3, 1, 4, 1, 5), (65, 63), (1 << 20, 3), (3, 1 << 20),
          (1, 1000, 1), (17, 1 << 16)]
LARGE = {"f64": [(4096, 4096)], "f32": [(256, 256, 256)]}
LONG_DOUBLE_MAX = 1 << 21  # points: above, the reference is complex128 (its error is far below the gates)
# round trips, absolute on inputs in [-1, 1): tolerances.py's constants, f32 times 5 as the parity tests' f32 round trips --
# the largest error of an f32 round trip of 3 x 2^20 points (Bluestein rows of 3, 2^20-point columns) is 2.9e-6
ROUNDTRIP = {"f64": tol.ROUNDTRIP_ABS["f64"], "f32": 5 * tol.ROUNDTRIP_ABS["f32"]}


def conv_len(n: int) -> int:
    return n if n & (n - 1) == 0 else 1 << (2 * n - 2).bit_length()


def log2_m_sum(ms) -> int:
    return sum(m.bit_length() - 1 for m in ms)


def nd_gates(dt: str, shape):
    s = log2_m_sum(conv_len(n) for n in shape if n > 1)
    return ND_FACTOR * tol.rel_gate(dt, s), ND_FACTOR * tol.bin_gate(dt, s)


def _input(shape, dt: str, seed: int = 0, count: int | None = None):
    n = int(np.prod(shape)) if count is None else count
    rng = np.random.default_rng([seed, n, len(shape)])
    ndt = np.float64 if dt == "f64" else np.float32
    return rng.uniform(-1, 1, n).astype(ndt), rng.uniform(-1, 1, n).astype(ndt)


def _ref(re, im, shape, direction: int):
    wide = int(np.prod(shape)) >= LONG_DOUBLE_MAX
    t = np.float64 if wide else np.longdouble
    z = (re.astype(t) + 1j * im.astype(t)).reshape(shape)
    out = np.fft.fftn(z) if direction == 1 else np.fft.ifftn(z)
    return out.reshape(-1)


def _errors(got_re, got_im, ref):
    r, i = np.asarray(ref.real, np.float64), np.asarray(ref.imag, np.float64)
    return tol.rel_l2(got_re, got_im, r, i), tol.max_bin_err(got_re, got_im, r, i)


def _check(tag, dt, shape, got_re, got_im, ref):
    rel, worst = _errors(got_re, got_im, ref)
    g_rel, g_bin = nd_gates(dt, shape)
    tol.record(tag, log2_m_sum(conv_len(n) for n in shape if n > 1), rel, worst, g_rel, g_bin)
    assert rel <= g_rel and worst <= g_bin, (tag, dt, shape, rel, g_rel, worst, g_bin)


def _planner(P, dt, shape):
    return (P.PlannerNd64 if dt == "f64" else P.PlannerNd32)(shape)


def _dev_fft(P, dt, re, im, direction, planner, **kw):
    import torch

    d_re, d_im = torch.from_numpy(re.copy()).cuda(), torch.from_numpy(im.copy()).cuda()
    P.fft_nd_batched(d_re, d_im, P.Direction(direction), planner, **kw)
    return d_re.cpu().numpy(), d_im.cpu().numpy()


def _cases():
    for dt in ("f64", "f32"):
        for shape in SHAPES + LARGE[dt]:
            yield dt, shape


@pytest.mark.parametrize("direction", [1, -1])
@pytest.mark.parametrize("dt,shape", list(_cases()), ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_shapes_match_numpy(gpu, dt, shape, direction):
    re, im = _input(shape, dt, seed=1)
    pl = _planner(gpu, dt, shape)
    g_re, g_im = _dev_fft(gpu, dt, re, im, direction, pl)
    _check(f"nd:{shape}", dt, shape, g_re, g_im, _ref(re, im, shape, direction))


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_every_narrow_side_matches_numpy(gpu, dt):
    """(512, S) for EVERY narrow side S = 2 .. TS - 1 (TS = 32 f64, 64 f32) through the real narrow transposes: one forward call runs
    the narrow-C transpose and the narrow-R transpose back, and 512 is no multiple of any span, so the last tile of each is ragged.
    Once with aligned planes (16-byte accesses on both sides where S allows) and once as a batch of 2 at an odd distance in planes one
    element off a 16-byte boundary (element accesses).  The host emulation (tests/test_block_emulator.py) checks every index of
    these kernels but computes the f32 reciprocal quotients of nd.hip's fdiv with the HOST's 1.0f / d: this is the check with the
    device's own.  The gate is the module's (nd_gates against numpy in long double); a misplaced element is an error of O(1).
    A shape list of its own: SHAPES feeds the error-budget file."""
    import torch

    tdt = torch.float64 if dt == "f64" else torch.float32
    for s in range(2, 32 if dt == "f64" else 64):
        shape, n = (512, s), 512 * s
        pl = _planner(gpu, dt, shape)
        arrays = [_input(shape, dt, seed=20 + b) for b in range(2)]
        refs = [_ref(re, im, shape, 1) for re, im in arrays]
        g_re, g_im = _dev_fft(gpu, dt, *arrays[0], 1, pl)
        _check(f"nd-narrow:{shape}", dt, shape, g_re, g_im, refs[0])
        dist = (n + 1) | 1
        b_re = torch.zeros(1 + dist + n, dtype=tdt, device="cuda")
        b_im = torch.zeros_like(b_re)
        v_re, v_im = b_re[1:], b_im[1:]
        for b, (re, im) in enumerate(arrays):
            v_re[b * dist:b * dist + n] = torch.from_numpy(re)
            v_im[b * dist:b * dist + n] = torch.from_numpy(im)
        gpu.fft_nd_batched(v_re, v_im, gpu.Direction.Forward, pl, batch=2, dist=dist)
        for b in range(2):
            _check(f"nd-narrow-off:{shape}[{b}]", dt, shape, v_re[b * dist:b * dist + n].cpu().numpy(), v_im[b * dist:b * dist + n].cpu().numpy(), refs[b])
        assert float(b_re[0]) == 0.0 and float(b_re[1 + dist - 1]) == 0.0  # the lead-in and the gap between the arrays keep their zeros


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_describe_names_the_schedule(gpu, dt):
    d = _planner(gpu, dt, (1, 1000, 64)).describe()
    assert "squeezed [1000x64]" in d and "bluestein M=2048" in d and "pow2" in d, d
    assert d.count("transpose") == 2, d
    assert _planner(gpu, dt, (1, 4096)).workspace_len(1) == 0  # one pow2 axis: the one-axis path, no workspace
    assert _planner(gpu, dt, (64, 64)).workspace_len(1) == 2 * 64 * 64  # pow2 only: the transposed copy


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("shape,n", [((1, 1000, 1), 1000), ((1, 4096), 4096), ((7,), 7)])
def test_one_axis_is_the_any_length_call(gpu, dt, shape, n):
    """a shape with one axis > 1 runs phast_fft_*_any_dev: the same bits for the same batch and dist"""
    import torch

    batch, dist = 3, n + (0 if n == 4096 else 5)
    re, im = _input(shape, dt, seed=2, count=(batch - 1) * dist + n)
    a_re, a_im = torch.from_numpy(re).cuda(), torch.from_numpy(im).cuda()
    b_re, b_im = a_re.clone(), a_im.clone()
    gpu.fft_nd_batched(a_re, a_im, gpu.Direction.Forward, _planner(gpu, dt, shape), batch=batch, dist=dist)
    any_pl = (gpu.PlannerAny64 if dt == "f64" else gpu.PlannerAny32)(n)
    gpu.fft_any_batched(b_re, b_im, n, gpu.Direction.Forward, any_pl, dist=dist)
    assert torch.equal(a_re, b_re) and torch.equal(a_im, b_im)


BITS_SHAPES = [(64, 64), (1009, 17), (3, 5, 7), (65, 63), (3, 1 << 12)]


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("shape", BITS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bits_do_not_depend_on_the_call(gpu, dt, shape):
    """batch of 3 at dist > prod n, the minimum workspace (chunked), the host-slice form and a second stream: the bits of
    single _dev calls"""
    import torch

    n = int(np.prod(shape))
    pl = _planner(gpu, dt, shape)
    arrays = [_input(shape, dt, seed=10 + b) for b in range(3)]
    for direction in (1, -1):
        want = [_dev_fft(gpu, dt, re, im, direction, pl) for re, im in arrays]
        dist = n + 7
        tdt = torch.float64 if dt == "f64" else torch.float32
        for ws in (None, torch.empty(pl.workspace_len(1), dtype=tdt, device="cuda")):
            b_re = torch.zeros(2 * dist + n, dtype=tdt, device="cuda")
            b_im = torch.zeros_like(b_re)
            for b, (re, im) in enumerate(arrays):
                b_re[b * dist:b * dist + n] = torch.from_numpy(re)
                b_im[b * dist:b * dist + n] = torch.from_numpy(im)
            gpu.fft_nd_batched(b_re, b_im, gpu.Direction(direction), pl, batch=3, dist=dist, workspace=ws)
            for b in range(3):
                assert np.array_equal(b_re[b * dist:b * dist + n].cpu().numpy(), want[b][0]), (ws is None, b)
                assert np.array_equal(b_im[b * dist:b * dist + n].cpu().numpy(), want[b][1]), (ws is None, b)
        re, im = arrays[0][0].copy(), arrays[0][1].copy()
        (gpu.fft_64_nd_with_planner if dt == "f64" else gpu.fft_32_nd_with_planner)(re, im, gpu.Direction(direction), pl)
        assert np.array_equal(re, want[0][0]) and np.array_equal(im, want[0][1])
        re, im = arrays[1][0].copy(), arrays[1][1].copy()
        (gpu.fft_64_nd if dt == "f64" else gpu.fft_32_nd)(re, im, shape, gpu.Direction(direction))
        assert np.array_equal(re, want[1][0]) and np.array_equal(im, want[1][1])
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            got = _dev_fft(gpu, dt, *arrays[2], direction, pl)
        torch.cuda.synchronize()
        assert np.array_equal(got[0], want[2][0]) and np.array_equal(got[1], want[2][1])


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_graph_replay(gpu, dt):
    """one _dev call captured on a side stream, replayed twice: the eager bits"""
    import torch

    shape = (1009, 17)
    re, im = _input(shape, dt, seed=4)
    pl = _planner(gpu, dt, shape)
    want = _dev_fft(gpu, dt, re, im, 1, pl)
    src_re, src_im = torch.from_numpy(re).cuda(), torch.from_numpy(im).cuda()
    d_re, d_im = src_re.clone(), src_im.clone()
    work = torch.empty(pl.workspace_len(1), dtype=d_re.dtype, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on the capture stream
        gpu.fft_nd_batched(d_re, d_im, gpu.Direction.Forward, pl, workspace=work)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        d_re.copy_(src_re)
        d_im.copy_(src_im)
        gpu.fft_nd_batched(d_re, d_im, gpu.Direction.Forward, pl, workspace=work)
    for _ in range(2):
        d_re.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(d_re.cpu().numpy(), want[0]) and np.array_equal(d_im.cpu().numpy(), want[1])


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("shape", [(64, 64), (65, 63), (1000, 3), (3, 1000), (2, 3, 4, 5)], ids=lambda s: "x".join(map(str, s)))
def test_unaligned_views_and_odd_distances(gpu, dt, shape):
    """buf[1:] / buf[3:] views and an odd dist give the bits of aligned calls (element accesses where 16 bytes do not fit)"""
    import torch

    n = int(np.prod(shape))
    pl = _planner(gpu, dt, shape)
    re, im = _input(shape, dt, seed=5)
    want = _dev_fft(gpu, dt, re, im, 1, pl)
    tdt = torch.float64 if dt == "f64" else torch.float32
    for off in (1, 3):
        b_re = torch.zeros(n + off, dtype=tdt, device="cuda")
        b_im = torch.zeros(n + off, dtype=tdt, device="cuda")
        v_re, v_im = b_re[off:], b_im[off:]
        v_re.copy_(torch.from_numpy(re))
        v_im.copy_(torch.from_numpy(im))
        gpu.fft_nd_batched(v_re, v_im, gpu.Direction.Forward, pl)
        assert np.array_equal(v_re.cpu().numpy(), want[0]) and np.array_equal(v_im.cpu().numpy(), want[1]), off
    dist = n + 1
    b_re = torch.zeros(dist + n, dtype=tdt, device="cuda")
    b_im = torch.zeros_like(b_re)
    for b in range(2):
        b_re[b * dist:b * dist + n] = torch.from_numpy(re)
        b_im[b * dist:b * dist + n] = torch.from_numpy(im)
    gpu.fft_nd_batched(b_re, b_im, gpu.Direction.Forward, pl, batch=2, dist=dist)
    for b in range(2):
        assert np.array_equal(b_re[b * dist:b * dist + n].cpu().numpy(), want[0])
        assert np.array_equal(b_im[b * dist:b * dist + n].cpu().numpy(), want[1])


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("shape", [(1000, 1000), (3, 5, 7), (1 << 20, 3), (17, 1 << 16)], ids=lambda s: "x".join(map(str, s)))
def test_round_trip(gpu, dt, shape):
    re, im = _input(shape, dt, seed=6)
    pl = _planner(gpu, dt, shape)
    f_re, f_im = _dev_fft(gpu, dt, re, im, 1, pl)
    b_re, b_im = _dev_fft(gpu, dt, f_re, f_im, -1, pl)
    err = max(np.abs(b_re.astype(np.float64) - re).max(), np.abs(b_im.astype(np.float64) - im).max())
    assert err <= ROUNDTRIP[dt], err


def test_multi_dim_tensor_views(gpu):
    """a contiguous tensor of the array's own shape is taken by its elements"""
    import torch

    shape = (12, 10)
    re, im = _input(shape, "f64", seed=7)
    pl = _planner(gpu, "f64", shape)
    want = _dev_fft(gpu, "f64", re, im, 1, pl)
    t_re, t_im = torch.from_numpy(re.reshape(shape)).cuda(), torch.from_numpy(im.reshape(shape)).cuda()
    gpu.fft_64_nd_with_planner(t_re, t_im, gpu.Direction.Forward, pl)
    assert np.array_equal(t_re.cpu().numpy().reshape(-1), want[0])


def test_cpp_mirror(gpu, tmp_path):
    from phastft_amd import build

    lib = build.build()
    exe = str(tmp_path / "nd_test")
    libdir = os.path.dirname(lib)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "nd_test.cpp"), "-o", exe, "-L", libdir, "-lphastft_hip",
                        f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, "gpu"], capture_output=True, text=True)
    sys.stdout.write(r.stdout)
    assert r.returncode == 0 and "nd: ok" in r.stdout, r.stdout + r.stderr


def test_gates_keep_their_margin():
    """the gates sit >= 3.7 x over the worst error measured on the MI355X over seeds 0-3 (tolerances.py's rule)"""
    budget = json.load(open(os.path.join(ROOT, "tests", "golden", "nd_error_budget.json")))
    entries = [e for e in budget["entries"] if e["kind"] == "c2c"]
    assert entries
    for e in entries:
        g_rel, g_bin = nd_gates(e["dt"], tuple(e["shape"]))
        assert g_rel >= 3.7 * e["rel"] and g_bin >= 3.7 * e["bin"], e
