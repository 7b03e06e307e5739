"""Multi-dimensional real transforms on the MI355X (R2C / C2R over every axis: csrc/planner_nd.hpp), against numpy's rfftn /
irfftn in long double (float64 for the arrays of 2^21 points and more).

Gates: as tests/test_gpu_nd.py, with the inner M of the packed last axis (PlannerR2cAny's convolution length; N / 2 for a
power of two, 1 for N <= 2) in the sum of log2 M_i.  The measured worst over seeds 0-3 is in tests/golden/nd_error_budget.json
(kind r2c / c2r)."""
import json
import os

import numpy as np
import pytest

from tests import tolerances as tol
from tests.test_gpu_nd import LONG_DOUBLE_MAX, ND_FACTOR, ROUNDTRIP, conv_len, log2_m_sum

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(64, 64), (1000, 1000), (1009, 17), (17, 1009), (3, 5, 7), (2, 3, 4, 6), (65, 63), (1 << 20, 3), (3, 1 << 20),
          (1, 1000, 1), (1000, 1), (7, 2), (5, 1), (9, 1024), (17, 1 << 16), (1, 1, 999)]
LARGE = {"f64": [(4096, 4096)], "f32": [(256, 256, 256)]}


def real_inner_m(n: int) -> int:
    if n <= 2:
        return 1
    if n & (n - 1) == 0:
        return n // 2
    return conv_len(n // 2) if n % 2 == 0 else conv_len(n)


def real_gates(dt: str, shape):
    ms = [conv_len(n) for n in shape[:-1] if n > 1] + [real_inner_m(shape[-1])]
    s = log2_m_sum(ms)
    return ND_FACTOR * tol.rel_gate(dt, s), ND_FACTOR * tol.bin_gate(dt, s)


def _real(shape, dt, seed=0):
    n = int(np.prod(shape))
    rng = np.random.default_rng([seed, n, len(shape), 7])
    return rng.uniform(-1, 1, n).astype(np.float64 if dt == "f64" else np.float32)


def _wide(shape):
    return np.float64 if int(np.prod(shape)) >= LONG_DOUBLE_MAX else np.longdouble


def _spectrum(shape, dt, seed=0):
    """a Hermitian half spectrum: rfftn of a real array, rounded to dt"""
    x = _real(shape, dt, seed + 100).astype(np.float64)
    X = np.fft.rfftn(x.reshape(shape)).reshape(-1)
    t = np.float64 if dt == "f64" else np.float32
    return X.real.astype(t), X.imag.astype(t)


def _planner(P, dt, shape):
    return (P.PlannerR2cNd64 if dt == "f64" else P.PlannerR2cNd32)(shape)


def _half(shape):
    return int(np.prod(shape[:-1], dtype=np.int64)) * (shape[-1] // 2 + 1)


def _dev_r2c(P, x, planner, **kw):
    import torch

    d_x = torch.from_numpy(x.copy()).cuda()
    h = planner.half
    o_re = torch.zeros(h, dtype=d_x.dtype, device="cuda")
    o_im = torch.zeros_like(o_re)
    P.r2c_nd_batched(d_x, o_re, o_im, planner, **kw)
    return o_re.cpu().numpy(), o_im.cpu().numpy()


def _dev_c2r(P, re, im, planner, **kw):
    import torch

    d_re, d_im = torch.from_numpy(re.copy()).cuda(), torch.from_numpy(im.copy()).cuda()
    out = torch.zeros(planner.n, dtype=d_re.dtype, device="cuda")
    P.c2r_nd_batched(d_re, d_im, out, planner, **kw)
    return out.cpu().numpy()


def _check(tag, dt, shape, got_re, got_im, ref_re, ref_im):
    r, i = np.asarray(ref_re, np.float64), np.asarray(ref_im, np.float64)
    rel, worst = tol.rel_l2(got_re, got_im, r, i), tol.max_bin_err(got_re, got_im, r, i)
    g_rel, g_bin = real_gates(dt, shape)
    tol.record(tag, 0, rel, worst, g_rel, g_bin)
    assert rel <= g_rel and worst <= g_bin, (tag, dt, shape, rel, g_rel, worst, g_bin)


def ref_r2c(x, shape):
    X = np.fft.rfftn(x.astype(_wide(shape)).reshape(shape)).reshape(-1)
    return X.real, X.imag


def ref_c2r(re, im, shape):
    t = _wide(shape)
    X = (re.astype(t) + 1j * im.astype(t)).reshape(shape[:-1] + (shape[-1] // 2 + 1,))
    return np.fft.irfftn(X, s=shape, axes=list(range(len(shape)))).reshape(-1)


def _cases():
    for dt in ("f64", "f32"):
        for shape in SHAPES + LARGE[dt]:
            yield dt, shape


IDS = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v  # noqa: E731


@pytest.mark.parametrize("dt,shape", list(_cases()), ids=IDS)
def test_r2c_matches_rfftn(gpu, dt, shape):
    x = _real(shape, dt, seed=1)
    g_re, g_im = _dev_r2c(gpu, x, _planner(gpu, dt, shape))
    _check(f"r2c_nd:{shape}", dt, shape, g_re, g_im, *ref_r2c(x, shape))


@pytest.mark.parametrize("dt,shape", list(_cases()), ids=IDS)
def test_c2r_matches_irfftn(gpu, dt, shape):
    re, im = _spectrum(shape, dt, seed=1)
    got = _dev_c2r(gpu, re, im, _planner(gpu, dt, shape))
    ref = ref_c2r(re, im, shape)
    _check(f"c2r_nd:{shape}", dt, shape, got, np.zeros_like(got), ref, np.zeros_like(ref))


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("shape,n", [((1, 1000), 1000), ((1, 1, 999), 999), ((1, 4096), 4096)], ids=IDS)
def test_one_axis_is_the_any_length_call(gpu, dt, shape, n):
    import torch

    batch, in_dist, out_dist = 3, n + 4, n // 2 + 3
    x = _real((batch * in_dist,), dt, seed=2)
    d_x = torch.from_numpy(x).cuda()
    outs = []
    for nd in (True, False):
        o_re = torch.zeros((batch - 1) * out_dist + n // 2 + 1, dtype=d_x.dtype, device="cuda")
        o_im = torch.zeros_like(o_re)
        if nd:
            gpu.r2c_nd_batched(d_x, o_re, o_im, _planner(gpu, dt, shape), batch=batch, in_dist=in_dist, out_dist=out_dist)
        else:
            pl = (gpu.PlannerR2cAny64 if dt == "f64" else gpu.PlannerR2cAny32)(n)
            gpu.r2c_any_batched(d_x, o_re, o_im, pl, batch, in_dist, out_dist)
        outs.append((o_re, o_im))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


BITS_SHAPES = [(64, 64), (1009, 17), (3, 5, 7), (9, 1024), (1000, 1), (4, 2)]


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("shape", BITS_SHAPES, ids=IDS)
def test_bits_do_not_depend_on_the_call(gpu, dt, shape):
    """batch of 3 at distances above the array, the minimum workspace, the host-slice form and a second stream: the bits of
    single _dev calls, for R2C and C2R"""
    import torch

    n, h = int(np.prod(shape)), _half(shape)
    pl = _planner(gpu, dt, shape)
    tdt = torch.float64 if dt == "f64" else torch.float32
    xs = [_real(shape, dt, seed=20 + b) for b in range(3)]
    specs = [_spectrum(shape, dt, seed=20 + b) for b in range(3)]
    want_f = [_dev_r2c(gpu, x, pl) for x in xs]
    want_b = [_dev_c2r(gpu, re, im, pl) for re, im in specs]
    rd, cd = n + 5, h + 3
    for ws in (None, torch.empty(pl.workspace_len(1), dtype=tdt, device="cuda")):
        d_x = torch.zeros(2 * rd + n, dtype=tdt, device="cuda")
        for b in range(3):
            d_x[b * rd:b * rd + n] = torch.from_numpy(xs[b])
        o_re = torch.zeros(2 * cd + h, dtype=tdt, device="cuda")
        o_im = torch.zeros_like(o_re)
        gpu.r2c_nd_batched(d_x, o_re, o_im, pl, batch=3, in_dist=rd, out_dist=cd, workspace=ws)
        for b in range(3):
            assert np.array_equal(o_re[b * cd:b * cd + h].cpu().numpy(), want_f[b][0]), (ws is None, b)
            assert np.array_equal(o_im[b * cd:b * cd + h].cpu().numpy(), want_f[b][1]), (ws is None, b)
        i_re = torch.zeros(2 * cd + h, dtype=tdt, device="cuda")
        i_im = torch.zeros_like(i_re)
        for b in range(3):
            i_re[b * cd:b * cd + h] = torch.from_numpy(specs[b][0])
            i_im[b * cd:b * cd + h] = torch.from_numpy(specs[b][1])
        out = torch.zeros(2 * rd + n, dtype=tdt, device="cuda")
        gpu.c2r_nd_batched(i_re, i_im, out, pl, batch=3, in_dist=cd, out_dist=rd, workspace=ws)
        for b in range(3):
            assert np.array_equal(out[b * rd:b * rd + n].cpu().numpy(), want_b[b]), (ws is None, b)
    ndt = np.float64 if dt == "f64" else np.float32
    o_re, o_im = np.zeros(h, ndt), np.zeros(h, ndt)
    (gpu.r2c_fft_f64_nd_with_planner if dt == "f64" else gpu.r2c_fft_f32_nd_with_planner)(xs[0], o_re, o_im, pl)
    assert np.array_equal(o_re, want_f[0][0]) and np.array_equal(o_im, want_f[0][1])
    (gpu.r2c_fft_f64_nd if dt == "f64" else gpu.r2c_fft_f32_nd)(xs[1], o_re, o_im, shape)
    assert np.array_equal(o_re, want_f[1][0]) and np.array_equal(o_im, want_f[1][1])
    out = np.zeros(n, ndt)
    (gpu.c2r_fft_f64_nd_with_planner if dt == "f64" else gpu.c2r_fft_f32_nd_with_planner)(*specs[0], out, pl)
    assert np.array_equal(out, want_b[0])
    (gpu.c2r_fft_f64_nd if dt == "f64" else gpu.c2r_fft_f32_nd)(*specs[1], out, shape)
    assert np.array_equal(out, want_b[1])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got_f = _dev_r2c(gpu, xs[2], pl)
        got_b = _dev_c2r(gpu, *specs[2], pl)
    torch.cuda.synchronize()
    assert np.array_equal(got_f[0], want_f[2][0]) and np.array_equal(got_f[1], want_f[2][1])
    assert np.array_equal(got_b, want_b[2])


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_graph_replay(gpu, dt):
    import torch

    shape = (1009, 17)
    pl = _planner(gpu, dt, shape)
    x = _real(shape, dt, seed=4)
    want = _dev_r2c(gpu, x, pl)
    src = torch.from_numpy(x).cuda()
    d_x = src.clone()
    o_re = torch.zeros(pl.half, dtype=src.dtype, device="cuda")
    o_im = torch.zeros_like(o_re)
    work = torch.empty(pl.workspace_len(1), dtype=src.dtype, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        gpu.r2c_nd_batched(d_x, o_re, o_im, pl, workspace=work)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        d_x.copy_(src)
        gpu.r2c_nd_batched(d_x, o_re, o_im, pl, workspace=work)
    for _ in range(2):
        o_re.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(o_re.cpu().numpy(), want[0]) and np.array_equal(o_im.cpu().numpy(), want[1])


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("shape", [(64, 64), (65, 63), (1000, 3), (3, 1001)], ids=IDS)
def test_unaligned_views(gpu, dt, shape):
    import torch

    n, h = int(np.prod(shape)), _half(shape)
    pl = _planner(gpu, dt, shape)
    x = _real(shape, dt, seed=5)
    re, im = _spectrum(shape, dt, seed=5)
    want_f, want_b = _dev_r2c(gpu, x, pl), _dev_c2r(gpu, re, im, pl)
    tdt = torch.float64 if dt == "f64" else torch.float32
    for off in (1, 3):
        d_x = torch.zeros(n + off, dtype=tdt, device="cuda")[off:]
        d_x.copy_(torch.from_numpy(x))
        o_re = torch.zeros(h + off, dtype=tdt, device="cuda")[off:]
        o_im = torch.zeros(h + off, dtype=tdt, device="cuda")[off:]
        gpu.r2c_nd_batched(d_x, o_re, o_im, pl)
        assert np.array_equal(o_re.cpu().numpy(), want_f[0]) and np.array_equal(o_im.cpu().numpy(), want_f[1]), off
        i_re = torch.zeros(h + off, dtype=tdt, device="cuda")[off:]
        i_im = torch.zeros(h + off, dtype=tdt, device="cuda")[off:]
        i_re.copy_(torch.from_numpy(re))
        i_im.copy_(torch.from_numpy(im))
        out = torch.zeros(n + off, dtype=tdt, device="cuda")[off:]
        gpu.c2r_nd_batched(i_re, i_im, out, pl)
        assert np.array_equal(out.cpu().numpy(), want_b), off


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("shape", [(1000, 1000), (3, 5, 7), (1 << 20, 3), (9, 1024), (5, 1)], ids=IDS)
def test_round_trip_and_read_only_inputs(gpu, dt, shape):
    """R2C -> C2R returns the input; R2C leaves its input and C2R its input planes bit-unchanged"""
    import torch

    pl = _planner(gpu, dt, shape)
    x = _real(shape, dt, seed=6)
    d_x = torch.from_numpy(x.copy()).cuda()
    o_re = torch.zeros(pl.half, dtype=d_x.dtype, device="cuda")
    o_im = torch.zeros_like(o_re)
    gpu.r2c_nd_batched(d_x, o_re, o_im, pl)
    assert np.array_equal(d_x.cpu().numpy(), x)
    keep_re, keep_im = o_re.clone(), o_im.clone()
    out = torch.zeros_like(d_x)
    gpu.c2r_nd_batched(o_re, o_im, out, pl)
    assert torch.equal(o_re, keep_re) and torch.equal(o_im, keep_im)
    err = float(np.abs(out.cpu().numpy().astype(np.float64) - x).max())
    assert err <= ROUNDTRIP[dt], err


def test_gates_keep_their_margin():
    budget = json.load(open(os.path.join(ROOT, "tests", "golden", "nd_error_budget.json")))
    entries = [e for e in budget["entries"] if e["kind"] in ("r2c", "c2r")]
    assert entries
    for e in entries:
        g_rel, g_bin = real_gates(e["dt"], tuple(e["shape"]))
        assert g_rel >= 3.7 * e["rel"] and g_bin >= 3.7 * e["bin"], e


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("shape", [(64, 64), (1009, 17)], ids=IDS)
def test_r2c_needs_one_copy_less(gpu, dt, shape):
    """R2C runs in one transposed copy: workspace_len(1) less one copy of the half spectrum works with the same bits; C2R
    needs two copies and refuses a workspace of one"""
    import torch

    pl = _planner(gpu, dt, shape)
    tdt = torch.float64 if dt == "f64" else torch.float32
    short = torch.empty(pl.workspace_len(1) - 2 * pl.half, dtype=tdt, device="cuda")
    x = _real(shape, dt, seed=8)
    assert all(np.array_equal(a, b) for a, b in zip(_dev_r2c(gpu, x, pl, workspace=short), _dev_r2c(gpu, x, pl)))
    re, im = _spectrum(shape, dt, seed=8)
    one_copy = torch.empty(2 * pl.half, dtype=tdt, device="cuda")
    with pytest.raises(gpu.PhastPanic):
        _dev_c2r(gpu, re, im, pl, workspace=one_copy)
