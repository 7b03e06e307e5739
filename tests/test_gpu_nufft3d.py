"""Three-dimensional non-uniform FFTs of types 1 and 2 on the MI355X (csrc/nufft_nd.hip, csrc/planner_nufft_nd.hpp) against
tests/nufft3d_reference.py, the direct sum in long double with exact phases, on inputs that are exact in both types.

The gate (tests/test_nufft3d_cpu.py: nufft3d_gate): C_EPS_3D * eps + tests/tolerances.py's formula on log2 G, G = g1 g2 g3, for
the rel-L2 and for the worst element / rms; C_EPS_3D comes from the numpy model of the schedule, not from the device.  The
measured worst per shape, eps, type and dtype over the seeds is in tests/golden/nufft3d_error_budget.json
(tests/golden/make_nufft3d_error_budget.py); tests/test_nufft3d_cpu.py's test_gates_keep_their_margin keeps the gates 2 x above
every entry of it.  The shapes (N1, N2, N3, M) reach one point on a grid of almost empty tiles, g = 8 on every axis (the tile's
reach is the whole ring), unequal and odd axes, grids set by 2w, a one-mode axis on every side, several tiles per axis, and the
long cell list of 2000 points within 1e-7 of (0.3, 0.7, 0.55), which spans many passes of the spread kernel through LDS.

Adjoint identity: the spread and the interpolation kernel form every kernel value the same way, (k1 k2) k3 in R, so
<nufft3d1(c), F> = <c, nufft3d2_Reverse(F)> holds to rounding.  The bound, relative to |nufft3d1(c)| |F|, is 8 x what DESIGN
section 19 records for two dimensions (3.2e-17 f64, 2.5e-8 f32, the larger of its two eps), because w times as many products
enter each sum: 2.56e-16 and 2.0e-7.  Measured on the MI355X: see DESIGN section 20."""
import functools
import json
import os

import numpy as np
import pytest

from tests import nufft3d_reference as R
from tests import tolerances as tol
from tests.test_nufft3d_cpu import nufft3d_gate, reference

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTS = ["f64", "f32"]
BUDGET = os.path.join(ROOT, "tests", "golden", "nufft3d_error_budget.json")
shape_id = R.shape_id


def _ndt(dt):
    return np.float64 if dt == "f64" else np.float32


def _tdt(dt):
    import torch

    return torch.float64 if dt == "f64" else torch.float32


def _dir(P, d):
    return P.Direction.Forward if d == R.FORWARD else P.Direction.Reverse


@functools.lru_cache(maxsize=None)
def _planner(P, dt, ns, kx, ky, kz, eps):
    cls = P.PlannerNufft3d64 if dt == "f64" else P.PlannerNufft3d32
    return cls(ns, np.frombuffer(kx, np.float64), np.frombuffer(ky, np.float64), np.frombuffer(kz, np.float64), eps)


def planner(P, dt, ns, pts, eps):
    """one planner per (type, modes (n1, n2, n3), points (x, y, z), eps), shared by the tests"""
    return _planner(P, dt, tuple(ns), *(np.ascontiguousarray(v, np.float64).tobytes() for v in pts), eps)


def run(P, pl, t, d, v, real=False, work=None, stream=None):
    """one vector (flat) through nufft3d{t}_batched: the input is never written, nothing is written past the output"""
    import torch

    dt = pl._dtype
    v = np.asarray(v).reshape(-1)
    d_re = torch.from_numpy(np.ascontiguousarray(v.real, dtype=dt)).cuda()
    d_im = None if real else torch.from_numpy(np.ascontiguousarray(v.imag, dtype=dt)).cuda()
    keep = d_re.clone(), None if real else d_im.clone()
    n_out = pl.n if t == 1 else pl.m_points
    o_re, o_im = (torch.full((n_out + 3,), 7.0, dtype=d_re.dtype, device="cuda") for _ in range(2))
    fn = P.nufft3d1_batched if t == 1 else P.nufft3d2_batched
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())  # the fills above
    got = fn(d_re, d_im, pl, _dir(P, d), out=(o_re[:n_out], o_im[:n_out]), work=work, stream=stream)
    torch.cuda.synchronize()
    assert got[0].data_ptr() == o_re.data_ptr()
    assert torch.equal(d_re, keep[0]) and (real or torch.equal(d_im, keep[1]))
    o_re, o_im = o_re.cpu().numpy(), o_im.cpu().numpy()
    assert (o_re[n_out:] == 7.0).all() and (o_im[n_out:] == 7.0).all()
    return o_re[:n_out], o_im[:n_out]


def measure(P, dt, shape, eps, t, seeds=R.SEEDS):
    """(worst rel-L2, worst element / rms) over both directions, complex and real data and the seeds"""
    ref = reference(shape)
    pl = planner(P, dt, shape[:3], (ref.x, ref.y, ref.z), eps)
    rel = worst = 0.0
    for seed in seeds:
        for d in (R.FORWARD, R.REVERSE):
            for real in (False, True):
                got = run(P, pl, t, d, ref.inp(t, real, seed), real)
                want = ref.ref[(t, d, real, seed)]
                rel, worst = max(rel, tol.rel_l2(*got, *want)), max(worst, tol.max_bin_err(*got, *want))
    return rel, worst, pl


@pytest.mark.parametrize("shape", R.SHAPES, ids=shape_id)
@pytest.mark.parametrize("dt", DTS)
def test_parity(gpu, dt, shape):
    """both types, both directions, complex and real input, seeds 0-1, at every eps of the type"""
    n1, n2, n3, m, _ = shape
    for eps in R.EPS[dt]:
        for t in (1, 2):
            rel, worst, pl = measure(gpu, dt, shape, eps, t)
            w = R.width(eps)
            gs = (R.grid(n1, w), R.grid(n2, w), R.grid(n3, w))
            assert pl.width == w and pl.grid_shape == gs and pl.grid_len == gs[0] * gs[1] * gs[2]
            assert pl.workspace_len(1) == 4 * pl.grid_len and pl.workspace_len(3) == 12 * pl.grid_len
            assert pl.n_modes == (n1, n2, n3) and pl.m_points == m and pl.n == n1 * n2 * n3
            g_rel, g_bin = nufft3d_gate(dt, pl.grid_len, eps)
            tol.record(f"nufft3d{t}:{shape_id(shape)}:{eps:g}", pl.grid_len.bit_length() - 1, rel, worst, g_rel, g_bin)
            print(f"nufft3d{t} {shape_id(shape)} {dt} eps {eps:g} w {pl.width} grid {pl.grid_shape}: rel {rel:.3e} / {g_rel:.3e}, "
                  f"element {worst:.3e} / {g_bin:.3e}")
            assert rel <= g_rel and worst <= g_bin, (shape, dt, eps, t, rel, g_rel, worst, g_bin)


ADJOINT_BOUND = {"f64": 8 * 3.2e-17, "f32": 8 * 2.5e-8}
BIT_SHAPES = [(12, 10, 9, 300, "u"), (33, 20, 7, 2000, "clump"), (70, 24, 10, 3000, "u")]


def _pair(a):
    return a.real.cpu().numpy().reshape(-1).astype(np.float64), a.imag.cpu().numpy().reshape(-1).astype(np.float64)


@pytest.mark.parametrize("dims", [(4, 4, 4), (3, 5, 2), (1, 1, 30), (6, 1, 5)], ids=lambda d: f"{d[0]}x{d[1]}x{d[2]}")
@pytest.mark.parametrize("dt", DTS)
def test_dft_special_case(gpu, dt, dims):
    """points on the grid (j1 / N1, j2 / N2, j3 / N3), M = N1 N2 N3: type 1 Forward is numpy's fftn of that array, within the gate"""
    eps = R.EPS[dt][-1]
    j = np.meshgrid(*(np.arange(n) for n in dims), indexing="ij")
    pl = planner(gpu, dt, dims, tuple((ji / n).reshape(-1) for ji, n in zip(j, dims)), eps)
    c = R.data(dims[0] * dims[1] * dims[2], 3, "c")
    got = run(gpu, pl, 1, R.FORWARD, c)
    f = np.fft.fftn(c.reshape(dims)).reshape(-1)
    want = f.real.copy(), f.imag.copy()
    rel, worst = tol.rel_l2(*got, *want), tol.max_bin_err(*got, *want)
    g_rel, g_bin = nufft3d_gate(dt, pl.grid_len, eps)
    print(f"dft {dims} {dt}: rel {rel:.3e} / {g_rel:.3e}, element {worst:.3e} / {g_bin:.3e}")
    assert rel <= g_rel and worst <= g_bin


@pytest.mark.parametrize("dt", DTS)
def test_one_mode_axes_are_the_lower_dimensional_transforms(gpu, dt):
    """N3 = 1: nufft3d1 equals the two-dimensional nufft2d1 of (x, y); N2 = N3 = 1: the one-dimensional nufft1 of x -- under the
    gate, not bitwise: the kernel of a one-mode axis and its 1 / phi^(0) are still applied"""
    import torch

    m = 500
    c = R.data(m, 5, "c")
    dev = torch.from_numpy(c.astype(np.complex128 if dt == "f64" else np.complex64)).cuda()
    for ns in ((24, 10, 1), (40, 1, 1)):
        x, y, z = R.points(*ns, m)
        for eps in R.EPS[dt]:
            a = gpu.nufft3d1(x, y, z, dev, ns, eps)
            b = gpu.nufft2d1(x, y, dev, ns[:2], eps) if ns[1] > 1 else gpu.nufft1(x, dev, ns[0], eps)
            assert a.shape == ns and b.shape == (ns[:2] if ns[1] > 1 else ns[:1])
            got, want = _pair(a), _pair(b)
            w = R.width(eps)
            g_rel, g_bin = nufft3d_gate(dt, R.grid(ns[0], w) * R.grid(ns[1], w) * R.grid(ns[2], w), eps)
            rel, worst = tol.rel_l2(*got, *want), tol.max_bin_err(*got, *want)
            print(f"reduction {ns} {dt} eps {eps:g}: rel {rel:.3e} / {g_rel:.3e}, element {worst:.3e} / {g_bin:.3e}")
            assert rel <= g_rel and worst <= g_bin, (ns, dt, eps, rel, worst)


@pytest.mark.parametrize("shape", BIT_SHAPES, ids=shape_id)
@pytest.mark.parametrize("dt", DTS)
def test_adjoint_identity(gpu, dt, shape):
    """<nufft3d1_F(c), F> = <c, nufft3d2_R(F)>: spreading and interpolation share their kernel values, so this holds to
    rounding even at eps = 1e-2 -- an index error in one kernel shows here where the eps-sized gate would hide it"""
    n1, n2, n3, m, kind = shape
    pts = R.points(n1, n2, n3, m, kind)
    c, f = R.data(m, 7, "c"), R.data(n1 * n2 * n3, 7, "f")
    for eps in (1e-2, R.EPS[dt][-1]):
        pl = planner(gpu, dt, shape[:3], pts, eps)
        a_re, a_im = run(gpu, pl, 1, R.FORWARD, c)
        b_re, b_im = run(gpu, pl, 2, R.REVERSE, f)
        a = a_re.astype(np.float64) + 1j * a_im.astype(np.float64)
        b = b_re.astype(np.float64) + 1j * b_im.astype(np.float64)
        lhs, rhs = np.vdot(f, a), np.vdot(b, c)   # <F, A c> and <A* F, c>
        scale = np.linalg.norm(a) * np.linalg.norm(f)
        print(f"adjoint {shape_id(shape)} {dt} eps {eps:g}: {abs(lhs - rhs) / scale:.3e} / {ADJOINT_BOUND[dt]:.3e}")
        assert abs(lhs - rhs) <= ADJOINT_BOUND[dt] * scale, (shape, dt, eps, abs(lhs - rhs) / scale, ADJOINT_BOUND[dt])


@pytest.mark.parametrize("shape", BIT_SHAPES, ids=shape_id)
@pytest.mark.parametrize("dt", DTS)
def test_bit_for_bit(gpu, dt, shape):
    """a transform alone has the bits of the same transform as the last of batch 3, with a workspace that forces chunks of one,
    at element-aligned pointers, on a side stream, under graph replay, and (type 2) through a planner built from the same points
    in another order"""
    import torch

    n1, n2, n3, m, kind = shape
    n = n1 * n2 * n3
    eps = R.EPS[dt][1]
    pts = R.points(n1, n2, n3, m, kind)
    pl = planner(gpu, dt, shape[:3], pts, eps)
    per, batch = pl.workspace_len(1), 3
    for t in (1, 2):
        n_in, n_out = (m, n) if t == 1 else (n, m)
        fn = gpu.nufft3d1_batched if t == 1 else gpu.nufft3d2_batched
        rows = [R.data(n_in, 20 + i, "c") for i in range(batch)]
        for d in (R.FORWARD, R.REVERSE):
            alone = [run(gpu, pl, t, d, v) for v in rows]
            in_dist, out_dist = (n_in + 5) | 1, (n_out + 3) | 1
            bufs = [torch.full((1 + batch * in_dist + 4,), 9.0, dtype=_tdt(dt), device="cuda") for _ in range(2)]
            assert bufs[0][1:].data_ptr() % 16 == np.dtype(_ndt(dt)).itemsize
            xin = [b[1:1 + batch * in_dist].view(batch, in_dist)[:, :n_in] for b in bufs]
            for i in range(batch):
                xin[0][i] = torch.from_numpy(np.ascontiguousarray(rows[i].real, dtype=_ndt(dt)))
                xin[1][i] = torch.from_numpy(np.ascontiguousarray(rows[i].imag, dtype=_ndt(dt)))
            keep = [b.clone() for b in bufs]
            for name, size in {"chunks of 1": per, "chunks of 2": 2 * per + 1, "one chunk": pl.workspace_len(batch)}.items():
                outs = [torch.full((1 + batch * out_dist + 4,), 9.0, dtype=_tdt(dt), device="cuda") for _ in range(2)]
                o = tuple(b[1:1 + batch * out_dist].view(batch, out_dist)[:, :n_out] for b in outs)
                fn(xin[0], xin[1], pl, _dir(gpu, d), out=o, work=torch.empty(size, dtype=_tdt(dt), device="cuda"))
                torch.cuda.synchronize()
                assert all(torch.equal(b, k) for b, k in zip(bufs, keep)), name  # the input and its gaps are not written
                for plane in range(2):
                    got = outs[plane].cpu().numpy()
                    assert got[0] == 9.0 and (got[1 + (batch - 1) * out_dist + n_out:] == 9.0).all(), name
                    for i in range(batch):
                        at = 1 + i * out_dist
                        assert np.array_equal(got[at:at + n_out], alone[i][plane]), (t, d, name, plane, i)
                        if i + 1 < batch:
                            assert (got[at + n_out:at + out_dist] == 9.0).all(), (name, plane, i)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            got = run(gpu, pl, t, d, rows[1], stream=side)
            assert np.array_equal(got[0], alone[1][0]) and np.array_equal(got[1], alone[1][1]), (t, d, "side stream")
    # graph replay, type 1 and type 2 Forward, on new data
    for t in (1, 2):
        n_in, n_out = (m, n) if t == 1 else (n, m)
        fn = gpu.nufft3d1_batched if t == 1 else gpu.nufft3d2_batched
        d_in = [torch.zeros(n_in, dtype=_tdt(dt), device="cuda") for _ in range(2)]
        out = tuple(torch.zeros(n_out, dtype=_tdt(dt), device="cuda") for _ in range(2))
        work = torch.empty(pl.workspace_len(1), dtype=_tdt(dt), device="cuda")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):  # warm-up on the capture stream
            fn(d_in[0], d_in[1], pl, out=out, work=work)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            fn(d_in[0], d_in[1], pl, out=out, work=work)
        for seed in (41, 42):
            v = R.data(n_in, seed, "c")
            want = run(gpu, pl, t, R.FORWARD, v)
            d_in[0].copy_(torch.from_numpy(np.ascontiguousarray(v.real, dtype=_ndt(dt))))
            d_in[1].copy_(torch.from_numpy(np.ascontiguousarray(v.imag, dtype=_ndt(dt))))
            out[0].zero_()
            out[1].zero_()
            g.replay()
            torch.cuda.synchronize()
            assert np.array_equal(out[0].cpu().numpy(), want[0]) and np.array_equal(out[1].cpu().numpy(), want[1]), (t, seed)
    # the same points in another order: every point's value has the same bits (type 2)
    order = np.random.default_rng(1).permutation(m)
    other = planner(gpu, dt, shape[:3], tuple(p[order] for p in pts), eps)
    v = R.data(n, 30, "f")
    for d in (R.FORWARD, R.REVERSE):
        a, b = run(gpu, pl, 2, d, v), run(gpu, other, 2, d, v)
        assert np.array_equal(a[0][order], b[0]) and np.array_equal(a[1][order], b[1]), d


@pytest.mark.parametrize("dt", DTS)
def test_overlap_and_codes(gpu, dt):
    """overlapping output, input or workspace, null planes, short distances and a short workspace come back as
    PHAST_ERR_INVALID_ARG and run nothing"""
    import ctypes as C

    import torch

    from phastft_amd import _lib

    ns, m, sfx = (12, 10, 9), 300, "64" if dt == "f64" else "32"
    n = ns[0] * ns[1] * ns[2]
    pl = planner(gpu, dt, ns, R.points(*ns, m), R.EPS[dt][1])
    lib, n_ = _lib.lib(), C.c_size_t
    for t in (1, 2):
        ni, no = (m, n) if t == 1 else (n, m)
        big = torch.zeros(4 * (m + n) + 2 * pl.workspace_len(1), dtype=_tdt(dt), device="cuda")
        at = lambda off: C.c_void_p(big.data_ptr() + off * big.element_size())  # noqa: E731
        px, py, por, poi, pw = at(0), at(ni), at(2 * ni), at(2 * ni + no), at(2 * ni + 2 * no)
        size = n_(pl.workspace_len(1))
        dev = getattr(lib, f"phast_nufft3d{t}_{sfx}_dev")
        call = lambda *a, d=1: dev(a[0], a[1], n_(ni), a[2], a[3], n_(no), n_(1), d, pl._h, a[4], a[5], None)  # noqa: E731
        assert call(None, py, por, poi, pw, size) == 16
        assert call(px, py, None, poi, pw, size) == 16
        assert call(px, py, por, None, pw, size) == 16
        assert call(px, py, por, poi, None, size) == 16
        assert call(px, py, por, poi, pw, n_(pl.workspace_len(1) - 1)) == 16               # a short workspace
        assert call(px, py, por, poi, pw, size, d=0) == 16                                 # no such direction
        assert call(px, py, px, poi, pw, size) == 16                                       # the output on the input
        assert call(px, py, at(ni - 1), poi, pw, size) == 16                               # ... on the end of its imaginary plane
        assert call(px, py, por, pw, pw, size) == 16                                       # ... on the workspace
        assert call(px, py, por, por, pw, size) == 16                                      # ... on its other plane
        assert call(px, py, por, at(2 * ni + no - 1), pw, size) == 16                      # ... by one element
        assert call(px, py, por, poi, at(ni - 1), size) == 16                              # the workspace on the input
        assert dev(px, py, n_(ni - 1), por, poi, n_(no), n_(2), 1, pl._h, pw, size, None) == 16   # in_dist below the row
        assert dev(px, py, n_(ni), por, poi, n_(no - 1), n_(2), 1, pl._h, pw, size, None) == 16   # out_dist below the row
        assert dev(px, py, n_(ni), por, poi, n_(no), n_(0), 1, pl._h, None, n_(0), None) == 0     # an empty batch
        torch.cuda.synchronize()
        assert not bool(big.any())  # none of the refused calls ran
        assert call(px, None, por, poi, pw, size) == 0                                     # real data is a call
    text = pl.describe()
    assert text.startswith(f"nufft3d N={ns[0]}x{ns[1]}x{ns[2]} M={m} eps=") and "grid=" + "x".join(str(g) for g in pl.grid_shape) in text
    assert pl.device_bytes() >= m * 28 + (pl.grid_len + 1) * 4 + sum(ns) * np.dtype(_ndt(dt)).itemsize
    grid_dim = getattr(lib, f"phast_planner_nufft3d{sfx}_grid_dim")
    assert [grid_dim(pl._h, a) for a in (-1, 0, 1, 2, 3)] == [0, *pl.grid_shape, 0]


@pytest.mark.parametrize("shape", BIT_SHAPES, ids=shape_id)
@pytest.mark.parametrize("dt", DTS)
def test_host_slice_and_one_shot_calls(gpu, dt, shape):
    """bit for bit at the shapes of test_bit_for_bit: host slices give the _dev bits, with and without a planner, complex and
    real; a wrong length is PHAST_ERR_PLANNER_SIZE; the conveniences on device tensors and the (batch, N1, N2, N3) shapes give
    them too; the stage timer leaves the result behind"""
    import torch

    n1, n2, n3, m, kind = shape
    eps = R.EPS[dt][1]
    n = n1 * n2 * n3
    sfx = "64" if dt == "f64" else "32"
    x, y, z = pts = R.points(n1, n2, n3, m, kind)
    pl = planner(gpu, dt, shape[:3], pts, eps)
    for t in (1, 2):
        ni = m if t == 1 else n
        si, so = ((m,), (n1, n2, n3)) if t == 1 else ((n1, n2, n3), (m,))
        shot, host = getattr(gpu, f"nufft3d{t}_{sfx}"), getattr(gpu, f"nufft3d{t}_{sfx}_with_planner")
        v = R.data(ni, 50, "c")
        re, im = (np.ascontiguousarray(a, dtype=_ndt(dt)).reshape(si) for a in (v.real, v.imag))
        for d in (R.FORWARD, R.REVERSE):
            for x_im in (im, None):
                want = run(gpu, pl, t, d, v, real=x_im is None)
                for call in (lambda a, b: host(re, x_im, a, b, pl, _dir(gpu, d)), lambda a, b: shot(x, y, z, re, x_im, a, b, eps, _dir(gpu, d))):
                    o_re, o_im = np.zeros(so, _ndt(dt)), np.zeros(so, _ndt(dt))
                    call(o_re, o_im)
                    assert np.array_equal(o_re.reshape(-1), want[0]) and np.array_equal(o_im.reshape(-1), want[1]), (t, d, x_im is None)
        o_re, o_im = np.zeros(so, _ndt(dt)), np.zeros(so, _ndt(dt))
        with pytest.raises(gpu.PhastPanic) as e:
            host(re.reshape(-1)[:-1].copy(), im.reshape(-1)[:-1].copy(), o_re, o_im, pl)
        assert e.value.code == 3  # PHAST_ERR_PLANNER_SIZE: a wrong planner size
        with pytest.raises(gpu.PhastPanic) as e:
            host(re, im.reshape(-1)[:-1].copy(), o_re, o_im, pl)
        assert e.value.code == 2  # PHAST_ERR_LEN_MISMATCH
        want = run(gpu, pl, t, R.FORWARD, v)
        dev = torch.from_numpy(v.astype(np.complex128 if dt == "f64" else np.complex64).reshape(si)).cuda()
        got = gpu.nufft3d1(x, y, z, dev, (n1, n2, n3), eps) if t == 1 else gpu.nufft3d2(x, y, z, dev, eps)
        assert got.dtype == dev.dtype and got.shape == so
        assert np.array_equal(got.real.cpu().numpy().reshape(-1), want[0]) and np.array_equal(got.imag.cpu().numpy().reshape(-1), want[1])
        rows = torch.stack([dev, 2 * dev]).reshape((2, 1) + si)  # leading axes are batches
        got = gpu.nufft3d1(x, y, z, rows, (n1, n2, n3), eps) if t == 1 else gpu.nufft3d2(x, y, z, rows, eps)
        assert got.shape == (2, 1) + so and np.array_equal(got[0, 0].real.cpu().numpy().reshape(-1), want[0])
        want_real = run(gpu, pl, t, R.FORWARD, v, real=True)
        got = gpu.nufft3d1(x, y, z, dev.real.contiguous(), (n1, n2, n3), eps) if t == 1 else gpu.nufft3d2(x, y, z, dev.real.contiguous(), eps)
        assert np.array_equal(got.real.cpu().numpy().reshape(-1), want_real[0]) and np.array_equal(got.imag.cpu().numpy().reshape(-1), want_real[1])
        # the batched call on shaped tensors: (batch, N1, N2, N3) on the mode side, and what it allocates
        fn = gpu.nufft3d1_batched if t == 1 else gpu.nufft3d2_batched
        d_re, d_im = torch.from_numpy(re).cuda(), torch.from_numpy(im).cuda()
        b_re, b_im = (torch.stack([a, a]) for a in (d_re, d_im))
        o = fn(b_re, b_im, pl)
        torch.cuda.synchronize()
        assert o[0].shape == (2,) + so and np.array_equal(o[0][1].cpu().numpy().reshape(-1), want[0])
        o = fn(d_re, d_im, pl)
        torch.cuda.synchronize()
        assert o[1].shape == so and np.array_equal(o[1].cpu().numpy().reshape(-1), want[1])
        d_or, d_oi = (torch.zeros(so, dtype=_tdt(dt), device="cuda") for _ in range(2))
        st = pl.time_stages(t, d_re, d_im, d_or, d_oi, 1, reps=1)
        assert len(st) == 3 and all(s >= 0 for s in st)
        assert np.array_equal(d_or.cpu().numpy().reshape(-1), want[0]) and np.array_equal(d_oi.cpu().numpy().reshape(-1), want[1])


def nufft3d_case(P, dt, shape, t, eps):
    """one call of batch 3 for tests/test_gpu_workspace_guard.py's drive()"""
    import torch

    from tests import test_gpu_workspace_guard as G

    n1, n2, n3, m, kind = shape
    n = n1 * n2 * n3
    ref = reference(shape)
    pl = planner(P, dt, shape[:3], (ref.x, ref.y, ref.z), eps)
    cells, per = pl.grid_len, pl.workspace_len(1)
    ni, no = (m, n) if t == 1 else (n, m)
    in_dist, out_dist = (ni + 5) | 1, (no + 3) | 1
    seeds = [0, 1, 0]
    xs = [ref.inp(t, False, s) for s in seeds]
    fn = P.nufft3d1_batched if t == 1 else P.nufft3d2_batched

    def call(tn, work):
        x = [torch.as_strided(tn[k], (G.BATCH, ni), (in_dist, 1)) for k in ("in_re", "in_im")]
        o = tuple(torch.as_strided(tn[k], (G.BATCH, no), (out_dist, 1)) for k in ("out_re", "out_im"))
        fn(x[0], x[1], pl, out=o, work=work)

    def gate(got):
        g_rel, g_bin = nufft3d_gate(dt, cells, eps)
        for i, s in enumerate(seeds):
            want = ref.ref[(t, R.FORWARD, False, s)]
            pair = got["out_re"][i], got["out_im"][i]
            assert tol.rel_l2(*pair, *want) <= g_rel and tol.max_bin_err(*pair, *want) <= g_bin, (shape, dt, t, i)

    planes = [G.Plane("in_re", "in", ni, in_dist, [v.real.astype(_ndt(dt)) for v in xs]),
              G.Plane("in_im", "in", ni, in_dist, [v.imag.astype(_ndt(dt)) for v in xs]),
              G.Plane("out_re", "out", no, out_dist), G.Plane("out_im", "out", no, out_dist)]
    return G.Case(f"nufft3d{t}:{shape_id(shape)}", dt, 2 * cells, planes, G._lengths(per, 2 * per + 1, pl.workspace_len(G.BATCH)), call, gate)


@pytest.mark.parametrize("t", [1, 2])
@pytest.mark.parametrize("dt", DTS)
def test_arena(gpu, dt, t):
    """one case per type in the poisoned, guarded arena: workspace lengths of one transform, one element more, two transforms
    and one element, and workspace_len(3), at bases 0, 1 and 16 / itemsize - 1 elements past a 16-byte boundary -- bands whole,
    inputs kept, the bits of a zero-filled workspace, the gaps keep their sentinel, and one element below one transform's length
    is refused with nothing written"""
    from tests import test_gpu_workspace_guard as G

    case = nufft3d_case(gpu, dt, (12, 10, 9, 300, "u"), t, R.EPS[dt][1])
    G.drive(gpu, case)
    G.overrun(gpu, case, "out_im")
