"""Non-uniform FFTs of types 1 and 2 on the MI355X (csrc/nufft.hip, csrc/planner_nufft.hpp) against tests/nufft_reference.py, the
direct sum in long double with exact phases, on inputs that are exact in both types.

The gate (tests/test_nufft_cpu.py: nufft_gate): C_EPS * eps + tests/tolerances.py's formula on log2 n_g, for the rel-L2 and for
the worst element / rms.  The measured worst per shape, eps, type and dtype over the seeds is in
tests/golden/nufft_error_budget.json (tests/golden/make_nufft_error_budget.py); test_gates_keep_their_margin keeps the gates
2 x above every entry.  The shapes (N, M) reach N = 1, M < N and M > N, n_g set by 2w (16, 100), odd and even widths and both
ends of the clamp through eps, more than one workgroup, and the long cell list of 4096 points within 1e-7 of 0.3."""
import functools
import json
import os

import numpy as np
import pytest

from tests import nufft_reference as R
from tests import tolerances as tol
from tests.test_nufft_cpu import nufft_gate, reference

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTS = ["f64", "f32"]
BUDGET = os.path.join(ROOT, "tests", "golden", "nufft_error_budget.json")


def shape_id(s):
    return f"{s[0]}x{s[1]}{'' if s[2] == 'u' else s[2]}"


def _ndt(dt):
    return np.float64 if dt == "f64" else np.float32


def _tdt(dt):
    import torch

    return torch.float64 if dt == "f64" else torch.float32


def _dir(P, d):
    return P.Direction.Forward if d == R.FORWARD else P.Direction.Reverse


@functools.lru_cache(maxsize=None)
def _planner(P, dt, n, key, eps):
    return (P.PlannerNufft64 if dt == "f64" else P.PlannerNufft32)(n, np.frombuffer(key, np.float64), eps)


def planner(P, dt, n, x, eps):
    """one planner per (type, modes, points, eps), shared by the tests"""
    return _planner(P, dt, n, np.ascontiguousarray(x, np.float64).tobytes(), eps)


def run(P, pl, t, d, v, real=False, work=None, stream=None):
    """one vector through nufft{t}_batched: the input is never written, nothing is written past the output"""
    import torch

    dt = pl._dtype
    v = np.asarray(v)
    d_re = torch.from_numpy(np.ascontiguousarray(v.real, dtype=dt)).cuda()
    d_im = None if real else torch.from_numpy(np.ascontiguousarray(v.imag, dtype=dt)).cuda()
    keep = d_re.clone(), None if real else d_im.clone()
    n_out = pl.n_modes if t == 1 else pl.m_points
    o_re, o_im = (torch.full((n_out + 3,), 7.0, dtype=d_re.dtype, device="cuda") for _ in range(2))
    fn = P.nufft1_batched if t == 1 else P.nufft2_batched
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
    pl = planner(P, dt, shape[0], ref.x, eps)
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
    n, m, _ = shape
    for eps in R.EPS[dt]:
        for t in (1, 2):
            rel, worst, pl = measure(gpu, dt, shape, eps, t)
            assert pl.width == R.width(eps) and pl.grid_len == R.grid(n, pl.width) and pl.workspace_len(3) == 6 * pl.grid_len
            g_rel, g_bin = nufft_gate(dt, pl.grid_len, eps)
            tol.record(f"nufft{t}:{shape_id(shape)}:{eps:g}", pl.grid_len.bit_length() - 1, rel, worst, g_rel, g_bin)
            print(f"nufft{t} {shape_id(shape)} {dt} eps {eps:g} w {pl.width} n_g {pl.grid_len}: rel {rel:.3e} / {g_rel:.3e}, "
                  f"element {worst:.3e} / {g_bin:.3e}")
            assert rel <= g_rel and worst <= g_bin, (shape, dt, eps, t, rel, g_rel, worst, g_bin)


@pytest.mark.parametrize("n", [8, 30, 101])
@pytest.mark.parametrize("dt", DTS)
def test_dft_special_case(gpu, dt, n):
    """x_j = j / N and M = N: type 1 Forward is the library's DFT, within the gate"""
    import torch

    eps = R.EPS[dt][-1]
    pl = planner(gpu, dt, n, np.arange(n) / n, eps)
    c = R.data(n, 3, "c")
    got = run(gpu, pl, 1, R.FORWARD, c)
    re, im = (torch.from_numpy(np.ascontiguousarray(a, dtype=_ndt(dt))).cuda() for a in (c.real, c.imag))
    gpu.fft_any_batched(re, im, n, gpu.Direction.Forward, (gpu.PlannerAny64 if dt == "f64" else gpu.PlannerAny32)(n))
    want = re.cpu().numpy().astype(np.float64), im.cpu().numpy().astype(np.float64)
    rel, worst = tol.rel_l2(*got, *want), tol.max_bin_err(*got, *want)
    g_rel, g_bin = nufft_gate(dt, pl.grid_len, eps)
    print(f"dft {n} {dt}: rel {rel:.3e} / {g_rel:.3e}, element {worst:.3e} / {g_bin:.3e}")
    assert rel <= g_rel and worst <= g_bin


@pytest.mark.parametrize("shape", [(16, 100, "u"), (101, 1000, "u"), (1000, 4096, "clump")], ids=shape_id)
@pytest.mark.parametrize("dt", DTS)
def test_adjoint_identity(gpu, dt, shape):
    """<nufft1_F(c), F> = <c, nufft2_R(F)>: spreading and interpolation share their kernel values, so this holds to rounding
    even at eps = 1e-2 -- an index error in one kernel shows here where the eps-sized gate would hide it"""
    n, m, kind = shape
    x = R.points(n, m, kind)
    c, f = R.data(m, 7, "c"), R.data(n, 7, "f")
    for eps in (1e-2, R.EPS[dt][-1]):
        pl = planner(gpu, dt, n, x, eps)
        a_re, a_im = run(gpu, pl, 1, R.FORWARD, c)
        b_re, b_im = run(gpu, pl, 2, R.REVERSE, f)
        a = a_re.astype(np.float64) + 1j * a_im.astype(np.float64)
        b = b_re.astype(np.float64) + 1j * b_im.astype(np.float64)
        lhs, rhs = np.vdot(f, a), np.vdot(b, c)   # <F, A c> and <A* F, c>
        scale = np.linalg.norm(a) * np.linalg.norm(f)
        gate = tol.parseval_gate(dt, pl.grid_len.bit_length() - 1)
        print(f"adjoint {shape_id(shape)} {dt} eps {eps:g}: {abs(lhs - rhs) / scale:.3e} / {gate:.3e}")
        assert abs(lhs - rhs) <= gate * scale, (shape, dt, eps, abs(lhs - rhs) / scale, gate)


@pytest.mark.parametrize("shape", [(101, 1000, "u"), (1000, 4096, "clump"), (4099, 2000, "u")], ids=shape_id)
@pytest.mark.parametrize("dt", DTS)
def test_bit_for_bit(gpu, dt, shape):
    """a transform alone has the bits of the same transform as the last of batch 3, with a workspace that forces chunks of one,
    at element-aligned pointers, on a side stream, under graph replay, and (type 2) through a planner built from the same points
    in another order"""
    import torch

    n, m, kind = shape
    eps = R.EPS[dt][1]
    x = R.points(n, m, kind)
    pl = planner(gpu, dt, n, x, eps)
    n_g, batch = pl.grid_len, 3
    for t in (1, 2):
        n_in, n_out = (m, n) if t == 1 else (n, m)
        fn = gpu.nufft1_batched if t == 1 else gpu.nufft2_batched
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
            for name, size in {"chunks of 1": 2 * n_g, "chunks of 2": 4 * n_g + 1, "one chunk": pl.workspace_len(batch)}.items():
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
        fn = gpu.nufft1_batched if t == 1 else gpu.nufft2_batched
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
    other = planner(gpu, dt, n, x[order], eps)
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

    n, m, sfx = 101, 1000, "64" if dt == "f64" else "32"
    pl = planner(gpu, dt, n, R.points(n, m), R.EPS[dt][1])
    lib, n_ = _lib.lib(), C.c_size_t
    for t in (1, 2):
        ni, no = (m, n) if t == 1 else (n, m)
        big = torch.zeros(4 * (m + n) + 2 * pl.workspace_len(1), dtype=_tdt(dt), device="cuda")
        at = lambda off: C.c_void_p(big.data_ptr() + off * big.element_size())  # noqa: E731
        px, py, por, poi, pw = at(0), at(ni), at(2 * ni), at(2 * ni + no), at(2 * ni + 2 * no)
        size = n_(pl.workspace_len(1))
        dev = getattr(lib, f"phast_nufft{t}_{sfx}_dev")
        call = lambda *a, d=1: dev(a[0], a[1], n_(ni), a[2], a[3], n_(no), n_(1), d, pl._h, a[4], a[5], None)  # noqa: E731
        assert call(None, py, por, poi, pw, size) == 16
        assert call(px, py, None, poi, pw, size) == 16
        assert call(px, py, por, None, pw, size) == 16
        assert call(px, py, por, poi, None, size) == 16
        assert call(px, py, por, poi, pw, n_(2 * pl.grid_len - 1)) == 16                   # a short workspace
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
    assert text.startswith(f"nufft N={n} M={m} eps=") and f"n_g={pl.grid_len}" in text
    assert pl.device_bytes() >= m * 12 + (pl.grid_len + 1) * 4 + n * np.dtype(_ndt(dt)).itemsize


@pytest.mark.parametrize("dt", DTS)
def test_host_slice_and_one_shot_calls(gpu, dt):
    """host slices give the _dev bits, with and without a planner, complex and real; a wrong length is PHAST_ERR_PLANNER_SIZE;
    the conveniences on device tensors give them too; the stage timer leaves the result behind"""
    import torch

    n, m, eps = 256, 37, R.EPS[dt][1]
    sfx = "64" if dt == "f64" else "32"
    x = R.points(n, m)
    pl = planner(gpu, dt, n, x, eps)
    for t in (1, 2):
        ni, no = (m, n) if t == 1 else (n, m)
        shot, host = getattr(gpu, f"nufft{t}_{sfx}"), getattr(gpu, f"nufft{t}_{sfx}_with_planner")
        v = R.data(ni, 50, "c")
        re, im = (np.ascontiguousarray(a, dtype=_ndt(dt)) for a in (v.real, v.imag))
        for d in (R.FORWARD, R.REVERSE):
            for x_im in (im, None):
                want = run(gpu, pl, t, d, v, real=x_im is None)
                for call in (lambda a, b: host(re, x_im, a, b, pl, _dir(gpu, d)), lambda a, b: shot(x, re, x_im, a, b, eps, _dir(gpu, d))):
                    o_re, o_im = np.zeros(no, _ndt(dt)), np.zeros(no, _ndt(dt))
                    call(o_re, o_im)
                    assert np.array_equal(o_re, want[0]) and np.array_equal(o_im, want[1]), (t, d, x_im is None)
        o_re, o_im = np.zeros(no, _ndt(dt)), np.zeros(no, _ndt(dt))
        with pytest.raises(gpu.PhastPanic) as e:
            host(re[:-1].copy(), im[:-1].copy(), o_re, o_im, pl)
        assert e.value.code == 3  # PHAST_ERR_PLANNER_SIZE
        with pytest.raises(gpu.PhastPanic) as e:
            host(re, im[:-1].copy(), o_re, o_im, pl)
        assert e.value.code == 2  # PHAST_ERR_LEN_MISMATCH
        want = run(gpu, pl, t, R.FORWARD, v)
        dev = torch.from_numpy(v.astype(np.complex128 if dt == "f64" else np.complex64)).cuda()
        got = gpu.nufft1(x, dev, n, eps) if t == 1 else gpu.nufft2(x, dev, eps)
        assert got.dtype == dev.dtype and got.shape == (no,)
        assert np.array_equal(got.real.cpu().numpy(), want[0]) and np.array_equal(got.imag.cpu().numpy(), want[1])
        rows = torch.stack([dev, 2 * dev]).reshape(2, 1, ni)  # leading axes are batches
        got = gpu.nufft1(x, rows, n, eps) if t == 1 else gpu.nufft2(x, rows, eps)
        assert got.shape == (2, 1, no) and np.array_equal(got[0, 0].real.cpu().numpy(), want[0])
        want_real = run(gpu, pl, t, R.FORWARD, v, real=True)
        got = gpu.nufft1(x, dev.real.contiguous(), n, eps) if t == 1 else gpu.nufft2(x, dev.real.contiguous(), eps)
        assert np.array_equal(got.real.cpu().numpy(), want_real[0]) and np.array_equal(got.imag.cpu().numpy(), want_real[1])
        d_re, d_im = torch.from_numpy(re).cuda(), torch.from_numpy(im).cuda()
        d_or, d_oi = (torch.zeros(no, dtype=_tdt(dt), device="cuda") for _ in range(2))
        st = pl.time_stages(t, d_re, d_im, d_or, d_oi, 1, reps=1)
        assert len(st) == 3 and all(s >= 0 for s in st)
        assert np.array_equal(d_or.cpu().numpy(), want[0]) and np.array_equal(d_oi.cpu().numpy(), want[1])


def nufft_case(P, dt, shape, t, eps):
    """one call of batch 3 for tests/test_gpu_workspace_guard.py's drive()"""
    import torch

    from tests import test_gpu_workspace_guard as G

    n, m, kind = shape
    ref = reference(shape)
    pl = planner(P, dt, n, ref.x, eps)
    n_g = pl.grid_len
    ni, no = (m, n) if t == 1 else (n, m)
    in_dist, out_dist = (ni + 5) | 1, (no + 3) | 1
    seeds = [0, 1, 0]
    dirs = R.FORWARD
    xs = [ref.inp(t, False, s) for s in seeds]
    fn = P.nufft1_batched if t == 1 else P.nufft2_batched

    def call(tn, work):
        x = [torch.as_strided(tn[k], (G.BATCH, ni), (in_dist, 1)) for k in ("in_re", "in_im")]
        o = tuple(torch.as_strided(tn[k], (G.BATCH, no), (out_dist, 1)) for k in ("out_re", "out_im"))
        fn(x[0], x[1], pl, out=o, work=work)

    def gate(got):
        g_rel, g_bin = nufft_gate(dt, n_g, eps)
        for i, s in enumerate(seeds):
            want = ref.ref[(t, dirs, False, s)]
            pair = got["out_re"][i], got["out_im"][i]
            assert tol.rel_l2(*pair, *want) <= g_rel and tol.max_bin_err(*pair, *want) <= g_bin, (shape, dt, t, i)

    planes = [G.Plane("in_re", "in", ni, in_dist, [v.real.astype(_ndt(dt)) for v in xs]),
              G.Plane("in_im", "in", ni, in_dist, [v.imag.astype(_ndt(dt)) for v in xs]),
              G.Plane("out_re", "out", no, out_dist), G.Plane("out_im", "out", no, out_dist)]
    return G.Case(f"nufft{t}:{shape_id(shape)}", dt, n_g, planes, G._lengths(2 * n_g, 4 * n_g + 1, pl.workspace_len(G.BATCH)), call, gate)


@pytest.mark.parametrize("t", [1, 2])
@pytest.mark.parametrize("dt", DTS)
def test_arena(gpu, dt, t):
    """one case per type in the poisoned, guarded arena: workspace lengths 2 n_g, 2 n_g + 1, 4 n_g + 1 and workspace_len(3) at
    bases 0, 1 and 16 / itemsize - 1 elements past a 16-byte boundary -- bands whole, inputs kept, the bits of a zero-filled
    workspace, the gaps keep their sentinel, and one element below 2 n_g is refused with nothing written"""
    from tests import test_gpu_workspace_guard as G

    case = nufft_case(gpu, dt, (101, 1000, "u"), t, R.EPS[dt][1])
    G.drive(gpu, case)
    G.overrun(gpu, case, "out_im")


def test_gates_keep_their_margin():
    """the gates sit >= 2 x over the worst errors measured on the MI355X, and no shape, eps, type or dtype is missing"""
    budget = json.load(open(BUDGET))
    want = {(dt, n, m, kind, eps, t) for dt in DTS for (n, m, kind) in R.SHAPES for eps in R.EPS[dt] for t in (1, 2)}
    have = {(e["dt"], e["n"], e["m"], e["kind"], e["eps"], e["type"]) for e in budget["entries"]}
    assert have == want and len(budget["entries"]) == len(want)
    for e in budget["entries"]:
        g_rel, g_bin = nufft_gate(e["dt"], e["n_g"], e["eps"])
        assert g_rel >= 2 * e["rel"] and g_bin >= 2 * e["bin"], e
