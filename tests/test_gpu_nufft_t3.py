"""The non-uniform FFT of type 3 on the MI355X (csrc/nufft_t3.hip, csrc/planner_nufft_t3.hpp) against
tests/nufft_t3_reference.py, the direct sum in long double with exact phases, on inputs that are exact in both types.

The gate (tests/test_nufft_t3_cpu.py: nufft_t3_gate): C3 eps + KAPPA Q 2^-53 + tests/tolerances.py's formula on log2 n_g, for
the rel-L2 and for the worst element / rms, Q = 2 pi (|C_s| + S) X.  The measured worst per case, eps and dtype over the seeds
is in tests/golden/nufft_t3_error_budget.json (tests/golden/make_nufft_t3_error_budget.py); test_gates_keep_their_margin keeps
the gates 2 x above every entry.  The cases (M, K) reach M = K = 1, K < M, odd and even widths and both ends of the clamp
through eps, more than one workgroup, centres 1000 and 10^6 half-widths away, the long cell list of a clump of sources, a
clump of targets, and the three degenerate widths."""
import functools
import json
import os

import numpy as np
import pytest

from tests import nufft_reference as R1
from tests import nufft_t3_reference as R
from tests import tolerances as tol
from tests.test_nufft_t3_cpu import nufft_t3_gate, reference, schedule

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTS = ["f64", "f32"]
BUDGET = os.path.join(ROOT, "tests", "golden", "nufft_t3_error_budget.json")


def _ndt(dt):
    return np.float64 if dt == "f64" else np.float32


def _tdt(dt):
    import torch

    return torch.float64 if dt == "f64" else torch.float32


def _dir(P, d):
    return P.Direction.Forward if d == R.FORWARD else P.Direction.Reverse


@functools.lru_cache(maxsize=None)
def _planner(P, dt, kx, ks, eps):
    return (P.PlannerNufftT3_64 if dt == "f64" else P.PlannerNufftT3_32)(np.frombuffer(kx, np.float64), np.frombuffer(ks, np.float64), eps)


def planner(P, dt, x, s, eps):
    """one planner per (type, sources, targets, eps), shared by the tests"""
    return _planner(P, dt, np.ascontiguousarray(x, np.float64).tobytes(), np.ascontiguousarray(s, np.float64).tobytes(), eps)


def run(P, pl, d, v, real=False, work=None, stream=None):
    """one vector through nufft3_batched: the input is never written, nothing is written past the output"""
    import torch

    dt = pl._dtype
    v = np.asarray(v)
    d_re = torch.from_numpy(np.ascontiguousarray(v.real, dtype=dt)).cuda()
    d_im = None if real else torch.from_numpy(np.ascontiguousarray(v.imag, dtype=dt)).cuda()
    keep = d_re.clone(), None if real else d_im.clone()
    n_out = pl.k_targets
    o_re, o_im = (torch.full((n_out + 3,), 7.0, dtype=d_re.dtype, device="cuda") for _ in range(2))
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())  # the fills above
    got = P.nufft3_batched(d_re, d_im, pl, _dir(P, d), out=(o_re[:n_out], o_im[:n_out]), work=work, stream=stream)
    torch.cuda.synchronize()
    assert got[0].data_ptr() == o_re.data_ptr()
    assert torch.equal(d_re, keep[0]) and (real or torch.equal(d_im, keep[1]))
    o_re, o_im = o_re.cpu().numpy(), o_im.cpu().numpy()
    assert (o_re[n_out:] == 7.0).all() and (o_im[n_out:] == 7.0).all()
    return o_re[:n_out], o_im[:n_out]


def measure(P, dt, case, eps, seeds=R.SEEDS):
    """(worst rel-L2, worst element / rms) over both directions, complex and real data and the seeds"""
    ref = reference(case)
    pl = planner(P, dt, ref.x, ref.s, eps)
    pick = slice(None) if ref.pick is None else list(ref.pick)
    rel = worst = 0.0
    for seed in seeds:
        for d in (R.FORWARD, R.REVERSE):
            for real in (False, True):
                got = run(P, pl, d, ref.inp(real, seed), real)
                got = got[0][pick], got[1][pick]
                want = ref.ref[(d, real, seed)]
                rel, worst = max(rel, tol.rel_l2(*got, *want)), max(worst, tol.max_bin_err(*got, *want))
    return rel, worst, pl


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
@pytest.mark.parametrize("dt", DTS)
def test_parity(gpu, dt, case):
    """both directions, complex and real input, seeds 0-1, at every eps of the type"""
    ref = reference(case)
    for eps in R.EPS[dt]:
        rel, worst, pl = measure(gpu, dt, case, eps)
        g = schedule(ref.x, ref.s, eps)
        assert pl.width == g["w"] and pl.grid_len == g["nf"] <= 2 ** 14 and pl.workspace_len(3) == 12 * pl.grid_len
        g_rel, g_bin = nufft_t3_gate(dt, 2 * pl.grid_len, eps, ref.q)
        tol.record(f"nufft3:{R.case_id(case)}:{eps:g}", pl.grid_len.bit_length(), rel, worst, g_rel, g_bin)
        print(f"nufft3 {R.case_id(case)} {dt} eps {eps:g} w {pl.width} n_f {pl.grid_len} Q {ref.q:.3g}: rel {rel:.3e} / {g_rel:.3e}, "
              f"element {worst:.3e} / {g_bin:.3e}")
        assert rel <= g_rel and worst <= g_bin, (case, dt, eps, rel, g_rel, worst, g_bin)


@pytest.mark.parametrize("dt", DTS)
def test_larger_case(gpu, dt):
    """M = 2^16, K = 2^15, n_f = 2^16 at eps = 1e-6, batch 3 in a workspace of 2: more than one chunk, and many workgroups per
    launch; a fixed random subset of 64 outputs against the direct sum"""
    import torch

    eps = 1e-6
    ref = reference(R.BIG)
    pl = planner(gpu, dt, ref.x, ref.s, eps)
    assert pl.grid_len == 2 ** 16
    m, k = R.BIG[:2]
    rows = [ref.inp(False, 0), ref.inp(False, 1), ref.inp(False, 0)]
    d_re, d_im = (torch.from_numpy(np.stack([np.ascontiguousarray(getattr(v, part), dtype=_ndt(dt)) for v in rows])).cuda()
                  for part in ("real", "imag"))
    work = torch.empty(pl.workspace_len(2), dtype=_tdt(dt), device="cuda")
    o_re, o_im = gpu.nufft3_batched(d_re, d_im, pl, work=work)
    torch.cuda.synchronize()
    g_rel, g_bin = nufft_t3_gate(dt, 2 * pl.grid_len, eps, ref.q)
    pick = list(ref.pick)
    for i, seed in enumerate((0, 1, 0)):
        got = o_re[i].cpu().numpy()[pick], o_im[i].cpu().numpy()[pick]
        want = ref.ref[(R.FORWARD, False, seed)]
        rel, worst = tol.rel_l2(*got, *want), tol.max_bin_err(*got, *want)
        print(f"nufft3 big {dt} row {i}: rel {rel:.3e} / {g_rel:.3e}, element {worst:.3e} / {g_bin:.3e}")
        assert rel <= g_rel and worst <= g_bin, (dt, i, rel, g_rel, worst, g_bin)
    assert torch.equal(o_re[0], o_re[2]) and torch.equal(o_im[0], o_im[2])


@pytest.mark.parametrize("n", [8, 30, 101])
@pytest.mark.parametrize("dt", DTS)
def test_dft_special_case(gpu, dt, n):
    """x_j = j and s_k = fftfreq: the library's DFT, within the gate"""
    import torch

    eps = R.EPS[dt][-1]
    x, s = np.arange(n, dtype=np.float64), np.fft.fftfreq(n)
    pl = planner(gpu, dt, x, s, eps)
    c = R.data(n, 3, "c")
    got = run(gpu, pl, R.FORWARD, c)
    re, im = (torch.from_numpy(np.ascontiguousarray(a, dtype=_ndt(dt))).cuda() for a in (c.real, c.imag))
    gpu.fft_any_batched(re, im, n, gpu.Direction.Forward, (gpu.PlannerAny64 if dt == "f64" else gpu.PlannerAny32)(n))
    want = re.cpu().numpy().astype(np.float64), im.cpu().numpy().astype(np.float64)
    rel, worst = tol.rel_l2(*got, *want), tol.max_bin_err(*got, *want)
    g_rel, g_bin = nufft_t3_gate(dt, 2 * pl.grid_len, eps, R.conditioning(x, s))
    print(f"dft {n} {dt}: rel {rel:.3e} / {g_rel:.3e}, element {worst:.3e} / {g_bin:.3e}")
    assert rel <= g_rel and worst <= g_bin


@pytest.mark.parametrize("dt", DTS)
def test_type_one_special_case(gpu, dt):
    """integer s_k = k(m) and x in [0, 1): nufft1 of the same inputs, within the sum of the two gates"""
    from tests.test_gpu_nufft import planner as planner1, run as run1
    from tests.test_nufft_cpu import nufft_gate

    n, m = 37, 100
    eps = R.EPS[dt][-1]
    x = np.random.default_rng(9).random(m)
    s = R1.modes(n).astype(np.float64)
    c = R.data(m, 4, "c")
    pl3, pl1 = planner(gpu, dt, x, s, eps), planner1(gpu, dt, n, x, eps)
    for d in (R.FORWARD, R.REVERSE):
        got, want = run(gpu, pl3, d, c), run1(gpu, pl1, 1, d, c)
        rel = tol.rel_l2(*got, *(a.astype(np.float64) for a in want))
        worst = tol.max_bin_err(*got, *(a.astype(np.float64) for a in want))
        a, b = nufft_t3_gate(dt, 2 * pl3.grid_len, eps, R.conditioning(x, s)), nufft_gate(dt, pl1.grid_len, eps)
        print(f"type 1 {dt} {d}: rel {rel:.3e} / {a[0] + b[0]:.3e}, element {worst:.3e} / {a[1] + b[1]:.3e}")
        assert rel <= a[0] + b[0] and worst <= a[1] + b[1]


@pytest.mark.parametrize("case", [R.CASES[2], R.CASES[3]], ids=R.case_id)
@pytest.mark.parametrize("dt", DTS)
def test_adjoint_identity(gpu, dt, case):
    """<A c, F> = <c, A* F> with A the Forward transform of a planner built from (x, s) and A* the Reverse one of a planner
    built from (s, x): the two sides use different grids, so this holds to eps, not to rounding"""
    x, s = R.points(case)
    m, k = len(x), len(s)
    c, f = R.data(m, 7, "c"), R.data(k, 7, "f")
    for eps in (1e-2, R.EPS[dt][-1]):
        fwd, adj = planner(gpu, dt, x, s, eps), planner(gpu, dt, s, x, eps)
        a_re, a_im = run(gpu, fwd, R.FORWARD, c)
        b_re, b_im = run(gpu, adj, R.REVERSE, f)
        a = a_re.astype(np.float64) + 1j * a_im.astype(np.float64)
        b = b_re.astype(np.float64) + 1j * b_im.astype(np.float64)
        lhs, rhs = np.vdot(f, a), np.vdot(b, c)   # <F, A c> and <A* F, c>
        scale = np.linalg.norm(a) * np.linalg.norm(f)
        gate = nufft_t3_gate(dt, 2 * fwd.grid_len, eps, R.conditioning(x, s))[0] + nufft_t3_gate(dt, 2 * adj.grid_len, eps, R.conditioning(s, x))[0]
        print(f"adjoint {R.case_id(case)} {dt} eps {eps:g}: {abs(lhs - rhs) / scale:.3e} / {gate:.3e}")
        # |<F, A c> - <A* F, c>| <= |F| |A c| (err of A c) + |c| |A* F| (err of A* F); both norms products are of one size
        assert abs(lhs - rhs) <= gate * max(scale, np.linalg.norm(b) * np.linalg.norm(c)), (case, dt, eps)


@pytest.mark.parametrize("case", [R.CASES[3], R.CASES[3][:4] + ("xclump",), (301, 64, 2.0, 8.0, "off")], ids=R.case_id)
@pytest.mark.parametrize("dt", DTS)
def test_bit_for_bit(gpu, dt, case):
    """a transform alone has the bits of the same transform as the last of batch 3, with a workspace that forces chunks of one,
    at element-aligned pointers, on a side stream, under graph replay, and through a planner built from the same targets in
    another order"""
    import torch

    eps = R.EPS[dt][1]
    x, s = R.points(case)
    m, k = len(x), len(s)
    pl = planner(gpu, dt, x, s, eps)
    n_g, batch = 2 * pl.grid_len, 3
    rows = [R.data(m, 20 + i, "c") for i in range(batch)]
    for d in (R.FORWARD, R.REVERSE):
        alone = [run(gpu, pl, d, v) for v in rows]
        in_dist, out_dist = (m + 5) | 1, (k + 3) | 1
        bufs = [torch.full((1 + batch * in_dist + 4,), 9.0, dtype=_tdt(dt), device="cuda") for _ in range(2)]
        assert bufs[0][1:].data_ptr() % 16 == np.dtype(_ndt(dt)).itemsize
        xin = [b[1:1 + batch * in_dist].view(batch, in_dist)[:, :m] for b in bufs]
        for i in range(batch):
            xin[0][i] = torch.from_numpy(np.ascontiguousarray(rows[i].real, dtype=_ndt(dt)))
            xin[1][i] = torch.from_numpy(np.ascontiguousarray(rows[i].imag, dtype=_ndt(dt)))
        keep = [b.clone() for b in bufs]
        for name, size in {"chunks of 1": 2 * n_g, "chunks of 2": 4 * n_g + 1, "one chunk": pl.workspace_len(batch)}.items():
            outs = [torch.full((1 + batch * out_dist + 4,), 9.0, dtype=_tdt(dt), device="cuda") for _ in range(2)]
            o = tuple(b[1:1 + batch * out_dist].view(batch, out_dist)[:, :k] for b in outs)
            gpu.nufft3_batched(xin[0], xin[1], pl, _dir(gpu, d), out=o, work=torch.empty(size, dtype=_tdt(dt), device="cuda"))
            torch.cuda.synchronize()
            assert all(torch.equal(b, kp) for b, kp in zip(bufs, keep)), name  # the input and its gaps are not written
            for plane in range(2):
                got = outs[plane].cpu().numpy()
                assert got[0] == 9.0 and (got[1 + (batch - 1) * out_dist + k:] == 9.0).all(), name
                for i in range(batch):
                    at = 1 + i * out_dist
                    assert np.array_equal(got[at:at + k], alone[i][plane]), (d, name, plane, i)
                    if i + 1 < batch:
                        assert (got[at + k:at + out_dist] == 9.0).all(), (name, plane, i)
        # 16-byte aligned rows at a distance that is a multiple of the group: the 16-byte post sweep
        v_dist = (k + 7) & ~3
        outs = [torch.full((batch * v_dist,), 9.0, dtype=_tdt(dt), device="cuda") for _ in range(2)]
        o = tuple(b.view(batch, v_dist)[:, :k] for b in outs)
        gpu.nufft3_batched(xin[0], xin[1], pl, _dir(gpu, d), out=o)
        torch.cuda.synchronize()
        for plane in range(2):
            got = outs[plane].cpu().numpy().reshape(batch, v_dist)
            assert (got[:, k:] == 9.0).all()
            for i in range(batch):
                assert np.array_equal(got[i, :k], alone[i][plane]), (d, "16-byte rows", plane, i)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        got = run(gpu, pl, d, rows[1], stream=side)
        assert np.array_equal(got[0], alone[1][0]) and np.array_equal(got[1], alone[1][1]), (d, "side stream")
    # graph replay, Forward, on new data
    d_in = [torch.zeros(m, dtype=_tdt(dt), device="cuda") for _ in range(2)]
    out = tuple(torch.zeros(k, dtype=_tdt(dt), device="cuda") for _ in range(2))
    work = torch.empty(pl.workspace_len(1), dtype=_tdt(dt), device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on the capture stream
        gpu.nufft3_batched(d_in[0], d_in[1], pl, out=out, work=work)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        gpu.nufft3_batched(d_in[0], d_in[1], pl, out=out, work=work)
    for seed in (41, 42):
        v = R.data(m, seed, "c")
        want = run(gpu, pl, R.FORWARD, v)
        d_in[0].copy_(torch.from_numpy(np.ascontiguousarray(v.real, dtype=_ndt(dt))))
        d_in[1].copy_(torch.from_numpy(np.ascontiguousarray(v.imag, dtype=_ndt(dt))))
        out[0].zero_()
        out[1].zero_()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out[0].cpu().numpy(), want[0]) and np.array_equal(out[1].cpu().numpy(), want[1]), seed
    # the same targets in another order: every target's value has the same bits
    order = np.random.default_rng(1).permutation(k)
    other = planner(gpu, dt, x, s[order], eps)
    v = R.data(m, 30, "c")
    for d in (R.FORWARD, R.REVERSE):
        a, b = run(gpu, pl, d, v), run(gpu, other, d, v)
        assert np.array_equal(a[0][order], b[0]) and np.array_equal(a[1][order], b[1]), d


@pytest.mark.parametrize("dt", DTS)
def test_overlap_and_codes(gpu, dt):
    """overlapping output, input or workspace, null planes, short distances and a short workspace come back as
    PHAST_ERR_INVALID_ARG and run nothing"""
    import ctypes as C

    import torch

    from phastft_amd import _lib

    case = R.CASES[3]
    x, s = R.points(case)
    m, k, sfx = len(x), len(s), "64" if dt == "f64" else "32"
    pl = planner(gpu, dt, x, s, R.EPS[dt][1])
    lib, n_ = _lib.lib(), C.c_size_t
    ni, no = m, k
    big = torch.zeros(4 * (m + k) + 2 * pl.workspace_len(1), dtype=_tdt(dt), device="cuda")
    at = lambda off: C.c_void_p(big.data_ptr() + off * big.element_size())  # noqa: E731
    px, py, por, poi, pw = at(0), at(ni), at(2 * ni), at(2 * ni + no), at(2 * ni + 2 * no)
    size = n_(pl.workspace_len(1))
    dev = getattr(lib, f"phast_nufft3_{sfx}_dev")
    call = lambda *a, d=1: dev(a[0], a[1], n_(ni), a[2], a[3], n_(no), n_(1), d, pl._h, a[4], a[5], None)  # noqa: E731
    assert call(None, py, por, poi, pw, size) == 16
    assert call(px, py, None, poi, pw, size) == 16
    assert call(px, py, por, None, pw, size) == 16
    assert call(px, py, por, poi, None, size) == 16
    assert call(px, py, por, poi, pw, n_(4 * pl.grid_len - 1)) == 16                   # a short workspace
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
    torch.cuda.synchronize()
    text = pl.describe()
    assert text.startswith(f"nufft_t3 M={m} K={k} eps=") and f"n_f={pl.grid_len} n_g={2 * pl.grid_len}" in text and "SX=75" in text
    assert f": nufft N={pl.grid_len} M={k}" in text
    item = np.dtype(_ndt(dt)).itemsize
    assert pl.device_bytes() >= m * (12 + 2 * item) + (pl.grid_len + 1) * 4 + 2 * k * item + k * 12 + (2 * pl.grid_len + 1) * 4 + pl.grid_len * item


@pytest.mark.parametrize("dt", DTS)
def test_host_slice_and_one_shot_calls(gpu, dt):
    """host slices give the _dev bits, with and without a planner, complex and real; a wrong length is PHAST_ERR_PLANNER_SIZE;
    the convenience on device tensors gives them too; the stage timer leaves the result behind"""
    import torch

    case = R.CASES[2][:4] + ("off",)
    eps = R.EPS[dt][1]
    sfx = "64" if dt == "f64" else "32"
    x, s = R.points(case)
    m, k = len(x), len(s)
    pl = planner(gpu, dt, x, s, eps)
    shot, host = getattr(gpu, f"nufft3_{sfx}"), getattr(gpu, f"nufft3_{sfx}_with_planner")
    v = R.data(m, 50, "c")
    re, im = (np.ascontiguousarray(a, dtype=_ndt(dt)) for a in (v.real, v.imag))
    for d in (R.FORWARD, R.REVERSE):
        for x_im in (im, None):
            want = run(gpu, pl, d, v, real=x_im is None)
            for call in (lambda a, b: host(re, x_im, a, b, pl, _dir(gpu, d)), lambda a, b: shot(x, s, re, x_im, a, b, eps, _dir(gpu, d))):
                o_re, o_im = np.zeros(k, _ndt(dt)), np.zeros(k, _ndt(dt))
                call(o_re, o_im)
                assert np.array_equal(o_re, want[0]) and np.array_equal(o_im, want[1]), (d, x_im is None)
    o_re, o_im = np.zeros(k, _ndt(dt)), np.zeros(k, _ndt(dt))
    with pytest.raises(gpu.PhastPanic) as e:
        host(re[:-1].copy(), im[:-1].copy(), o_re, o_im, pl)
    assert e.value.code == 3  # PHAST_ERR_PLANNER_SIZE
    with pytest.raises(gpu.PhastPanic) as e:
        host(re, im, o_re[:-1].copy(), o_im[:-1].copy(), pl)
    assert e.value.code == 3
    with pytest.raises(gpu.PhastPanic) as e:
        host(re, im[:-1].copy(), o_re, o_im, pl)
    assert e.value.code == 2  # PHAST_ERR_LEN_MISMATCH
    want = run(gpu, pl, R.FORWARD, v)
    dev = torch.from_numpy(v.astype(np.complex128 if dt == "f64" else np.complex64)).cuda()
    got = gpu.nufft3(x, s, dev, eps)
    assert got.dtype == dev.dtype and got.shape == (k,)
    assert np.array_equal(got.real.cpu().numpy(), want[0]) and np.array_equal(got.imag.cpu().numpy(), want[1])
    rows = torch.stack([dev, 2 * dev]).reshape(2, 1, m)  # leading axes are batches
    got = gpu.nufft3(x, s, rows, eps)
    assert got.shape == (2, 1, k) and np.array_equal(got[0, 0].real.cpu().numpy(), want[0])
    want_real = run(gpu, pl, R.FORWARD, v, real=True)
    got = gpu.nufft3(x, s, dev.real.contiguous(), eps)
    assert np.array_equal(got.real.cpu().numpy(), want_real[0]) and np.array_equal(got.imag.cpu().numpy(), want_real[1])
    d_re, d_im = torch.from_numpy(re).cuda(), torch.from_numpy(im).cuda()
    d_or, d_oi = (torch.zeros(k, dtype=_tdt(dt), device="cuda") for _ in range(2))
    st = pl.time_stages(d_re, d_im, d_or, d_oi, 1, reps=1)
    assert len(st) == 4 and all(t >= 0 for t in st)
    assert np.array_equal(d_or.cpu().numpy(), want[0]) and np.array_equal(d_oi.cpu().numpy(), want[1])


def nufft_t3_case(P, dt, case, eps):
    """one call of batch 3 for tests/test_gpu_workspace_guard.py's drive()"""
    import torch

    from tests import test_gpu_workspace_guard as G

    ref = reference(case)
    pl = planner(P, dt, ref.x, ref.s, eps)
    n_g = 2 * pl.grid_len
    ni, no = case[0], case[1]
    in_dist, out_dist = (ni + 5) | 1, (no + 3) | 1
    seeds = [0, 1, 0]
    xs = [ref.inp(False, sd) for sd in seeds]

    def call(tn, work):
        x = [torch.as_strided(tn[key], (G.BATCH, ni), (in_dist, 1)) for key in ("in_re", "in_im")]
        o = tuple(torch.as_strided(tn[key], (G.BATCH, no), (out_dist, 1)) for key in ("out_re", "out_im"))
        P.nufft3_batched(x[0], x[1], pl, out=o, work=work)

    def gate(got):
        g_rel, g_bin = nufft_t3_gate(dt, n_g, eps, ref.q)
        for i, sd in enumerate(seeds):
            want = ref.ref[(R.FORWARD, False, sd)]
            pair = got["out_re"][i], got["out_im"][i]
            assert tol.rel_l2(*pair, *want) <= g_rel and tol.max_bin_err(*pair, *want) <= g_bin, (case, dt, i)

    planes = [G.Plane("in_re", "in", ni, in_dist, [v.real.astype(_ndt(dt)) for v in xs]),
              G.Plane("in_im", "in", ni, in_dist, [v.imag.astype(_ndt(dt)) for v in xs]),
              G.Plane("out_re", "out", no, out_dist), G.Plane("out_im", "out", no, out_dist)]
    return G.Case(f"nufft3:{R.case_id(case)}", dt, n_g, planes, G._lengths(2 * n_g, 4 * n_g + 1, pl.workspace_len(G.BATCH)), call, gate)


@pytest.mark.parametrize("dt", DTS)
def test_arena(gpu, dt):
    """one case in the poisoned, guarded arena: workspace lengths 2 n_g, 2 n_g + 1, 4 n_g + 1 and workspace_len(3) at bases 0, 1
    and 16 / itemsize - 1 elements past a 16-byte boundary -- bands whole, inputs kept, the bits of a zero-filled workspace,
    the gaps keep their sentinel, and one element below 2 n_g is refused with nothing written"""
    from tests import test_gpu_workspace_guard as G

    case = nufft_t3_case(gpu, dt, R.CASES[3], R.EPS[dt][1])
    G.drive(gpu, case)
    G.overrun(gpu, case, "out_im")


def budget_keys():
    return {(dt, R.case_id(c), eps) for dt in DTS for c in R.CASES for eps in R.EPS[dt]}


def test_gates_keep_their_margin():
    """the gates sit >= 2 x over the worst errors measured on the MI355X, no case, eps or dtype is missing, and the device and
    the numpy model of the schedule are within 3 x of each other, the rounding term of the gate aside (a transform of one
    output at eps = 1e-14 is a few ulp either way: DESIGN.md §21)"""
    budget = json.load(open(BUDGET))
    have = {(e["dt"], e["case"], e["eps"]) for e in budget["entries"]}
    assert have == budget_keys() and len(budget["entries"]) == len(have)
    for e in budget["entries"]:
        g_rel, g_bin = nufft_t3_gate(e["dt"], e["n_g"], e["eps"], e["q"])
        assert g_rel >= 2 * e["rel"] and g_bin >= 2 * e["bin"], e
        log_g = e["n_g"].bit_length() - 1
        for got, mod, floor in ((e["rel"], e["model_rel"], tol.rel_gate(e["dt"], log_g)), (e["bin"], e["model_bin"], tol.bin_gate(e["dt"], log_g))):
            assert got <= 3 * mod + floor and mod <= 3 * got + floor, e
