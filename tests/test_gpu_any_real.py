"""Real transforms (R2C / C2R) of any length on the MI355X (csrc/any_real.hip, csrc/planner_any_real.hpp), against numpy's
pocketfft rfft / irfft in long double.

Gates: tests/tolerances.py's formulas with log2 N replaced by log2 M (M = the inner convolution length: of the N/2-point
Bluestein transform for even N, of the N-point one for odd N), times REAL_FACTOR = 2, as tests/test_gpu_any_len.py does.  The
measured worst over seeds 0-3 (tests/golden/any_real_error_budget.json, written on the MI355X by
tests/golden/make_any_real_error_budget.py) sits at least 3 x below them (test_gates_keep_their_margin).  A naive chirp phase
pi n^2 / N in double fails them by orders of magnitude (tests/test_any_real_cpu.py::test_gates_catch_a_naive_chirp)."""
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from tests import tolerances as tol

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REAL_FACTOR = 2.0
NAMED = [1000, 1002, 1009, 4094, 4097, 65538, 10 ** 5, 999_999, 10 ** 6, 1_000_003, 3 << 20]


def conv_len(n: int) -> int:
    return n if n & (n - 1) == 0 else 1 << (2 * n - 2).bit_length()


def inner_m(n: int) -> int:
    """the length whose log2 the gates use: the inner convolution of the Bluestein transform, or N itself (powers of two, 1, 2)"""
    if n & (n - 1) == 0:
        return n
    return conv_len(n if n & 1 else n // 2)


def real_gates(dt: str, n: int):
    lm = inner_m(n).bit_length() - 1
    return REAL_FACTOR * tol.rel_gate(dt, lm), REAL_FACTOR * tol.bin_gate(dt, lm)


def _ndt(dt):
    return np.float64 if dt == "f64" else np.float32


def _signal(n: int, dt: str, seed: int = 0):
    return np.random.default_rng([seed, n, 7]).uniform(-1, 1, n).astype(_ndt(dt))


def _spectrum(n: int, dt: str, seed: int = 0):
    """a Hermitian half spectrum: rfft of a real signal, rounded to dt"""
    X = np.fft.rfft(_signal(n, dt, seed + 100).astype(np.longdouble))
    return np.asarray(X.real, _ndt(dt)), np.asarray(X.imag, _ndt(dt))


def _ref_r2c(x):
    return np.fft.rfft(x.astype(np.longdouble))


def _ref_c2r(re, im, n):
    return np.fft.irfft(re.astype(np.longdouble) + 1j * im.astype(np.longdouble), n)


def _check(tag, dt, n, got_re, got_im, ref_re, ref_im):
    r, i = np.asarray(ref_re, np.float64), np.asarray(ref_im, np.float64)
    rel, worst = tol.rel_l2(got_re, got_im, r, i), tol.max_bin_err(got_re, got_im, r, i)
    g_rel, g_bin = real_gates(dt, n)
    tol.record(tag, inner_m(n).bit_length() - 1, rel, worst, g_rel, g_bin)
    assert rel <= g_rel and worst <= g_bin, (tag, dt, n, rel, g_rel, worst, g_bin)


def _check_r2c(dt, n, got, x):
    ref = _ref_r2c(x)
    _check(f"r2c_any:{n}", dt, n, got[0], got[1], ref.real, ref.imag)


def _check_c2r(dt, n, got, re, im):
    ref = np.asarray(_ref_c2r(re, im, n), np.float64)
    _check(f"c2r_any:{n}", dt, n, got, np.zeros_like(got), ref, np.zeros_like(ref))


def _planner(P, dt, n):
    return (P.PlannerR2cAny64 if dt == "f64" else P.PlannerR2cAny32)(n)


def _dev_r2c(P, dt, x, planner):
    """one R2C through the device-tensor path; the input tensor is checked unmodified"""
    import torch

    n = len(x)
    d_x = torch.from_numpy(x.copy()).cuda()
    o_re = torch.full((n // 2 + 1,), 5.0, dtype=d_x.dtype, device="cuda")
    o_im = torch.full_like(o_re, 5.0)
    (P.r2c_fft_f64_any_with_planner if dt == "f64" else P.r2c_fft_f32_any_with_planner)(d_x, o_re, o_im, planner)
    assert np.array_equal(d_x.cpu().numpy(), x)
    return o_re.cpu().numpy(), o_im.cpu().numpy()


def _dev_c2r(P, dt, re, im, n, planner):
    import torch

    d_re, d_im = torch.from_numpy(re.copy()).cuda(), torch.from_numpy(im.copy()).cuda()
    out = torch.full((n,), 5.0, dtype=d_re.dtype, device="cuda")
    (P.c2r_fft_f64_any_with_planner if dt == "f64" else P.c2r_fft_f32_any_with_planner)(d_re, d_im, out, planner)
    assert np.array_equal(d_re.cpu().numpy(), re) and np.array_equal(d_im.cpu().numpy(), im)
    return out.cpu().numpy()


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_every_length_up_to_300(gpu, dt):
    for n in range(1, 301):
        pl = _planner(gpu, dt, n)
        x = _signal(n, dt, seed=1)
        _check_r2c(dt, n, _dev_r2c(gpu, dt, x, pl), x)
        re, im = _spectrum(n, dt, seed=1)
        _check_c2r(dt, n, _dev_c2r(gpu, dt, re, im, n, pl), re, im)


@pytest.mark.parametrize("n", NAMED)
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_named_lengths(gpu, dt, n):
    pl = _planner(gpu, dt, n)
    assert pl.m == inner_m(n) and f"M={pl.m}" in pl.describe()
    assert pl.workspace_len(3) == 3 * 2 * pl.m and pl.device_bytes() >= 2 * pl.m * np.dtype(_ndt(dt)).itemsize
    x = _signal(n, dt)
    _check_r2c(dt, n, _dev_r2c(gpu, dt, x, pl), x)
    re, im = _spectrum(n, dt)
    _check_c2r(dt, n, _dev_c2r(gpu, dt, re, im, n, pl), re, im)


def test_large_length_f64(gpu):
    """2^24 + 2: H = 2^23 + 1, M = 2^25 (1 GiB of workspace), R2C and C2R"""
    n = (1 << 24) + 2
    pl = gpu.PlannerR2cAny64(n)
    assert pl.m == 1 << 25
    x = _signal(n, "f64")
    _check_r2c("f64", n, _dev_r2c(gpu, "f64", x, pl), x)
    re, im = _spectrum(n, "f64")
    _check_c2r("f64", n, _dev_c2r(gpu, "f64", re, im, n, pl), re, im)


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_round_trip(gpu, dt):
    for n in (1, 2, 3, 17, 1000, 1002, 65537, 10 ** 6, 1_000_003):
        pl = _planner(gpu, dt, n)
        x = _signal(n, dt, seed=2)
        f_re, f_im = _dev_r2c(gpu, dt, x, pl)
        back = _dev_c2r(gpu, dt, f_re, f_im, n, pl)
        rel = tol.rel_l2(back, np.zeros_like(back), x.astype(np.float64), np.zeros(n))
        assert rel <= 2 * real_gates(dt, n)[0], (dt, n, rel)


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_exact_zeros(gpu, dt):
    """Im X[0] = 0 exactly; Im X[N/2] = 0 exactly for even N (every path: direct, odd, packed, power of two)"""
    for n in (1, 2, 3, 6, 7, 10, 1001, 1002, 4096, 65538, 999_999, 10 ** 6):
        pl = _planner(gpu, dt, n)
        g_re, g_im = _dev_r2c(gpu, dt, _signal(n, dt, seed=5) + 1, pl)
        assert g_im[0] == 0.0, (n, g_im[0])
        if n % 2 == 0:
            assert g_im[n // 2] == 0.0, (n, g_im[n // 2])


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_powers_of_two_are_the_r2c_path(gpu, dt):
    """N = 2^k >= 4: phast_r2c_fft_*_dev / phast_c2r_fft_*_dev themselves, bit for bit (no workspace)"""
    import torch

    for k in range(2, 21):
        n = 1 << k
        pa = _planner(gpu, dt, n)
        pr = (gpu.PlannerR2c64 if dt == "f64" else gpu.PlannerR2c32)(n)
        assert pa.workspace_len(4) == 0 and pa.m == 0
        x = torch.from_numpy(_signal(n, dt, seed=k)).cuda()
        a_re, a_im = torch.empty(n // 2 + 1, dtype=x.dtype, device="cuda"), torch.empty(n // 2 + 1, dtype=x.dtype, device="cuda")
        b_re, b_im = torch.empty_like(a_re), torch.empty_like(a_im)
        gpu.r2c_any_batched(x, a_re, a_im, pa, 1)
        gpu.r2c_fft_batched(x, b_re, b_im, pr, 1)
        assert torch.equal(a_re, b_re) and torch.equal(a_im, b_im), (dt, k)
        a_out, b_out = torch.empty(n, dtype=x.dtype, device="cuda"), torch.empty(n, dtype=x.dtype, device="cuda")
        gpu.c2r_any_batched(a_re, a_im, a_out, pa, 1)
        gpu.c2r_fft_batched(b_re, b_im, b_out, pr, 1)
        assert torch.equal(a_out, b_out), (dt, k)


def _restated_preprocess_c2r(re, im, n):
    """the power-of-two path's C2R (oracle pho_c2r_preprocess, then the N/2-point inverse and the interleave) restated in
    long double with exact twiddles -- what a non-Hermitian input gives for even N"""
    h = n // 2
    X = re.astype(np.longdouble) + 1j * im.astype(np.longdouble)
    k = np.arange(h)
    A, B = X[k], np.conj(X[h - k])
    w = np.exp(np.longdouble(2) * np.pi * 1j * k.astype(np.longdouble) / n)   # conj(W^k), W = exp(-2 pi i / N)
    z = 0.5 * (A + B) + 0.5j * w * (A - B)
    y = np.fft.ifft(z)
    out = np.empty(n, np.longdouble)
    out[0::2], out[1::2] = y.real, y.imag
    return out


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_non_hermitian_c2r(gpu, dt):
    """even N: the preprocess formula of the power-of-two path (so nothing changes at a power-of-two boundary: N = 1024 is
    checked against the same restatement); odd N, N = 1, 2: numpy's irfft, which ignores Im X[0] (and Im X[N/2] for N = 2)"""
    for n in (1, 2, 3, 10, 1001, 1002, 1024, 4094, 65538, 99_999):
        rng = np.random.default_rng([n, 9])
        re, im = (rng.uniform(-1, 1, n // 2 + 1).astype(_ndt(dt)) for _ in range(2))
        got = _dev_c2r(gpu, dt, re, im, n, _planner(gpu, dt, n))
        if n % 2 == 0 and n > 2:
            want = np.asarray(_restated_preprocess_c2r(re, im, n), np.float64)
        else:
            want = np.asarray(_ref_c2r(re, im, n), np.float64)
        _check(f"c2r_any_nonherm:{n}", dt, n, got, np.zeros_like(got), want, np.zeros_like(want))


@pytest.mark.parametrize("n", [1002, 999, 2])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_batches_chunks_ragged_dists_and_views(gpu, dt, n):
    """batch 5 at ragged distances (odd in_dist / out_dist), planes at buf[1:] and buf[3:], a workspace of 2 transforms (three
    chunks): every transform bit-identical to the same transform run alone; everything between the transforms untouched;
    the whole batch in one chunk gives the same bits again"""
    import torch

    P = gpu
    pl = _planner(P, dt, n)
    h1, batch = n // 2 + 1, 5
    ndt = _ndt(dt)
    # R2C
    in_dist, out_dist = n + 3, h1 + 2
    buf = np.full(1 + (batch - 1) * in_dist + n, 7.0, ndt)
    singles = []
    for b in range(batch):
        x = _signal(n, dt, seed=10 + b)
        buf[1 + b * in_dist:1 + b * in_dist + n] = x
        singles.append(_dev_r2c(P, dt, x, pl))
    d_in = torch.from_numpy(buf.copy()).cuda()
    o = torch.full((3 + (batch - 1) * out_dist + h1,), -7.0, dtype=d_in.dtype, device="cuda")
    o_re, o_im = o.clone(), o.clone()
    work = torch.empty(max(1, pl.workspace_len(2)) + 1, dtype=d_in.dtype, device="cuda")
    P.r2c_any_batched(d_in[1:], o_re[3:], o_im[3:], pl, batch, in_dist=in_dist, out_dist=out_dist, workspace=work[1:])
    g_re, g_im = o_re.cpu().numpy(), o_im.cpu().numpy()
    mask = np.ones(len(g_re), bool)
    for b in range(batch):
        s = slice(3 + b * out_dist, 3 + b * out_dist + h1)
        assert np.array_equal(g_re[s], singles[b][0]) and np.array_equal(g_im[s], singles[b][1]), b
        mask[s] = False
    assert np.all(g_re[mask] == -7.0) and np.all(g_im[mask] == -7.0)
    assert np.array_equal(d_in.cpu().numpy(), buf)
    o2_re, o2_im = o.clone(), o.clone()
    P.r2c_any_batched(d_in[1:], o2_re[3:], o2_im[3:], pl, batch, in_dist=in_dist, out_dist=out_dist)
    assert torch.equal(o2_re, o_re) and torch.equal(o2_im, o_im)
    # C2R
    c_in_dist, c_out_dist = h1 + 1, n + 5
    b_re = np.full(3 + (batch - 1) * c_in_dist + h1, 3.0, ndt)
    b_im = b_re.copy()
    singles = []
    for b in range(batch):
        re, im = _spectrum(n, dt, seed=20 + b)
        b_re[3 + b * c_in_dist:3 + b * c_in_dist + h1], b_im[3 + b * c_in_dist:3 + b * c_in_dist + h1] = re, im
        singles.append(_dev_c2r(P, dt, re, im, n, pl))
    d_re, d_im = torch.from_numpy(b_re.copy()).cuda(), torch.from_numpy(b_im.copy()).cuda()
    out = torch.full((1 + (batch - 1) * c_out_dist + n,), -3.0, dtype=d_re.dtype, device="cuda")
    P.c2r_any_batched(d_re[3:], d_im[3:], out[1:], pl, batch, in_dist=c_in_dist, out_dist=c_out_dist, workspace=work[:max(1, pl.workspace_len(2))])
    g = out.cpu().numpy()
    mask = np.ones(len(g), bool)
    for b in range(batch):
        s = slice(1 + b * c_out_dist, 1 + b * c_out_dist + n)
        assert np.array_equal(g[s], singles[b]), b
        mask[s] = False
    assert np.all(g[mask] == -3.0)
    assert np.array_equal(d_re.cpu().numpy(), b_re) and np.array_equal(d_im.cpu().numpy(), b_im)
    out2 = torch.full_like(out, -3.0)
    P.c2r_any_batched(d_re[3:], d_im[3:], out2[1:], pl, batch, in_dist=c_in_dist, out_dist=c_out_dist)
    assert torch.equal(out2, out)
    # argument errors: a short workspace, a short dist, a length that is not the planner's
    if pl.m:
        with pytest.raises(P.PhastPanic) as ei:
            P.r2c_any_batched(d_in[1:], o_re[3:], o_im[3:], pl, batch, in_dist=in_dist, out_dist=out_dist,
                              workspace=work[:2 * pl.m - 1])
        assert ei.value.code == 16
    with pytest.raises(P.PhastPanic) as ei:
        P.r2c_any_batched(d_in, o_re, o_im, pl, 2, in_dist=n - 1, out_dist=out_dist)
    assert ei.value.code == 16
    with pytest.raises(P.PhastPanic) as ei:
        P.c2r_any_batched(d_re, d_im, out, pl, 2, in_dist=h1 - 1, out_dist=c_out_dist)
    assert ei.value.code == 16
    lib = P._lib.lib()
    fs = "f64" if dt == "f64" else "f32"
    ws = P._any_workspace(pl, 1)
    import ctypes as C

    rc = getattr(lib, f"phast_r2c_fft_{fs}_any_dev")(C.c_void_p(d_in.data_ptr()), C.c_void_p(o_re.data_ptr()),
                                                     C.c_void_p(o_im.data_ptr()), C.c_size_t(n + 1), C.c_size_t(1),
                                                     C.c_size_t(n + 1), C.c_size_t(h1 + 1), pl._h, ws.ptr, C.c_size_t(ws.len),
                                                     P._stream())
    assert rc == 3


def _up4(k: int) -> int:
    return (k + 3) & ~3


@pytest.mark.parametrize("n", [1000, 1001, 4094])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_batches_at_aligned_distances(gpu, dt, n):
    """batch 3 on fresh (aligned) tensors, at the default distances and at distances rounded up to 4 elements (16 bytes of
    f32, 32 of f64), whole and in chunks of 2: the batched 16-byte caller-side accesses of the pad and post sweeps.  Every
    transform is bit-identical to the same transform run alone."""
    import torch

    P, batch, h1 = gpu, 3, n // 2 + 1
    pl = _planner(P, dt, n)
    tdt = torch.float64 if dt == "f64" else torch.float32
    xs = [_signal(n, dt, seed=40 + b) for b in range(batch)]
    specs = [_spectrum(n, dt, seed=50 + b) for b in range(batch)]
    r2c_singles = [_dev_r2c(P, dt, x, pl) for x in xs]
    c2r_singles = [_dev_c2r(P, dt, re, im, n, pl) for re, im in specs]
    for real_dist, cx_dist in ((n, h1), (_up4(n), _up4(h1))):
        for work_batch in (batch, 2):
            work = torch.empty(pl.workspace_len(work_batch), dtype=tdt, device="cuda")
            x = torch.zeros((batch - 1) * real_dist + n, dtype=tdt, device="cuda")
            for b in range(batch):
                x[b * real_dist:b * real_dist + n] = torch.from_numpy(xs[b])
            o_re = torch.zeros((batch - 1) * cx_dist + h1, dtype=tdt, device="cuda")
            o_im = torch.zeros_like(o_re)
            P.r2c_any_batched(x, o_re, o_im, pl, batch, in_dist=real_dist, out_dist=cx_dist, workspace=work)
            g_re, g_im = o_re.cpu().numpy(), o_im.cpu().numpy()
            for b in range(batch):
                s = slice(b * cx_dist, b * cx_dist + h1)
                assert np.array_equal(g_re[s], r2c_singles[b][0]) and np.array_equal(g_im[s], r2c_singles[b][1]), \
                    (real_dist, cx_dist, work_batch, b)
            i_re, i_im = torch.zeros_like(o_re), torch.zeros_like(o_im)
            for b in range(batch):
                i_re[b * cx_dist:b * cx_dist + h1] = torch.from_numpy(specs[b][0])
                i_im[b * cx_dist:b * cx_dist + h1] = torch.from_numpy(specs[b][1])
            out = torch.zeros_like(x)
            P.c2r_any_batched(i_re, i_im, out, pl, batch, in_dist=cx_dist, out_dist=real_dist, workspace=work)
            g = out.cpu().numpy()
            for b in range(batch):
                assert np.array_equal(g[b * real_dist:b * real_dist + n], c2r_singles[b]), (real_dist, cx_dist, work_batch, b)


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_powers_of_two_need_an_even_real_distance(gpu, dt):
    """N = 2^k >= 4 runs the power-of-two real path, which reads and writes the real side as (even, odd) pairs: a batch at an
    odd real-side distance (R2C in_dist, C2R out_dist) is PHAST_ERR_INVALID_ARG there (phastft_hip.h).  An even one that is
    not N works, bit-identical to single transforms."""
    import torch

    P, n, batch = gpu, 1024, 2
    h1 = n // 2 + 1
    pl = _planner(P, dt, n)
    tdt = torch.float64 if dt == "f64" else torch.float32
    x = torch.zeros((batch - 1) * (n + 2) + n, dtype=tdt, device="cuda")
    o_re, o_im = torch.zeros(batch * h1, dtype=tdt, device="cuda"), torch.zeros(batch * h1, dtype=tdt, device="cuda")
    with pytest.raises(P.PhastPanic) as ei:
        P.r2c_any_batched(x, o_re, o_im, pl, batch, in_dist=n + 1)
    assert ei.value.code == 16
    with pytest.raises(P.PhastPanic) as ei:
        P.c2r_any_batched(o_re, o_im, x, pl, batch, out_dist=n + 1)
    assert ei.value.code == 16
    xs = [_signal(n, dt, seed=60 + b) for b in range(batch)]
    for b in range(batch):
        x[b * (n + 2):b * (n + 2) + n] = torch.from_numpy(xs[b])
    P.r2c_any_batched(x, o_re, o_im, pl, batch, in_dist=n + 2)
    for b in range(batch):
        want = _dev_r2c(P, dt, xs[b], pl)
        s = slice(b * h1, (b + 1) * h1)
        assert np.array_equal(o_re.cpu().numpy()[s], want[0]) and np.array_equal(o_im.cpu().numpy()[s], want[1]), b
    out = torch.zeros_like(x)
    P.c2r_any_batched(o_re, o_im, out, pl, batch, out_dist=n + 2)
    for b in range(batch):
        want = _dev_c2r(P, dt, o_re.cpu().numpy()[b * h1:(b + 1) * h1], o_im.cpu().numpy()[b * h1:(b + 1) * h1], n, pl)
        assert np.array_equal(out.cpu().numpy()[b * (n + 2):b * (n + 2) + n], want), b


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_host_slices_equal_device_calls(gpu, dt):
    for n in (1, 2, 5, 1000, 1002, 4097, 65538):
        pl = _planner(gpu, dt, n)
        x = _signal(n, dt, seed=3)
        d_re, d_im = _dev_r2c(gpu, dt, x, pl)
        h1 = n // 2 + 1
        for with_planner in (True, False):
            h_re, h_im, xc = np.zeros(h1, _ndt(dt)), np.zeros(h1, _ndt(dt)), x.copy()
            if with_planner:
                (gpu.r2c_fft_f64_any_with_planner if dt == "f64" else gpu.r2c_fft_f32_any_with_planner)(xc, h_re, h_im, pl)
            else:
                (gpu.r2c_fft_f64_any if dt == "f64" else gpu.r2c_fft_f32_any)(xc, h_re, h_im)
            assert np.array_equal(h_re, d_re) and np.array_equal(h_im, d_im) and np.array_equal(xc, x), (n, with_planner)
        re, im = _spectrum(n, dt, seed=3)
        d_out = _dev_c2r(gpu, dt, re, im, n, pl)
        for with_planner in (True, False):
            out, rc, ic = np.zeros(n, _ndt(dt)), re.copy(), im.copy()
            if with_planner:
                (gpu.c2r_fft_f64_any_with_planner if dt == "f64" else gpu.c2r_fft_f32_any_with_planner)(rc, ic, out, pl)
            else:
                (gpu.c2r_fft_f64_any if dt == "f64" else gpu.c2r_fft_f32_any)(rc, ic, out)
            assert np.array_equal(out, d_out) and np.array_equal(rc, re) and np.array_equal(ic, im), (n, with_planner)


def test_two_threads_two_streams_one_planner(gpu):
    import torch

    n = 1_000_002
    pl = gpu.PlannerR2cAny64(n)
    inputs = [_signal(n, "f64", seed=20 + t) for t in range(2)]
    want = [_dev_r2c(gpu, "f64", x, pl) for x in inputs]
    spectra = [_spectrum(n, "f64", seed=30 + t) for t in range(2)]
    want_c2r = [_dev_c2r(gpu, "f64", re, im, n, pl) for re, im in spectra]
    errors = []

    def worker(t):
        try:
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                for _ in range(4):
                    d_x = torch.from_numpy(inputs[t]).cuda()
                    o_re = torch.empty(n // 2 + 1, dtype=torch.float64, device="cuda")
                    o_im = torch.empty_like(o_re)
                    gpu.r2c_fft_f64_any_with_planner(d_x, o_re, o_im, pl)
                    if not (np.array_equal(o_re.cpu().numpy(), want[t][0]) and np.array_equal(o_im.cpu().numpy(), want[t][1])):
                        errors.append(("r2c", t))
                    d_re, d_im = torch.from_numpy(spectra[t][0]).cuda(), torch.from_numpy(spectra[t][1]).cuda()
                    out = torch.empty(n, dtype=torch.float64, device="cuda")
                    gpu.c2r_fft_f64_any_with_planner(d_re, d_im, out, pl)
                    if not np.array_equal(out.cpu().numpy(), want_c2r[t]):
                        errors.append(("c2r", t))
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    th = [threading.Thread(target=worker, args=(t,)) for t in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors


@pytest.mark.parametrize("n", [100_002, 99_999])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_graph_capture(gpu, dt, n):
    """an R2C and a C2R _dev call captured on a side stream (a single-stream linear capture), replayed twice: the eager results"""
    import torch

    pl = _planner(gpu, dt, n)
    x = _signal(n, dt, seed=4)
    re, im = _spectrum(n, dt, seed=4)
    want = _dev_r2c(gpu, dt, x, pl)
    want_c2r = _dev_c2r(gpu, dt, re, im, n, pl)
    d_x, d_re, d_im = (torch.from_numpy(a).cuda() for a in (x, re, im))
    o_re, o_im = torch.zeros(n // 2 + 1, dtype=d_x.dtype, device="cuda"), torch.zeros(n // 2 + 1, dtype=d_x.dtype, device="cuda")
    out = torch.zeros(n, dtype=d_x.dtype, device="cuda")
    work = torch.empty(pl.workspace_len(1), dtype=d_x.dtype, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # warm-up on the capture stream
        gpu.r2c_any_batched(d_x, o_re, o_im, pl, 1, workspace=work)
        gpu.c2r_any_batched(d_re, d_im, out, pl, 1, workspace=work)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        gpu.r2c_any_batched(d_x, o_re, o_im, pl, 1, workspace=work)
        gpu.c2r_any_batched(d_re, d_im, out, pl, 1, workspace=work)
    for _ in range(2):
        o_re.zero_()
        o_im.zero_()
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(o_re.cpu().numpy(), want[0]) and np.array_equal(o_im.cpu().numpy(), want[1])
        assert np.array_equal(out.cpu().numpy(), want_c2r)


def test_cpp_mirror(gpu, tmp_path):
    from phastft_amd import build

    lib = build.build()
    exe = str(tmp_path / "any_real_test")
    libdir = os.path.dirname(lib)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "any_real_test.cpp"), "-o", exe, "-L", libdir, "-lphastft_hip",
                        f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, "gpu"], capture_output=True, text=True)
    sys.stdout.write(r.stdout)
    assert r.returncode == 0 and "any_real: ok" in r.stdout, r.stdout + r.stderr


def test_gates_keep_their_margin():
    """the gates above sit >= 3 x over the worst error measured on the MI355X over seeds 0-3"""
    budget = json.load(open(os.path.join(ROOT, "tests", "golden", "any_real_error_budget.json")))
    assert budget["entries"]
    for e in budget["entries"]:
        g_rel, g_bin = real_gates(e["dt"], e["n"])
        assert g_rel >= 3 * e["rel"] and g_bin >= 3 * e["bin"], e
