"""Complex transforms of any length on the MI355X (Bluestein on the power-of-two engine: csrc/any_len.hip, csrc/planner_any.hpp),
against numpy's pocketfft in long double (which handles any N).

Gates: tests/tolerances.py's formulas with log2 N replaced by log2 M (M = the convolution length, 2^ceil(log2(2N - 1))), times
ANY_FACTOR = 2.  The measured worst over seeds 0-3 (tests/golden/any_len_error_budget.json, written on the MI355X by
tests/golden/make_any_len_error_budget.py) sits at least 3.7 x below them (test_gates_keep_their_margin; measured: >= 8.2 x
on rel-L2, >= 14.7 x on the worst bin).  At N = 1_000_003 (M = 2^21) the f64 rel-L2 gate is 2 * 8e-16 * 21 = 3.4e-14: about
9000 x below the ~3e-10 phase error of the naive chirp pi n^2 / N in double, which these gates therefore catch."""
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
ANY_FACTOR = 2.0
NAMED = [1000, 1009, 4095, 4097, 65537, 10 ** 5, 1_000_003, 10 ** 6]


def conv_len(n: int) -> int:
    return n if n & (n - 1) == 0 else 1 << (2 * n - 2).bit_length()


def any_gates(dt: str, n: int):
    lm = conv_len(n).bit_length() - 1
    return ANY_FACTOR * tol.rel_gate(dt, lm), ANY_FACTOR * tol.bin_gate(dt, lm)


def _input(n: int, dt: str, seed: int = 0):
    rng = np.random.default_rng([seed, n])
    ndt = np.float64 if dt == "f64" else np.float32
    return rng.uniform(-1, 1, n).astype(ndt), rng.uniform(-1, 1, n).astype(ndt)


def _ref(re, im, direction: int):
    z = re.astype(np.longdouble) + 1j * im.astype(np.longdouble)
    return np.fft.fft(z) if direction == 1 else np.fft.ifft(z)


def _errors(got_re, got_im, ref):
    r, i = np.asarray(ref.real, np.float64), np.asarray(ref.imag, np.float64)
    return tol.rel_l2(got_re, got_im, r, i), tol.max_bin_err(got_re, got_im, r, i)


def _check(tag, dt, n, got_re, got_im, ref):
    rel, worst = _errors(got_re, got_im, ref)
    g_rel, g_bin = any_gates(dt, n)
    tol.record(tag, conv_len(n).bit_length() - 1, rel, worst, g_rel, g_bin)
    assert rel <= g_rel and worst <= g_bin, (tag, dt, n, rel, g_rel, worst, g_bin)


def _planner(P, dt, n):
    return (P.PlannerAny64 if dt == "f64" else P.PlannerAny32)(n)


def _dev_fft(P, dt, re, im, direction, planner):
    import torch

    d_re, d_im = torch.from_numpy(re.copy()).cuda(), torch.from_numpy(im.copy()).cuda()
    (P.fft_64_any_with_planner if dt == "f64" else P.fft_32_any_with_planner)(d_re, d_im, P.Direction(direction), planner)
    return d_re.cpu().numpy(), d_im.cpu().numpy()


@pytest.mark.parametrize("direction", [1, -1])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_every_length_up_to_300(gpu, dt, direction):
    for n in range(1, 301):
        re, im = _input(n, dt, seed=1)
        pl = _planner(gpu, dt, n)
        g_re, g_im = _dev_fft(gpu, dt, re, im, direction, pl)
        _check(f"any:{n}", dt, n, g_re, g_im, _ref(re, im, direction))


@pytest.mark.parametrize("n", NAMED)
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_named_lengths(gpu, dt, n):
    re, im = _input(n, dt)
    pl = _planner(gpu, dt, n)
    assert pl.m == conv_len(n) and f"M={pl.m}" in pl.describe()
    assert pl.device_bytes() >= 2 * pl.m * re.itemsize and pl.workspace_len(3) == 3 * 2 * pl.m
    for direction in (1, -1):
        g_re, g_im = _dev_fft(gpu, dt, re, im, direction, pl)
        _check(f"any:{n}", dt, n, g_re, g_im, _ref(re, im, direction))


def test_large_lengths_f64(gpu):
    """3 * 2^20 (M = 2^23) and 2^24 + 1 (M = 2^26, 2 GiB of workspace), forward, f64: ~40 s, most of it the long-double
    reference on the host."""
    for n in (3 << 20, (1 << 24) + 1):
        re, im = _input(n, "f64")
        pl = gpu.PlannerAny64(n)
        g_re, g_im = _dev_fft(gpu, "f64", re, im, 1, pl)
        _check(f"any:{n}", "f64", n, g_re, g_im, _ref(re, im, 1))
        del pl


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_powers_of_two_are_the_dit_path(gpu, dt):
    """N = 2^k: the power-of-two path itself, bit for bit (no workspace)"""
    import torch

    for k in range(0, 23):
        n = 1 << k
        re, im = _input(n, dt, seed=k)
        pa = _planner(gpu, dt, n)
        pd = (gpu.PlannerDit64 if dt == "f64" else gpu.PlannerDit32)(n)
        assert pa.workspace_len(4) == 0
        for direction in (gpu.Direction.Forward, gpu.Direction.Reverse):
            a_re, a_im = torch.from_numpy(re.copy()).cuda(), torch.from_numpy(im.copy()).cuda()
            b_re, b_im = a_re.clone(), a_im.clone()
            gpu.fft_any_batched(a_re, a_im, n, direction, pa)
            gpu.fft_dit_batched(b_re, b_im, n, direction, pd)
            assert torch.equal(a_re, b_re) and torch.equal(a_im, b_im), (dt, k)


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_round_trip(gpu, dt):
    for n in (3, 17, 1000, 65537, 1_000_003):
        re, im = _input(n, dt, seed=2)
        pl = _planner(gpu, dt, n)
        f_re, f_im = _dev_fft(gpu, dt, re, im, 1, pl)
        b_re, b_im = _dev_fft(gpu, dt, f_re, f_im, -1, pl)
        rel = tol.rel_l2(b_re, b_im, re.astype(np.float64), im.astype(np.float64))
        assert rel <= 2 * any_gates(dt, n)[0], (dt, n, rel)


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_batches_chunks_and_unaligned_planes(gpu, dt):
    """dist > N, planes at buf[1:], a workspace of 2 transforms for 5 (three chunks): every transform bit-identical to the same
    transform run alone; the elements between the transforms untouched"""
    import torch

    P = gpu
    n, batch, dist = 1000, 5, 1003
    pl = _planner(P, dt, n)
    ndt = np.float64 if dt == "f64" else np.float32
    buf_re = np.full(1 + (batch - 1) * dist + n, 7.0, ndt)
    buf_im = np.full_like(buf_re, -7.0)
    singles = []
    for b in range(batch):
        re, im = _input(n, dt, seed=10 + b)
        buf_re[1 + b * dist:1 + b * dist + n], buf_im[1 + b * dist:1 + b * dist + n] = re, im
        singles.append(_dev_fft(P, dt, re, im, 1, pl))
    d_re, d_im = torch.from_numpy(buf_re.copy()).cuda(), torch.from_numpy(buf_im.copy()).cuda()
    work = torch.empty(pl.workspace_len(2) + 1, dtype=d_re.dtype, device="cuda")
    P.fft_any_batched(d_re[1:], d_im[1:], n, P.Direction.Forward, pl, dist=dist, workspace=work)
    g_re, g_im = d_re.cpu().numpy(), d_im.cpu().numpy()
    for b in range(batch):
        s = slice(1 + b * dist, 1 + b * dist + n)
        assert np.array_equal(g_re[s], singles[b][0]) and np.array_equal(g_im[s], singles[b][1]), b
    mask = np.ones(len(buf_re), bool)
    for b in range(batch):
        mask[1 + b * dist:1 + b * dist + n] = False
    assert np.all(g_re[mask] == 7.0) and np.all(g_im[mask] == -7.0)
    # the whole batch in one chunk: the same bits again
    d2_re, d2_im = torch.from_numpy(buf_re.copy()).cuda(), torch.from_numpy(buf_im.copy()).cuda()
    P.fft_any_batched(d2_re[1:], d2_im[1:], n, P.Direction.Forward, pl, dist=dist)
    assert torch.equal(d2_re, d_re) and torch.equal(d2_im, d_im)
    # a workspace below 2 M, and a length that is not the planner's
    with pytest.raises(P.PhastPanic) as ei:
        P.fft_any_batched(d_re[1:], d_im[1:], n, P.Direction.Forward, pl, dist=dist, workspace=work[:2 * pl.m - 1])
    assert ei.value.code == 16
    with pytest.raises(P.PhastPanic) as ei:
        P.fft_any_batched(d_re[:999], d_im[:999], 999, P.Direction.Forward, pl)
    assert ei.value.code == 3


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_host_slices_equal_device_calls(gpu, dt):
    for n in (5, 1000, 4097, 65537):
        re, im = _input(n, dt, seed=3)
        pl = _planner(gpu, dt, n)
        for direction in (1, -1):
            d_re, d_im = _dev_fft(gpu, dt, re, im, direction, pl)
            h_re, h_im = re.copy(), im.copy()
            (gpu.fft_64_any_with_planner if dt == "f64" else gpu.fft_32_any_with_planner)(h_re, h_im, gpu.Direction(direction), pl)
            assert np.array_equal(h_re, d_re) and np.array_equal(h_im, d_im), (n, direction)
            p_re, p_im = re.copy(), im.copy()
            (gpu.fft_64_any if dt == "f64" else gpu.fft_32_any)(p_re, p_im, gpu.Direction(direction))
            assert np.array_equal(p_re, d_re) and np.array_equal(p_im, d_im), (n, direction)


def test_two_threads_two_streams_one_planner(gpu):
    import torch

    n = 1_000_003
    pl = gpu.PlannerAny64(n)
    inputs = [_input(n, "f64", seed=20 + t) for t in range(2)]
    want = [_dev_fft(gpu, "f64", re, im, 1, pl) for re, im in inputs]
    errors = []

    def worker(t):
        try:
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                for _ in range(6):
                    d_re, d_im = torch.from_numpy(inputs[t][0]).cuda(), torch.from_numpy(inputs[t][1]).cuda()
                    gpu.fft_64_any_with_planner(d_re, d_im, gpu.Direction.Forward, pl)
                    got = (d_re.cpu().numpy(), d_im.cpu().numpy())
                    if not (np.array_equal(got[0], want[t][0]) and np.array_equal(got[1], want[t][1])):
                        errors.append(t)
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    th = [threading.Thread(target=worker, args=(t,)) for t in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_graph_capture(gpu, dt):
    """one _dev call captured on a side stream (a single-stream linear capture), replayed twice: the eager result"""
    import torch

    n = 10 ** 5
    re, im = _input(n, dt, seed=4)
    pl = _planner(gpu, dt, n)
    want = _dev_fft(gpu, dt, re, im, 1, pl)
    src_re, src_im = torch.from_numpy(re).cuda(), torch.from_numpy(im).cuda()
    d_re, d_im = src_re.clone(), src_im.clone()
    work = torch.empty(pl.workspace_len(1), dtype=d_re.dtype, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # warm-up on the capture stream
        gpu.fft_any_batched(d_re, d_im, n, gpu.Direction.Forward, pl, workspace=work)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        d_re.copy_(src_re)
        d_im.copy_(src_im)
        gpu.fft_any_batched(d_re, d_im, n, gpu.Direction.Forward, pl, workspace=work)
    for _ in range(2):
        d_re.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(d_re.cpu().numpy(), want[0]) and np.array_equal(d_im.cpu().numpy(), want[1])


def test_cpp_mirror(gpu, tmp_path):
    from phastft_amd import build

    lib = build.build()
    exe = str(tmp_path / "any_len_test")
    libdir = os.path.dirname(lib)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "any_len_test.cpp"), "-o", exe, "-L", libdir, "-lphastft_hip",
                        f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, "gpu"], capture_output=True, text=True)
    sys.stdout.write(r.stdout)
    assert r.returncode == 0 and "any_len: ok" in r.stdout, r.stdout + r.stderr


def test_gates_keep_their_margin():
    """the gates above sit >= 3.7 x over the worst error measured on the MI355X over seeds 0-3 (tolerances.py's rule)"""
    budget = json.load(open(os.path.join(ROOT, "tests", "golden", "any_len_error_budget.json")))
    assert budget["entries"]
    for e in budget["entries"]:
        g_rel, g_bin = any_gates(e["dt"], e["n"])
        assert g_rel >= 3.7 * e["rel"] and g_bin >= 3.7 * e["bin"], e
