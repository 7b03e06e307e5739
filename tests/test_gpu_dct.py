"""DCT / DST of types II and III on the MI355X (csrc/dct.hip, csrc/planner_dct.hpp), against scipy.fft.dct / dst / idct / idst
in long double.

Gates: tests/tolerances.py's formulas with log2 N replaced by log2 of the inner real transform's length (inner_m of
tests/test_gpu_any_real.py: the transform is one R2C or C2R of the same N between two sweeps), times the any-length factor 2.
The measured worst over seeds 0-3 (tests/golden/dct_error_budget.json, written on the MI355X by
tests/golden/make_dct_error_budget.py) sits at least 3 x below them (test_gates_keep_their_margin).  Twiddles of the wrong
angle or evaluated in f32 fail them (tests/test_dct_cpu.py::test_gates_catch_wrong_twiddles)."""
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import scipy.fft as sf

from tests import tolerances as tol
from tests.test_gpu_any_real import inner_m

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANY_FACTOR = 2.0
NORMS = [None, "ortho", "forward"]
KINDS = [("dct", 2), ("dct", 3), ("dst", 2), ("dst", 3)]
NAMED = [1000, 1001, 4094, 4096, 65537, 10 ** 6, 999_999, 1 << 20, 3 << 20]


def dct_gates(dt: str, n: int):
    lm = inner_m(n).bit_length() - 1
    return ANY_FACTOR * tol.rel_gate(dt, lm), ANY_FACTOR * tol.bin_gate(dt, lm)


def _ndt(dt):
    return np.float64 if dt == "f64" else np.float32


def _tdt(dt):
    import torch

    return torch.float64 if dt == "f64" else torch.float32


def _signal(n: int, dt: str, seed: int = 0):
    return np.random.default_rng([seed, n, 11]).uniform(-1, 1, n).astype(_ndt(dt))


def ref(kind: str, t: int, x, norm):
    f = sf.dct if kind == "dct" else sf.dst
    return np.asarray(f(x.astype(np.longdouble), type=t, norm=norm), np.float64)


def errors(got, want):
    z = np.zeros(len(want))
    g = np.asarray(got, np.float64)
    return tol.rel_l2(g, z, want, z), tol.max_bin_err(g, z, want, z)


def check(tag, dt, n, got, want):
    rel, worst = errors(got, want)
    g_rel, g_bin = dct_gates(dt, n)
    tol.record(tag, inner_m(n).bit_length() - 1, rel, worst, g_rel, g_bin)
    assert rel <= g_rel and worst <= g_bin, (tag, dt, n, rel, g_rel, worst, g_bin)


def planner(P, dt, n):
    return (P.PlannerDct64 if dt == "f64" else P.PlannerDct32)(n)


def run_dev(P, dt, kind, t, x, norm, pl):
    """one transform through the device-tensor path; the input tensor is checked unmodified"""
    import torch

    d_x = torch.from_numpy(x.copy()).cuda()
    out = torch.full((len(x),), 5.0, dtype=d_x.dtype, device="cuda")
    (P.dct_batched if kind == "dct" else P.dst_batched)(d_x, out, pl, 1, type=t, norm=norm)
    assert np.array_equal(d_x.cpu().numpy(), x)
    return out.cpu().numpy()


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_every_length_up_to_300(gpu, dt):
    for n in range(1, 301):
        pl = planner(gpu, dt, n)
        x = _signal(n, dt)
        for kind, t in KINDS:
            for norm in NORMS:
                check(f"{kind}{t}:{norm}:{n}", dt, n, run_dev(gpu, dt, kind, t, x, norm, pl), ref(kind, t, x, norm))


@pytest.mark.parametrize("n", NAMED)
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_named_lengths(gpu, dt, n):
    pl = planner(gpu, dt, n)
    x = _signal(n, dt, seed=1)
    for kind, t in KINDS:
        for norm in NORMS if n < 10 ** 5 else [None]:
            check(f"{kind}{t}:{norm}:{n}", dt, n, run_dev(gpu, dt, kind, t, x, norm, pl), ref(kind, t, x, norm))


def test_large_length_f32(gpu):
    n = 1 << 24
    pl = planner(gpu, "f32", n)
    x = _signal(n, "f32", seed=2)
    for kind, t in KINDS:
        check(f"{kind}{t}:None:{n}", "f32", n, run_dev(gpu, "f32", kind, t, x, None, pl), ref(kind, t, x, None))


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_round_trip(gpu, dt):
    """idct(dct(x)) and idst(dst(x)) for every norm and both types, through the Python inverse mapping"""
    import torch

    for n in (1, 2, 7, 100, 1000, 4096, 65537):
        x = _signal(n, dt, seed=3)
        d_x = torch.from_numpy(x).cuda()
        for kind in ("dct", "dst"):
            fwd = getattr(gpu, f"{kind}_{dt}")
            inv = gpu.idct if kind == "dct" else gpu.idst
            for t in (2, 3):
                for norm in NORMS:
                    y, z = torch.empty_like(d_x), torch.empty_like(d_x)
                    fwd(d_x, y, type=t, norm=norm)
                    inv(y, z, type=t, norm=norm)
                    check(f"round:{kind}{t}:{norm}:{n}", dt, n, z.cpu().numpy(), x.astype(np.float64))


@pytest.mark.parametrize("n", [1, 2, 3, 1001, 4096, 10_002])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_bits_do_not_depend_on_the_call(gpu, dt, n):
    """batch vs single, chunked vs full workspace, host slice vs _dev, in place vs out of place, buf[1:] views and odd
    distances vs aligned ones: the same bits; out of place the input is never written"""
    import torch

    pl = planner(gpu, dt, n)
    batch = 5
    xs = np.stack([_signal(n, dt, seed=10 + b) for b in range(batch)])
    fns = {"dct": (gpu.dct_batched, getattr(gpu, f"dct_{dt}_with_planner")),
           "dst": (gpu.dst_batched, getattr(gpu, f"dst_{dt}_with_planner"))}
    for kind, t in KINDS:
        batched, host = fns[kind]
        for norm in NORMS:
            single = np.stack([run_dev(gpu, dt, kind, t, xs[b], norm, pl) for b in range(batch)])
            h = np.empty(n, _ndt(dt))
            host(xs[0], h, pl, type=t, norm=norm)
            assert np.array_equal(h, single[0]), (kind, t, norm, "host")
            d_in = torch.from_numpy(xs.reshape(-1).copy()).cuda()
            out = torch.zeros(batch * n, dtype=_tdt(dt), device="cuda")
            batched(d_in, out, pl, batch, type=t, norm=norm)
            assert np.array_equal(out.cpu().numpy().reshape(batch, n), single), (kind, t, norm, "batch")
            assert np.array_equal(d_in.cpu().numpy(), xs.reshape(-1)), (kind, t, norm, "input written")
            small = torch.empty(pl.workspace_len(1), dtype=_tdt(dt), device="cuda")  # one transform per chunk
            out.zero_()
            batched(d_in, out, pl, batch, type=t, norm=norm, workspace=small)
            assert np.array_equal(out.cpu().numpy().reshape(batch, n), single), (kind, t, norm, "chunked")
            two = torch.empty(pl.workspace_len(2) + 1, dtype=_tdt(dt), device="cuda")[1:]  # two per chunk, unaligned base
            out.zero_()
            batched(d_in, out, pl, batch, type=t, norm=norm, workspace=two)
            assert np.array_equal(out.cpu().numpy().reshape(batch, n), single), (kind, t, norm, "chunked, unaligned ws")
            inpl = d_in.clone()
            batched(inpl, inpl, pl, batch, type=t, norm=norm)
            assert np.array_equal(inpl.cpu().numpy().reshape(batch, n), single), (kind, t, norm, "in place")
            # odd distances on buf[1:] views
            di, do = n + 3, n + 1
            buf_in = torch.zeros(1 + batch * di, dtype=_tdt(dt), device="cuda")
            view_in = buf_in[1:]
            for b in range(batch):
                view_in[b * di:b * di + n] = torch.from_numpy(xs[b])
            keep = view_in.cpu().numpy()
            buf_out = torch.zeros(1 + batch * do, dtype=_tdt(dt), device="cuda")
            batched(view_in, buf_out[1:], pl, batch, type=t, norm=norm, in_dist=di, out_dist=do)
            got = buf_out[1:].cpu().numpy()
            for b in range(batch):
                assert np.array_equal(got[b * do:b * do + n], single[b]), (kind, t, norm, "views", b)
            assert np.array_equal(view_in.cpu().numpy(), keep)


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_two_streams_and_threads_one_planner(gpu, dt):
    """two threads, each on its own stream, share one planner: every result equals the single-stream one"""
    import torch

    n, batch = 99_999, 3
    pl = planner(gpu, dt, n)
    xs = np.stack([_signal(n, dt, seed=20 + b) for b in range(batch)])
    d_in = torch.from_numpy(xs.reshape(-1)).cuda()
    want = {}
    for kind, t in KINDS:
        out = torch.empty_like(d_in)
        (gpu.dct_batched if kind == "dct" else gpu.dst_batched)(d_in, out, pl, batch, type=t, norm="ortho")
        want[(kind, t)] = out.cpu().numpy()
    torch.cuda.synchronize()
    errs = []

    def worker(idx):
        try:
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                for rep in range(3):
                    for kind, t in KINDS[idx::2] + KINDS[1 - idx::2]:
                        out = torch.empty_like(d_in)
                        (gpu.dct_batched if kind == "dct" else gpu.dst_batched)(d_in, out, pl, batch, type=t, norm="ortho")
                        s.synchronize()
                        if not np.array_equal(out.cpu().numpy(), want[(kind, t)]):
                            errs.append((idx, rep, kind, t))
        except Exception as e:  # noqa: BLE001 -- reported below
            errs.append(repr(e))

    th = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errs, errs


@pytest.mark.parametrize("n", [100_002, 99_999, 1 << 16])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_graph_capture(gpu, dt, n):
    """a DCT-II and a DST-III _dev call captured on a side stream, replayed twice: the eager results"""
    import torch

    pl = planner(gpu, dt, n)
    x = _signal(n, dt, seed=4)
    want2 = run_dev(gpu, dt, "dct", 2, x, None, pl)
    want3 = run_dev(gpu, dt, "dst", 3, x, "ortho", pl)
    d_x = torch.from_numpy(x).cuda()
    o2, o3 = torch.zeros_like(d_x), torch.zeros_like(d_x)
    work = torch.empty(pl.workspace_len(1), dtype=d_x.dtype, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on the capture stream
        gpu.dct_batched(d_x, o2, pl, 1, type=2, workspace=work)
        gpu.dst_batched(d_x, o3, pl, 1, type=3, norm="ortho", workspace=work)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        gpu.dct_batched(d_x, o2, pl, 1, type=2, workspace=work)
        gpu.dst_batched(d_x, o3, pl, 1, type=3, norm="ortho", workspace=work)
    for _ in range(2):
        o2.zero_()
        o3.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(o2.cpu().numpy(), want2) and np.array_equal(o3.cpu().numpy(), want3)


def test_cpp_mirror(gpu, tmp_path):
    from phastft_amd import build

    lib = build.build()
    exe = str(tmp_path / "dct_test")
    libdir = os.path.dirname(lib)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "dct_test.cpp"), "-o", exe, "-L", libdir, "-lphastft_hip",
                        f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, "gpu"], capture_output=True, text=True)
    sys.stdout.write(r.stdout)
    assert r.returncode == 0 and "dct: ok" in r.stdout, r.stdout + r.stderr


def test_gates_keep_their_margin():
    """the gates above sit >= 3 x over the worst error measured on the MI355X over seeds 0-3"""
    budget = json.load(open(os.path.join(ROOT, "tests", "golden", "dct_error_budget.json")))
    assert budget["entries"]
    for e in budget["entries"]:
        g_rel, g_bin = dct_gates(e["dt"], e["n"])
        assert g_rel >= 3 * e["rel"] and g_bin >= 3 * e["bin"], e
