"""The Lomb-Scargle periodogram on the MI355X (csrc/lomb.hip, csrc/planner_lomb.hpp) against tests/lomb_reference.py, the
definitions in long double with exact phases, on signals that are exact in both types.

The gate (tests/test_lomb_cpu.py: lomb_gate) on max_k |got - ref| / max_k |ref|: C_L g3 / sqrt(d) for power and normalize,
C_L g3 / d for amplitude, g3 the type-3 gate of the inner planner and d the smallest clamped CCt or SSt over the gated
frequencies (>= 0.01; the others, and M = 1, are asserted finite).  The measured worst per case, eps, type, mean setting and
normalisation over the seeds is in tests/golden/lomb_error_budget.json (tests/golden/make_lomb_error_budget.py);
test_gates_keep_their_margin keeps the gates 2 x above every entry."""
import functools
import json
import os

import numpy as np
import pytest

from tests import lomb_reference as R
from tests.test_lomb_cpu import MEANS, lomb_gate, reference

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTS = ["f64", "f32"]
BUDGET = os.path.join(ROOT, "tests", "golden", "lomb_error_budget.json")


def _ndt(dt):
    return np.float64 if dt == "f64" else np.float32


def _tdt(dt):
    import torch

    return torch.float64 if dt == "f64" else torch.float32


@functools.lru_cache(maxsize=None)
def _planner(P, dt, kt, kf, kw, fm, eps):
    w = None if kw is None else np.frombuffer(kw, np.float64)
    return (P.PlannerLomb64 if dt == "f64" else P.PlannerLomb32)(np.frombuffer(kt, np.float64), np.frombuffer(kf, np.float64), w, fm, eps)


def planner(P, dt, t, f, w, fm, eps):
    """one planner per (type, times, frequencies, weights, mean setting, eps), shared by the tests"""
    raw = lambda v: None if v is None else np.ascontiguousarray(v, np.float64).tobytes()  # noqa: E731
    return _planner(P, dt, raw(t), raw(f), raw(w), bool(fm), eps)


def run(P, pl, y, norm, work=None, stream=None):
    """one signal through lombscargle_batched: the input is never written, nothing is written past the output"""
    import torch

    amp = norm == "amplitude"
    d_y = torch.from_numpy(np.ascontiguousarray(y, dtype=pl._dtype)).cuda()
    keep = d_y.clone()
    k = pl.k_freqs
    outs = [torch.full((k + 3,), 7.0, dtype=d_y.dtype, device="cuda") for _ in range(2 if amp else 1)]
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())  # the fills above
    o = tuple(b[:k] for b in outs)
    P.lombscargle_batched(d_y, pl, norm, out=o if amp else o[0], work=work, stream=stream)
    torch.cuda.synchronize()
    assert torch.equal(d_y, keep)
    got = [b.cpu().numpy() for b in outs]
    assert all((g[k:] == 7.0).all() for g in got)
    return got[0][:k] + 1j * got[1][:k] if amp else got[0][:k]


def as64(v):
    return v.astype(np.complex128 if np.iscomplexobj(v) else np.float64)


def measure(P, dt, ref, eps, fm, norm, seeds=R.SEEDS):
    """(worst error over the seeds, weights and none; the smallest d; the planner)"""
    worst, d = 0.0, 1.0
    for weighted in (False, True):
        pl = planner(P, dt, ref.t, ref.f, ref.w if weighted else None, fm, eps)
        key = (weighted, fm, dt)
        for sd in seeds:
            got = as64(run(P, pl, ref.y[sd], norm))
            assert np.isfinite(got).all(), (ref.case, dt, eps, weighted, fm, norm, sd)
            worst = max(worst, R.error(got, ref.ref[(weighted, fm, norm, sd, dt)], ref.mask[key]))
        d = min(d, ref.d[key])
    return worst, d, pl


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
@pytest.mark.parametrize("dt", DTS)
def test_parity(gpu, dt, case):
    """every eps of the type, weights and none, both mean settings, the three normalisations (M = 1: power), seeds 0-1"""
    ref = reference(case)
    for eps in R.EPS[dt]:
        for fm in MEANS:
            for norm in ref.norms():
                err, d, pl = measure(gpu, dt, ref, eps, fm, norm)
                gate = lomb_gate(dt, 2 * pl.grid_len, eps, ref.q, d, norm)
                print(f"lomb {R.case_id(case)} {dt} eps {eps:g} fm {int(fm)} {norm}: n_f {pl.grid_len} d {d:.3g} err {err:.3e} / {gate:.3e}")
                assert err <= gate, (case, dt, eps, fm, norm, err, gate)
                assert pl.slab == 2048 and pl.workspace_len(3) > 3 * (case[0] + 2 * case[1] + 4 * pl.grid_len)


@pytest.mark.parametrize("case", [R.CASES[2], R.CASES[3]], ids=R.case_id)
@pytest.mark.parametrize("dt", DTS)
def test_offset_signal(gpu, dt, case):
    """y + 1000 with the floating mean gives the centred signal's result within the same gate (the long double reference of
    the offset signal IS the centred one's): this fails if Y is taken off after the transform, at eps |c| of the offset"""
    ref = reference(case, 1000.0)
    eps = R.EPS[dt][-1]
    for norm in R.NORMS:
        err, d, pl = measure(gpu, dt, ref, eps, True, norm)
        gate = lomb_gate(dt, 2 * pl.grid_len, eps, ref.q, d, norm)
        print(f"lomb offset {R.case_id(case)} {dt} {norm}: err {err:.3e} / {gate:.3e}")
        assert err <= gate, (case, dt, norm, err, gate)


@pytest.mark.parametrize("case", [R.CASES[3], (301, 64, "far")], ids=R.case_id)
@pytest.mark.parametrize("dt", DTS)
def test_bit_for_bit(gpu, dt, case):
    """a signal alone has the bits of the same signal as the last of batch 3, in a workspace of workspace_min(), at
    element-aligned pointers and odd distances, on a side stream, under graph replay and through the host form"""
    import torch

    eps = R.EPS[dt][1]
    t, f = R.points(case)
    m, k = len(t), len(f)
    batch = 3
    rows = [R.signal(case, 20 + i, 3.0 * i) for i in range(batch)]
    for fm in MEANS:
        pl = planner(gpu, dt, t, f, R.weights(case), fm, eps)
        for norm in R.NORMS:
            amp = norm == "amplitude"
            alone = [run(gpu, pl, v, norm) for v in rows]
            planes = lambda v: (v.real, v.imag) if amp else (v,)  # noqa: E731
            sig_dist, out_dist = (m + 5) | 1, (k + 3) | 1
            buf = torch.full((1 + batch * sig_dist + 4,), 9.0, dtype=_tdt(dt), device="cuda")
            assert buf[1:].data_ptr() % 16 == np.dtype(_ndt(dt)).itemsize
            y = buf[1:1 + batch * sig_dist].view(batch, sig_dist)[:, :m]
            for i in range(batch):
                y[i] = torch.from_numpy(np.ascontiguousarray(rows[i], dtype=_ndt(dt)))
            keep = buf.clone()
            for name, size in {"workspace_min": pl.workspace_min(), "chunks of 2": pl.workspace_len(2) + 1, "one chunk": pl.workspace_len(batch)}.items():
                outs = [torch.full((1 + batch * out_dist + 4,), 9.0, dtype=_tdt(dt), device="cuda") for _ in range(2 if amp else 1)]
                o = tuple(b[1:1 + batch * out_dist].view(batch, out_dist)[:, :k] for b in outs)
                gpu.lombscargle_batched(y, pl, norm, out=o if amp else o[0], work=torch.empty(size, dtype=_tdt(dt), device="cuda"))
                torch.cuda.synchronize()
                assert torch.equal(buf, keep), name  # the input and its gaps are not written
                for plane, b in enumerate(outs):
                    got = b.cpu().numpy()
                    assert got[0] == 9.0 and (got[1 + (batch - 1) * out_dist + k:] == 9.0).all(), name
                    for i in range(batch):
                        at = 1 + i * out_dist
                        assert np.array_equal(got[at:at + k], planes(alone[i])[plane]), (fm, norm, name, plane, i)
                        if i + 1 < batch:
                            assert (got[at + k:at + out_dist] == 9.0).all(), (name, plane, i)
            # 16-byte aligned rows at a distance that is a multiple of the group: the 16-byte post sweep
            v_dist = (k + 7) & ~3
            outs = [torch.full((batch * v_dist,), 9.0, dtype=_tdt(dt), device="cuda") for _ in range(2 if amp else 1)]
            o = tuple(b.view(batch, v_dist)[:, :k] for b in outs)
            gpu.lombscargle_batched(y, pl, norm, out=o if amp else o[0])
            torch.cuda.synchronize()
            for plane, b in enumerate(outs):
                got = b.cpu().numpy().reshape(batch, v_dist)
                assert (got[:, k:] == 9.0).all()
                for i in range(batch):
                    assert np.array_equal(got[i, :k], planes(alone[i])[plane]), (fm, norm, "16-byte rows", plane, i)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            assert np.array_equal(run(gpu, pl, rows[1], norm, stream=side), alone[1]), (fm, norm, "side stream")
            # the host form
            host = gpu.lombscargle_f64_with_planner if dt == "f64" else gpu.lombscargle_f32_with_planner
            h_re, h_im = np.zeros(k, _ndt(dt)), np.zeros(k, _ndt(dt))
            host(np.ascontiguousarray(rows[2], dtype=_ndt(dt)), h_re, pl, norm, h_im if amp else None)
            assert np.array_equal(h_re, planes(alone[2])[0]) and (not amp or np.array_equal(h_im, alone[2].imag)), (fm, norm, "host")
        # graph replay, power, on new data
        d_y = torch.zeros(m, dtype=_tdt(dt), device="cuda")
        out = torch.zeros(k, dtype=_tdt(dt), device="cuda")
        work = torch.empty(pl.workspace_len(1), dtype=_tdt(dt), device="cuda")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):  # warm-up on the capture stream
            gpu.lombscargle_batched(d_y, pl, "power", out=out, work=work)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            gpu.lombscargle_batched(d_y, pl, "power", out=out, work=work)
        for seed in (41, 42):
            v = R.signal(case, seed)
            want = run(gpu, pl, v, "power")
            d_y.copy_(torch.from_numpy(np.ascontiguousarray(v, dtype=_ndt(dt))))
            out.zero_()
            g.replay()
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy(), want), (fm, seed)


def lomb_case(P, dt, case, eps, fm, norm):
    """one call of batch 3 for tests/test_gpu_workspace_guard.py's drive()"""
    import torch

    from tests import test_gpu_workspace_guard as G

    ref = reference(case)
    pl = planner(P, dt, ref.t, ref.f, ref.w, fm, eps)
    m, k = case[0], case[1]
    sig_dist, out_dist = (m + 5) | 1, (k + 3) | 1
    seeds = [0, 1, 0]
    amp = norm == "amplitude"

    def call(tn, work):
        y = torch.as_strided(tn["y"], (G.BATCH, m), (sig_dist, 1))
        o = tuple(torch.as_strided(tn[key], (G.BATCH, k), (out_dist, 1)) for key in (("out_re", "out_im") if amp else ("out_re",)))
        P.lombscargle_batched(y, pl, norm, out=o if amp else o[0], work=work)

    def gate(got):
        key = (True, fm, dt)
        g = lomb_gate(dt, 2 * pl.grid_len, eps, ref.q, ref.d[key], norm)
        for i, sd in enumerate(seeds):
            v = as64(got["out_re"][i]) + (1j * as64(got["out_im"][i]) if amp else 0)
            assert R.error(v, ref.ref[(True, fm, norm, sd, dt)], ref.mask[key]) <= g, (case, dt, i)

    planes = [G.Plane("y", "in", m, sig_dist, [ref.y[sd].astype(_ndt(dt)) for sd in seeds]), G.Plane("out_re", "out", k, out_dist)]
    if amp:
        planes.append(G.Plane("out_im", "out", k, out_dist))
    lengths = G._lengths(pl.workspace_min(), pl.workspace_len(2) + 1, pl.workspace_len(G.BATCH))
    return G.Case(f"lomb:{R.case_id(case)}:{norm}", dt, 2 * pl.grid_len, planes, lengths, call, gate)


@pytest.mark.parametrize("fm,norm", [(True, "amplitude"), (False, "normalize")])
@pytest.mark.parametrize("dt", DTS)
def test_arena(gpu, dt, fm, norm):
    """one case in the poisoned, guarded arena: workspace lengths workspace_min(), that plus 1, chunks of two plus 1 and
    workspace_len(3) at bases 0, 1 and 16 / itemsize - 1 elements past a 16-byte boundary -- bands whole, inputs kept, the
    bits of a zero-filled workspace, the gaps keep their sentinel, and one element below workspace_min() is refused with
    nothing written"""
    from tests import test_gpu_workspace_guard as G

    case = lomb_case(gpu, dt, R.CASES[3], R.EPS[dt][1], fm, norm)
    G.drive(gpu, case)
    G.overrun(gpu, case, "out_re")


@pytest.mark.parametrize("dt", DTS)
def test_planted_sinusoid(gpu, dt):
    """300 random times, a sinusoid at one of 257 frequencies under noise: the argmax is the planted bin, and normalize stays
    in [0, 1 + gate]"""
    rng = np.random.default_rng(61)
    t = rng.uniform(0, R.SPAN, 300)
    f = np.linspace(0.05, 5.0, 257)
    planted = 101
    y = (2.0 * np.sin(2 * np.pi * f[planted] * t + 0.7) + 0.5 * rng.standard_normal(300) + 10.0).astype(np.float32).astype(np.float64)
    eps = R.EPS[dt][-1]
    pl = planner(gpu, dt, t, f, None, True, eps)
    from tests import nufft_t3_reference as R3

    for norm in ("power", "normalize"):
        got = as64(run(gpu, pl, y, norm))
        assert int(np.argmax(got)) == planted, (norm, int(np.argmax(got)))
    d = R.smallest_d(R.tables(t, f, R.normalised(None, 300), True, R.EPSNEG[dt]))
    assert d >= R.D_MIN
    gate = lomb_gate(dt, 2 * pl.grid_len, eps, R3.conditioning(t, f), d, "normalize")
    assert got.min() >= -gate and got.max() <= 1 + gate and got.max() > 0.8, (got.min(), got.max())


@pytest.mark.parametrize("dt", DTS)
def test_convenience_against_scipy(gpu, dt):
    """lombscargle(x, y, freqs, ...) with scipy's argument meanings on a centred case, leading axes as batches, against scipy
    within the gate plus scipy's own 1e-10 / d (tests/test_lomb_cpu.py)"""
    import torch
    from scipy.signal import lombscargle

    case = R.CASES[2]
    ref = reference(case)
    ys = np.stack([ref.y[0], ref.y[1]]).reshape(2, 1, -1)
    dev = torch.from_numpy(ys.astype(_ndt(dt))).cuda()
    eps = R.EPS[dt][-1]
    for normalize, norm in ((False, "power"), (True, "normalize"), ("amplitude", "amplitude")):
        for fm in MEANS:
            got = gpu.lombscargle(ref.t, dev, 2 * np.pi * ref.f, False, normalize, weights=ref.w, floating_mean=fm, eps=eps)
            assert got.shape == (2, 1, case[1]) and got.is_complex() == (norm == "amplitude")
            key = (True, fm, dt)
            pl = planner(gpu, dt, ref.t, ref.f, ref.w, fm, eps)
            gate = lomb_gate(dt, 2 * pl.grid_len, eps, ref.q, ref.d[key], norm) + 1e-10 / ref.d[key]
            for i in range(2):
                want = lombscargle(ref.t, ref.y[i], 2 * np.pi * ref.f, normalize=normalize, weights=ref.w, floating_mean=fm)
                assert R.error(as64(got[i, 0].cpu().numpy()), want, ref.mask[key]) <= gate, (normalize, fm, i)
    pre = gpu.lombscargle(ref.t, dev[0, 0] + 5.0, 2 * np.pi * ref.f, precenter=True, eps=eps)
    want = lombscargle(ref.t, ref.y[0] - ref.y[0].mean(), 2 * np.pi * ref.f)
    key = (False, False, dt)
    assert ref.mask[key].all()
    assert R.error(as64(pre.cpu().numpy()), want) <= lomb_gate(dt, 2 * pl.grid_len, eps, ref.q, ref.d[key], "power") + 1e-10 / ref.d[key]


@pytest.mark.parametrize("dt", DTS)
def test_codes_describe_and_stages(gpu, dt):
    """null planes, a missing imaginary plane for amplitude, short distances, a short workspace and a wrong length come back
    with their codes and run nothing; describe names the parts; the stage timer leaves the result behind"""
    import ctypes as C

    import torch

    from phastft_amd import _lib

    case = R.CASES[2]
    ref = reference(case)
    m, k = case[0], case[1]
    pl = planner(gpu, dt, ref.t, ref.f, None, True, R.EPS[dt][1])
    dev = getattr(_lib.lib(), f"phast_lombscargle_{dt}_dev")
    big = torch.zeros(m + 2 * k + pl.workspace_len(2), dtype=_tdt(dt), device="cuda")
    at = lambda off: C.c_void_p(big.data_ptr() + off * big.element_size())  # noqa: E731
    py, por, poi, pw, n_ = at(0), at(m), at(m + k), at(m + 2 * k), C.c_size_t
    size = n_(pl.workspace_len(1))
    assert dev(None, por, poi, n_(m), n_(1), n_(m), n_(k), 0, pl._h, pw, size, None) == 16
    assert dev(py, None, poi, n_(m), n_(1), n_(m), n_(k), 0, pl._h, pw, size, None) == 16
    assert dev(py, por, None, n_(m), n_(1), n_(m), n_(k), 2, pl._h, pw, size, None) == 16      # amplitude needs out_im
    assert dev(py, por, poi, n_(m), n_(1), n_(m), n_(k), 3, pl._h, pw, size, None) == 16      # no such normalisation
    assert dev(py, por, poi, n_(m), n_(1), n_(m), n_(k), 0, pl._h, None, size, None) == 16
    assert dev(py, por, poi, n_(m), n_(1), n_(m), n_(k), 0, pl._h, pw, n_(pl.workspace_min() - 1), None) == 16
    assert dev(py, por, poi, n_(m), n_(2), n_(m - 1), n_(k), 0, pl._h, pw, size, None) == 16  # sig_dist below the row
    assert dev(py, por, poi, n_(m), n_(2), n_(m), n_(k - 1), 0, pl._h, pw, size, None) == 16  # out_dist below the row
    assert dev(py, por, poi, n_(m - 1), n_(1), n_(m), n_(k), 0, pl._h, pw, size, None) == 3   # PHAST_ERR_PLANNER_SIZE
    assert dev(py, por, poi, n_(m), n_(0), n_(m), n_(k), 0, pl._h, None, n_(0), None) == 0    # an empty batch
    torch.cuda.synchronize()
    assert not bool(big.any())  # none of the refused calls ran
    assert dev(py, por, None, n_(m), n_(1), n_(m), n_(k), 0, pl._h, pw, size, None) == 0      # power needs no out_im
    torch.cuda.synchronize()
    text = pl.describe()
    assert text.startswith(f"lomb M={m} K={k} floating_mean slab=2048 x 1 around nufft_t3 M={m} K={k} eps=")
    item = np.dtype(_ndt(dt)).itemsize
    assert pl.device_bytes() >= (m + 4 * k) * item and pl.workspace_min() == pl.workspace_len(1)
    host = gpu.lombscargle_f64_with_planner if dt == "f64" else gpu.lombscargle_f32_with_planner
    y = np.ascontiguousarray(ref.y[0], dtype=_ndt(dt))
    with pytest.raises(gpu.PhastPanic) as e:
        host(y[:-1].copy(), np.zeros(k, _ndt(dt)), pl)
    assert e.value.code == 3
    with pytest.raises(gpu.PhastPanic) as e:
        host(y, np.zeros(k - 1, _ndt(dt)), pl)
    assert e.value.code == 2  # PHAST_ERR_LEN_MISMATCH
    want = run(gpu, pl, ref.y[0], "power")
    d_y, d_o = torch.from_numpy(y).cuda(), torch.zeros(k, dtype=_tdt(dt), device="cuda")
    st = pl.time_stages(d_y, d_o, None, 1, "power", reps=1)
    assert len(st) == 3 and all(v >= 0 for v in st)
    assert np.array_equal(d_o.cpu().numpy(), want)


def budget_keys():
    return {(dt, R.case_id(c), eps, fm, norm) for dt in DTS for c in R.CASES for eps in R.EPS[dt] for fm in MEANS
            for norm in (R.NORMS[:1] if c[0] == 1 else R.NORMS)}


def test_gates_keep_their_margin():
    """the gates sit >= 2 x over the worst errors measured on the MI355X and no case, eps, type, mean setting or
    normalisation is missing"""
    budget = json.load(open(BUDGET))
    have = {(e["dt"], e["case"], e["eps"], e["fm"], e["norm"]) for e in budget["entries"]}
    assert have == budget_keys() and len(budget["entries"]) == len(have)
    for e in budget["entries"]:
        assert lomb_gate(e["dt"], e["n_g"], e["eps"], e["q"], e["d"], e["norm"]) >= 2 * e["err"], e
