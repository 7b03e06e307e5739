#!/usr/bin/env python3
"""Rates of the non-uniform FFT: time per call, the three stages, spread and interpolate in points * w per second, the pre and
deconvolve sweeps' bytes / time against this box's copy rate (phast_stream_probe_dev, measured in the same run), and the whole
call against one n_g-point engine call alone (the power-of-two path of PlannerAny*(n_g), timed in the same way).  Every timed
region starts behind a cache drain (a read of 1 GiB nothing else uses), as bench.py times its regions -- this tool does not
import bench.py.

    python tools/nufft_rate.py [reps] [f64|f32]

End-to-end: device events around `reps` back-to-back calls of one transform.  Stages: PlannerNufft*.time_stages (events between
the three launch groups of one call).  Sweep bytes per transform (T = element size, complex data): pre reads 2 N T and N T of the
table and writes 2 n_g T; deconvolve reads 2 N T of the workspace and N T of the table and writes 2 N T.  The f32 planner takes
eps >= 1e-6, so it has no 1e-12 rows."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import phastft_amd as P  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
ONLY = sys.argv[2] if len(sys.argv) > 2 else None   # one type only
CASES = [(1 << 20, 1 << 20, "uniform"), (1 << 20, 1 << 23, "uniform"), (1 << 16, 1 << 24, "uniform"), (1 << 20, 1 << 20, "clumped")]
EPS = {"f64": (1e-6, 1e-12), "f32": (1e-6,)}

_drain_buf = None


def drain():
    global _drain_buf
    if _drain_buf is None:
        _drain_buf = torch.ones(1 << 27, dtype=torch.float64, device="cuda")
    _drain_buf.sum()


def timed(call, reps=REPS):
    """us per call over `reps` back-to-back calls behind a drain"""
    call()   # warm-up
    torch.cuda.synchronize()
    drain()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def main():
    probe = P.stream_probe(1024, 5)
    copy = probe["copy"]
    print(f"# {P.device_info()['name']}: copy probe {copy:.0f} GB/s (read {probe['read']:.0f}, write {probe['write']:.0f}); reps {REPS}")
    print("# case: t/call; stages in us (a, FFT_n_g, c); gather rate in 1e9 points*w / s; sweep GB/s and fraction of the copy probe;"
          " the call vs FFT_n_g alone")
    rng = np.random.default_rng(0)
    for n, m, kind in CASES:
        x = rng.random(m) if kind == "uniform" else 0.3 + 1e-7 * rng.random(m)   # every point within 1e-7 of 0.3: one or two cells
        for dt, tdt in (("f64", torch.float64), ("f32", torch.float32)):
            for eps in EPS[dt]:
                if (ONLY and dt != ONLY) or (kind == "clumped" and eps != 1e-6):
                    continue
                reps = REPS if kind == "uniform" else 2
                pl = (P.PlannerNufft64 if dt == "f64" else P.PlannerNufft32)(n, x, eps)
                n_g, w, esz = pl.grid_len, pl.width, torch.empty(0, dtype=tdt).element_size()
                work = torch.empty(pl.workspace_len(1), dtype=tdt, device="cuda")
                eng = (P.PlannerAny64 if dt == "f64" else P.PlannerAny32)(n_g)   # a power of two: the engine itself
                w_re, w_im = work[:n_g], work[n_g:2 * n_g]
                t_eng = timed(lambda: P.fft_any_batched(w_re, w_im, n_g, P.Direction.Forward, eng))
                for t in (1, 2):
                    ni, no = (m, n) if t == 1 else (n, m)
                    re = torch.empty(ni, dtype=tdt, device="cuda").uniform_(-1, 1)
                    im = torch.empty(ni, dtype=tdt, device="cuda").uniform_(-1, 1)
                    out = (torch.empty(no, dtype=tdt, device="cuda"), torch.empty(no, dtype=tdt, device="cuda"))
                    fn = P.nufft1_batched if t == 1 else P.nufft2_batched
                    t_call = timed(lambda: fn(re, im, pl, out=out, work=work), reps)
                    drain()
                    torch.cuda.synchronize()
                    st = [v * 1e3 for v in pl.time_stages(t, re, im, out[0], out[1], 1, work, reps)]
                    gather_us, sweep_us = (st[0], st[2]) if t == 1 else (st[2], st[0])
                    sweep_bytes = (5 * n) * esz if t == 1 else (3 * n + 2 * n_g) * esz
                    rate = sweep_bytes / (sweep_us * 1e3)
                    print(f"{dt} type {t} N=2^{n.bit_length() - 1} M=2^{m.bit_length() - 1} {kind} eps={eps:g} w={w} n_g=2^{n_g.bit_length() - 1}:"
                          f" {t_call:10.2f} us/call; stages {st[0]:.1f} {st[1]:.1f} {st[2]:.1f} us;"
                          f" {'spread' if t == 1 else 'interpolate'} {m * w / (gather_us * 1e3):.2f} Gpw/s;"
                          f" {'deconvolve' if t == 1 else 'pre'} {rate:.0f} GB/s = {rate / copy:.2f} of copy;"
                          f" call vs FFT_n_g {t_eng:.1f} us: {t_call / t_eng:.2f} x", flush=True)
                    del re, im, out
                del pl, eng, work, w_re, w_im
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
