#!/usr/bin/env python3
"""Rates of the three-dimensional non-uniform FFT: time per call, the three stages, spread and interpolate in points * w^3 per
second, the pre and deconvolve sweeps' bytes / time against this box's copy rate (phast_stream_probe_dev, measured in the same
run), and the whole call against one 3-D transform of the (g1, g2, g3) grid alone (PlannerNd*((g1, g2, g3)), timed in the same
way).  Every timed region starts behind a cache drain (a read of 1 GiB nothing else uses), as bench.py times its regions -- this
tool does not import bench.py.  Beside them, one case of tools/nufft2d_rate.py (f64, 1024 x 1024 modes, M = 2^22, eps 1e-6) in
points * w^2 per second of the untiled 2-D spread kernel: the one figure the tiled kernel can be read against.

    python tools/nufft3d_rate.py [reps] [f64|f32] [log]

writes what it prints to `log` (profiles/nufft3d_rate.log by default).  Without a GPU the log says "unmeasured" and names this
command.

End-to-end: device events around `reps` back-to-back calls of one transform.  Stages: PlannerNufft3d*.time_stages (events
between the three launch groups of one call).  Sweep bytes per transform (T = element size, complex data, N = N1 N2 N3,
G = g1 g2 g3): pre reads 2 N T (and the tables) and writes 2 G T; deconvolve reads 2 N T of the workspace and writes 2 N T.
The f32 planner takes eps >= 1e-6, so it has no 1e-12 rows."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
ONLY = sys.argv[2] if len(sys.argv) > 2 and sys.argv[2] in ("f64", "f32") else None   # one type only
LOG = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "nufft3d_rate.log")
CASES = [((128, 128, 128), 1 << 22), ((128, 128, 128), 1 << 24)]   # uniform points
EPS = {"f64": (1e-6, 1e-12), "f32": (1e-6,)}

_drain_buf = None
_lines = []


def say(line):
    print(line, flush=True)
    _lines.append(line)


def drain(torch):
    global _drain_buf
    if _drain_buf is None:
        _drain_buf = torch.ones(1 << 27, dtype=torch.float64, device="cuda")
    _drain_buf.sum()


def timed(torch, call, reps=REPS):
    """us per call over `reps` back-to-back calls behind a drain"""
    call()   # warm-up
    torch.cuda.synchronize()
    drain(torch)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def main():
    import numpy as np
    import torch

    import phastft_amd as P

    probe = P.stream_probe(1024, 5)
    copy = probe["copy"]
    say(f"# {P.device_info()['name']}: copy probe {copy:.0f} GB/s (read {probe['read']:.0f}, write {probe['write']:.0f}); reps {REPS}")
    say("# case: t/call; stages in us (a, FFT of the grid, c); gather rate in 1e9 points*w^3 / s; sweep GB/s and fraction of the"
        " copy probe; the call vs the FFT of the grid alone")
    rng = np.random.default_rng(0)
    for ns, m in CASES:
        x, y, z = rng.random(m), rng.random(m), rng.random(m)
        n = ns[0] * ns[1] * ns[2]
        for dt, tdt in (("f64", torch.float64), ("f32", torch.float32)):
            for eps in EPS[dt]:
                if ONLY and dt != ONLY:
                    continue
                pl = (P.PlannerNufft3d64 if dt == "f64" else P.PlannerNufft3d32)(ns, x, y, z, eps)
                cells, w, esz = pl.grid_len, pl.width, torch.empty(0, dtype=tdt).element_size()
                work = torch.empty(pl.workspace_len(1), dtype=tdt, device="cuda")
                eng = (P.PlannerNd64 if dt == "f64" else P.PlannerNd32)(pl.grid_shape)
                w_re, w_im, w_nd = work[:cells], work[cells:2 * cells], work[2 * cells:]
                w_re.zero_()
                w_im.zero_()
                t_eng = timed(torch, lambda: P.fft_nd_batched(w_re, w_im, P.Direction.Forward, eng, workspace=w_nd))
                for t in (1, 2):
                    ni, no = (m, n) if t == 1 else (n, m)
                    re = torch.empty(ni, dtype=tdt, device="cuda").uniform_(-1, 1)
                    im = torch.empty(ni, dtype=tdt, device="cuda").uniform_(-1, 1)
                    out = (torch.empty(no, dtype=tdt, device="cuda"), torch.empty(no, dtype=tdt, device="cuda"))
                    fn = P.nufft3d1_batched if t == 1 else P.nufft3d2_batched
                    t_call = timed(torch, lambda: fn(re, im, pl, out=out, work=work))
                    drain(torch)
                    torch.cuda.synchronize()
                    st = [v * 1e3 for v in pl.time_stages(t, re, im, out[0], out[1], 1, work, REPS)]
                    gather_us, sweep_us = (st[0], st[2]) if t == 1 else (st[2], st[0])
                    sweep_bytes = (4 * n) * esz if t == 1 else (2 * n + 2 * cells) * esz
                    rate = sweep_bytes / (sweep_us * 1e3)
                    say(f"{dt} type {t} N={'x'.join(map(str, ns))} M=2^{m.bit_length() - 1} eps={eps:g} w={w} grid={'x'.join(map(str, pl.grid_shape))}:"
                        f" {t_call:10.2f} us/call; stages {st[0]:.1f} {st[1]:.1f} {st[2]:.1f} us;"
                        f" {'spread' if t == 1 else 'interpolate'} {m * w ** 3 / (gather_us * 1e3):.2f} Gpw3/s;"
                        f" {'deconvolve' if t == 1 else 'pre'} {rate:.0f} GB/s = {rate / copy:.2f} of copy;"
                        f" call vs FFT of the grid {t_eng:.1f} us: {t_call / t_eng:.2f} x")
                    del re, im, out
                del pl, eng, work, w_re, w_im, w_nd
                torch.cuda.empty_cache()
    # the untiled 2-D spread on the same box: one case of tools/nufft2d_rate.py
    m, eps = 1 << 22, 1e-6
    pl = P.PlannerNufft2d64((1024, 1024), rng.random(m), rng.random(m), eps)
    work = torch.empty(pl.workspace_len(1), dtype=torch.float64, device="cuda")
    re, im = (torch.empty(m, dtype=torch.float64, device="cuda").uniform_(-1, 1) for _ in range(2))
    out = tuple(torch.empty(1024 * 1024, dtype=torch.float64, device="cuda") for _ in range(2))
    P.nufft2d1_batched(re, im, pl, out=out, work=work)
    drain(torch)
    torch.cuda.synchronize()
    st = [v * 1e3 for v in pl.time_stages(1, re, im, out[0], out[1], 1, work, REPS)]
    say(f"2-D f64 type 1 N=1024x1024 M=2^22 eps={eps:g} w={pl.width}: stages {st[0]:.1f} {st[1]:.1f} {st[2]:.1f} us;"
        f" spread {m * pl.width ** 2 / (st[0] * 1e3):.2f} Gpw2/s (untiled: one thread per grid point)")


if __name__ == "__main__":
    try:
        import torch as _torch

        have = _torch.cuda.is_available()
    except Exception:
        have = False
    if have:
        main()
    else:
        say("unmeasured: no GPU here.  Run `python tools/nufft3d_rate.py` on the MI355X.")
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    with open(LOG, "w") as f:
        f.write("\n".join(_lines) + "\n")
