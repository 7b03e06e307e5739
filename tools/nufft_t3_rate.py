#!/usr/bin/env python3
"""Rates of the type-3 non-uniform FFT: time per call, the four stages, the fused spread and the interpolation in points * w per
second, the post sweep's bytes / time against this box's copy rate (phast_stream_probe_dev, measured in the same run), and the
whole call against one n_g-point engine call alone (the power-of-two path of PlannerAny*(n_g), timed in the same way).  Every
timed region starts behind a cache drain (a read of 1 GiB nothing else uses), as bench.py times its regions -- this tool does
not import bench.py.

    python tools/nufft_t3_rate.py [reps] [f64|f32]

End-to-end: device events around `reps` back-to-back calls of one transform.  Stages: PlannerNufftT3_*.time_stages (events
between the four launch groups of one call).  Post bytes per transform (T = element size): it reads and writes the two output
planes and reads the two planes of the table, 6 K T.  The sources are uniform on [-1, 1] and the targets uniform on
[-S, S], S = 2^18 - 4, so 8 S X + w is just below 2^21: n_f = 2^21, filled from end to end, and n_g = 2^22.  The f32 planner
takes eps >= 1e-6, so it has no 1e-12 rows."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import phastft_amd as P  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
ONLY = sys.argv[2] if len(sys.argv) > 2 else None   # one type only
CASES = [(1 << 20, 1 << 20), (1 << 23, 1 << 20)]    # (M, K): half a source per cell of n_f, and four
EPS = {"f64": (1e-6, 1e-12), "f32": (1e-6,)}
X, S = 1.0, float((1 << 18) - 4)

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
    print("# case: t/call; stages in us (a spread+pre, b FFT_n_g, c interpolate, d post); gather rates in 1e9 points*w / s; post GB/s and"
          " fraction of the copy probe; the call vs FFT_n_g alone")
    rng = np.random.default_rng(0)
    for m, k in CASES:
        x, s = rng.uniform(-X, X, m), rng.uniform(-S, S, k)
        x[:2], s[:2] = (-X, X), (-S, S)
        for dt, tdt in (("f64", torch.float64), ("f32", torch.float32)):
            for eps in EPS[dt]:
                if ONLY and dt != ONLY:
                    continue
                pl = (P.PlannerNufftT3_64 if dt == "f64" else P.PlannerNufftT3_32)(x, s, eps)
                n_f, w, esz = pl.grid_len, pl.width, torch.empty(0, dtype=tdt).element_size()
                n_g = 2 * n_f
                work = torch.empty(pl.workspace_len(1), dtype=tdt, device="cuda")
                eng = (P.PlannerAny64 if dt == "f64" else P.PlannerAny32)(n_g)   # a power of two: the engine itself
                w_re, w_im = work[:n_g], work[n_g:2 * n_g]
                t_eng = timed(lambda: P.fft_any_batched(w_re, w_im, n_g, P.Direction.Forward, eng))
                re = torch.empty(m, dtype=tdt, device="cuda").uniform_(-1, 1)
                im = torch.empty(m, dtype=tdt, device="cuda").uniform_(-1, 1)
                out = (torch.empty(k, dtype=tdt, device="cuda"), torch.empty(k, dtype=tdt, device="cuda"))
                t_call = timed(lambda: P.nufft3_batched(re, im, pl, out=out, work=work))
                drain()
                torch.cuda.synchronize()
                st = [v * 1e3 for v in pl.time_stages(re, im, out[0], out[1], 1, work, REPS)]
                rate = 6 * k * esz / (st[3] * 1e3)
                print(f"{dt} M=2^{m.bit_length() - 1} K=2^{k.bit_length() - 1} eps={eps:g} w={w} n_f=2^{n_f.bit_length() - 1}"
                      f" n_g=2^{n_g.bit_length() - 1}: {t_call:10.2f} us/call; stages {st[0]:.1f} {st[1]:.1f} {st[2]:.1f} {st[3]:.1f} us;"
                      f" spread {m * w / (st[0] * 1e3):.2f} Gpw/s; interpolate {k * w / (st[2] * 1e3):.2f} Gpw/s;"
                      f" post {rate:.0f} GB/s = {rate / copy:.2f} of copy; call vs FFT_n_g {t_eng:.1f} us: {t_call / t_eng:.2f} x", flush=True)
                del pl, eng, work, w_re, w_im, re, im, out
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
