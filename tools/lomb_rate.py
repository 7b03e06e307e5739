#!/usr/bin/env python3
"""Rates of the Lomb-Scargle periodogram, in one run: this box's copy rate (phast_stream_probe_dev); the whole call
(floating mean, power) and each of its stages (PlannerLomb*.time_stages: events around the sweeps in front of the transform,
the type-3 call, and the post sweep); the call over the bare type-3 call of the same planner; and the sweeps' bytes / time as
a fraction of copy.  Every timed region starts behind a cache drain (a read of 1 GiB nothing else uses), as bench.py times
its regions -- this tool does not import bench.py.

    python tools/lomb_rate.py [reps]

The times are M uniform random points of [0, M) and the frequencies K equally spaced ones up to 1/2 (the mean Nyquist rate):
n_f = 2 M.  Sweep bytes (T = element size): the first pass reads the signal and the weights (2 M T), the strength sweep reads
both again and writes the strengths (3 M T), each per signal; the post sweep reads A1's two planes and the four tables and
writes the power (7 K T per signal; the weights and the tables are shared by the batch and are counted for every signal, so
the fraction is a lower bound at batch 16).  The yardstick is the DCT's sweeps: 0.75 of copy."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import phastft_amd as P  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
EPS = 1e-6
CASES = [(1 << 20, 1 << 20), (1 << 16, 1 << 20)]  # (M, K)
BATCHES = (1, 16)

_drain_buf = None


def drain():
    global _drain_buf
    if _drain_buf is None:
        _drain_buf = torch.ones(1 << 27, dtype=torch.float64, device="cuda")
    _drain_buf.sum()


def timed(fn):
    """us per call of `reps` back-to-back calls behind a drain"""
    fn()  # warm-up
    torch.cuda.synchronize()
    drain()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS * 1e3


def main():
    probe = P.stream_probe(1024, 5)
    copy = probe["copy"]
    print(f"# {P.device_info()['name']}: copy probe {copy:.0f} GB/s (read {probe['read']:.0f}, write {probe['write']:.0f}); reps {REPS}; eps {EPS:g}")
    print("# case: t/call; stages in us (sweeps in front / type-3 call / post sweep); the call over its type-3 stage; the sweeps' GB/s as"
          " a fraction of copy (yardstick: the DCT sweeps' 0.75)")
    for dt, tdt in (("f64", torch.float64), ("f32", torch.float32)):
        for m, k in CASES:
            rng = np.random.default_rng(m + k)
            t = rng.uniform(0.0, float(m), m)
            f = np.arange(1, k + 1) * (0.5 / k)
            pl = (P.PlannerLomb64 if dt == "f64" else P.PlannerLomb32)(t, f, None, True, EPS)
            esz = torch.empty(0, dtype=tdt).element_size()
            for batch in BATCHES:
                y = torch.empty((batch, m), dtype=tdt, device="cuda").uniform_(-1, 1)
                out = torch.empty((batch, k), dtype=tdt, device="cuda")
                work = torch.empty(pl.workspace_len(batch), dtype=tdt, device="cuda")
                t_call = timed(lambda: P.lombscargle_batched(y, pl, "power", out=out, work=work))
                drain()
                torch.cuda.synchronize()
                st = [v * 1e3 for v in pl.time_stages(y.reshape(-1), out.reshape(-1), None, batch, "power", work, REPS)]
                b_pre, b_post = 5 * m * esz * batch, 7 * k * esz * batch
                r_pre, r_post = b_pre / (st[0] * 1e3), b_post / (st[2] * 1e3)
                print(f"{dt} lomb {batch} x M={m} K={k} (n_f {pl.grid_len}, slab {pl.slab} x {-(-m // pl.slab)}): {t_call:9.1f} us;"
                      f" stages {st[0]:.1f} / {st[1]:.1f} / {st[2]:.1f} us; call = {sum(st) / st[1]:.3f} x its type-3 stage;"
                      f" sweeps in front {b_pre / 1e6:.0f} MB at {r_pre:.0f} GB/s = {r_pre / copy:.2f} copy, post {b_post / 1e6:.0f} MB at"
                      f" {r_post:.0f} GB/s = {r_post / copy:.2f} copy", flush=True)
                del y, out, work
            del pl
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
