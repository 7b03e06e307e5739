#!/usr/bin/env python3
"""Rates of overlap-save convolution: per number of taps K, the automatic block B and B / 2, 2 B, 4 B -- time per call, ns per
output sample, the call against the batched R2C + C2R of the same rows alone (r2c_any_batched / c2r_any_batched on rows that
already hold the segments) in the same run, and each sweep's bytes / time against this box's copy rate
(phast_stream_probe_dev, measured in the same run).  Every timed region starts behind a cache drain (a read of 1 GiB nothing
else uses), as bench.py times its regions -- this tool does not import bench.py.

    python tools/conv_rate.py [reps]

End-to-end: device events around `reps` back-to-back calls.  Stages: PlannerConv*.time_stages (events between the five stages
of one call).  Sweep bytes (T = element size, fd = B and bd = B / 2 + 1 rounded up to 16 bytes): the segment sweep reads the
signal once from HBM (L T; the K - 1 samples two rows share hit the caches) and writes segs fd T; the spectrum sweep reads
and writes both planes, 4 segs bd T; the save sweep reads and writes out_len T each.  The yardstick is the DCT's sweeps: 0.75
of copy.  One signal of L = 2^24 samples, mode "same", taps uniform(-1, 1)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import phastft_amd as P  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
LENGTH = 1 << 24
TAPS = (32, 1000, 16384)

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
    print(f"# {P.device_info()['name']}: copy probe {copy:.0f} GB/s (read {probe['read']:.0f}, write {probe['write']:.0f}); reps {REPS}")
    print(f"# one signal of L = {LENGTH}, mode same.  case: t/call, ns per output sample, its ratio to the batched R2C + C2R of"
          " the same rows alone; the five stages in us; each sweep's GB/s as a fraction of copy (yardstick 0.75); '<- auto' is"
          " the block of block = 0")
    for dt, tdt, ndt in (("f64", torch.float64, np.float64), ("f32", torch.float32, np.float32)):
        esz = torch.empty(0, dtype=tdt).element_size()
        vec = 16 // esz
        x = torch.empty(LENGTH, dtype=tdt, device="cuda").uniform_(-1, 1)
        for k in TAPS:
            h = np.random.default_rng([k, 29]).uniform(-1, 1, k).astype(ndt)
            Conv = P.PlannerConv64 if dt == "f64" else P.PlannerConv32
            auto = Conv(LENGTH, h, "same").block
            for b in (auto // 2, auto, 2 * auto, 4 * auto):
                if b < k:
                    continue
                pl = Conv(LENGTH, h, "same", block=b)
                pr = (P.PlannerR2cAny64 if dt == "f64" else P.PlannerR2cAny32)(b)
                segs, n = pl.segments, pl.out_len
                fd, bd = -(-b // vec) * vec, -(-(b // 2 + 1) // vec) * vec
                y = torch.empty(n, dtype=tdt, device="cuda")
                work = torch.empty(pl.workspace_len(1), dtype=tdt, device="cuda")
                rows = torch.empty(segs * fd, dtype=tdt, device="cuda").uniform_(-1, 1)
                re, im = (torch.empty(segs * bd, dtype=tdt, device="cuda") for _ in range(2))
                r_work = torch.empty(max(1, pr.workspace_len(segs)), dtype=tdt, device="cuda")
                t_call = timed(lambda: P.conv_batched(x, y, pl, 1, workspace=work))
                t_r2c = timed(lambda: P.r2c_any_batched(rows, re, im, pr, segs, in_dist=fd, out_dist=bd, workspace=r_work))
                t_c2r = timed(lambda: P.c2r_any_batched(re, im, rows, pr, segs, in_dist=bd, out_dist=fd, workspace=r_work))
                drain()
                torch.cuda.synchronize()
                st = [v * 1e3 for v in pl.time_stages(x, y, 1, work, REPS)]
                sweeps = (("segment", st[0], (LENGTH + segs * fd) * esz), ("spectrum", st[2], 4 * segs * bd * esz),
                          ("save", st[4], 2 * n * esz))
                rates = "; ".join(f"{name} {nb / 1e6:.0f} MB at {nb / (t * 1e3):.0f} GB/s = {nb / (t * 1e3) / copy:.2f} copy"
                                  f" ({'meets' if nb / (t * 1e3) / copy >= 0.75 else 'BELOW'} 0.75)" for name, t, nb in sweeps)
                print(f"{dt} K={k} B={b} S={b - k + 1} ({segs} segments){' <- auto' if b == auto else ''}: {t_call:9.1f} us ="
                      f" {t_call * 1e3 / n:.3f} ns/sample = {t_call / (t_r2c + t_c2r):.2f} x R2C + C2R of the rows"
                      f" ({t_r2c:.1f} + {t_c2r:.1f} us); stages segment {st[0]:.1f} / R2C {st[1]:.1f} / spectrum {st[2]:.1f} /"
                      f" C2R {st[3]:.1f} / save {st[4]:.1f} us; {rates}", flush=True)
                del y, work, rows, re, im, r_work, pl, pr
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
