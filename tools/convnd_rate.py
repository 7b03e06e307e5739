#!/usr/bin/env python3
"""Rates of N-d overlap-save convolution: per case the automatic block B and B / 2, 2 B per axis -- time per call, ns per output
sample, the call against the batched N-d R2C + C2R of the same tiles alone (r2c_nd_batched / c2r_nd_batched on rows that
already hold the tiles) in the same run, and each sweep's bytes / time against this box's copy rate (phast_stream_probe_dev,
measured in the same run).  Every timed region starts behind a cache drain (a read of 1 GiB nothing else uses), as bench.py
times its regions -- this tool does not import bench.py.

    python tools/convnd_rate.py [reps]

End-to-end: device events around `reps` back-to-back calls.  Stages: PlannerConvNd*.time_stages (events between the five stages
of one call).  Sweep bytes (T = element size, fd = prod B and bd = the half spectrum's points, rounded up to 16 bytes): the tile
sweep reads the array once from HBM (prod L T; what neighbouring tiles share is taken to hit the caches) and writes tiles fd T;
the spectrum sweep reads and writes both planes, 4 tiles bd T; the save sweep reads and writes prod out T each.  The yardstick
is the DCT's sweeps: 0.75 of copy.  One array, mode "same", taps uniform(-1, 1)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import phastft_amd as P  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
CASES = (((4096, 4096), (5, 5)), ((4096, 4096), (31, 31)), ((4096, 4096), (129, 129)), ((256, 256, 256), (7, 7, 7)))

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
    print("# one array, mode same.  case: t/call, ns per output sample, its ratio to the batched N-d R2C + C2R of the same tiles"
          " alone; the five stages in us; each sweep's GB/s as a fraction of copy (yardstick 0.75); '<- auto' is the block of"
          " block = None")
    for dt, tdt, ndt in (("f64", torch.float64, np.float64), ("f32", torch.float32, np.float32)):
        esz = torch.empty(0, dtype=tdt).element_size()
        vec = 16 // esz
        for shape, kshape in CASES:
            length = int(np.prod(shape))
            x = torch.empty(length, dtype=tdt, device="cuda").uniform_(-1, 1)
            h = np.random.default_rng([*kshape, 29]).uniform(-1, 1, kshape).astype(ndt)
            Conv = P.PlannerConvNd64 if dt == "f64" else P.PlannerConvNd32
            auto = Conv(shape, h, "same").block
            for b in (tuple(v // 2 for v in auto), auto, tuple(2 * v for v in auto)):
                if any(v < k for v, k in zip(b, kshape)):
                    continue
                pl = Conv(shape, h, "same", block=b)
                pr = (P.PlannerR2cNd64 if dt == "f64" else P.PlannerR2cNd32)(b)
                tiles, n, pts = pl.tiles, pl.out_len, int(np.prod(b))
                fd, bd = -(-pts // vec) * vec, -(-pr.half // vec) * vec
                y = torch.empty(n, dtype=tdt, device="cuda")
                work = torch.empty(pl.workspace_len(1), dtype=tdt, device="cuda")
                rows = torch.empty(tiles * fd, dtype=tdt, device="cuda").uniform_(-1, 1)
                re, im = (torch.empty(tiles * bd, dtype=tdt, device="cuda") for _ in range(2))
                r_work = torch.empty(max(1, pr.workspace_len(tiles)), dtype=tdt, device="cuda")
                t_call = timed(lambda: P.convnd_batched(x, y, pl, 1, workspace=work))
                t_r2c = timed(lambda: P.r2c_nd_batched(rows, re, im, pr, tiles, in_dist=fd, out_dist=bd, workspace=r_work))
                t_c2r = timed(lambda: P.c2r_nd_batched(re, im, rows, pr, tiles, in_dist=bd, out_dist=fd, workspace=r_work))
                drain()
                torch.cuda.synchronize()
                st = [v * 1e3 for v in pl.time_stages(x, y, 1, work, REPS)]
                sweeps = (("tile", st[0], (length + tiles * fd) * esz), ("spectrum", st[2], 4 * tiles * bd * esz),
                          ("save", st[4], 2 * n * esz))
                rates = "; ".join(f"{name} {nb / 1e6:.0f} MB at {nb / (t * 1e3):.0f} GB/s = {nb / (t * 1e3) / copy:.2f} copy"
                                  f" ({'meets' if nb / (t * 1e3) / copy >= 0.75 else 'BELOW'} 0.75)" for name, t, nb in sweeps)
                print(f"{dt} L={'x'.join(map(str, shape))} K={'x'.join(map(str, kshape))} B={'x'.join(map(str, b))} ({tiles} tiles)"
                      f"{' <- auto' if b == auto else ''}: {t_call:9.1f} us = {t_call * 1e3 / n:.3f} ns/sample ="
                      f" {t_call / (t_r2c + t_c2r):.2f} x R2C + C2R of the tiles ({t_r2c:.1f} + {t_c2r:.1f} us); stages tile {st[0]:.1f} /"
                      f" R2C {st[1]:.1f} / spectrum {st[2]:.1f} / C2R {st[3]:.1f} / save {st[4]:.1f} us; {rates}", flush=True)
                del y, work, rows, re, im, r_work, pl, pr
                torch.cuda.empty_cache()
            del x


if __name__ == "__main__":
    main()
