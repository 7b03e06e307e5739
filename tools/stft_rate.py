#!/usr/bin/env python3
"""Rates of the STFT and its inverse: time per call against the batched R2C / C2R of the same frames alone (r2c_any_batched /
c2r_any_batched on rows that already hold the frames) in the same run, and each sweep's bytes / time against this box's copy
rate (phast_stream_probe_dev, measured in the same run).  Every timed region starts behind a cache drain (a read of 1 GiB
nothing else uses), as bench.py times its regions -- this tool does not import bench.py.

    python tools/stft_rate.py [reps]

End-to-end: device events around `reps` back-to-back calls.  Stages: PlannerStft*.time_stages (events between the sweep and
the real transform of one call).  Sweep bytes (T = element size, fd = F rounded up to 16 bytes): the frame sweep reads the
signal once from HBM (L T; its F / H re-reads hit the caches) and writes frames fd T; the overlap-add sweep reads frames fd T
and writes L T.  Window: Hann, center, reflect.  The yardstick is the DCT's sweeps: 0.75 of copy at 16 x 10^6."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import phastft_amd as P  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
CASES = [(1 << 20, 1024, 256, 16), (1 << 20, 1000, 250, 16), (1 << 24, 4096, 1024, 1)]  # (L, F, H, signals)

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
    print("# case: t/call and its ratio to the batched R2C / C2R of the same frames alone; stages sweep / transform in us; the"
          " sweep's GB/s on (L + frames fd) T bytes as a fraction of copy (yardstick: the DCT sweeps' 0.75)")
    for dt, tdt, ndt in (("f64", torch.float64, np.float64), ("f32", torch.float32, np.float32)):
        for length, f, h, batch in CASES:
            w = (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(f) / f)).astype(ndt)
            pl = (P.PlannerStft64 if dt == "f64" else P.PlannerStft32)(length, f, h, window=w)
            pr = (P.PlannerR2cAny64 if dt == "f64" else P.PlannerR2cAny32)(f)
            esz = torch.empty(0, dtype=tdt).element_size()
            fd = (f * esz + 15) // 16 * 16 // esz
            rows, pts = batch * pl.frames, batch * pl.frames * pl.bins
            x = torch.empty(length * batch, dtype=tdt, device="cuda").uniform_(-1, 1)
            y = torch.empty_like(x)
            re, im = torch.empty(pts, dtype=tdt, device="cuda"), torch.empty(pts, dtype=tdt, device="cuda")
            work = torch.empty(pl.workspace_len(batch), dtype=tdt, device="cuda")
            frames = torch.empty(rows * fd, dtype=tdt, device="cuda").uniform_(-1, 1)
            r_work = torch.empty(max(1, pr.workspace_len(rows)), dtype=tdt, device="cuda")
            t_fwd = timed(lambda: P.stft_batched(x, re, im, pl, batch, workspace=work))
            t_r2c = timed(lambda: P.r2c_any_batched(frames, re, im, pr, rows, in_dist=fd, workspace=r_work))
            t_inv = timed(lambda: P.istft_batched(re, im, y, pl, batch, workspace=work))
            t_c2r = timed(lambda: P.c2r_any_batched(re, im, frames, pr, rows, out_dist=fd, workspace=r_work))
            nbytes = (length * batch + rows * fd) * esz
            for name, inverse, t_call, t_inner, inner in (("stft", False, t_fwd, t_r2c, "R2C"), ("istft", True, t_inv, t_c2r, "C2R")):
                drain()
                torch.cuda.synchronize()
                st = [v * 1e3 for v in pl.time_stages(y if inverse else x, re, im, inverse, batch, work, REPS)]
                rate = nbytes / (st[0] * 1e3)
                print(f"{dt} {name} {batch} x L={length} F={f} H={h} ({rows} frames): {t_call:9.1f} us = {t_call / t_inner:.2f} x"
                      f" {inner} of the frames ({t_inner:.1f} us); stages sweep {st[0]:.1f} / transform {st[1]:.1f} us;"
                      f" sweep {nbytes / 1e6:.0f} MB at {rate:.0f} GB/s = {rate / copy:.2f} copy"
                      f" ({'meets' if rate / copy >= 0.75 else 'BELOW'} 0.75)", flush=True)
            del x, y, re, im, work, frames, r_work, pl, pr
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
