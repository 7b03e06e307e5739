#!/usr/bin/env python3
"""Rates of Welch spectral estimation, in one run: this box's copy rate (phast_stream_probe_dev); the whole psd call against
stft_batched of the same frames (uncentred, n_fft = nperseg, the same hop and window); each stage of a call
(PlannerPsd*.time_stages: events around the mean and frame sweeps, the real transform, and the accumulate and final sweeps)
with the sweeps' bytes / time as a fraction of copy; and the accumulate and final sweeps with the planner's slab rule against
one slab per signal (slab = segments).  Every timed region starts behind a cache drain (a read of 1 GiB nothing else uses), as
bench.py times its regions -- this tool does not import bench.py.

    python tools/psd_rate.py [reps]

Sweep bytes (T = element size, fd and bd = nfft and bins rounded up to 16 bytes, rows = signals x segments): the mean and
frame sweeps read the signals once from HBM (the re-reads of overlapping segments and the window hit the caches) and write fd
per row and 8 bytes per row of means; the accumulate sweep reads 2 bd per row and writes, per slab, bd doubles; the final sweep
reads them and writes bins per signal.  The yardstick is the DCT's sweeps: 0.75 of copy."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import phastft_amd as P  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
CASES = [(16, 1 << 20, 1024, 256), (16, 1 << 20, 1000, 250), (1, 1 << 24, 256, 128)]  # (signals, L, nperseg, hop)

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
    print("# case: t/call and its ratio to stft_batched of the same frames; stages in us with the sweeps' GB/s as a fraction of copy"
          " (yardstick: the DCT sweeps' 0.75); the accumulate and final sweeps with the slab rule against one slab per signal")
    for dt, tdt, ndt in (("f64", torch.float64, np.float64), ("f32", torch.float32, np.float32)):
        for batch, length, p, h in CASES:
            pl = (P.PlannerPsd64 if dt == "f64" else P.PlannerPsd32)(length, p, h)
            hann = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(p) / p)
            ps = (P.PlannerStft64 if dt == "f64" else P.PlannerStft32)(length, p, h, window=hann.astype(ndt), center=False)
            assert ps.frames == pl.segments and ps.bins == pl.bins
            esz = torch.empty(0, dtype=tdt).element_size()
            vec = 16 // esz
            fd, bd = -(-p // vec) * vec, -(-pl.bins // vec) * vec
            rows = batch * pl.segments
            x = torch.empty(length * batch, dtype=tdt, device="cuda").uniform_(-1, 1)
            out = torch.empty(batch * pl.bins, dtype=tdt, device="cuda")
            work = torch.empty(pl.workspace_len(batch), dtype=tdt, device="cuda")
            t_psd = timed(lambda: P.psd_batched(x, out, pl, batch, workspace=work))
            s_re, s_im = (torch.empty(rows * ps.bins, dtype=tdt, device="cuda") for _ in range(2))
            s_work = torch.empty(ps.workspace_len(batch), dtype=tdt, device="cuda")
            t_stft = timed(lambda: P.stft_batched(x, s_re, s_im, ps, batch, workspace=s_work))
            del s_re, s_im, s_work
            drain()
            torch.cuda.synchronize()
            st = [v * 1e3 for v in pl.time_stages(x, out, batch, True, work, REPS)]
            drain()
            torch.cuda.synchronize()
            one = [v * 1e3 for v in pl.time_stages(x, out, batch, True, work, REPS, slab=pl.segments)]
            slabs = -(-pl.segments // pl.slab)
            b_frame = (length * batch + fd * rows) * esz + 8 * rows
            b_acc = 2 * bd * rows * esz + 2 * 8 * bd * slabs * batch + pl.bins * batch * esz
            r_frame, r_acc, r_one = b_frame / (st[0] * 1e3), b_acc / (st[2] * 1e3), 2 * bd * rows * esz / (one[2] * 1e3)
            print(f"{dt} psd {batch} x L={length} P={p} H={h} ({rows} frames, {pl.bins} bins, slab {pl.slab} x {slabs}): {t_psd:9.1f} us ="
                  f" {t_psd / t_stft:.2f} x stft ({t_stft:.1f} us); stages mean + frame {st[0]:.1f} / transform {st[1]:.1f} / accumulate + final"
                  f" {st[2]:.1f} us; mean + frame {b_frame / 1e6:.0f} MB at {r_frame:.0f} GB/s = {r_frame / copy:.2f} copy, accumulate + final"
                  f" {b_acc / 1e6:.0f} MB at {r_acc:.0f} GB/s = {r_acc / copy:.2f} copy; with one slab per signal {one[2]:.1f} us ="
                  f" {r_one / copy:.3f} copy: the rule buys {one[2] / st[2]:.1f} x", flush=True)
            del x, out, work, pl, ps
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
