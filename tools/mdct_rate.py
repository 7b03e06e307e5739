#!/usr/bin/env python3
"""Rates of the MDCT and its inverse, in one run: this box's copy rate (phast_stream_probe_dev); each stage of a call
(PlannerMdct*.time_stages: events around the pre sweep, the complex transform and the post sweep -- for the inverse the post and
the overlap-add sweeps together) with the sweeps' bytes / time as a fraction of copy; the whole call against the batched complex
transform of the same rows alone (fft_any_batched on planes that already hold them); and the whole call against the STFT with
n_fft = 2N, hop = N on the same signal.  Every timed region starts behind a cache drain (a read of 1 GiB nothing else uses),
as bench.py times its regions -- this tool does not import bench.py.

    python tools/mdct_rate.py [reps]

Sweep bytes (T = element size, hd and nd = N / 2 and N rounded up to 16 bytes, rows = signals x frames): the fold-and-pre sweep
reads the signals once from HBM (their second read and the window hit the caches) and writes 2 hd per row; the forward post sweep
reads 2 hd and writes N per row; the inverse's pre sweep reads N and writes 2 hd per row; its post and overlap-add sweeps read
2 hd, write and read nd per row and write the signals.  Window: sine.  The yardstick is the DCT's sweeps: 0.75 of copy
(DESIGN.md §14)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import phastft_amd as P  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
CASES = [(1024, 1 << 24, 1), (960, 1 << 24, 1), (1024, 1 << 18, 64), (960, 1 << 18, 64)]  # (N, L, signals)

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
    print("# case: t/call, its ratio to the batched complex transform of the same rows alone and to the STFT (n_fft = 2N, hop = N) of"
          " the same signals; stages in us with the sweeps' GB/s as a fraction of copy (yardstick: the DCT sweeps' 0.75)")
    for dt, tdt, ndt in (("f64", torch.float64, np.float64), ("f32", torch.float32, np.float32)):
        for n, length, batch in CASES:
            pl = (P.PlannerMdct64 if dt == "f64" else P.PlannerMdct32)(length, n)
            pa = (P.PlannerAny64 if dt == "f64" else P.PlannerAny32)(n // 2)
            ps = (P.PlannerStft64 if dt == "f64" else P.PlannerStft32)(length, 2 * n, n, window=P.mdct_window("sine", n, ndt))
            esz = torch.empty(0, dtype=tdt).element_size()
            vec = 16 // esz
            hd, nd = -(-(n // 2) // vec) * vec, -(-n // vec) * vec
            rows = batch * pl.frames
            x = torch.empty(length * batch, dtype=tdt, device="cuda").uniform_(-1, 1)
            y = torch.empty_like(x)
            X = torch.empty(rows * n, dtype=tdt, device="cuda")
            work = torch.empty(pl.workspace_len(batch), dtype=tdt, device="cuda")
            z_re = torch.empty(rows * hd, dtype=tdt, device="cuda").uniform_(-1, 1)
            z_im = torch.empty(rows * hd, dtype=tdt, device="cuda").uniform_(-1, 1)
            a_work = torch.empty(max(1, pa.workspace_len(rows)), dtype=tdt, device="cuda")
            t_fwd = timed(lambda: P.mdct_batched(x, X, pl, batch, workspace=work))
            t_inv = timed(lambda: P.imdct_batched(X, y, pl, batch, workspace=work))
            t_fft = timed(lambda: P.fft_any_batched(z_re, z_im, n // 2, P.Direction.Forward, pa, dist=hd, workspace=a_work))
            del z_re, z_im, a_work
            s_pts = batch * ps.frames * ps.bins
            s_re, s_im = torch.empty(s_pts, dtype=tdt, device="cuda"), torch.empty(s_pts, dtype=tdt, device="cuda")
            s_work = torch.empty(ps.workspace_len(batch), dtype=tdt, device="cuda")
            t_stft = timed(lambda: P.stft_batched(x, s_re, s_im, ps, batch, workspace=s_work))
            t_istft = timed(lambda: P.istft_batched(s_re, s_im, y, ps, batch, workspace=s_work))
            del s_re, s_im, s_work
            sig = length * batch
            nbytes = {False: ((sig + 2 * hd * rows) * esz, (2 * hd + n) * rows * esz),
                      True: ((n + 2 * hd) * rows * esz, ((2 * hd + 2 * nd) * rows + sig) * esz)}
            for name, inverse, t_call, t_other, other in (("mdct", False, t_fwd, t_stft, "stft"), ("imdct", True, t_inv, t_istft, "istft")):
                drain()
                torch.cuda.synchronize()
                st = [v * 1e3 for v in pl.time_stages(y if inverse else x, X, inverse, batch, work, REPS)]
                r_pre, r_post = nbytes[inverse][0] / (st[0] * 1e3), nbytes[inverse][1] / (st[2] * 1e3)
                print(f"{dt} {name} {batch} x L={length} N={n} ({rows} frames): {t_call:9.1f} us = {t_call / t_fft:.2f} x the FFT of the"
                      f" rows ({t_fft:.1f} us) = {t_call / t_other:.2f} x {other} ({t_other:.1f} us); stages pre {st[0]:.1f} / transform"
                      f" {st[1]:.1f} / {'post + overlap-add' if inverse else 'post'} {st[2]:.1f} us; pre {nbytes[inverse][0] / 1e6:.0f} MB at"
                      f" {r_pre:.0f} GB/s = {r_pre / copy:.2f} copy, {'post + overlap-add' if inverse else 'post'}"
                      f" {nbytes[inverse][1] / 1e6:.0f} MB at {r_post:.0f} GB/s = {r_post / copy:.2f} copy", flush=True)
            del x, y, X, work, pl, pa, ps
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
