#!/usr/bin/env python3
"""Rates of the polyphase synthesis bank, in one run: this box's copy rate (phast_stream_probe_dev); the transform and the unfold
of PlannerSynthesizer (time_stages) on 16 signals' worth of frames that reconstruct 2^20 samples at (M, T, D) = (64, 8, 64),
(1024, 8, 1024), (1024, 8, 768) and (4096, 4, 4096), f64 and f32, real and complex output, each as a fraction of the copy rate on
its bytes and of the FMA rate its arithmetic implies; beside them the two routes the library had before: PlannerStft's inverse
uncentred at F = M, H = D (the same framing at T = 1) and, for (64, 8, 64) real, 2 M PlannerUpfirdn passes with up = D over the
channels.  Every timed region starts behind a cache drain (a read of 1 GiB nothing else uses), as bench.py times its regions --
this tool does not import bench.py.

    python tools/synthesizer_rate.py [reps]

Bytes of the unfold: every element of v read once and every output sample written once ((F M + out_len) elements per signal
and plane; the taps are shared by all tiles and stay in cache).  Bytes of the transform: its input planes read once and v
written once.  Arithmetic of the unfold: ceil(K / D) fused multiply-adds per output.  FMA rate of the device: compute units x the
peak clock (2.4 GHz) x 128 lanes (f32) or 64 (f64) per CU and cycle."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import phastft_amd as P  # noqa: E402

ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
REPS = int(ARGS[0]) if ARGS else 10
L = 1 << 20
BATCH = 16
CASES = [(64, 8, 64), (1024, 8, 1024), (1024, 8, 768), (4096, 4, 4096)]
PEAK_GHZ = 2.4  # the MI355X's peak engine clock: 256 CUs x 128 lanes x 2.4 GHz is its 78.6 T FMA/s of f32

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


def stages(pl, *bufs, **kw):
    """(us, us) of time_stages behind a drain, after one warm-up"""
    pl.time_stages(*bufs, reps=1, **kw)
    drain()
    return [1e3 * v for v in pl.time_stages(*bufs, reps=REPS, **kw)]


def main():
    info = P.device_info()
    cus = info["compute_units"]
    probe = P.stream_probe(1024, 5)
    copy = probe["copy"]
    print(f"# {info['name']}: copy probe {copy:.0f} GB/s (read {probe['read']:.0f}, write {probe['write']:.0f}); {cus} CUs at"
          f" {PEAK_GHZ:.2f} GHz: {cus * PEAK_GHZ * 128 / 1e3:.1f} T FMA/s f32, {cus * PEAK_GHZ * 64 / 1e3:.1f} f64; reps {REPS}")
    print(f"# {BATCH} signals, F frames with (F - 1) D + M T <= {L}, prototype pfb_prototype(M, T); transform and unfold from time_stages;"
          " unfold: GB/s on (F M + out_len) elements per signal and plane as a fraction of copy, G FMA/s on ceil(K / D) per output as"
          " a fraction of the device's rate; transform: GB/s on its planes in and v out")
    for dt, tdt in (("f64", torch.float64), ("f32", torch.float32)):
        esz = 8 if dt == "f64" else 4
        peak = cus * PEAK_GHZ * (64 if dt == "f64" else 128)  # G FMA/s
        cls = P.PlannerSynthesizer64 if dt == "f64" else P.PlannerSynthesizer32
        for M, T, D in CASES:
            g = P.pfb_prototype(M, T)
            K = len(g)
            F = (L - K) // D + 1
            for cplx in (False, True):
                pl = cls(F, g, M, D, complex_output=cplx)
                planes = 2 if cplx else 1
                y = torch.empty((2, BATCH * F * pl.bins), dtype=tdt, device="cuda").uniform_(-1, 1)
                out = torch.empty((2, BATCH * pl.out_len), dtype=tdt, device="cuda")
                work = torch.empty(max(1, pl.workspace_len(BATCH)), dtype=tdt, device="cuda")
                fft, unfold = stages(pl, y[0], y[1], out[0], out[1] if cplx else None, batch=BATCH, workspace=work)
                kind = "complex" if cplx else "real"
                terms = -(-K // D)
                gbs = BATCH * planes * (F * M + pl.out_len) * esz / (unfold * 1e3)
                gfma = BATCH * planes * pl.out_len * terms / (unfold * 1e3)
                tbs = BATCH * (2 * F * pl.bins + planes * F * M) * esz / (fft * 1e3)
                print(f"{dt} {kind} M={M} T={T} D={D} F={F} out_len={pl.out_len} terms={terms}: transform {fft:9.1f} us = {tbs:.0f} GB/s ="
                      f" {tbs / copy:.3f} copy; unfold {unfold:9.1f} us = {gbs:.0f} GB/s = {gbs / copy:.3f} copy; {gfma:.0f} G FMA/s ="
                      f" {gfma / peak:.3f} of {peak:.0f}", flush=True)
                del pl, work
                if not cplx:  # the same framing at T = 1: the inverse STFT with a window of M ones
                    sl = (F - 1) * D + M
                    ps = (P.PlannerStft64 if dt == "f64" else P.PlannerStft32)(sl, M, D, None, center=False)
                    assert ps.frames == F
                    s_sig = torch.empty(BATCH * sl, dtype=tdt, device="cuda")
                    s_work = torch.empty(ps.workspace_len(BATCH), dtype=tdt, device="cuda")
                    sweep, sfft = stages(ps, s_sig, y[0], y[1], inverse=True, batch=BATCH, workspace=s_work)
                    print(f"{dt} real M={M} D={D}: PlannerStft inverse F=M H=D ({ps.frames} frames): transform {sfft:9.1f} us, overlap-add"
                          f" {sweep:9.1f} us", flush=True)
                    del ps, s_sig, s_work
                if not cplx and (M, T, D) == CASES[0]:  # channel k by upfirdn: 2 M real passes with up = D
                    pu = (P.PlannerUpfirdn64 if dt == "f64" else P.PlannerUpfirdn32)(F, g, D, 1)
                    u_out = torch.empty((BATCH, pu.out_len), dtype=tdt, device="cuda")
                    rows = y[0][:BATCH * F].view(BATCH, F)
                    one = timed(lambda: P.upfirdn_batched(rows, pu, out=u_out))
                    print(f"{dt} real M={M} T={T} D={D}: one PlannerUpfirdn pass (up = D) {one:9.1f} us; 2 M = {2 * M} passes"
                          f" {2 * M * one:9.1f} us (without the modulation)", flush=True)
                    del pu, u_out, rows
                del y, out
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
