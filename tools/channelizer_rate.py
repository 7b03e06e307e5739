#!/usr/bin/env python3
"""Rates of the polyphase channelizer, in one run: this box's copy rate (phast_stream_probe_dev); the fold and the transform
of PlannerChannelizer (time_stages) on 16 signals of 2^20 samples at (M, T, D) = (64, 8, 64), (1024, 8, 1024), (1024, 8, 768)
and (4096, 4, 4096), f64 and f32, real and complex, the fold as a fraction of the copy rate on its bytes and of the FMA rate
its arithmetic implies; beside them the two routes the library had before: PlannerStft uncentred at F = M, H = D (the same
framing at T = 1) and, for (64, 8, 64) real, 2 M PlannerUpfirdn passes over the demodulated planes.  Every timed region starts
behind a cache drain (a read of 1 GiB nothing else uses), as bench.py times its regions -- this tool does not import bench.py.

    python tools/channelizer_rate.py [reps]
    python tools/channelizer_rate.py --build-variant     (no GPU needed)

Where D mod M = 0 the f64 fold holds a tap in a register across the frames of a thread and the f32 fold does not.
--build-variant builds lib/libphastft_hip_chan_other.so, the library with that choice flipped (-DPHAST_CHAN_OTHER_BRANCH);
when it is there, a fresh child process loads it and times the same folds through the other branch.

Bytes of the fold: every sample read once and every fold element written once ((L + out_frames M) elements per signal and
plane; the taps are shared by all tiles and stay in cache).  Arithmetic: T fused multiply-adds per fold element.  FMA rate of
the device: compute units x the peak clock (2.4 GHz) x 128 lanes (f32) or 64 (f64) per CU and cycle."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
VARIANT = os.path.join(ROOT, "phastft_amd", "lib", "libphastft_hip_chan_other.so")

if "--build-variant" in sys.argv:
    from phastft_amd import build

    print(build.build(extra=("-DPHAST_CHAN_OTHER_BRANCH",), tag="_chan_other"))
    sys.exit(0)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import phastft_amd as P  # noqa: E402

OTHER_BRANCH = os.environ.get("PHASTFT_HIP_LIB") == VARIANT
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
    if not OTHER_BRANCH:
        probe = P.stream_probe(1024, 5)
        copy = probe["copy"]
        print(f"# {info['name']}: copy probe {copy:.0f} GB/s (read {probe['read']:.0f}, write {probe['write']:.0f}); {cus} CUs at"
              f" {PEAK_GHZ:.2f} GHz: {cus * PEAK_GHZ * 128 / 1e3:.1f} T FMA/s f32, {cus * PEAK_GHZ * 64 / 1e3:.1f} f64; reps {REPS}")
        print(f"# {BATCH} signals of L = {L}, prototype pfb_prototype(M, T); fold and transform from time_stages; fold: GB/s on (L +"
              " frames M) elements per signal and plane as a fraction of copy, G FMA/s on T per element as a fraction of the device's rate")
    for dt, tdt in (("f64", torch.float64), ("f32", torch.float32)):
        esz = 8 if dt == "f64" else 4
        peak = cus * PEAK_GHZ * (64 if dt == "f64" else 128)  # G FMA/s
        cls = P.PlannerChannelizer64 if dt == "f64" else P.PlannerChannelizer32
        for M, T, D in CASES:
            if OTHER_BRANCH and D % M:
                continue
            h = P.pfb_prototype(M, T)
            for cplx in (False, True):
                pl = cls(L, h, M, D, complex_input=cplx)
                planes = 2 if cplx else 1
                x = [torch.empty(BATCH * L, dtype=tdt, device="cuda").uniform_(-1, 1) for _ in range(planes)]
                out = torch.empty((2, BATCH * pl.out_frames * pl.bins), dtype=tdt, device="cuda")
                work = torch.empty(max(1, pl.workspace_len(BATCH)), dtype=tdt, device="cuda")
                fold, fft = stages(pl, x[0], x[1] if cplx else None, out[0], out[1], batch=BATCH, workspace=work)
                kind = "complex" if cplx else "real"
                if OTHER_BRANCH:
                    print(f"{dt} {kind} M={M} T={T} D={D}: fold through the {'general' if dt == 'f64' else 'register-held tap'} branch {fold:9.1f} us",
                          flush=True)
                    continue
                elems = BATCH * planes * pl.out_frames * M
                gbs = (BATCH * planes * L + elems) * esz / (fold * 1e3)
                gfma = elems * T / (fold * 1e3)
                print(f"{dt} {kind} M={M} T={T} D={D} frames={pl.out_frames} tile={pl.tile_frames}x{pl.tile_cols} periods={pl.periods}:"
                      f" fold {fold:9.1f} us, transform {fft:9.1f} us; fold {gbs:.0f} GB/s = {gbs / copy:.3f} copy; {gfma:.0f} G FMA/s ="
                      f" {gfma / peak:.3f} of {peak:.0f}", flush=True)
                del pl, out, work
                if not cplx:  # the same framing at T = 1: the STFT with a window of M
                    ps = (P.PlannerStft64 if dt == "f64" else P.PlannerStft32)(L, M, D, h[:M], center=False)
                    s_out = torch.empty((2, BATCH * ps.frames * ps.bins), dtype=tdt, device="cuda")
                    s_work = torch.empty(ps.workspace_len(BATCH), dtype=tdt, device="cuda")
                    sweep, sfft = stages(ps, x[0], s_out[0], s_out[1], batch=BATCH, workspace=s_work)
                    print(f"{dt} real M={M} D={D}: PlannerStft F=M H=D ({ps.frames} frames): sweep {sweep:9.1f} us, transform {sfft:9.1f} us",
                          flush=True)
                    del ps, s_out, s_work
                if not cplx and (M, T, D) == CASES[0]:  # channel k by upfirdn: 2 M real passes over the demodulated planes
                    pu = (P.PlannerUpfirdn64 if dt == "f64" else P.PlannerUpfirdn32)(L, h, 1, D)
                    u_out = torch.empty((BATCH, pu.out_len), dtype=tdt, device="cuda")
                    rows = x[0].view(BATCH, L)
                    one = timed(lambda: P.upfirdn_batched(rows, pu, out=u_out))
                    print(f"{dt} real M={M} T={T} D={D}: one PlannerUpfirdn pass {one:9.1f} us; 2 M = {2 * M} passes {2 * M * one:9.1f} us"
                          " (without the demodulation)", flush=True)
                    del pu, u_out, rows
                del x
                torch.cuda.empty_cache()
    if not OTHER_BRANCH:
        if os.path.exists(VARIANT):
            print("# the same folds at D mod M = 0 through the branch the library does not take there (f64: general; f32: register-held tap)", flush=True)
            env = dict(os.environ, PHASTFT_HIP_LIB=VARIANT)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), str(REPS)], env=env, capture_output=True, text=True, timeout=600)
            sys.stdout.write(r.stdout)
            if r.returncode:
                sys.stdout.write(r.stderr[-2000:])
        else:
            print("# lib/libphastft_hip_chan_other.so is not built (--build-variant): the other branch was not timed at D mod M = 0")


if __name__ == "__main__":
    main()
