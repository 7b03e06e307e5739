#!/usr/bin/env python3
"""Rates of sample-rate conversion, in one run: this box's copy rate (phast_stream_probe_dev); the polyphase kernel at
(up, down) = (160, 147) with resample_poly's filter, (1, 4) and (4, 1) with the same design, on batches that fill the chip,
as a fraction of the copy rate on its bytes and of the FMA rate its arithmetic implies; the same conversion of one signal of
L = 2^20 through resample_poly, through the Fourier method and through PlannerConv on the zero-stuffed signal (the only route
without this unit), in ns per output sample; and the taps per phase at which the Fourier route overtakes the direct one.
Every timed region starts behind a cache drain (a read of 1 GiB nothing else uses), as bench.py times its regions -- this
tool does not import bench.py.

    python tools/resample_rate.py [reps]

Bytes of the kernel: every sample read once and every output written once (L + out_len elements per signal; the taps are
shared by all tiles and stay in cache).  Arithmetic: Kp fused multiply-adds per output, the padded taps of a row included.
FMA rate of the device: compute units x the peak clock (2.4 GHz) x 128 lanes (f32) or 64 (f64) per CU and cycle."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import phastft_amd as P  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
L = 1 << 20
BATCH = 16
RATES = [(160, 147), (1, 4), (4, 1)]
PEAK_GHZ = 2.4  # the MI355X's peak engine clock: 256 CUs x 128 lanes x 2.4 GHz is its 78.6 T FMA/s (157.3 TFLOPS) of f32

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


def poly_planner(dt, n_in, up, down, taps=None):
    """resample_poly's planner: the default filter, or `taps` per phase of the same design"""
    half = 10 * max(up, down) if taps is None else taps * up // 2
    h = P.firwin_lowpass(2 * half + 1, 1.0 / max(up, down)) * up
    pre = down - half % down
    h = np.concatenate((np.zeros(pre), h))
    return (P.PlannerUpfirdn64 if dt == "f64" else P.PlannerUpfirdn32)(n_in, h, up, down, (half + pre) // down, -(-n_in * up // down))


def main():
    probe = P.stream_probe(1024, 5)
    copy = probe["copy"]
    cus, ghz = P.device_info()["compute_units"], PEAK_GHZ
    print(f"# {P.device_info()['name']}: copy probe {copy:.0f} GB/s (read {probe['read']:.0f}, write {probe['write']:.0f}); {cus} CUs at"
          f" {ghz:.2f} GHz: {cus * ghz * 128 / 1e3:.1f} T FMA/s f32, {cus * ghz * 64 / 1e3:.1f} f64; reps {REPS}")
    print(f"# kernel: {BATCH} signals of L = {L}; t/call, GB/s on L + out_len elements per signal as a fraction of copy, G FMA/s on Kp per"
          " output as a fraction of the device's rate, and which of the two is nearer its ceiling")
    for dt, tdt in (("f64", torch.float64), ("f32", torch.float32)):
        esz = 8 if dt == "f64" else 4
        peak = cus * ghz * (64 if dt == "f64" else 128)  # G FMA/s
        for up, down in RATES:
            pl = poly_planner(dt, L, up, down)
            x = torch.empty((BATCH, L), dtype=tdt, device="cuda").uniform_(-1, 1)
            out = torch.empty((BATCH, pl.out_len), dtype=tdt, device="cuda")
            us = timed(lambda: P.upfirdn_batched(x, pl, out=out))
            kp = -(-pl.num_taps // up)
            gbs = BATCH * (L + pl.out_len) * esz / (us * 1e3)
            gfma = BATCH * pl.out_len * kp / (us * 1e3)
            bound = "memory" if gbs / copy > gfma / peak else "FMA"
            print(f"{dt} upfirdn {up}/{down} K={pl.num_taps} Kp={kp} tile={pl.tile} chunk={pl.chunk}: {us:9.1f} us; {gbs:.0f} GB/s = {gbs / copy:.3f} copy;"
                  f" {gfma:.0f} G FMA/s = {gfma / peak:.3f} of {peak:.0f}; nearer the {bound} bound", flush=True)
            del x, out, pl
    print(f"# one signal of L = {L}: ns per output sample through resample_poly (direct), resample (Fourier) and PlannerConv on the"
          " zero-stuffed signal with every down-th sample kept afterwards (its time is the convolution alone)")
    for dt, tdt in (("f64", torch.float64), ("f32", torch.float32)):
        for up, down in RATES:
            pl = poly_planner(dt, L, up, down)
            n_out = pl.out_len
            x = torch.empty(L, dtype=tdt, device="cuda").uniform_(-1, 1)
            out = torch.empty(n_out, dtype=tdt, device="cuda")
            t_poly = timed(lambda: P.upfirdn_batched(x, pl, out=out))
            pf = (P.PlannerResample64 if dt == "f64" else P.PlannerResample32)(L, n_out)
            work = torch.empty(pf.workspace_len(1), dtype=tdt, device="cuda")
            t_four = timed(lambda: P.resample_batched(x, pf, out=out, work=work))
            del work, pf
            taps = P.firwin_lowpass(20 * max(up, down) + 1, 1.0 / max(up, down)) * up
            pc = (P.PlannerConv64 if dt == "f64" else P.PlannerConv32)(L * up, taps, "same")
            stuffed = torch.zeros(L * up, dtype=tdt, device="cuda")
            stuffed[::up] = x
            full = torch.empty(pc.out_len, dtype=tdt, device="cuda")
            cwork = torch.empty(pc.workspace_len(1), dtype=tdt, device="cuda")
            t_conv = timed(lambda: P.conv_batched(stuffed, full, pc, 1, workspace=cwork))
            print(f"{dt} {up}/{down} -> {n_out} samples, K={taps.size}: resample_poly {t_poly:.1f} us = {t_poly * 1e3 / n_out:.4f} ns/sample;"
                  f" resample {t_four:.1f} us = {t_four * 1e3 / n_out:.4f}; PlannerConv on {L * up} samples (block {pc.block}) {t_conv:.1f} us ="
                  f" {t_conv * 1e3 / n_out:.4f}: {t_conv / t_poly:.1f} x resample_poly", flush=True)
            del pc, stuffed, full, cwork, x, out, pl
            torch.cuda.empty_cache()
    print(f"# crossover: {BATCH} signals of L = {L}, up/down = 1/4 and 4/1: the direct kernel at Kp taps per phase against the Fourier"
          " method (which does not depend on the filter)")
    for dt, tdt in (("f64", torch.float64), ("f32", torch.float32)):
        for up, down in ((1, 4), (4, 1)):
            n_out = L * up // down
            x = torch.empty((BATCH, L), dtype=tdt, device="cuda").uniform_(-1, 1)
            out = torch.empty((BATCH, n_out), dtype=tdt, device="cuda")
            pf = (P.PlannerResample64 if dt == "f64" else P.PlannerResample32)(L, n_out)
            work = torch.empty(pf.workspace_len(BATCH), dtype=tdt, device="cuda")
            t_four = timed(lambda: P.resample_batched(x, pf, out=out, work=work))
            del work, pf
            line, cross = [], None
            for kp in (8, 16, 32, 64, 128, 256, 512, 1024, 2048):
                pl = poly_planner(dt, L, up, down, taps=kp)
                t = timed(lambda: P.upfirdn_batched(x, pl, out=out))
                line.append(f"Kp {-(-pl.num_taps // up)}: {t:.0f}")
                if cross is None and t > t_four:
                    cross = -(-pl.num_taps // up)
                del pl
            print(f"{dt} {up}/{down}: Fourier {t_four:.0f} us; direct, us: {', '.join(line)}; the Fourier method is faster from Kp = {cross} on",
                  flush=True)
            del x, out
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
