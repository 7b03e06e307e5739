#!/usr/bin/env python3
"""Rates of the discrete wavelet transform, in one run: this box's copy rate (phast_stream_probe_dev); wavedec and waverec of
16 signals of 2^20 samples, f64 and f32, haar, db4 and db10, one level and eight, symmetric extension, as a fraction of the copy
rate on their bytes and of the FMA rate their arithmetic implies; and the only route without this unit: per level two
PlannerUpfirdn calls (down = 2) on a signal extended beforehand, the extension copy timed on its own.  Every timed region
starts behind a cache drain (a read of 1 GiB nothing else uses), as bench.py times its regions -- this tool does not import
bench.py.

    python tools/dwt_rate.py [reps]

Bytes: per level every sample read once and every coefficient written once (n_{l-1} + 2 n_l elements per signal; the inverse
moves the same the other way).  Arithmetic: 2F fused multiply-adds per coefficient pair (cA[i], cD[i]), 2F per output pair of
the inverse.  FMA rate of the device: compute units x the peak clock (2.4 GHz) x 128 lanes (f32) or 64 (f64) per CU and cycle.
LDS bank conflicts of the parity-split staging (SQ_LDS_BANK_CONFLICT) need a counters-only rocprofv3 --pmc run of their own:
this tool does not make it and says so."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import phastft_amd as P  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
L = 1 << 20
BATCH = 16
WAVELETS = ["haar", "db4", "db10"]
LEVELS = [1, 8]
MODE = "symmetric"
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


def upfirdn_route(dt, tdt, name, levels, x):
    """(us of the extension copies, us of the upfirdn calls) of the same cascade through PlannerUpfirdn: per level the signal
    extended symmetrically by F - 1 samples on either side (torch.cat of flipped ends: a padded copy in memory), then one call
    per filter with down = 2 that keeps the n_l outputs from F / 2 on"""
    dec_lo, dec_hi = P.wavelet_filters(name)[:2]
    f = dec_lo.size
    kind = P.PlannerUpfirdn64 if dt == "f64" else P.PlannerUpfirdn32
    lens = [L]
    for _ in range(levels):
        lens.append((lens[-1] + f - 1) // 2)
    plans = [(kind(lens[l] + 2 * (f - 1), dec_lo, 1, 2, f // 2, lens[l + 1]), kind(lens[l] + 2 * (f - 1), dec_hi, 1, 2, f // 2, lens[l + 1]))
             for l in range(levels)]
    outs = [(torch.empty((BATCH, lens[l + 1]), dtype=tdt, device="cuda"), torch.empty((BATCH, lens[l + 1]), dtype=tdt, device="cuda"))
            for l in range(levels)]

    def extend(a):
        if f == 2:
            return torch.cat((a[:, :1], a, a[:, -1:]), dim=1)
        return torch.cat((a[:, :f - 1].flip(1), a, a[:, -(f - 1):].flip(1)), dim=1)

    def copies():
        a = x
        for l in range(levels):
            extend(a)
            a = outs[l][0]

    def filters():
        a = x
        for l in range(levels):
            p = padded[l]
            P.upfirdn_batched(p, plans[l][0], out=outs[l][0])
            P.upfirdn_batched(p, plans[l][1], out=outs[l][1])
            a = outs[l][0]
        return a

    padded, a = [], x
    for l in range(levels):   # the padded copies the timed filter calls read (one run of the cascade)
        padded.append(extend(a))
        P.upfirdn_batched(padded[l], plans[l][0], out=outs[l][0])
        P.upfirdn_batched(padded[l], plans[l][1], out=outs[l][1])
        a = outs[l][0]
    return timed(copies), timed(filters), outs


def main():
    probe = P.stream_probe(1024, 5)
    copy = probe["copy"]
    cus, ghz = P.device_info()["compute_units"], PEAK_GHZ
    print(f"# {P.device_info()['name']}: copy probe {copy:.0f} GB/s (read {probe['read']:.0f}, write {probe['write']:.0f}); {cus} CUs at"
          f" {ghz:.2f} GHz: {cus * ghz * 128 / 1e3:.1f} T FMA/s f32, {cus * ghz * 64 / 1e3:.1f} f64; reps {REPS}")
    print(f"# {BATCH} signals of L = {L}, mode {MODE}; t/call, GB/s on n_(l-1) + 2 n_l elements per level and signal as a fraction of copy,"
          " G FMA/s on 2F per coefficient pair as a fraction of the device's rate, and which of the two is nearer its ceiling")
    for dt, tdt in (("f64", torch.float64), ("f32", torch.float32)):
        esz = 8 if dt == "f64" else 4
        peak = cus * ghz * (64 if dt == "f64" else 128)  # G FMA/s
        for name in WAVELETS:
            for levels in LEVELS:
                pl = (P.PlannerDwt64 if dt == "f64" else P.PlannerDwt32)(L, name, levels, MODE)
                f, lens = pl.filter_len, pl.level_lens
                x = torch.empty((BATCH, L), dtype=tdt, device="cuda").uniform_(-1, 1)
                co = torch.empty((BATCH, pl.coeff_len), dtype=tdt, device="cuda")
                back = torch.empty((BATCH, L), dtype=tdt, device="cuda")
                work = torch.empty(max(1, pl.workspace_len(BATCH)), dtype=tdt, device="cuda")
                elements = sum(lens[l - 1] + 2 * lens[l] for l in range(1, levels + 1))
                fmas = sum(2 * f * lens[l] for l in range(1, levels + 1))
                for what, fn in (("wavedec", lambda: P.wavedec_batched(x, pl, out=co, work=work)),
                                 ("waverec", lambda: P.waverec_batched(co, pl, out=back, work=work))):
                    us = timed(fn)
                    gbs = BATCH * elements * esz / (us * 1e3)
                    gfma = BATCH * fmas / (us * 1e3)
                    bound = "memory" if gbs / copy > gfma / peak else "FMA"
                    print(f"{dt} {what} {name} F={f} J={levels} tile={pl.tile}: {us:9.1f} us; {gbs:.0f} GB/s = {gbs / copy:.3f} copy;"
                          f" {gfma:.0f} G FMA/s = {gfma / peak:.3f} of {peak:.0f}; nearer the {bound} bound", flush=True)
                err = float((back - x).abs().max())
                t_dec = timed(lambda: P.wavedec_batched(x, pl, out=co, work=work))
                t_copy, t_fir, outs = upfirdn_route(dt, tdt, name, levels, x)
                off, n = pl.bands()[0]
                same = bool(torch.equal(outs[-1][0], co[:, off:off + n]))
                print(f"{dt} {name} J={levels}: round trip max |err| {err:.2e}; the route without this unit, two upfirdn calls per level on an"
                      f" extended copy: filters {t_fir:.1f} us + extension copies {t_copy:.1f} us = {(t_fir + t_copy) / t_dec:.2f} x wavedec"
                      f" ({t_fir / t_dec:.2f} x without the copies); cA_J bit-identical to wavedec's: {same}", flush=True)
                del x, co, back, work, pl, outs
                torch.cuda.empty_cache()
    print("# SQ_LDS_BANK_CONFLICT of the parity-split staging: NOT measured here (it needs a counters-only rocprofv3 --pmc run of its own)")


if __name__ == "__main__":
    main()
