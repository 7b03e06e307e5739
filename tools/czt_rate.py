#!/usr/bin/env python3
"""Rates of the chirp-Z transform: time per call, the five stages, each sweep's bytes / time against this box's copy rate
(phast_stream_probe_dev, measured in the same run), and the whole call against two L-point engine calls alone (the
power-of-two path of PlannerAny*(L), timed in the same way).  Every timed region starts behind a cache drain (a read of 1 GiB
nothing else uses), as bench.py times its regions -- this tool does not import bench.py.

    python tools/czt_rate.py [reps]

End-to-end: device events around `reps` back-to-back calls.  Stages: PlannerCzt*.time_stages (events between the five launch
groups of one call).  Sweep bytes per transform (T = element size, complex input): pre reads 2 N T, writes 2 L T; spectrum reads
2 L T + 2 L T (table), writes 2 L T; post reads 2 M T of the workspace, writes 2 M T."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import phastft_amd as P  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
CASES = [(10 ** 6, 10 ** 6), (1 << 22, 1024), (1024, 1 << 22)]

_drain_buf = None


def drain():
    global _drain_buf
    if _drain_buf is None:
        _drain_buf = torch.ones(1 << 27, dtype=torch.float64, device="cuda")
    _drain_buf.sum()


def timed(call):
    """us per call over REPS back-to-back calls behind a drain"""
    call()   # warm-up
    torch.cuda.synchronize()
    drain()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS * 1e3


def main():
    probe = P.stream_probe(1024, 5)
    copy = probe["copy"]
    print(f"# {P.device_info()['name']}: copy probe {copy:.0f} GB/s (read {probe['read']:.0f}, write {probe['write']:.0f}); reps {REPS}")
    print("# case: t/call; stages in us (pre, fwd L, spectrum, inv L, post); sweep GB/s and fraction of the copy probe;"
          " the call vs two L-point transforms alone")
    for dt, tdt in (("f64", torch.float64), ("f32", torch.float32)):
        for n, m in CASES:
            pl = (P.PlannerCzt64 if dt == "f64" else P.PlannerCzt32)(n, m, 0.37 / n, 0.123456789)
            ell, esz = pl.conv_len, torch.empty(0, dtype=tdt).element_size()
            re = torch.empty(n, dtype=tdt, device="cuda").uniform_(-1, 1)
            im = torch.empty(n, dtype=tdt, device="cuda").uniform_(-1, 1)
            out = (torch.empty(m, dtype=tdt, device="cuda"), torch.empty(m, dtype=tdt, device="cuda"))
            work = torch.empty(pl.workspace_len(1), dtype=tdt, device="cuda")
            t_call = timed(lambda: P.czt_batched(re, im, pl, out=out, work=work))
            drain()
            torch.cuda.synchronize()
            st = [x * 1e3 for x in pl.time_stages(re, im, out[0], out[1], 1, work, REPS)]
            eng = (P.PlannerAny64 if dt == "f64" else P.PlannerAny32)(ell)   # a power of two: the engine itself
            w_re, w_im = work[:ell], work[ell:2 * ell]
            t_eng = timed(lambda: P.fft_any_batched(w_re, w_im, ell, P.Direction.Forward, eng))
            b_pre, b_spec, b_post = (2 * n + 2 * ell) * esz, 6 * ell * esz, 4 * m * esz
            rates = [b / (t * 1e3) for b, t in ((b_pre, st[0]), (b_spec, st[2]), (b_post, st[4]))]   # GB/s
            print(f"{dt} N={n} M={m} L=2^{ell.bit_length() - 1}: {t_call:9.2f} us/call;"
                  f" stages {st[0]:.1f} {st[1]:.1f} {st[2]:.1f} {st[3]:.1f} {st[4]:.1f} us;"
                  f" sweeps {rates[0]:.0f} / {rates[1]:.0f} / {rates[2]:.0f} GB/s = {rates[0] / copy:.2f} / {rates[1] / copy:.2f} /"
                  f" {rates[2] / copy:.2f} of copy; call {t_call:.1f} us vs 2 x FFT_L {2 * t_eng:.1f} us ({t_call / (2 * t_eng):.2f} x),"
                  f" vs stages {sum(st):.1f} us", flush=True)
            del re, im, out, work, pl, eng, w_re, w_im
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
