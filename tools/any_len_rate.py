#!/usr/bin/env python3
"""Rates of the arbitrary-length (Bluestein) transforms: time per transform, N/t, the two inner M-point transforms and each
sweep's bytes / time against this box's copy rate (phast_stream_probe_dev, measured in the same run).  Every timed region starts
behind a cache drain (a read of 1 GiB nothing else uses), as bench.py times its regions -- this tool does not import bench.py.

    python tools/any_len_rate.py [reps]

End-to-end: device events around `reps` back-to-back calls.  Stages: PlannerAny*.time_stages (events between the five
launch groups of one call).  Sweep bytes per transform (T = element size): chirp-pad reads 2 N T, writes 2 M T; spectrum reads
2 M T + 2 M T (table), writes 2 M T; chirp-post reads 2 N T (the first N of the workspace), writes 2 N T."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import phastft_amd as P  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
CASES = [(10 ** 4, 1), (10 ** 6, 1), (1_000_003, 1), (3 << 20, 1), (10 ** 7, 1), (10 ** 4, 64), (10 ** 6, 16)]

_drain_buf = None


def drain():
    global _drain_buf
    if _drain_buf is None:
        _drain_buf = torch.ones(1 << 27, dtype=torch.float64, device="cuda")
    _drain_buf.sum()


def main():
    probe = P.stream_probe(1024, 5)
    copy = probe["copy"]
    print(f"# {P.device_info()['name']}: copy probe {copy:.0f} GB/s (read {probe['read']:.0f}, write {probe['write']:.0f}); reps {REPS}")
    print("# case: t/transform, N/t; stages in us (pre, fwd M, spectrum, inv M, post); sweep GB/s and fraction of the copy probe;"
          " end-to-end vs (2 inner + sweeps)")
    for dt, tdt in (("f64", torch.float64), ("f32", torch.float32)):
        for n, batch in CASES:
            pl = (P.PlannerAny64 if dt == "f64" else P.PlannerAny32)(n)
            m, esz = pl.m, torch.empty(0, dtype=tdt).element_size()
            re = torch.empty(n * batch, dtype=tdt, device="cuda").uniform_(-1, 1)
            im = torch.empty(n * batch, dtype=tdt, device="cuda").uniform_(-1, 1)
            work = torch.empty(pl.workspace_len(batch), dtype=tdt, device="cuda")
            P.fft_any_batched(re, im, n, P.Direction.Forward, pl, workspace=work)   # warm-up
            torch.cuda.synchronize()
            drain()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(REPS):
                P.fft_any_batched(re, im, n, P.Direction.Forward, pl, workspace=work)
            e1.record()
            torch.cuda.synchronize()
            t_call = e0.elapsed_time(e1) / REPS * 1e3   # us per call
            drain()
            torch.cuda.synchronize()
            st = [x * 1e3 for x in pl.time_stages(re, im, batch, n, work, REPS)]
            b_pre, b_spec, b_post = (2 * n + 2 * m) * esz * batch, 6 * m * esz * batch, 4 * n * esz * batch
            rates = [b / (t * 1e3) for b, t in ((b_pre, st[0]), (b_spec, st[2]), (b_post, st[4]))]   # GB/s
            model = sum(st)
            print(f"{dt} N={n} M=2^{m.bit_length() - 1} x{batch}: {t_call / batch:9.2f} us/transform, {n * batch / t_call / 1e3:7.2f} GS/s;"
                  f" stages {st[0]:.1f} {st[1]:.1f} {st[2]:.1f} {st[3]:.1f} {st[4]:.1f} us;"
                  f" sweeps {rates[0]:.0f} / {rates[1]:.0f} / {rates[2]:.0f} GB/s = {rates[0] / copy:.2f} / {rates[1] / copy:.2f} /"
                  f" {rates[2] / copy:.2f} of copy; call {t_call:.1f} us vs stages {model:.1f} us ({t_call / model - 1:+.1%})", flush=True)
            del re, im, work, pl
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
