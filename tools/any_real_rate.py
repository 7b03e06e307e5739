#!/usr/bin/env python3
"""Rates of the arbitrary-length real transforms (R2C / C2R): time per transform against the complex any-length transform of
the same N in the same run, the two inner M-point transforms and each sweep's bytes / time against this box's copy rate
(phast_stream_probe_dev, measured in the same run).  Every timed region starts behind a cache drain (a read of 1 GiB nothing
else uses), as bench.py times its regions -- this tool does not import bench.py.

    python tools/any_real_rate.py [reps]

End-to-end: device events around `reps` back-to-back calls.  Stages: PlannerR2cAny*.time_stages / time_c2r_stages (events
between the five launch groups of one call).  Sweep bytes per transform (T = element size, h1 = N // 2 + 1, M the inner
convolution length): pad reads N T (R2C) or 2 h1 T (C2R) and writes 2 M T; spectrum reads 4 M T, writes 2 M T; post: R2C
reads 2 h1 T of the workspace and writes 2 h1 T; C2R even reads 2 (N / 2) T and writes N T, C2R odd reads 2 N T and writes
N T."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import phastft_amd as P  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
CASES = [(10 ** 4, 1), (10 ** 6, 1), (999_999, 1), (1_000_003, 1), (10 ** 7, 1), (10 ** 4, 64), (10 ** 6, 16)]

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
    print("# case: t/transform and the ratio to the complex any-length transform of the same N (fft_any_batched); stages in us"
          " (pad, fwd M, spectrum, inv M, post); sweep GB/s and fraction of the copy probe; end-to-end vs the stage sum")
    for dt, tdt in (("f64", torch.float64), ("f32", torch.float32)):
        for n, batch in CASES:
            pl = (P.PlannerR2cAny64 if dt == "f64" else P.PlannerR2cAny32)(n)
            m, esz, h1 = pl.m, torch.empty(0, dtype=tdt).element_size(), n // 2 + 1
            x = torch.empty(n * batch, dtype=tdt, device="cuda").uniform_(-1, 1)
            o_re = torch.empty(h1 * batch, dtype=tdt, device="cuda")
            o_im = torch.empty_like(o_re)
            y = torch.empty_like(x)
            work = torch.empty(pl.workspace_len(batch), dtype=tdt, device="cuda")
            t_r2c = timed(lambda: P.r2c_any_batched(x, o_re, o_im, pl, batch, workspace=work))
            t_c2r = timed(lambda: P.c2r_any_batched(o_re, o_im, y, pl, batch, workspace=work))
            pc = (P.PlannerAny64 if dt == "f64" else P.PlannerAny32)(n)
            c_re, c_im = torch.empty_like(x).uniform_(-1, 1), torch.empty_like(x).uniform_(-1, 1)
            c_work = torch.empty(pc.workspace_len(batch), dtype=tdt, device="cuda")
            t_cx = timed(lambda: P.fft_any_batched(c_re, c_im, n, P.Direction.Forward, pc, workspace=c_work))
            del pc, c_re, c_im, c_work
            torch.cuda.empty_cache()
            for kind, t_call in (("r2c", t_r2c), ("c2r", t_c2r)):
                drain()
                torch.cuda.synchronize()
                if kind == "r2c":
                    st = [v * 1e3 for v in pl.time_stages(x, o_re, o_im, batch, work, REPS)]
                    b_pad, b_post = (n + 2 * m) * esz * batch, 4 * h1 * esz * batch
                else:
                    st = [v * 1e3 for v in pl.time_c2r_stages(o_re, o_im, y, batch, work, REPS)]
                    b_pad, b_post = (2 * h1 + 2 * m) * esz * batch, (3 * n if n & 1 else 2 * n) * esz * batch
                b_spec = 6 * m * esz * batch
                rates = [b / (t * 1e3) for b, t in ((b_pad, st[0]), (b_spec, st[2]), (b_post, st[4]))]   # GB/s
                model = sum(st)
                print(f"{dt} {kind} N={n} M=2^{m.bit_length() - 1} x{batch}: {t_call / batch:9.2f} us/transform"
                      f" = {t_call / t_cx:.2f} x complex ({t_cx / batch:.2f} us), {n * batch / t_call / 1e3:6.2f} GS/s;"
                      f" stages {st[0]:.1f} {st[1]:.1f} {st[2]:.1f} {st[3]:.1f} {st[4]:.1f} us;"
                      f" sweeps {rates[0]:.0f} / {rates[1]:.0f} / {rates[2]:.0f} GB/s = {rates[0] / copy:.2f} / {rates[1] / copy:.2f} /"
                      f" {rates[2] / copy:.2f} of copy; call {t_call:.1f} us vs stages {model:.1f} us ({t_call / model - 1:+.1%})",
                      flush=True)
            del x, o_re, o_im, y, work, pl
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
