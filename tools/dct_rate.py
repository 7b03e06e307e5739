#!/usr/bin/env python3
"""Rates of the DCT / DST of types II and III: time per transform against the R2C (type II) or C2R (type III) of the same N
and batch in the same run, and each sweep's bytes / time against this box's copy rate (phast_stream_probe_dev, measured in
the same run) and against its floor of FP64 sincospi evaluations at 2.4e11 per second.  Every timed region
starts behind a cache drain (a read of 1 GiB nothing else uses), as bench.py times its regions -- this tool does not import
bench.py.

    python tools/dct_rate.py [reps]

End-to-end: device events around `reps` back-to-back calls.  Stages: PlannerDct*.time_stages (events between the pre sweep,
the real transform and the post sweep of one call).  Sweep bytes per transform (T = element size, h1 = N // 2 + 1): the
permutation sweeps (II-pre, III-post) read N T and write N T; the twiddle sweeps (II-post, III-pre) read 2 h1 T and write
N T, or read N T and write 2 h1 T, and evaluate h1 sincospi each.  The end-to-end target is the inner transform plus both
sweeps' bytes at 0.75 of copy plus 4 us."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import phastft_amd as P  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
CASES = [(1 << 20, 1), (10 ** 6, 1), (999_999, 1), (1 << 24, 1), (10 ** 6, 16), (1024, 4096)]
SINCOSPI_PER_S = 2.4e11

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
    print(f"# {P.device_info()['name']}: copy probe {copy:.0f} GB/s (read {probe['read']:.0f}, write {probe['write']:.0f}); "
          f"reps {REPS}; sincospi floor at {SINCOSPI_PER_S:.1e}/s (DESIGN.md §12)")
    print("# case: t/call, ratio to the inner R2C / C2R of the same N and batch; stages pre / inner / post in us; each sweep's"
          " GB/s as a fraction of copy and its floor max(bytes at copy, evaluations at the sincospi rate); end-to-end target"
          " = inner + sweep bytes at 0.75 copy + 4 us")
    for dt, tdt in (("f64", torch.float64), ("f32", torch.float32)):
        for n, batch in CASES:
            pl = (P.PlannerDct64 if dt == "f64" else P.PlannerDct32)(n)
            pr = (P.PlannerR2cAny64 if dt == "f64" else P.PlannerR2cAny32)(n)
            esz, h1 = torch.empty(0, dtype=tdt).element_size(), n // 2 + 1
            x = torch.empty(n * batch, dtype=tdt, device="cuda").uniform_(-1, 1)
            y = torch.empty_like(x)
            work = torch.empty(pl.workspace_len(batch), dtype=tdt, device="cuda")
            o_re = torch.empty(h1 * batch, dtype=tdt, device="cuda").uniform_(-1, 1)
            o_im = torch.empty_like(o_re).uniform_(-1, 1)
            r_work = torch.empty(max(1, pr.workspace_len(batch)), dtype=tdt, device="cuda")
            t_r2c = timed(lambda: P.r2c_any_batched(x, o_re, o_im, pr, batch, workspace=r_work))
            t_c2r = timed(lambda: P.c2r_any_batched(o_re, o_im, y, pr, batch, workspace=r_work))
            b_perm, b_tw = 2 * n * esz * batch, (n + 2 * h1) * esz * batch
            floor_tw = max(b_tw / (copy * 1e3), h1 * batch / SINCOSPI_PER_S * 1e6)  # us
            floor_perm = b_perm / (copy * 1e3)
            for kind in ("dct", "dst"):
                fn = P.dct_batched if kind == "dct" else P.dst_batched
                for t in (2, 3):
                    t_call = timed(lambda: fn(x, y, pl, batch, type=t, workspace=work))
                    drain()
                    torch.cuda.synchronize()
                    st = [v * 1e3 for v in pl.time_stages(x, y, kind, t, None, batch, work, REPS)]
                    t_inner = t_r2c if t == 2 else t_c2r
                    if t == 2:
                        (b_pre, f_pre), (b_post, f_post) = (b_perm, floor_perm), (b_tw, floor_tw)
                    else:
                        (b_pre, f_pre), (b_post, f_post) = (b_tw, floor_tw), (b_perm, floor_perm)
                    r_pre, r_post = b_pre / (st[0] * 1e3), b_post / (st[2] * 1e3)
                    target = t_inner + (b_pre + b_post) / (0.75 * copy * 1e3) + 4.0
                    print(f"{dt} {kind}{'II' if t == 2 else 'III'} N={n} x{batch}: {t_call:9.1f} us = {t_call / t_inner:.2f} x"
                          f" {'R2C' if t == 2 else 'C2R'} ({t_inner:.1f} us); stages {st[0]:.1f} / {st[1]:.1f} / {st[2]:.1f} us;"
                          f" pre {r_pre:.0f} GB/s = {r_pre / copy:.2f} copy (floor {f_pre:.1f} us, {st[0] / f_pre:.2f} x);"
                          f" post {r_post:.0f} GB/s = {r_post / copy:.2f} copy (floor {f_post:.1f} us, {st[2] / f_post:.2f} x);"
                          f" target {target:.1f} us: {'met' if t_call <= target else 'MISSED'}", flush=True)
            del x, y, work, o_re, o_im, r_work, pl, pr
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
