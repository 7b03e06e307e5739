#!/usr/bin/env python3
"""Rates of building a NUFFT planner's point tables: the host-path constructor (points in host memory, sorted on the host,
tables copied to the device: wall clock, copy included), `from_device` and `set_points` (points in device memory, sorted on the
device: DESIGN.md §22; both block, wall clock), all three in one run on one box, every timed region behind a cache drain (a read
of 1 GiB nothing else uses), as bench.py times its regions -- this tool does not import bench.py.  Beside them the three stages of
one `set_points` between device events (keys, sort of the pairs, tables), the sort in keys per second, and the sort's bytes / time
against this box's copy rate (phast_stream_probe_dev, measured in the same run).

    python tools/nufft_sort_rate.py [reps] [log]

writes what it prints to `log` (profiles/nufft_sort_rate.log by default).  Without a GPU the log says "unmeasured" and names this
command.

Bytes of the sort stage, M keys of `bits` bits in P = ceil(bits / 4) passes: a pass reads the keys for the histogram (4 M), reads
keys and indices for the scatter (8 M; 4 M in the first pass, whose indices are the positions) and writes both (8 M): 20 M P - 4 M.
The counts and their scan are M / 64 bytes a pass and are left out."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
LOG = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "nufft_sort_rate.log")
CASES = [((1 << 20,), 1 << 20), ((1 << 20,), 1 << 24), ((128, 128, 128), 1 << 20), ((128, 128, 128), 1 << 24)]
EPS = 1e-6

_drain_buf = None
_lines = []


def say(line):
    print(line, flush=True)
    _lines.append(line)


def drain(torch):
    global _drain_buf
    if _drain_buf is None:
        _drain_buf = torch.ones(1 << 27, dtype=torch.float64, device="cuda")
    _drain_buf.sum()
    torch.cuda.synchronize()


def wall(torch, call, reps):
    """ms per blocking call: the mean of `reps`, each behind a drain"""
    total = 0.0
    for _ in range(reps):
        drain(torch)
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        total += time.perf_counter() - t0
    return total / reps * 1e3


def main():
    import numpy as np
    import torch

    import phastft_amd as P

    probe = P.stream_probe(1024, 5)
    copy = probe["copy"]
    say(f"# {P.device_info()['name']}: copy probe {copy:.0f} GB/s (read {probe['read']:.0f}, write {probe['write']:.0f}); reps {REPS}"
        f" (host constructor: {min(REPS, 2)})")
    say("# case: wall-clock ms of the host-path constructor, from_device and set_points; the stages of one set_points in us"
        " (keys, sort, tables); the sort in 1e9 keys / s, its GB/s and fraction of the copy probe; host constructor / set_points")
    rng = np.random.default_rng(0)
    for ns, m in CASES:
        dims = len(ns)
        cls = P.PlannerNufft64 if dims == 1 else P.PlannerNufft3d64
        n_arg = ns[0] if dims == 1 else ns
        for which in ("uniform", "clumped"):
            pts = [rng.uniform(-3, 3, m) if which == "uniform" else 0.3 + rng.uniform(-1e-7, 1e-7, m) for _ in range(dims)]
            dev = [torch.from_numpy(p).cuda() for p in pts]
            keep = []

            def host():
                keep[:] = [cls(n_arg, *pts, EPS)]

            def from_device():
                keep[:] = [cls.from_device(n_arg, *dev, EPS)]

            host()   # warm-up: the engine's plans, the allocator
            t_host = wall(torch, host, min(REPS, 2))
            t_new = wall(torch, from_device, REPS)
            pl = keep[0]
            t_set = wall(torch, lambda: pl.set_points(*dev), REPS)
            st = [0.0, 0.0, 0.0]
            for _ in range(REPS):
                drain(torch)
                st = [a + b * 1e3 / REPS for a, b in zip(st, pl.time_set_points(*dev))]
            bits = pl.grid_len.bit_length() - 1
            passes = (bits + 3) // 4
            sort_bytes = (20 * passes - 4) * m
            rate = sort_bytes / (st[1] * 1e3)
            say(f"{dims}-D N={'x'.join(map(str, ns))} M=2^{m.bit_length() - 1} {which} eps={EPS:g} w={pl.width} cells=2^{bits} passes={passes}:"
                f" host {t_host:9.2f} ms; from_device {t_new:8.2f} ms; set_points {t_set:8.2f} ms;"
                f" stages {st[0]:.1f} {st[1]:.1f} {st[2]:.1f} us; sort {m / (st[1] * 1e3):.2f} Gkeys/s, {rate:.0f} GB/s = {rate / copy:.2f} of copy;"
                f" host / set_points {t_host / t_set:.1f} x")
            del pl, keep, dev
            torch.cuda.empty_cache()


if __name__ == "__main__":
    try:
        import torch as _torch

        have = _torch.cuda.is_available()
    except Exception:
        have = False
    if have:
        main()
    else:
        say("unmeasured: no GPU here.  Run `python tools/nufft_sort_rate.py` on the MI355X.")
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    with open(LOG, "w") as f:
        f.write("\n".join(_lines) + "\n")
