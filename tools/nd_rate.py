#!/usr/bin/env python3
"""Rates of the multi-dimensional transforms: time per transform and prod(n)/t for f64 and f32, forward and inverse; each
step of a complex forward call (PlannerNd*.time_steps: events between the steps of one call) with the transposes' bytes / time
against this box's copy rate (phast_stream_probe_dev, measured in the same run); the end-to-end call against the sum of its
steps.  Every timed region starts behind a cache drain (a read of 1 GiB nothing else uses), as bench.py times its regions --
this tool does not import bench.py.  Per-kernel times: run it once under rocprofv3 --kernel-trace --stats.

    python tools/nd_rate.py [reps]

A transpose reads and writes both planes once: 4 prod(n) T bytes (T = element size), read + write counted as the copy
probe counts them."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import phastft_amd as P  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
COMPLEX = [((4096, 4096), ("f64", "f32")), ((1000, 1000), ("f64", "f32")), ((1 << 20, 3), ("f64", "f32")),
           ((64, 64, 64), ("f64", "f32")), ((256, 256, 256), ("f64", "f32")), ((1024, 1024, 1024), ("f32",))]
REAL = [(4096, 4096), (1000, 1000)]

_drain_buf = None


def drain():
    global _drain_buf
    if _drain_buf is None:
        _drain_buf = torch.ones(1 << 27, dtype=torch.float64, device="cuda")
    _drain_buf.sum()


def timed(fn):
    """us per call of fn over REPS back-to-back calls behind a drain"""
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


def shape_s(shape):
    return "x".join(map(str, shape))


def complex_case(shape, dt, copy):
    tdt = torch.float64 if dt == "f64" else torch.float32
    pl = (P.PlannerNd64 if dt == "f64" else P.PlannerNd32)(shape)
    n, esz = pl.n, torch.empty(0, dtype=tdt).element_size()
    re = torch.empty(n, dtype=tdt, device="cuda").uniform_(-1, 1)
    im = torch.empty(n, dtype=tdt, device="cuda").uniform_(-1, 1)
    work = torch.empty(pl.workspace_len(1), dtype=tdt, device="cuda")
    t = {}
    for d in (P.Direction.Forward, P.Direction.Reverse):
        t[d] = timed(lambda: P.fft_nd_batched(re, im, d, pl, workspace=work))
    drain()
    torch.cuda.synchronize()
    steps = [x * 1e3 for x in pl.time_steps(re, im, 1, None, work, REPS)]
    kinds = [s.split()[0] for s in pl.describe().split("schedule: ")[1].split("; ")]
    tr = [s for s, k in zip(steps, kinds) if k == "transpose"]
    rows = [s for s, k in zip(steps, kinds) if k != "transpose"]
    gbs = [4 * n * esz / (s * 1e3) for s in tr]
    fr = " ".join(f"{g:.0f} GB/s = {g / copy:.2f}" for g in gbs)
    model = sum(steps)
    print(f"{dt} {shape_s(shape):>14}: fwd {t[P.Direction.Forward]:9.1f} us {n / t[P.Direction.Forward] / 1e3:6.2f} GS/s, "
          f"inv {t[P.Direction.Reverse]:9.1f} us {n / t[P.Direction.Reverse] / 1e3:6.2f} GS/s; rows "
          f"{' '.join(f'{s:.1f}' for s in rows)} us; transposes {' '.join(f'{s:.1f}' for s in tr)} us ({fr} of copy); "
          f"call {t[P.Direction.Forward]:.1f} us vs steps {model:.1f} us ({t[P.Direction.Forward] / model - 1:+.1%})",
          flush=True)
    if dt == "f64" and shape == (4096, 4096):
        try:
            z = torch.complex(re, im).reshape(shape)
            t_torch = timed(lambda: torch.fft.fft2(z))
            print(f"     (information only: torch.fft.fft2 on the same data as complex128, interleaved, another library: "
                  f"{t_torch:.1f} us)", flush=True)
        except Exception as e:  # noqa: BLE001
            print(f"     (torch.fft.fft2 did not run: {e})", flush=True)
    del re, im, work, pl
    torch.cuda.empty_cache()


def real_case(shape, dt):
    tdt = torch.float64 if dt == "f64" else torch.float32
    pl = (P.PlannerR2cNd64 if dt == "f64" else P.PlannerR2cNd32)(shape)
    n, h = pl.n, pl.half
    x = torch.empty(n, dtype=tdt, device="cuda").uniform_(-1, 1)
    o_re = torch.empty(h, dtype=tdt, device="cuda")
    o_im = torch.empty(h, dtype=tdt, device="cuda")
    out = torch.empty(n, dtype=tdt, device="cuda")
    work = torch.empty(pl.workspace_len(1), dtype=tdt, device="cuda")
    t_f = timed(lambda: P.r2c_nd_batched(x, o_re, o_im, pl, workspace=work))
    t_b = timed(lambda: P.c2r_nd_batched(o_re, o_im, out, pl, workspace=work))
    print(f"{dt} {shape_s(shape):>14} real: R2C {t_f:9.1f} us {n / t_f / 1e3:6.2f} GS/s, C2R {t_b:9.1f} us "
          f"{n / t_b / 1e3:6.2f} GS/s", flush=True)
    del x, o_re, o_im, out, work, pl
    torch.cuda.empty_cache()


def main():
    probe = P.stream_probe(1024, 5)
    copy = probe["copy"]
    print(f"# {P.device_info()['name']}: copy probe {copy:.0f} GB/s (read {probe['read']:.0f}, write {probe['write']:.0f}); "
          f"reps {REPS}")
    print("# complex: t per transform and GS/s (prod n / t) forward / inverse; forward steps in schedule order (row "
          "transforms, transposes); transpose GB/s (4 N T bytes) and fraction of the copy probe; the call vs the sum of steps")
    for shape, dts in COMPLEX:
        for dt in dts:
            complex_case(shape, dt, copy)
    for shape in REAL:
        for dt in ("f64", "f32"):
            real_case(shape, dt)


if __name__ == "__main__":
    main()
