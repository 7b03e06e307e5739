#!/usr/bin/env python3
"""Rates of the continuous wavelet transform, in one run: this box's copy rate (phast_stream_probe_dev); the four stages of
PlannerCwt (time_stages: forward, bank, inverse, crop) on batches that fill the chip -- 16 real signals of 2^16 points at 64
scales, one real signal of 2^20 points at 32 scales -- f64 and f32, Morlet and DOG (m = 2), P = L and a padded P (L = 3/4 of
the power of two); the bank kernel as a fraction of the copy rate on the bytes it writes, which is its only yardstick; beside
them the route a user had before this planner for the same result: a precomputed S x P complex filter tensor, one torch
multiply that broadcasts the spectrum over it, and fft_any_batched in place on the S rows.  Times and peak device memory
(torch's allocator) of both.  Every timed region starts behind a cache drain (a read of 1 GiB nothing else uses), as bench.py
times its regions -- this tool does not import bench.py.

    python tools/cwt_rate.py [reps] > profiles/cwt_rate.log

Bytes of the bank: 2 planes x S x P elements written per signal; what it reads (the spectrum once per scale group) is 1 / 8
of a plane or less.  Bytes of the old route's multiply: the filter read, the product written (the spectrum stays in cache):
two plane-sized streams, behind a third that built the filter."""
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import phastft_amd as P  # noqa: E402

ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
REPS = int(ARGS[0]) if ARGS else 10
# (batch, P, S)
SHAPES = [(16, 1 << 16, 64), (1, 1 << 20, 32)]

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


def peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def filter_tensor(pn, scales, wavelet, cdt):
    """conj(c_j psi_hat(s_j w_k)), L2 norm, as an (S, P) complex device tensor built with torch in double"""
    k = torch.arange(pn, device="cuda", dtype=torch.float64)
    w = 2 * math.pi * torch.where(k <= pn // 2, k, k - pn) / pn
    x = torch.as_tensor(scales, device="cuda")[:, None] * w[None, :]
    c = torch.sqrt(2 * math.pi * torch.as_tensor(scales, device="cuda"))[:, None]
    if wavelet == "morlet":
        f = math.pi ** -0.25 * torch.where(x > 0, torch.exp(-(x - 6.0) ** 2 / 2), torch.zeros_like(x))
    else:  # dog, m = 2: conj(-(i^2)) = 1
        f = x ** 2 * torch.exp(-x * x / 2) / math.sqrt(math.gamma(2.5))
    return (c * f).to(cdt)


def main():
    info = P.device_info()
    probe = P.stream_probe(1024, 5)
    copy = probe["copy"]
    print(f"# {info['name']}: copy probe {copy:.0f} GB/s (read {probe['read']:.0f}, write {probe['write']:.0f}); reps {REPS}")
    print("# stages from time_stages (us): forward, bank, inverse, crop; bank: GB/s on the 2 S P elements per signal it writes, as a"
          " fraction of copy; old route: filter tensor (built once, not timed) x spectrum by torch, then fft_any_batched on the rows")
    for dt, tdt, cdt in (("f64", torch.float64, torch.complex128), ("f32", torch.float32, torch.complex64)):
        esz = 8 if dt == "f64" else 4
        cls = P.PlannerCwt64 if dt == "f64" else P.PlannerCwt32
        anyc = P.PlannerAny64 if dt == "f64" else P.PlannerAny32
        for batch, pn, s in SHAPES:
            for length in (pn, 3 * pn // 4):
                scales = P.cwt_scales(length, dj=(math.log2(length / 2.0)) / (s - 1) - 1e-9)[:s]
                assert len(scales) == s
                x = torch.empty(batch * length, dtype=tdt, device="cuda").uniform_(-1, 1)
                for wavelet in ("morlet", "dog"):
                    state = {}

                    def new():
                        pl = cls(length, scales, wavelet, None, "l2", pn, True)
                        out = torch.empty((2, batch * s * length), dtype=tdt, device="cuda")
                        work = torch.empty(pl.workspace_len(batch), dtype=tdt, device="cuda")
                        pl.time_stages(x, None, out[0], out[1], batch, workspace=work, reps=1)
                        state.update(pl=pl, out=out, work=work)

                    mem_new = peak_mib(new)
                    pl, out, work = state["pl"], state["out"], state["work"]
                    drain()
                    st = [1e3 * v for v in pl.time_stages(x, None, out[0], out[1], batch, workspace=work, reps=REPS)]
                    xs, outs = x.view(batch, length), tuple(o.view(batch, s, length) for o in out)
                    call = timed(lambda: P.cwt_batched(xs, pl, out=outs, work=work))
                    gbs = batch * 2 * s * pn * esz / (st[1] * 1e3)
                    print(f"{dt} {wavelet} batch={batch} L={length} P={pn} S={s}: call {call:9.1f} us; forward {st[0]:9.1f} bank {st[1]:9.1f}"
                          f" inverse {st[2]:9.1f} crop {st[3]:9.1f}; bank {gbs:.0f} GB/s = {gbs / copy:.3f} copy; peak memory"
                          f" {mem_new:.0f} MiB (output {2 * batch * s * length * esz / 2 ** 20:.0f})", flush=True)
                    del pl, out, work, outs, state
                    torch.cuda.empty_cache()

                    # the route of the parent commit: filter tensor, torch multiply, fft_any_batched
                    filt = filter_tensor(pn, scales, wavelet, cdt)
                    pa = anyc(pn)
                    old = {}

                    def old_route():
                        spec = torch.fft.fft(x.view(batch, length), n=pn)            # (batch, P)
                        y = spec[:, None, :] * filt[None, :, :]                      # (batch, S, P)
                        re, im = y.real.contiguous().view(-1), y.imag.contiguous().view(-1)
                        P.fft_any_batched(re, im, pn, P.Direction.Reverse, pa)
                        old["w"] = (re.view(batch, s, pn)[..., :length], im.view(batch, s, pn)[..., :length])

                    mem_old = peak_mib(old_route) + filt.numel() * filt.element_size() / 2 ** 20
                    t_old = timed(old_route)
                    print(f"{dt} {wavelet} batch={batch} L={length} P={pn} S={s}: old route {t_old:9.1f} us = {t_old / call:.2f} x the call;"
                          f" peak memory {mem_old:.0f} MiB = {mem_old / mem_new:.2f} x", flush=True)
                    del filt, pa, old
                    torch.cuda.empty_cache()
                del x


if __name__ == "__main__":
    main()
