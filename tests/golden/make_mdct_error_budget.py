#!/usr/bin/env python3
"""Writes tests/golden/mdct_error_budget.json on the MI355X: per type, shape (N, L) and direction, the worst over seeds 0-3 and
both framings of the rel-L2 and of the worst coefficient or sample (relative to the rms one) against reference (b) of
tests/mdct_reference.py in long double, with random uniform windows; and of the round trip through the sine, Vorbis and
Kaiser-Bessel-derived windows as an absolute error.  tests/test_gpu_mdct.py keeps its gates >= 3 x above the first two.

    python tests/golden/make_mdct_error_budget.py [out.json]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import phastft_amd as P  # noqa: E402
from tests import mdct_reference as R  # noqa: E402
from tests.test_gpu_mdct import SHAPES, WINDOWS, forward, framings, inverse, planner, reference, _signal, _window  # noqa: E402


def main(out):
    entries = []
    for dt in ("f64", "f32"):
        for n, length in SHAPES:
            worst = {"mdct": [0.0, 0.0], "imdct": [0.0, 0.0]}
            round_abs = 0.0
            for padded in framings(n, length):
                pl = None
                for seed in range(4):
                    w, X, Xr, back = reference(dt, n, length, padded, seed)
                    pl = pl or planner(P, dt, length, n, w, padded)
                    for name, got, want in (("mdct", forward(P, pl, _signal(length, dt, seed)), X), ("imdct", inverse(P, pl, Xr), back)):
                        worst[name] = [max(a, b) for a, b in zip(worst[name], R.errors(got, want))]
                reference.cache_clear()
                for win in WINDOWS:
                    pw = planner(P, dt, length, n, _window(n, dt, win), padded)
                    for seed in range(4):
                        x = _signal(length, dt, seed)
                        rt = inverse(P, pw, forward(P, pw, x))
                        lo, hi = (0, length) if padded else (n, pw.frames * n)
                        round_abs = max(round_abs, float(np.abs(rt[lo:hi].astype(np.float64) - x[lo:hi]).max()))
            g_rel, g_bin = R.mdct_gates(dt, n)
            for name, (rel, worst_bin) in worst.items():
                entries.append({"dt": dt, "n": n, "len": length, "dir": name, "log2_inner": R.inner_log2(n), "rel": rel, "bin": worst_bin,
                                "gate_rel": g_rel, "gate_bin": g_bin, "margin_rel": g_rel / rel if rel else None,
                                "margin_bin": g_bin / worst_bin if worst_bin else None, "round_trip_abs": round_abs})
                print(json.dumps(entries[-1]), flush=True)
    doc = {"what": "worst over seeds 0-3 and both framings of the rel-L2 and the worst coefficient / sample (over the rms one) of mdct"
                   " and imdct with random uniform windows vs reference (b) of tests/mdct_reference.py in long double; round_trip_abs:"
                   " max |imdct(mdct(x)) - x| over the sine, vorbis and kbd windows, x uniform in [-1, 1)",
           "device": P.device_info()["name"], "entries": entries}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "mdct_error_budget.json"))
