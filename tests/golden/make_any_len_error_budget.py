#!/usr/bin/env python3
"""Writes tests/golden/any_len_error_budget.json on the MI355X: the worst rel-L2 and worst bin (relative to the rms bin) of the
arbitrary-length transforms against numpy's long-double pocketfft, over seeds 0-3, forward and inverse, per type and length.
tests/test_gpu_any_len.py keeps its gates >= 3.7 x above these.

    python tests/golden/make_any_len_error_budget.py [out.json]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import phastft_amd as P  # noqa: E402
from tests import tolerances as tol  # noqa: E402
from tests.test_gpu_any_len import _dev_fft, _input, _ref, any_gates, conv_len  # noqa: E402

SIZES = [2, 3, 5, 7, 12, 100, 127, 255, 300, 1000, 1009, 4095, 4097, 65537, 10 ** 5, 1_000_003, 10 ** 6]
LARGE_F64 = [3 << 20]


def main(out):
    entries = []
    for dt in ("f64", "f32"):
        for n in SIZES + (LARGE_F64 if dt == "f64" else []):
            pl = (P.PlannerAny64 if dt == "f64" else P.PlannerAny32)(n)
            rel_w = bin_w = 0.0
            for seed in range(4):
                re, im = _input(n, dt, seed)
                for direction in (1, -1):
                    g_re, g_im = _dev_fft(P, dt, re, im, direction, pl)
                    ref = _ref(re, im, direction)
                    r, i = np.asarray(ref.real, np.float64), np.asarray(ref.imag, np.float64)
                    rel_w = max(rel_w, tol.rel_l2(g_re, g_im, r, i))
                    bin_w = max(bin_w, tol.max_bin_err(g_re, g_im, r, i))
            g_rel, g_bin = any_gates(dt, n)
            entries.append({"dt": dt, "n": n, "m": conv_len(n), "rel": rel_w, "bin": bin_w,
                            "gate_rel": g_rel, "gate_bin": g_bin, "margin_rel": g_rel / rel_w if rel_w else None,
                            "margin_bin": g_bin / bin_w if bin_w else None})
            print(json.dumps(entries[-1]), flush=True)
    doc = {"what": "worst rel-L2 / worst bin over seeds 0-3, forward and inverse, vs numpy long-double FFT",
           "device": P.device_info()["name"], "entries": entries}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "any_len_error_budget.json"))
