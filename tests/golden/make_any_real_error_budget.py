#!/usr/bin/env python3
"""Writes tests/golden/any_real_error_budget.json on the MI355X: the worst rel-L2 and worst bin (relative to the rms bin) of the
arbitrary-length real transforms against numpy's long-double rfft / irfft, over seeds 0-3, R2C and C2R (of a Hermitian
spectrum), per type and length.  tests/test_gpu_any_real.py keeps its gates >= 3 x above these.

    python tests/golden/make_any_real_error_budget.py [out.json]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import phastft_amd as P  # noqa: E402
from tests import tolerances as tol  # noqa: E402
from tests.test_gpu_any_real import (_dev_c2r, _dev_r2c, _planner, _ref_c2r, _ref_r2c, _signal, _spectrum, inner_m,  # noqa: E402
                                     real_gates)

SIZES = [1, 2, 3, 5, 6, 7, 12, 100, 127, 255, 300, 1000, 1002, 1009, 4094, 4097, 65538, 10 ** 5, 999_999, 10 ** 6, 1_000_003]
LARGE_F64 = [3 << 20]


def main(out):
    entries = []
    for dt in ("f64", "f32"):
        for n in SIZES + (LARGE_F64 if dt == "f64" else []):
            pl = _planner(P, dt, n)
            rel_w = bin_w = 0.0
            for seed in range(4):
                x = _signal(n, dt, seed)
                g_re, g_im = _dev_r2c(P, dt, x, pl)
                ref = _ref_r2c(x)
                r, i = np.asarray(ref.real, np.float64), np.asarray(ref.imag, np.float64)
                rel_w = max(rel_w, tol.rel_l2(g_re, g_im, r, i))
                bin_w = max(bin_w, tol.max_bin_err(g_re, g_im, r, i))
                re, im = _spectrum(n, dt, seed)
                got = _dev_c2r(P, dt, re, im, n, pl)
                ref = np.asarray(_ref_c2r(re, im, n), np.float64)
                z = np.zeros(n)
                rel_w = max(rel_w, tol.rel_l2(got, z, ref, z))
                bin_w = max(bin_w, tol.max_bin_err(got, z, ref, z))
            g_rel, g_bin = real_gates(dt, n)
            entries.append({"dt": dt, "n": n, "m": inner_m(n), "rel": rel_w, "bin": bin_w,
                            "gate_rel": g_rel, "gate_bin": g_bin, "margin_rel": g_rel / rel_w if rel_w else None,
                            "margin_bin": g_bin / bin_w if bin_w else None})
            print(json.dumps(entries[-1]), flush=True)
    doc = {"what": "worst rel-L2 / worst bin over seeds 0-3, R2C and C2R, vs numpy long-double rfft / irfft",
           "device": P.device_info()["name"], "entries": entries}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "any_real_error_budget.json"))
