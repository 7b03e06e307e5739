#!/usr/bin/env python3
"""Writes tests/golden/nd_error_budget.json on the MI355X: the worst rel-L2 and worst bin (relative to the rms bin) of the
multi-dimensional transforms against numpy's long-double fftn / ifftn / rfftn / irfftn (float64 from 2^21 points on), over
seeds 0-3, per type, kind and shape (complex: forward and inverse).  tests/test_gpu_nd.py and tests/test_gpu_real_nd.py keep
their gates >= 3.7 x above these.

    python tests/golden/make_nd_error_budget.py [out.json]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import phastft_amd as P  # noqa: E402
from tests import tolerances as tol  # noqa: E402
from tests import test_gpu_nd as C  # noqa: E402
from tests import test_gpu_real_nd as R  # noqa: E402


def _entry(kind, dt, shape, rel, b, gates):
    e = {"kind": kind, "dt": dt, "shape": list(shape), "rel": rel, "bin": b, "gate_rel": gates[0], "gate_bin": gates[1],
         "margin_rel": gates[0] / rel if rel else None, "margin_bin": gates[1] / b if b else None}
    print(json.dumps(e), flush=True)
    return e


def main(out):
    entries = []
    for dt, shape in C._cases():
        pl = C._planner(P, dt, shape)
        rel_w = bin_w = 0.0
        for seed in range(4):
            re, im = C._input(shape, dt, seed)
            for direction in (1, -1):
                g_re, g_im = C._dev_fft(P, dt, re, im, direction, pl)
                rel, b = C._errors(g_re, g_im, C._ref(re, im, shape, direction))
                rel_w, bin_w = max(rel_w, rel), max(bin_w, b)
        entries.append(_entry("c2c", dt, shape, rel_w, bin_w, C.nd_gates(dt, shape)))
    for dt, shape in R._cases():
        pl = R._planner(P, dt, shape)
        w = {"r2c": [0.0, 0.0], "c2r": [0.0, 0.0]}
        for seed in range(4):
            x = R._real(shape, dt, seed)
            g_re, g_im = R._dev_r2c(P, x, pl)
            r_re, r_im = (np.asarray(v, np.float64) for v in R.ref_r2c(x, shape))
            w["r2c"] = [max(w["r2c"][0], tol.rel_l2(g_re, g_im, r_re, r_im)), max(w["r2c"][1], tol.max_bin_err(g_re, g_im, r_re, r_im))]
            s_re, s_im = R._spectrum(shape, dt, seed)
            got = R._dev_c2r(P, s_re, s_im, pl)
            ref = np.asarray(R.ref_c2r(s_re, s_im, shape), np.float64)
            z = np.zeros_like(ref)
            w["c2r"] = [max(w["c2r"][0], tol.rel_l2(got, z, ref, z)), max(w["c2r"][1], tol.max_bin_err(got, z, ref, z))]
        for kind in ("r2c", "c2r"):
            entries.append(_entry(kind, dt, shape, w[kind][0], w[kind][1], R.real_gates(dt, shape)))
    doc = {"what": "worst rel-L2 / worst bin over seeds 0-3 vs numpy long-double fftn / ifftn / rfftn / irfftn "
                   "(float64 from 2^21 points on)",
           "device": P.device_info()["name"], "entries": entries}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "nd_error_budget.json"))
