#!/usr/bin/env python3
"""Writes tests/golden/nufft_t3_error_budget.json on the MI355X: per dtype, case (M, K, point set) and eps of
tests/test_gpu_nufft_t3.py, the worst over seeds 0-1, both directions and complex and real data of the rel-L2 and of the worst
element / rms against tests/nufft_t3_reference.py (the direct sum in long double with exact phases), and beside each the same
two figures of the numpy model of the schedule (tests/test_nufft_t3_cpu.py: double arithmetic for f64, float32 kernel values,
grids and tables for f32) and the conditioning Q of the case.  tests/test_gpu_nufft_t3.py keeps its gates >= 2 x above the
device's figures.

    python tests/golden/make_nufft_t3_error_budget.py [out.json]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import phastft_amd as P  # noqa: E402
from tests import nufft_t3_reference as R  # noqa: E402
from tests import tolerances as tol  # noqa: E402
from tests.test_gpu_nufft_t3 import measure  # noqa: E402
from tests.test_nufft_t3_cpu import model, nufft_t3_gate, reference  # noqa: E402


def model_figures(dt, case, eps):
    ref = reference(case)
    rel = worst = 0.0
    for seed in R.SEEDS:
        for d in (R.FORWARD, R.REVERSE):
            for real in (False, True):
                got = model(ref.x, ref.s, ref.inp(real, seed), eps, d, np.float64 if dt == "f64" else np.float32)
                want = ref.ref[(d, real, seed)]
                rel = max(rel, tol.rel_l2(got.real, got.imag, *want))
                worst = max(worst, tol.max_bin_err(got.real, got.imag, *want))
    return rel, worst


def main(out):
    entries = []
    for dt in ("f64", "f32"):
        for case in R.CASES:
            for eps in R.EPS[dt]:
                rel, worst, pl = measure(P, dt, case, eps)
                m_rel, m_bin = model_figures(dt, case, eps)
                q = float(reference(case).q)
                g_rel, g_bin = nufft_t3_gate(dt, 2 * pl.grid_len, eps, q)
                entries.append({"dt": dt, "case": R.case_id(case), "m": case[0], "k": case[1], "kind": case[4], "eps": eps,
                                "w": pl.width, "n_f": pl.grid_len, "n_g": 2 * pl.grid_len, "q": q, "rel": rel, "bin": worst,
                                "model_rel": m_rel, "model_bin": m_bin, "gate_rel": g_rel, "gate_bin": g_bin,
                                "margin_rel": g_rel / rel if rel else None, "margin_bin": g_bin / worst if worst else None})
                print(json.dumps(entries[-1]), flush=True)
    doc = {"what": "worst over seeds 0-1, both directions, complex and real data of the rel-L2 and of the worst element / rms vs "
                   "tests/nufft_t3_reference.py in long double; model_*: the numpy model of the schedule; q: 2 pi (|C_s| + S) X",
           "device": P.device_info()["name"], "entries": entries}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "nufft_t3_error_budget.json"))
