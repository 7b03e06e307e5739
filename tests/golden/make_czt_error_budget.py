#!/usr/bin/env python3
"""Writes tests/golden/czt_error_budget.json on the MI355X: per type and shape (N, M, step, start) of tests/test_gpu_czt.py, the
worst over seeds 0-3 of the rel-L2 and of the worst bin / rms bin against tests/czt_reference.py (the direct sum in long double
with exact phases).  tests/test_gpu_czt.py keeps its gates >= 2 x above these.

    python tests/golden/make_czt_error_budget.py [out.json]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import phastft_amd as P  # noqa: E402
from tests.test_czt_cpu import SHAPES, conv_len, czt_gate, step_of  # noqa: E402
from tests.test_gpu_czt import _signal, errors, planner, reference, run  # noqa: E402


def main(out):
    entries = []
    for dt in ("f64", "f32"):
        for shape in SHAPES:
            n, m, _, start = shape
            step = step_of(shape)
            pl = planner(P, dt, n, m, step, start)
            rel = worst = 0.0
            for seed in range(4):
                r, w = errors(*run(P, pl, *_signal(n, dt, seed)), *reference(dt, n, m, step, start, seed))
                rel, worst = max(rel, r), max(worst, w)
            reference.cache_clear()
            g_rel, g_bin = czt_gate(dt, n, m)
            entries.append({"dt": dt, "n": n, "m": m, "step": step, "start": start, "conv_len": conv_len(n, m), "rel": rel, "bin": worst,
                            "gate_rel": g_rel, "gate_bin": g_bin, "margin_rel": g_rel / rel if rel else None,
                            "margin_bin": g_bin / worst if worst else None})
            print(json.dumps(entries[-1]), flush=True)
    doc = {"what": "worst over seeds 0-3 of the rel-L2 and of the worst bin / rms bin vs tests/czt_reference.py in long double",
           "device": P.device_info()["name"], "entries": entries}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "czt_error_budget.json"))
