#!/usr/bin/env python3
"""Writes tests/golden/convnd_error_budget.json on the MI355X: per type and shape (L; K; B) of tests/convnd_reference.py, the worst
over seeds 0-3, every mode and both flips of the rel-L2 over the output against tests/convnd_reference.py (the direct sum in
long double).  tests/test_gpu_convnd.py keeps its gate >= 2 x above these.

    python tests/golden/make_convnd_error_budget.py [out.json]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import phastft_amd as P  # noqa: E402
from tests import convnd_reference as R  # noqa: E402
from tests.test_gpu_convnd import CASES, _ndt, convnd_gate, planner, rel_l2, run  # noqa: E402


def main(out):
    entries = []
    for dt in ("f64", "f32"):
        for shape in R.SHAPES:
            L, K, B = shape
            worst, where, block = 0.0, None, None
            for seed in range(4):
                for mode, flip in CASES:
                    if not R.has_mode(L, K, mode):
                        continue
                    x, h, want = R.expected(L, K, np.dtype(_ndt(dt)).name, mode, flip, seed)
                    pl = planner(P, dt, L, h, mode, flip, B)
                    rel = rel_l2(run(P, pl, x), want)
                    if block is None or convnd_gate(dt, pl.block) < convnd_gate(dt, block):
                        block = pl.block  # an automatic block may differ between the modes: the tightest gate counts
                    if rel > worst:
                        worst, where = rel, f"{mode}:{int(flip)}:seed{seed}"
                R.case.cache_clear()
            gate = convnd_gate(dt, block)
            entries.append({"dt": dt, "shape": R.shape_id(shape), "block": list(block), "rel": worst, "where": where, "gate_rel": gate,
                            "margin_rel": gate / worst if worst else None})
            print(json.dumps(entries[-1]), flush=True)
    doc = {"what": "worst over seeds 0-3, every mode and both flips of the rel-L2 over the output vs tests/convnd_reference.py in"
                   " long double", "device": P.device_info()["name"], "entries": entries}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "convnd_error_budget.json"))
