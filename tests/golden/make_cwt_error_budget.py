#!/usr/bin/env python3
"""Writes tests/golden/cwt_error_budget.json on the MI355X: per type, input kind (real / complex), family, norm and shape
(L, P, S), the worst use of the two gates of tests/test_gpu_cwt.py -- rel-L2 and worst bin of tests/tolerances.py at the inner
log2 of P, per row -- measured as the test measures it, over the rows and the batch.  Every entry must stay >= 2 x inside its
gate (use <= 0.5); the script exits 1 if one does not.

    python tests/golden/make_cwt_error_budget.py [out.json]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import phastft_amd as P  # noqa: E402
from tests import cwt_reference as R  # noqa: E402
from tests.test_gpu_cwt import DTS, KINDS, measure, shape_id  # noqa: E402


def main(out):
    entries = []
    for dt in DTS:
        for kind in KINDS:
            for family in R.FAMILIES:
                for norm in R.NORMS:
                    for shape in R.SHAPES:
                        rel, worst = measure(P, dt, shape, family, norm, kind == "real")
                        entries.append({"dt": dt, "kind": kind, "family": family, "norm": norm, "shape": shape_id(shape),
                                        "log2": R.inner_log2(shape[1]), "rel": rel, "bin": worst, "use": max(rel, worst)})
                        print(json.dumps(entries[-1]), flush=True)
    doc = {"what": "the worst use of each gate of tests/test_gpu_cwt.py (1 = at the gate) against tests/cwt_reference.py in long double",
           "device": P.device_info()["name"], "entries": entries}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
    top = max(e["use"] for e in entries)
    print(f"largest use {top:.3f}")
    return 0 if top <= 0.5 else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "cwt_error_budget.json")))
