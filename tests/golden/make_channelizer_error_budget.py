#!/usr/bin/env python3
"""Writes tests/golden/channelizer_error_budget.json on the MI355X: per type, kind (real / complex) and case (L, K, M, D), the
worst use of the two gates of tests/test_gpu_channelizer.py -- rel-L2 and worst bin, each with the fold's term (T + 2) u |A|
carried through the transform -- measured as the test measures it, over the windows and the batch.  Every entry must stay
>= 2 x inside its gate (use <= 0.5); the script exits 1 if one does not.

    python tests/golden/make_channelizer_error_budget.py [out.json]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import phastft_amd as P  # noqa: E402
from tests import channelizer_reference as R  # noqa: E402
from tests.test_gpu_channelizer import DTS, KINDS, measure  # noqa: E402


def main(out):
    entries = []
    for dt in DTS:
        for kind in KINDS:
            for case in R.CASES:
                rel, worst = measure(P, dt, case, kind == "complex")
                entries.append({"dt": dt, "kind": kind, "case": R.case_id(case), "products": R.t_of(case[1], case[2]), "rel": rel,
                                "bin": worst, "use": max(rel, worst)})
                print(json.dumps(entries[-1]), flush=True)
    doc = {"what": "the worst use of each gate of tests/test_gpu_channelizer.py (1 = at the gate) against tests/channelizer_reference.py"
                   " in long double",
           "device": P.device_info()["name"], "entries": entries}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
    top = max(e["use"] for e in entries)
    print(f"largest use {top:.3f}")
    return 0 if top <= 0.5 else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "channelizer_error_budget.json")))
