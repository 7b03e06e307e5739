#!/usr/bin/env python3
"""Writes tests/golden/synthesizer_error_budget.json on the MI355X: per type, kind (real / complex output) and case (F, K, M, D),
the worst use of the two gates of tests/test_gpu_synthesizer.py -- per output and in L2, each the chain's term (t + 3) u A plus
the transform's gate carried through B -- measured as the test measures it, over the windows and the batch.  Every entry must
stay >= 2 x inside its gate (use <= 0.5); the script exits 1 if one does not.

    python tests/golden/make_synthesizer_error_budget.py [out.json]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import phastft_amd as P  # noqa: E402
from tests import synthesizer_reference as R  # noqa: E402
from tests.test_gpu_synthesizer import DTS, KINDS, measure  # noqa: E402


def main(out):
    entries = []
    for dt in DTS:
        for kind in KINDS:
            for case in R.CASES:
                worst, l2 = measure(P, dt, case, kind == "real")
                entries.append({"dt": dt, "kind": kind, "case": R.case_id(case), "terms": -(-case[1] // case[3]), "output": worst,
                                "l2": l2, "use": max(worst, l2)})
                print(json.dumps(entries[-1]), flush=True)
    doc = {"what": "the worst use of each gate of tests/test_gpu_synthesizer.py (1 = at the gate) against tests/synthesizer_reference.py"
                   " in long double",
           "device": P.device_info()["name"], "entries": entries}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
    top = max(e["use"] for e in entries)
    print(f"largest use {top:.3f}")
    return 0 if top <= 0.5 else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "synthesizer_error_budget.json")))
