#!/usr/bin/env python3
"""Writes tests/golden/resample_error_budget.json on the MI355X: per type and case, the worst use of its gate, measured as
tests/test_gpu_resample.py measures it.  Polyphase cases (L, K, up, down): the largest |got - ref| / ((Kp + 2) u sum |h x|)
over the windows and the batch.  Fourier cases (L, num): the larger of rel-L2 / its gate and worst sample / its gate of
tests/tolerances.py at the log2 of the larger inner transform.  Every entry must stay >= 2 x inside its gate (use <= 0.5); the
script exits 1 if one does not.

    python tests/golden/make_resample_error_budget.py [out.json]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import phastft_amd as P  # noqa: E402
from tests import resample_reference as R  # noqa: E402
from tests.test_gpu_resample import DTS, case_id, measure_fourier, measure_poly  # noqa: E402


def main(out):
    entries = []
    for dt in DTS:
        for case in R.UPFIRDN_CASES:
            entries.append({"dt": dt, "method": "upfirdn", "case": case_id(case), "products": R.products(case[1], case[2]),
                            "use": measure_poly(P, dt, case)})
            print(json.dumps(entries[-1]), flush=True)
        for case in R.FOURIER_CASES:
            rel, worst = measure_fourier(P, dt, case)
            entries.append({"dt": dt, "method": "resample", "case": case_id(case), "log2": R.fourier_log2(*case), "rel": rel, "bin": worst,
                            "use": max(rel, worst)})
            print(json.dumps(entries[-1]), flush=True)
    doc = {"what": "the worst use of each gate of tests/test_gpu_resample.py (1 = at the gate) against tests/resample_reference.py in"
                   " long double",
           "device": P.device_info()["name"], "entries": entries}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
    top = max(e["use"] for e in entries)
    print(f"largest use {top:.3f}")
    return 0 if top <= 0.5 else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "resample_error_budget.json")))
