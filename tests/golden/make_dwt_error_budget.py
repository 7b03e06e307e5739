#!/usr/bin/env python3
"""Writes tests/golden/dwt_error_budget.json on the MI355X: per type, case and mode, the worst use of its gate, measured as
tests/test_gpu_dwt.py measures it.  Cascade cases (L, F, J): the larger of |got - ref| / (l (F + 2) u Abs_l) over the packed
coefficients and of |got - ref| / (J (F + 2) u AbsS) over the samples waverec rebuilds from random coefficients, over the
batch.  Round trips (wavelet, L, J): |waverec(wavedec(x)) - x| over 2 J (F + 2) u AbsS(AbsA(|x|)) plus the reference's own
long double defect.  Every entry must stay >= 2 x inside its gate (use <= 0.5); the script exits 1 if one does not.

    python tests/golden/make_dwt_error_budget.py [out.json]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import phastft_amd as P  # noqa: E402
from tests import dwt_reference as R  # noqa: E402
from tests.test_gpu_dwt import CASES, DTS, ROUND_TRIPS, case_id, measure, measure_round_trip  # noqa: E402


def main(out):
    entries = []
    for dt in DTS:
        for case in CASES:
            for mode in R.MODES:
                fwd, inv = measure(P, dt, case, mode)
                entries.append({"dt": dt, "what": "cascade", "case": case_id(case), "mode": mode, "wavedec": fwd, "waverec": inv,
                                "use": max(fwd, inv)})
        for name, L, J in ROUND_TRIPS:
            for mode in R.MODES:
                entries.append({"dt": dt, "what": "round trip", "case": f"{name}x{L}x{J}", "mode": mode,
                                "use": measure_round_trip(P, dt, name, L, J, mode)})
    doc = {"what": "the worst use of each gate of tests/test_gpu_dwt.py (1 = at the gate) against tests/dwt_reference.py in long double",
           "device": P.device_info()["name"], "entries": entries}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
    top = max(entries, key=lambda e: e["use"])
    print(f"largest use {top['use']:.3f}: {top}")
    return 0 if top["use"] <= 0.5 else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "dwt_error_budget.json")))
