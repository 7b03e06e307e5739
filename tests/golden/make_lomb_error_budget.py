#!/usr/bin/env python3
"""Writes tests/golden/lomb_error_budget.json on the MI355X: per type, case (M, K, kind of times), eps, mean setting and
normalisation, the worst over seeds 0-1 and over weights / none of max_k |got - ref| / max_k |ref| at the gated frequencies
against tests/lomb_reference.py in long double, measured as tests/test_gpu_lomb.py measures it, with d, n_g and Q of the
gate, and -- for M <= 1000 -- the same figure of the numpy model of the schedule (tests/test_lomb_cpu.py, seed 0).  Every
entry must stay >= 2 x below the gate; the script exits 1 if one does not.

    python tests/golden/make_lomb_error_budget.py [out.json]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import phastft_amd as P  # noqa: E402
from tests import lomb_reference as R  # noqa: E402
from tests.test_gpu_lomb import DTS, measure  # noqa: E402
from tests.test_lomb_cpu import MEANS, lomb_gate, lomb_model, reference  # noqa: E402


def main(out):
    entries = []
    for case in R.CASES:
        ref = reference(case)
        for dt in DTS:
            for eps in R.EPS[dt]:
                for fm in MEANS:
                    for norm in ref.norms():
                        err, d, pl = measure(P, dt, ref, eps, fm, norm)
                        model = None
                        if case[0] <= 1000:
                            model = max(R.error(lomb_model(ref, wt, fm, norm, 0, eps, dt), ref.ref[(wt, fm, norm, 0, dt)], ref.mask[(wt, fm, dt)])
                                        for wt in (False, True))
                        gate = lomb_gate(dt, 2 * pl.grid_len, eps, ref.q, d, norm)
                        entries.append({"dt": dt, "case": R.case_id(case), "eps": eps, "fm": fm, "norm": norm, "n_g": 2 * pl.grid_len,
                                        "q": ref.q, "d": d, "err": err, "model": model, "gate": gate, "margin": gate / err if err else None})
                        print(json.dumps(entries[-1]), flush=True)
    doc = {"what": "worst over seeds 0-1 and weights / none of max |got - ref| / max |ref| at the gated frequencies vs"
                   " tests/lomb_reference.py in long double; model: the numpy model of the schedule, seed 0",
           "device": P.device_info()["name"], "entries": entries}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
    margins = [e["margin"] for e in entries if e["margin"] is not None]
    print(f"smallest margin {min(margins):.2f}")
    return 0 if min(margins) >= 2 else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "lomb_error_budget.json")))
