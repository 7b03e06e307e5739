#!/usr/bin/env python3
"""Writes tests/golden/engine_batch_error_budget.json on the MI355X: per (type, case, rules) of tests/test_gpu_engine_batches.py
the worst rel-L2 and worst bin (relative to the rms bin) over the transforms that file compares with numpy's long-double FFT
(transforms 0, c // 2, c - 1 and both sides of every scratch-chunk boundary), the gates they are held to (the any-length and
any-real modules' own), `use` = the larger of error / gate, and the plan that ran (describe_call).  The cases run through the test
file's own functions, so its other assertions -- the single-transform bits, the gaps, the plan -- hold for what is recorded.
tests/test_gpu_engine_batches.py::test_gates_keep_their_margin requires every case to be present with use <= 0.5.

    python tests/golden/make_engine_batch_error_budget.py [out.json]
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import phastft_amd as P  # noqa: E402
from tests import test_gpu_engine_batches as E  # noqa: E402


def main(out):
    entries = []

    def keep(e, t0):
        e = {k: v for k, v in e.items() if k not in ("bits", "bytes")}
        e["seconds"] = round(time.perf_counter() - t0, 2)
        entries.append(e)
        print(json.dumps(e), flush=True)

    P.debug_set_guard_bytes(1 << 20)   # as the test module's fixture
    try:
        for dt, n, c, rules in E.cases():
            t0 = time.perf_counter()
            keep(E.run_case(P, dt, n, c, rules), t0)
        t0 = time.perf_counter()
        keep(E.run_scratch_chunks(P), t0)
        for dt, n, c in E.REAL_CASES:
            t0 = time.perf_counter()
            keep(E.run_real_case(P, dt, n, c), t0)
    finally:
        P.debug_set_guard_bytes(0)
    worst = max(entries, key=lambda e: e["use"])
    doc = {"what": "worst rel-L2 and worst bin / rms bin over the transforms tests/test_gpu_engine_batches.py compares with numpy's"
                   " long-double FFT, per (type, N, batch c, rules); use = max(rel / gate_rel, bin / gate_bin); plan = describe_call",
           "device": P.device_info()["name"], "worst_use": worst["use"],
           "worst_case": [worst["dt"], worst["n"], worst["c"], worst["rules"]], "entries": entries}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "engine_batch_error_budget.json"))
