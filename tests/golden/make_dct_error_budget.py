#!/usr/bin/env python3
"""Writes tests/golden/dct_error_budget.json on the MI355X: the worst rel-L2 and worst bin (relative to the rms bin) of the
DCT / DST of types II and III against scipy.fft.dct / dst in long double, over seeds 0-3, all four transforms and all three
norms, per type and length.  tests/test_gpu_dct.py keeps its gates >= 3 x above these.

    python tests/golden/make_dct_error_budget.py [out.json]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import phastft_amd as P  # noqa: E402
from tests.test_gpu_dct import KINDS, NORMS, _signal, dct_gates, errors, planner, ref, run_dev  # noqa: E402
from tests.test_gpu_any_real import inner_m  # noqa: E402

SIZES = [1, 2, 3, 4, 5, 7, 8, 16, 17, 100, 101, 255, 300, 1000, 1001, 4094, 4096, 65537, 999_999, 10 ** 6, 1 << 20]
LARGE = {"f64": [3 << 20], "f32": [3 << 20, 1 << 24]}


def main(out):
    entries = []
    for dt in ("f64", "f32"):
        for n in SIZES + LARGE[dt]:
            pl = planner(P, dt, n)
            rel_w = bin_w = 0.0
            for seed in range(4):
                x = _signal(n, dt, seed)
                for kind, t in KINDS:
                    for norm in NORMS if n < 10 ** 5 else [None, "ortho"]:
                        rel, worst = errors(run_dev(P, dt, kind, t, x, norm, pl), ref(kind, t, x, norm))
                        rel_w, bin_w = max(rel_w, rel), max(bin_w, worst)
            g_rel, g_bin = dct_gates(dt, n)
            entries.append({"dt": dt, "n": n, "m": inner_m(n), "rel": rel_w, "bin": bin_w,
                            "gate_rel": g_rel, "gate_bin": g_bin, "margin_rel": g_rel / rel_w if rel_w else None,
                            "margin_bin": g_bin / bin_w if bin_w else None})
            print(json.dumps(entries[-1]), flush=True)
    doc = {"what": "worst rel-L2 / worst bin over seeds 0-3, DCT-II/III and DST-II/III, every norm (above 10^5 points:"
                   " backward and ortho), vs scipy.fft long double", "device": P.device_info()["name"], "entries": entries}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "dct_error_budget.json"))
