#!/usr/bin/env python3
"""Writes tests/golden/psd_error_budget.json on the MI355X: per type and shape (L, P, H, F), the worst over seeds 0-3 and over
the configurations (both detrends, both scalings at fs = 2.5, Hann and a random window; the two large shapes: the default
configuration) of the rel-L2 error of the auto spectrum, the cross spectrum with both auto spectra, and the spectrogram against
tests/psd_reference.py in long double, measured as tests/test_gpu_psd.py measures it.  Every entry must stay >= 3 x below the
gate; the script exits 1 if one does not.

    python tests/golden/make_psd_error_budget.py [out.json]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import phastft_amd as P  # noqa: E402
from tests.test_gpu_psd import CONFIGS, SHAPES, check_all, planner, psd_gate, psd_log2m, reference  # noqa: E402

LARGE = [(1 << 20, 1024, 256, 1024), (10 ** 6, 1000, 250, 1000)]


def main(out):
    entries = []
    for dt in ("f64", "f32"):
        for shape in SHAPES + LARGE:
            worst = 0.0
            for cfg in CONFIGS[:1] if shape in LARGE else CONFIGS:
                pl = planner(P, dt, shape, *cfg)
                for seed in range(4):
                    worst = max(worst, check_all(f"{shape}:{cfg}:{seed}", dt, shape, cfg, P, pl, seed=seed))
                reference.cache_clear()
            gate = psd_gate(dt, shape[3])
            entries.append({"dt": dt, "len": shape[0], "nperseg": shape[1], "hop": shape[2], "nfft": shape[3], "log2_inner": psd_log2m(shape[3]),
                            "rel": worst, "gate_rel": gate, "margin_rel": gate / worst if worst else None})
            print(json.dumps(entries[-1]), flush=True)
    doc = {"what": "worst over seeds 0-3 and the configurations of the rel-L2 error of psd, csd (over |sqrt(Pxx Pyy)|, with both auto"
                   " spectra) and the spectrogram vs tests/psd_reference.py in long double, x uniform in [-1, 1)",
           "device": P.device_info()["name"], "entries": entries}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
    margins = [e["margin_rel"] for e in entries if e["margin_rel"] is not None]
    print(f"smallest margin {min(margins):.2f}")
    return 0 if min(margins) >= 3 else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "psd_error_budget.json")))
