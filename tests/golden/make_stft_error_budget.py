#!/usr/bin/env python3
"""Writes tests/golden/stft_error_budget.json on the MI355X: per type and shape (L, F, H), the worst over seeds 0-3 of the
forward rel-L2 and worst bin (relative to the rms bin) over the whole spectrogram, and of the rel-L2 over the signal of the
inverse and of the round trip, against tests/stft_reference.py in long double.  Shapes up to L = 5000 run both center values,
both pad modes and all three windows; the two long ones run center / reflect with the Hann and the uniform(0.5, 1.5) window.
tests/test_gpu_stft.py keeps its gates >= 2 x above these.

    python tests/golden/make_stft_error_budget.py [out.json]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import phastft_amd as P  # noqa: E402
from tests import stft_reference as R  # noqa: E402
from tests import tolerances as tol  # noqa: E402
from tests.test_gpu_any_real import inner_m  # noqa: E402
from tests.test_gpu_stft import MODES, SHAPES, forward, inverse, planner, reference, rel_l2, stft_gates, _signal  # noqa: E402

LONG = [(1 << 20, 1024, 256), (10 ** 6, 1000, 250)]


def main(out):
    entries = []
    for dt in ("f64", "f32"):
        for shape in SHAPES + LONG:
            length, f, h = shape
            small = shape in SHAPES
            worst = {"stft_rel": 0.0, "stft_bin": 0.0, "istft_rel": 0.0, "round_rel": 0.0}
            for center, pad in MODES if small else [(True, "reflect")]:
                for win in R.WINDOWS if small else ("hann", "uniform"):
                    pl = None
                    for seed in range(4):
                        w, spec, re, im, back = reference(dt, length, f, h, center, pad, win, seed)
                        pl = pl or planner(P, dt, length, f, h, w, center, pad)
                        x = _signal(length, dt, seed)
                        g_re, g_im = forward(P, pl, x)
                        want_re, want_im = (np.asarray(v, np.float64).reshape(-1) for v in (spec.real, spec.imag))
                        worst["stft_rel"] = max(worst["stft_rel"], tol.rel_l2(g_re, g_im, want_re, want_im))
                        worst["stft_bin"] = max(worst["stft_bin"], tol.max_bin_err(g_re, g_im, want_re, want_im))
                        if back is not None:
                            _, cnt = R.envelope(w, length, f, h, center)
                            worst["istft_rel"] = max(worst["istft_rel"], rel_l2(inverse(P, pl, re, im), back))
                            worst["round_rel"] = max(worst["round_rel"], rel_l2(inverse(P, pl, g_re, g_im),
                                                                               np.where(cnt > 0, x.astype(np.float64), 0.0)))
                    reference.cache_clear()
            g_rel, g_bin = stft_gates(dt, f)
            rel = max(worst["stft_rel"], worst["istft_rel"], worst["round_rel"])
            entries.append({"dt": dt, "len": length, "f": f, "h": h, "m": inner_m(f), **worst, "rel": rel, "bin": worst["stft_bin"],
                            "gate_rel": g_rel, "gate_bin": g_bin, "margin_rel": g_rel / rel if rel else None,
                            "margin_bin": g_bin / worst["stft_bin"] if worst["stft_bin"] else None})
            print(json.dumps(entries[-1]), flush=True)
    doc = {"what": "worst over seeds 0-3 of the forward rel-L2 / worst bin and of the inverse and round-trip rel-L2, every center"
                   " value, pad mode and window (the two long shapes: center / reflect, Hann and uniform), vs tests/stft_reference.py"
                   " in long double", "device": P.device_info()["name"], "entries": entries}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "stft_error_budget.json"))
