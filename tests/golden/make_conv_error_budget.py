#!/usr/bin/env python3
"""Writes tests/golden/conv_error_budget.json on the MI355X: per type and shape (L, K, B) of tests/test_gpu_conv.py, the worst
over seeds 0-3, both tap kinds (uniform(-1, 1) and a Hann-windowed half-band sinc), every mode and both flips of the rel-L2
over the output against tests/conv_reference.py (the direct sum in long double).  tests/test_gpu_conv.py keeps its gate
>= 2 x above these.

    python tests/golden/make_conv_error_budget.py [out.json]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import phastft_amd as P  # noqa: E402
from tests import conv_reference as R  # noqa: E402
from tests.test_gpu_any_real import inner_m  # noqa: E402
from tests.test_gpu_conv import CASES, SHAPES, _full, _signal, _taps, block_of, conv_gate, planner, reference, rel_l2, run  # noqa: E402


def main(out):
    entries = []
    for dt in ("f64", "f32"):
        for shape in SHAPES:
            length, k, block = shape
            b = block_of(shape)
            worst, where = 0.0, None
            for seed in range(4):
                for kind in R.TAPS:
                    for mode, flip in CASES:
                        if mode == "valid" and length < k:
                            continue
                        pl = planner(P, dt, length, _taps(kind, k, dt, seed), mode, flip, block)
                        assert pl.block == b
                        rel = rel_l2(run(P, pl, _signal(length, dt, seed)), reference(dt, length, k, kind, mode, flip, seed))
                        if rel > worst:
                            worst, where = rel, f"{kind}:{mode}:{int(flip)}:seed{seed}"
                _full.cache_clear()
            gate = conv_gate(dt, b)
            entries.append({"dt": dt, "len": length, "k": k, "block_arg": block, "block": b, "m": inner_m(b), "rel": worst,
                            "where": where, "gate_rel": gate, "margin_rel": gate / worst if worst else None})
            print(json.dumps(entries[-1]), flush=True)
    doc = {"what": "worst over seeds 0-3, both tap kinds, every mode and both flips of the rel-L2 over the output vs"
                   " tests/conv_reference.py in long double", "device": P.device_info()["name"], "entries": entries}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "conv_error_budget.json"))
