#!/usr/bin/env python3
"""Writes tests/golden/nufft3d_error_budget.json on the MI355X: per dtype, shape (N1, N2, N3, M, kind), eps and type of
tests/test_gpu_nufft3d.py, the worst over seeds 0-1, both directions and complex and real data of the rel-L2 and of the worst
element / rms against tests/nufft3d_reference.py (the direct sum in long double with exact phases), and beside each the same two
figures of the numpy model of the schedule (the CPU leg: double arithmetic for f64, float32 kernel values, grid and tables for
f32; tests/test_nufft3d_cpu.py: model_entry, over both directions, complex and real data and both seeds).  C_EPS_3D is fixed by
the MODEL; tests/test_nufft3d_cpu.py keeps its gates >= 2 x above the device's figures too; `need_c_eps` is what the device alone
would ask of C_EPS_3D for that, per dtype.

    python tests/golden/make_nufft3d_error_budget.py [out.json]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import phastft_amd as P  # noqa: E402
from tests import nufft3d_reference as R  # noqa: E402
from tests import tolerances as tol  # noqa: E402
from tests.test_gpu_nufft3d import measure  # noqa: E402
from tests.test_nufft3d_cpu import model_entry, nufft3d_gate  # noqa: E402


def main(out):
    entries, need = [], {"f64": 0.0, "f32": 0.0}
    for dt in ("f64", "f32"):
        for shape in R.SHAPES:
            for eps in R.EPS[dt]:
                for t in (1, 2):
                    rel, worst, pl = measure(P, dt, shape, eps, t)
                    m_rel, m_bin = model_entry(shape, dt, eps, t)
                    g_rel, g_bin = nufft3d_gate(dt, pl.grid_len, eps)
                    log_g = pl.grid_len.bit_length() - 1
                    need[dt] = max(need[dt], (2 * rel - tol.rel_gate(dt, log_g)) / eps, (2 * worst - tol.bin_gate(dt, log_g)) / eps)
                    entries.append({"dt": dt, "n1": shape[0], "n2": shape[1], "n3": shape[2], "m": shape[3], "kind": shape[4], "eps": eps, "type": t,
                                    "w": pl.width, "grid": list(pl.grid_shape), "grid_len": pl.grid_len, "rel": rel, "bin": worst,
                                    "model_rel": m_rel, "model_bin": m_bin, "gate_rel": g_rel, "gate_bin": g_bin,
                                    "margin_rel": g_rel / rel if rel else None, "margin_bin": g_bin / worst if worst else None})
                    print(json.dumps(entries[-1]), flush=True)
    doc = {"what": "worst over seeds 0-1, both directions, complex and real data of the rel-L2 and of the worst element / rms vs "
                   "tests/nufft3d_reference.py in long double; model_*: the numpy model of the schedule; need_c_eps: the least "
                   "C_EPS_3D that leaves every device entry a factor 2",
           "device": P.device_info()["name"], "need_c_eps": need, "entries": entries}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
    print("need_c_eps", need)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "nufft3d_error_budget.json"))
