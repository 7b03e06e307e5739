"""The three-dimensional non-uniform FFT through the C++ mirror (include/phastft.hpp): tests/cpp/nufft3d_host_test.cpp, compiled
with g++ against libphastft_hip.so, does one type 1 (through PlannerNufft3d64/32) and one type 2 (the one-shot form) at
(N1, N2, N3, M) = (5, 7, 3, 40) against the values of tests/nufft3d_reference.py, which it reads from stdin with the gates of
tests/test_nufft3d_cpu.py."""
import os
import subprocess
import sys

import pytest

from tests import nufft3d_reference as R
from tests.test_nufft3d_cpu import nufft3d_gate, reference

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (5, 7, 3, 40, "u")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from phastft_amd import build

    lib = build.LIB if os.path.exists(build.LIB) else build.build()   # the library the package loads
    out = str(tmp_path_factory.mktemp("cpp") / "nufft3d_host_test")
    libdir = os.path.dirname(lib)
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "nufft3d_host_test.cpp"), "-o", out, "-L", libdir, "-lphastft_hip",
           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def test_cpp_mirror_against_the_reference(gpu, exe):
    n1, n2, n3, m, _ = SHAPE
    ref = reference(SHAPE)
    lines = [f"{n1} {n2} {n3} {m}"]
    for dt in ("f64", "f32"):
        eps = R.EPS[dt][-1]
        w = R.width(eps)
        lines.append(" ".join(repr(float(v)) for v in (eps, *nufft3d_gate(dt, R.grid(n1, w) * R.grid(n2, w) * R.grid(n3, w), eps))))
    c, f = ref.inp(1, False, 0), ref.inp(2, False, 0)
    arrays = [ref.x, ref.y, ref.z, c.real, c.imag, *ref.ref[(1, R.FORWARD, False, 0)], f.real, f.imag, *ref.ref[(2, R.FORWARD, False, 0)]]
    lines += [" ".join(repr(float(v)) for v in a) for a in arrays]
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    sys.stdout.write(r.stdout)
    assert r.returncode == 0 and "nufft3d host: ok (0 failures)" in r.stdout, r.stdout + r.stderr
    assert r.stdout.count(" type ") == 4 and "FAIL" not in r.stdout
