"""The two-dimensional non-uniform FFT through the C++ mirror (include/phastft.hpp): tests/cpp/nufft2d_host_test.cpp, compiled
with g++ against libphastft_hip.so, does one type 1 (through PlannerNufft2d64/32) and one type 2 (the one-shot form) at
(N1, N2, M) = (7, 5, 40) against the values of tests/nufft2d_reference.py, which it reads from stdin with the gates of
tests/test_nufft2d_cpu.py."""
import os
import subprocess
import sys

import pytest

from tests import nufft2d_reference as R
from tests.test_nufft2d_cpu import nufft2d_gate, reference

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (7, 5, 40, "u")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from phastft_amd import build

    lib = build.LIB if os.path.exists(build.LIB) else build.build()   # the library the package loads
    out = str(tmp_path_factory.mktemp("cpp") / "nufft2d_host_test")
    libdir = os.path.dirname(lib)
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "nufft2d_host_test.cpp"), "-o", out, "-L", libdir, "-lphastft_hip",
           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def test_cpp_mirror_against_the_reference(gpu, exe):
    n1, n2, m, _ = SHAPE
    ref = reference(SHAPE)
    lines = [f"{n1} {n2} {m}"]
    for dt in ("f64", "f32"):
        eps = R.EPS[dt][-1]
        w = R.width(eps)
        lines.append(" ".join(repr(float(v)) for v in (eps, *nufft2d_gate(dt, R.grid(n1, w) * R.grid(n2, w), eps))))
    c, f = ref.inp(1, False, 0), ref.inp(2, False, 0)
    arrays = [ref.x, ref.y, c.real, c.imag, *ref.ref[(1, R.FORWARD, False, 0)], f.real, f.imag, *ref.ref[(2, R.FORWARD, False, 0)]]
    lines += [" ".join(repr(float(v)) for v in a) for a in arrays]
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    sys.stdout.write(r.stdout)
    assert r.returncode == 0 and "nufft2d host: ok (0 failures)" in r.stdout, r.stdout + r.stderr
    assert r.stdout.count(" type ") == 4 and "FAIL" not in r.stdout
