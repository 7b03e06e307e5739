"""The type-3 non-uniform FFT through the C++ mirror (include/phastft.hpp): tests/cpp/nufft_t3_host_test.cpp, compiled with g++
against libphastft_hip.so.  Without a GPU: the mirror compiles, and every argument error of the C ABI arrives as phastft::Panic
with the C ABI's code (the checks come before the device is touched).  With one: a transform through PlannerNufftT3_64/32 and
through the one-shot form at (M, K) = (100, 37), centres offset, against the values of tests/nufft_t3_reference.py, which the
program reads from stdin with the gates of tests/test_nufft_t3_cpu.py."""
import os
import subprocess
import sys

import pytest

from tests import nufft_t3_reference as R
from tests.test_nufft_t3_cpu import nufft_t3_gate, reference, schedule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = (100, 37, 2.0, 8.0, "off")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from phastft_amd import build

    lib = build.LIB if os.path.exists(build.LIB) else build.build()   # the library the package loads
    out = str(tmp_path_factory.mktemp("cpp") / "nufft_t3_host_test")
    libdir = os.path.dirname(lib)
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "nufft_t3_host_test.cpp"), "-o", out, "-L", libdir, "-lphastft_hip",
           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def test_cpp_mirror_argument_errors(exe):
    r = subprocess.run([exe, "args"], capture_output=True, text=True)
    sys.stdout.write(r.stdout)
    assert r.returncode == 0 and "nufft_t3 host: ok (0 failures)" in r.stdout and "FAIL" not in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_mirror_against_the_reference(gpu, exe):
    ref = reference(CASE)
    lines = [f"{CASE[0]} {CASE[1]}"]
    for dt in ("f64", "f32"):
        eps = R.EPS[dt][-1]
        n_g = 2 * schedule(ref.x, ref.s, eps)["nf"]
        lines.append(" ".join(repr(float(v)) for v in (eps, *nufft_t3_gate(dt, n_g, eps, ref.q))))
    c = ref.inp(False, 0)
    arrays = [ref.x, ref.s, c.real, c.imag, *ref.ref[(R.FORWARD, False, 0)]]
    lines += [" ".join(repr(float(v)) for v in a) for a in arrays]
    r = subprocess.run([exe, "values"], input="\n".join(lines) + "\n", capture_output=True, text=True)
    sys.stdout.write(r.stdout)
    assert r.returncode == 0 and "nufft_t3 host: ok (0 failures)" in r.stdout, r.stdout + r.stderr
    assert r.stdout.count(" value ") == 4 and "FAIL" not in r.stdout
