"""tests/cpp/cwt_test.cpp -- the C++ mirror (include/phastft.hpp) of the continuous wavelet transform (PlannerCwt64/32) -- compiled
with g++ against the built library and run: without an argument the argument codes and a good constructor that works or fails
loudly for want of a device, on the GPU the host forms against the definition in long double."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    from phastft_amd import build

    lib = build.build()
    exe = str(tmp_path / "cwt_test")
    libdir = os.path.dirname(lib)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "cwt_test.cpp"), "-o", exe, "-L", libdir, "-lphastft_hip",
                        f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_cpp_mirror_argument_codes(tmp_path):
    r = subprocess.run([_build(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and "cwt: ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_mirror_on_gpu(gpu, tmp_path):
    r = subprocess.run([_build(tmp_path), "gpu"], capture_output=True, text=True)
    sys.stdout.write(r.stdout)
    assert r.returncode == 0 and "cwt: ok" in r.stdout, r.stdout + r.stderr
