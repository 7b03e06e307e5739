"""tests/cpp/dwt_test.cpp -- the C++ mirror (include/phastft.hpp) of the discrete wavelet transform (PlannerDwt64/32) -- compiled with g++ against
the built library and run: without a GPU the argument codes and the loud failure of everything else, on the GPU the host
forms against the definitions in long double."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    from phastft_amd import build

    lib = build.build()
    exe = str(tmp_path / "dwt_test")
    libdir = os.path.dirname(lib)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "dwt_test.cpp"), "-o", exe, "-L", libdir, "-lphastft_hip",
                        f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_cpp_mirror_without_gpu(tmp_path):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present: test_cpp_mirror_on_gpu runs the mirror there")
    r = subprocess.run([_build(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and "dwt: ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_mirror_on_gpu(gpu, tmp_path):
    r = subprocess.run([_build(tmp_path), "gpu"], capture_output=True, text=True)
    sys.stdout.write(r.stdout)
    assert r.returncode == 0 and "dwt: ok" in r.stdout, r.stdout + r.stderr
