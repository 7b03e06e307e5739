"""NUFFT planners from points in device memory through the C++ mirror (include/phastft.hpp) over the C ABI:
tests/cpp/nufft_dev_points_host_test.cpp, compiled with g++ against libphastft_hip.so and the HIP runtime (it allocates the device
arrays itself), builds a 1-D and a 3-D planner with from_device, re-points them with set_points_dev (a host-built 1-D planner
too), in f64 and f32, and compares every output of a type 1 and a type 2 call for EQUALITY with a planner the host constructor
built at the same points."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from phastft_amd import build

    lib = build.LIB if os.path.exists(build.LIB) else build.build()   # the library the package loads
    out = str(tmp_path_factory.mktemp("cpp") / "nufft_dev_points_host_test")
    libdir = os.path.dirname(lib)
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "nufft_dev_points_host_test.cpp"), "-o", out, "-L", libdir, "-lphastft_hip",
           "-L", "/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def test_cpp_mirror_equals_the_host_built_planner(gpu, exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    sys.stdout.write(r.stdout)
    assert r.returncode == 0 and "nufft dev points host: ok (0 failures, 10 comparisons)" in r.stdout, r.stdout + r.stderr
    assert r.stdout.count(": equal") == 10 and "FAIL" not in r.stdout
