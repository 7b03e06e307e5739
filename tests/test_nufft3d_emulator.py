"""The four kernels of the three-dimensional non-uniform FFT (csrc/nufft_nd.hip at D = 3) run thread by thread ON THE HOST under
AddressSanitizer and UndefinedBehaviorSanitizer -- no GPU, no HIP runtime.  The spread kernel is tiled: a workgroup stages the
points round its tile through LDS between barriers, walks cell runs that wrap on every axis and meets whole-ring neighbourhoods
on the short axes, which is where a staged gather goes out of bounds or loses a barrier.

tests/cpp/nufft3d_emu_test.cpp is a stand-alone program on tests/emu/block_shim.hpp (a workgroup's threads are fibers that meet
at __syncthreads()), built with tests.emu.BLOCK_FLAGS and linked by the toolchain's clang++ without the HIP runtime.  It drives
spread, interpolate, pre and deconvolve through launch_nufft_nd in BOTH thread orders, ascending and descending, at
(N1, N2, N3, M, w) = (1, 1, 1, 1, 2), (2, 3, 4, 5, 3), (5, 7, 3, 40, 16), (12, 10, 9, 300, 4), (33, 20, 7, 1000, 13) and at a
clump of exactly kNufft3dChunk points in one cell and of one point more (the constant is read from csrc/nufft_nd.hpp and the
program prints the one it was built with), batch 1 and 3, f64 and f32, complex and real input, with caller planes and the
workspace at 16-byte and at element alignment, on buffers of exactly the bytes the contract covers.  Every element is compared
with a long double statement of its stage.  This is the only sanitizer run of these kernels."""
import os
import re
import subprocess
import sys

import pytest

from phastft_amd import build as B
from tests import emu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "nufft3d_emu_test.cpp")
SANITIZER = ("ERROR: AddressSanitizer", "runtime error:", "LeakSanitizer")


@pytest.fixture(scope="module")
def exe():
    out_dir = os.path.join(emu.HERE, "build")
    os.makedirs(out_dir, exist_ok=True)
    obj, prog = os.path.join(out_dir, "nufft3d_emu_test.o"), os.path.join(out_dir, "nufft3d_emu_test")
    deps = [SRC, emu.BLOCK_SHIM, os.path.join(ROOT, "tests", "cpp", "sanitizer_exit.hpp"), os.path.join(B.SRC, "nufft_nd.hip")] + B._deps()
    if B._stale(prog, deps):
        inc = ["-I", B.SRC, "-I", B.INCLUDE, "-I", emu.HERE, "-I", os.path.dirname(SRC)]
        r = subprocess.run([B.hipcc(), *emu.BLOCK_FLAGS, *inc, "-c", SRC, "-o", obj], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        r = subprocess.run([emu._host_linker(), "-fsanitize=address,undefined", obj, "-o", prog], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
    return prog


def test_the_four_kernels_under_the_host_sanitizers(exe):
    """in bounds, aligned as promised, every named element written and right in both thread orders, nothing else touched; f64
    and f32 run side by side as two processes"""
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "UBSAN_OPTIONS")}
    runs = [(dt, subprocess.Popen([exe, dt], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)) for dt in ("f64", "f32")]
    chunk = int(re.search(r"constexpr unsigned kNufft3dChunk = (\d+);", open(os.path.join(B.SRC, "nufft_nd.hpp")).read()).group(1))
    for dt, proc in runs:
        out = proc.communicate()[0]
        sys.stdout.write(out)
        failures = [line for line in out.splitlines() if line.startswith("FAIL ")]
        assert not failures, "\n".join(failures[:12])
        for needle in SANITIZER:
            assert needle not in out, out[-4000:]
        assert proc.returncode == 0, out[-4000:]
        assert "nufft3d: ok (0 failures)" in out
        assert re.search(r"launches [1-9]\d* threads [1-9]\d* barriers [1-9]\d* elements [1-9]", out)  # kernels ran, elements were compared
        assert f"chunk {chunk} " in out   # the program was built with the header's constant
        for m in (chunk, chunk + 1):      # one full pass through LDS, and a full pass followed by a pass of one point
            assert f"clump: {m} points in one cell" in out
        for kernel in ("spread", "interp", "pre", "deconv"):
            m = re.search(rf"nufft_nd_{kernel}_kernel +worst error / gate (\S+)", out)
            assert m and 0 < float(m.group(1)) <= 1.0, (dt, kernel, out[-2000:])
