"""The four kernels of the two-dimensional non-uniform FFT (csrc/nufft_nd.hip at D = 2) run thread by thread ON THE HOST under
AddressSanitizer and UndefinedBehaviorSanitizer -- no GPU, no HIP runtime: both gathers index through tables (cell_start, perm)
over a w x w neighbourhood that wraps in two directions, which is where a gather goes out of bounds.

tests/cpp/nufft2d_emu_test.cpp is a stand-alone program on tests/emu/block_shim.hpp (the unit also holds the tiled spread of
three dimensions, which meets at __syncthreads()), built with tests.emu.BLOCK_FLAGS and linked by the toolchain's clang++ without
the HIP runtime, exactly as tests/test_nufft3d_emulator.py builds its own.  It drives spread, interpolate, pre and deconvolve
through launch_nufft_nd in BOTH thread orders, ascending and descending, at (N1, N2, M, w) = (1, 1, 1, 2), (2, 3, 5, 3), (7, 5, 40, 16),
(16, 12, 300, 4), (33, 20, 1000, 13), batch 1 and 3, f64 and f32, complex and real input, with caller planes and the workspace
at 16-byte and at element alignment, batch 3 at odd distances and at multiples of the 16-byte group, on buffers of exactly the bytes the contract covers; the points start with the binning
test's specials in x and the reversed specials in y, so the support wraps both ends of both axes.  Every element is compared
with a long double statement of its stage."""
import os
import re
import subprocess
import sys

import pytest

from phastft_amd import build as B
from tests import emu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "nufft2d_emu_test.cpp")
SANITIZER = ("ERROR: AddressSanitizer", "runtime error:", "LeakSanitizer")


@pytest.fixture(scope="module")
def exe():
    out_dir = os.path.join(emu.HERE, "build")
    os.makedirs(out_dir, exist_ok=True)
    obj, prog = os.path.join(out_dir, "nufft2d_emu_test.o"), os.path.join(out_dir, "nufft2d_emu_test")
    deps = [SRC, emu.BLOCK_SHIM, os.path.join(ROOT, "tests", "cpp", "sanitizer_exit.hpp"), os.path.join(B.SRC, "nufft_nd.hip")] + B._deps()
    if B._stale(prog, deps):
        inc = ["-I", B.SRC, "-I", B.INCLUDE, "-I", emu.HERE, "-I", os.path.dirname(SRC)]
        r = subprocess.run([B.hipcc(), *emu.BLOCK_FLAGS, *inc, "-c", SRC, "-o", obj], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        r = subprocess.run([emu._host_linker(), "-fsanitize=address,undefined", obj, "-o", prog], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
    return prog


def test_the_four_kernels_under_the_host_sanitizers(exe):
    """in bounds, aligned as promised, every named element written and right, nothing else touched"""
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "UBSAN_OPTIONS")}
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    out = r.stdout + r.stderr
    sys.stdout.write(out)
    failures = [line for line in out.splitlines() if line.startswith("FAIL ")]
    assert not failures, "\n".join(failures[:12])
    for needle in SANITIZER:
        assert needle not in out, out[-4000:]
    assert r.returncode == 0, out[-4000:]
    assert "nufft2d: ok (0 failures)" in out
    assert re.search(r"launches [1-9]\d* threads [1-9]\d* elements [1-9]", out)  # kernels ran, elements were compared
    for kernel in ("spread", "interp", "pre", "deconv"):
        m = re.search(rf"nufft_nd_{kernel}_kernel +worst error / gate (\S+)", out)
        assert m and 0 < float(m.group(1)) <= 1.0, (kernel, out[-2000:])
