"""The two kernels of the type-3 non-uniform FFT (csrc/nufft_t3.hip) run thread by thread ON THE HOST under AddressSanitizer
and UndefinedBehaviorSanitizer -- no GPU, no HIP runtime: the spread indexes through four tables (cell_start, the sorted
positions, the prephase pairs, perm), which is where a gather goes out of bounds.

tests/cpp/nufft_t3_emu_test.cpp is a stand-alone program on tests/emu/sweep_shim.hpp, built with tests.emu.SWEEP_FLAGS and
linked by the toolchain's clang++ without the HIP runtime.  It drives spread and post through launch_nufft_t3 at
(M, K, w) = (1, 1, 2), (5, 3, 3), (40, 7, 16), (300, 64, 4), (1000, 257, 13), batch 1 and 3, f64 and f32, both directions, complex
and real input, with caller planes and the workspace at 16-byte and at element alignment, on buffers of exactly the bytes the
contract covers, from tables made by the planner's own builders.  Every element is compared with a long double statement of
its stage."""
import os
import re
import subprocess
import sys

import pytest

from phastft_amd import build as B
from tests import emu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "nufft_t3_emu_test.cpp")
SANITIZER = ("ERROR: AddressSanitizer", "runtime error:", "LeakSanitizer")


@pytest.fixture(scope="module")
def exe():
    out_dir = os.path.join(emu.HERE, "build")
    os.makedirs(out_dir, exist_ok=True)
    obj, prog = os.path.join(out_dir, "nufft_t3_emu_test.o"), os.path.join(out_dir, "nufft_t3_emu_test")
    deps = [SRC, emu.SWEEP_SHIM, os.path.join(ROOT, "tests", "cpp", "sanitizer_exit.hpp"), os.path.join(B.SRC, "nufft_t3.hip")] + B._deps()
    if B._stale(prog, deps):
        inc = ["-I", B.SRC, "-I", B.INCLUDE, "-I", emu.HERE, "-I", os.path.dirname(SRC)]
        r = subprocess.run([B.hipcc(), *emu.SWEEP_FLAGS, *inc, "-c", SRC, "-o", obj], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        r = subprocess.run([emu._host_linker(), "-fsanitize=address,undefined", obj, "-o", prog], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
    return prog


def test_the_two_kernels_under_the_host_sanitizers(exe):
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
    assert "nufft_t3: ok (0 failures)" in out
    assert re.search(r"launches [1-9]\d* threads [1-9]\d* elements [1-9]", out)  # kernels ran, elements were compared
    for kernel in ("spread", "post"):
        m = re.search(rf"nufft_t3_{kernel}_kernel +worst error / gate (\S+)", out)
        assert m and 0 < float(m.group(1)) <= 1.0, (kernel, out[-2000:])
