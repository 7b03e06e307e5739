"""The kernels of the discrete wavelet transform (csrc/dwt.hip), run thread by thread ON THE HOST under AddressSanitizer and
UndefinedBehaviorSanitizer -- no GPU, no HIP runtime.

tests/cpp/dwt_emu_test.cpp is a stand-alone program: it #includes dwt.hip as it stands over tests/emu/block_shim.hpp (both
kernels stage their run through LDS between barriers, so a workgroup's threads are fibers), drives them level by level through
their launchers with arguments built as the planner builds them, aligned and one element off, whole and in chunks of one
signal, on buffers of exactly the contract's elements, in both fiber orders.  Every coefficient and every reconstructed sample
is compared bit for bit with the documented order of its sum, on data whose sums round, through an extension map of the
program's own.

The last two tests turn the checker on itself: one textual change in a copy of dwt.hpp or dwt.hip, first on the include path,
must fail the program."""
import os
import re
import shutil
import subprocess
import sys

from phastft_amd import build as _b
from tests.emu import BLOCK_FLAGS, BLOCK_SHIM, _host_linker
from tests.emu import HERE as EMU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
SRC = os.path.join(CPP, "dwt_emu_test.cpp")
HIP = os.path.join(_b.SRC, "dwt.hip")
HPP = os.path.join(_b.SRC, "dwt.hpp")
SANITIZER = ("ERROR: AddressSanitizer", "runtime error:", "LeakSanitizer")


def build_emulator(out: str | None = None, override_dir: str | None = None) -> str:
    """the program, or (override_dir) one whose dwt.hip and dwt.hpp are the copies in that directory"""
    exe = out or os.path.join(EMU, "build", "dwt_emu_test")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    deps = [SRC, BLOCK_SHIM, os.path.join(CPP, "sanitizer_exit.hpp"), os.path.abspath(__file__), HIP] + _b._deps(HIP)
    if override_dir or _b._stale(exe, deps):
        obj = exe + ".o"
        cmd = [_b.hipcc(), *BLOCK_FLAGS, *(["-I", override_dir] if override_dir else []), "-I", _b.SRC, "-I", _b.INCLUDE, "-I", EMU,
               "-I", CPP, "-c", SRC, "-o", obj]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed for the dwt emulator:\n{r.stdout}\n{r.stderr}")
        r = subprocess.run([_host_linker(), "-fsanitize=address,undefined", obj, "-o", exe], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"link failed for the dwt emulator:\n{r.stdout}\n{r.stderr}")
    return exe


def run(program, *args):
    # the environment as it is, but for settings that would change what the sanitizers report
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "UBSAN_OPTIONS")}
    r = subprocess.run([program, *args], capture_output=True, text=True, env=env)
    return r.returncode, r.stdout + r.stderr


def test_the_kernels():
    """both kernels: in bounds, every named element written and right to the bit, nothing else touched"""
    rc, out = run(build_emulator())
    sys.stdout.write(out[-3000:])
    failures = [line for line in out.splitlines() if line.startswith("FAIL ")]
    assert not failures, "\n".join(failures[:12])
    for needle in SANITIZER:
        assert needle not in out, out[-4000:]
    assert rc == 0, out[-4000:]
    assert "dwt: ok (0 failures)" in out
    assert re.search(r"launches [1-9]\d{2,}", out) and re.search(r"barriers [1-9]\d{2,}", out)  # kernels ran, through barriers


def mutated(tmp_path, path, old, new):
    """the program with `old` -> `new` in a copy of `path` (dwt.hip or dwt.hpp); the copies precede the product's files on the
    include path (dwt.hip names dwt.hpp in quotes: its own directory is searched first)"""
    for p in (HIP, HPP):
        shutil.copy(p, tmp_path / os.path.basename(p))
    text = open(path).read()
    assert text.count(old) == 1, f"{os.path.basename(path)} no longer has exactly one {old!r}: update this self-test"
    (tmp_path / os.path.basename(path)).write_text(text.replace(old, new))
    return build_emulator(out=str(tmp_path / "dwt_emu_test"), override_dir=str(tmp_path))


def test_checker_sees_a_symmetric_map_off_by_one(tmp_path):
    """(a) the mirrored half of the symmetric extension is 2n - u instead of 2n - 1 - u: the sample behind the signal's end
    (AddressSanitizer on a buffer of exactly L samples) or the wrong neighbour (wrong bits), and only in that mode"""
    rc, out = run(mutated(tmp_path, HPP, "return u < n ? u : 2 * n - 1 - u;", "return u < n ? u : 2 * n - u;"))
    assert rc != 0, out[-4000:]
    assert "ERROR: AddressSanitizer" in out or re.search(r"FAIL analysis \[.* symmetric .*\]: element \d+ of signal \d+ = ", out), out[-4000:]
    assert not re.search(r"FAIL \w+ \[[^\]]* (zero|constant|reflect|periodic|periodization) ", out), out[-4000:]


def test_checker_sees_a_staged_run_one_sample_short(tmp_path):
    """(b) the run of the signal an analysis tile stages ends one sample early: the last coefficient of a tile reads what LDS
    held before -- wrong bits, and only in the analysis kernel"""
    rc, out = run(mutated(tmp_path, HIP, "const unsigned count = 2 * n + f - 2;", "const unsigned count = 2 * n + f - 3;"))
    assert rc != 0, out[-4000:]
    assert re.search(r"FAIL analysis \[.*\]: element \d+ of signal \d+ = .* must be exactly", out), out[-4000:]
    assert "FAIL synthesis" not in out
