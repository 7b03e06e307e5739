"""The bank kernel of the continuous wavelet transform and its pad / crop sweep (csrc/cwt.hip), run thread by thread ON THE
HOST under AddressSanitizer and UndefinedBehaviorSanitizer -- no GPU, no HIP runtime.

tests/cpp/cwt_emu_test.cpp is a stand-alone program: it #includes cwt.hip as it stands over tests/emu/block_shim.hpp, drives
the kernels through their launchers with arguments built as the planner builds them -- whole calls and chunks of 1 and 3 rows,
rows in the caller's planes and in workspace rows, real and complex input, every family --, aligned and one element off, on
buffers of exactly the contract's elements, in both fiber orders.  Every element is compared bit for bit with the expression
order cwt.hpp documents.

The last two tests turn the checker on itself: one textual change in a copy of cwt.hip, first on the include path, must fail
the program."""
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
SRC = os.path.join(CPP, "cwt_emu_test.cpp")
HIP = os.path.join(_b.SRC, "cwt.hip")
HPP = os.path.join(_b.SRC, "cwt.hpp")
SANITIZER = ("ERROR: AddressSanitizer", "runtime error:", "LeakSanitizer")


def build_emulator(out: str | None = None, override_dir: str | None = None) -> str:
    """the program, or (override_dir) one whose cwt.hip and cwt.hpp are the copies in that directory"""
    exe = out or os.path.join(EMU, "build", "cwt_emu_test")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    deps = [SRC, BLOCK_SHIM, os.path.join(CPP, "sanitizer_exit.hpp"), os.path.abspath(__file__), HIP] + _b._deps(HIP)
    if override_dir or _b._stale(exe, deps):
        obj = exe + ".o"
        cmd = [_b.hipcc(), *BLOCK_FLAGS, *(["-I", override_dir] if override_dir else []), "-I", _b.SRC, "-I", _b.INCLUDE, "-I", EMU,
               "-I", CPP, "-c", SRC, "-o", obj]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed for the cwt emulator:\n{r.stdout}\n{r.stderr}")
        r = subprocess.run([_host_linker(), "-fsanitize=address,undefined", obj, "-o", exe], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"link failed for the cwt emulator:\n{r.stdout}\n{r.stderr}")
    return exe


def run(program, *args):
    # the environment as it is, but for settings that would change what the sanitizers report
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "UBSAN_OPTIONS")}
    r = subprocess.run([program, *args], capture_output=True, text=True, env=env)
    return r.returncode, r.stdout + r.stderr


def test_the_kernels():
    """in bounds, every named element written and right to the bit, nothing else touched"""
    rc, out = run(build_emulator())
    sys.stdout.write(out[-3000:])
    failures = [line for line in out.splitlines() if line.startswith("FAIL ")]
    assert not failures, "\n".join(failures[:12])
    for needle in SANITIZER:
        assert needle not in out, out[-4000:]
    assert rc == 0, out[-4000:]
    assert "cwt: ok (0 failures)" in out
    assert re.search(r"launches [1-9]\d{2,}", out)  # the kernels ran (no LDS: no barriers)
    m = re.search(r"(\d+) of them mirrored reads, (\d+) zero fills", out)
    assert m and int(m.group(1)) > 1000 and int(m.group(2)) > 1000   # both upper halves were exercised


def mutated(tmp_path, old, new):
    """the program with `old` -> `new` in a copy of cwt.hip; the copies precede the product's files on the include path
    (cwt.hip names cwt.hpp in quotes: its own directory is searched first)"""
    for p in (HIP, HPP):
        shutil.copy(p, tmp_path / os.path.basename(p))
    text = open(HIP).read()
    assert text.count(old) == 1, f"cwt.hip no longer has exactly one {old!r}: update this self-test"
    (tmp_path / "cwt.hip").write_text(text.replace(old, new))
    return build_emulator(out=str(tmp_path / "cwt_emu_test"), override_dir=str(tmp_path))


def test_checker_sees_a_shifted_mirror(tmp_path):
    """(a) the mirrored bin of a real signal taken as P - k - 1: wrong bits in the upper half of DOG rows of real input, and
    nowhere else"""
    rc, out = run(mutated(tmp_path, "const unsigned long long mk = a.p - k;", "const unsigned long long mk = a.p - k - 1;"))
    assert rc != 0, out[-4000:]
    fails = [line for line in out.splitlines() if line.startswith("FAIL ")]
    assert fails and all(re.search(r"family=2 .*real=1 .*bin \d+ = .* must be exactly", line) for line in fails), out[-4000:]
    assert re.search(r"cwt: FAILED \([1-9]\d* failures\)", out), out[-4000:]
    for needle in SANITIZER:
        assert needle not in out, out[-4000:]


def test_checker_sees_a_dropped_zero_fill(tmp_path):
    """(b) the upper half of an analytic family's rows left unwritten: those elements keep the pattern they started with"""
    rc, out = run(mutated(tmp_path, "cwt_zero_rows<T>(a, b, j_lo, j_hi, k0, whole);", ""))
    assert rc != 0, out[-4000:]
    fails = [line for line in out.splitlines() if line.startswith("FAIL ")]
    assert fails and all(re.search(r"family=[013] .*bin \d+ = \(nan, nan\), must be exactly \(0, 0\)", line) for line in fails), out[-4000:]
    for needle in SANITIZER:
        assert needle not in out, out[-4000:]
