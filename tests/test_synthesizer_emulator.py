"""The unfold kernel of the polyphase synthesis bank (csrc/synthesizer.hip), run thread by thread ON THE HOST under
AddressSanitizer and UndefinedBehaviorSanitizer -- no GPU, no HIP runtime.

tests/cpp/synthesizer_emu_test.cpp is a stand-alone program: it #includes synthesizer.hip as it stands over
tests/emu/block_shim.hpp, drives the kernels through their launchers with arguments built as the planner builds them -- one
plane and two planes of padded rows, and the dense rows of one channel --, aligned and one element off, on buffers of exactly
the contract's elements, in both fiber orders.  The samples are compared bit for bit with the documented order -- acc =
fma(tab[n - m D], v[m][n mod M], acc), m ascending -- on data whose sums round.

The last two tests turn the checker on itself: one textual change in a copy of synthesizer.hip, first on the include path,
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
SRC = os.path.join(CPP, "synthesizer_emu_test.cpp")
HIP = os.path.join(_b.SRC, "synthesizer.hip")
HPP = os.path.join(_b.SRC, "synthesizer.hpp")
SANITIZER = ("ERROR: AddressSanitizer", "runtime error:", "LeakSanitizer")


def build_emulator(out: str | None = None, override_dir: str | None = None) -> str:
    """the program, or (override_dir) one whose synthesizer.hip and synthesizer.hpp are the copies in that directory"""
    exe = out or os.path.join(EMU, "build", "synthesizer_emu_test")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    deps = [SRC, BLOCK_SHIM, os.path.join(CPP, "sanitizer_exit.hpp"), os.path.abspath(__file__), HIP] + _b._deps(HIP)
    if override_dir or _b._stale(exe, deps):
        obj = exe + ".o"
        cmd = [_b.hipcc(), *BLOCK_FLAGS, *(["-I", override_dir] if override_dir else []), "-I", _b.SRC, "-I", _b.INCLUDE, "-I", EMU,
               "-I", CPP, "-c", SRC, "-o", obj]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed for the synthesizer emulator:\n{r.stdout}\n{r.stderr}")
        r = subprocess.run([_host_linker(), "-fsanitize=address,undefined", obj, "-o", exe], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"link failed for the synthesizer emulator:\n{r.stdout}\n{r.stderr}")
    return exe


def run(program, *args):
    # the environment as it is, but for settings that would change what the sanitizers report
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "UBSAN_OPTIONS")}
    r = subprocess.run([program, *args], capture_output=True, text=True, env=env)
    return r.returncode, r.stdout + r.stderr


def test_the_kernel():
    """in bounds, every named sample written and right to the bit, nothing else touched"""
    rc, out = run(build_emulator())
    sys.stdout.write(out[-3000:])
    failures = [line for line in out.splitlines() if line.startswith("FAIL ")]
    assert not failures, "\n".join(failures[:12])
    for needle in SANITIZER:
        assert needle not in out, out[-4000:]
    assert rc == 0, out[-4000:]
    assert "synthesizer: ok (0 failures, 0 of them at D mod M = 0)" in out
    assert re.search(r"launches [1-9]\d{2,}", out)  # the kernels ran (no LDS: no barriers)


def mutated(tmp_path, old, new):
    """the program with `old` -> `new` in a copy of synthesizer.hip; the copies precede the product's files on the include
    path (synthesizer.hip names synthesizer.hpp in quotes: its own directory is searched first)"""
    for p in (HIP, HPP):
        shutil.copy(p, tmp_path / os.path.basename(p))
    text = open(HIP).read()
    assert text.count(old) == 1, f"synthesizer.hip no longer has exactly one {old!r}: update this self-test"
    (tmp_path / "synthesizer.hip").write_text(text.replace(old, new))
    return build_emulator(out=str(tmp_path / "synthesizer_emu_test"), override_dir=str(tmp_path))


def test_checker_sees_a_rotated_column(tmp_path):
    """(a) the column taken as (n - m D) mod M, from the tap's index, in place of n mod M: wrong bits, and only in the shapes
    whose hop is no multiple of M (the program marks them rot=1) -- where D mod M = 0 the two are the same column"""
    rc, out = run(mutated(tmp_path, "(unsigned long long)m_lo * a.ld + col : 0;", "(unsigned long long)m_lo * a.ld + jt[i] % m : 0;"))
    assert rc != 0, out[-4000:]
    fails = [line for line in out.splitlines() if line.startswith("FAIL ")]
    assert fails and all(re.search(r"rot=1 .*sample \d+ of signal \d+ = .* must be exactly", line) for line in fails), out[-4000:]
    assert re.search(r"synthesizer: FAILED \([1-9]\d* failures, 0 of them at D mod M = 0\)", out), out[-4000:]
    for needle in SANITIZER:
        assert needle not in out, out[-4000:]


def test_checker_sees_a_dropped_clamp(tmp_path):
    """(b) m_hi without its clamp to F - 1: the samples behind the last frame's start read rows that do not exist -- behind a
    buffer of exactly F rows (AddressSanitizer), or, between the signals of a batch, a neighbour's row (wrong bits)"""
    rc, out = run(mutated(tmp_path, "if (m_hi > (long long)a.f - 1) m_hi = (long long)a.f - 1;", ""))
    assert rc != 0, out[-4000:]
    assert "ERROR: AddressSanitizer" in out or re.search(r"FAIL synth_unfold \[.*\]: plane \d sample \d+ of signal \d+ = ", out), out[-4000:]
