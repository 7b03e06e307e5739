"""The fold kernel of the polyphase channelizer (csrc/channelizer.hip), run thread by thread ON THE HOST under AddressSanitizer
and UndefinedBehaviorSanitizer -- no GPU, no HIP runtime.

tests/cpp/channelizer_emu_test.cpp is a stand-alone program: it #includes channelizer.hip as it stands over
tests/emu/block_shim.hpp (the kernel stages the signal through LDS between barriers, so a workgroup's threads are fibers),
drives the kernel through its launcher with arguments built as the planner builds them -- one plane into padded rows, whole
and in chunks, and two planes into dense rows --, aligned and one element off, on buffers of exactly the contract's elements,
in both fiber orders.  The elements are compared bit for bit with the documented order -- acc = fma(h[r0 + j M],
x[m D - r0 - j M], acc), j ascending -- on data whose sums round.

The last two tests turn the checker on itself: one textual change in a copy of channelizer.hip, first on the include path,
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
SRC = os.path.join(CPP, "channelizer_emu_test.cpp")
HIP = os.path.join(_b.SRC, "channelizer.hip")
HPP = os.path.join(_b.SRC, "channelizer.hpp")
SANITIZER = ("ERROR: AddressSanitizer", "runtime error:", "LeakSanitizer")


def build_emulator(out: str | None = None, override_dir: str | None = None) -> str:
    """the program, or (override_dir) one whose channelizer.hip and channelizer.hpp are the copies in that directory"""
    exe = out or os.path.join(EMU, "build", "channelizer_emu_test")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    deps = [SRC, BLOCK_SHIM, os.path.join(CPP, "sanitizer_exit.hpp"), os.path.abspath(__file__), HIP] + _b._deps(HIP)
    if override_dir or _b._stale(exe, deps):
        obj = exe + ".o"
        cmd = [_b.hipcc(), *BLOCK_FLAGS, *(["-I", override_dir] if override_dir else []), "-I", _b.SRC, "-I", _b.INCLUDE, "-I", EMU,
               "-I", CPP, "-c", SRC, "-o", obj]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed for the channelizer emulator:\n{r.stdout}\n{r.stderr}")
        r = subprocess.run([_host_linker(), "-fsanitize=address,undefined", obj, "-o", exe], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"link failed for the channelizer emulator:\n{r.stdout}\n{r.stderr}")
    return exe


def run(program, *args):
    # the environment as it is, but for settings that would change what the sanitizers report
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "UBSAN_OPTIONS")}
    r = subprocess.run([program, *args], capture_output=True, text=True, env=env)
    return r.returncode, r.stdout + r.stderr


def test_the_kernel():
    """in bounds, every named element written and right to the bit, nothing else touched"""
    rc, out = run(build_emulator())
    sys.stdout.write(out[-3000:])
    failures = [line for line in out.splitlines() if line.startswith("FAIL ")]
    assert not failures, "\n".join(failures[:12])
    for needle in SANITIZER:
        assert needle not in out, out[-4000:]
    assert rc == 0, out[-4000:]
    assert "channelizer: ok (0 failures, 0 of them at D mod M = 0)" in out
    assert re.search(r"launches [1-9]\d{2,}", out) and re.search(r"barriers [1-9]\d{2,}", out)  # the kernel ran, through barriers


def mutated(tmp_path, old, new):
    """the program with `old` -> `new` in a copy of channelizer.hip; the copies precede the product's files on the include
    path (channelizer.hip names channelizer.hpp in quotes: its own directory is searched first)"""
    for p in (HIP, HPP):
        shutil.copy(p, tmp_path / os.path.basename(p))
    text = open(HIP).read()
    assert text.count(old) == 1, f"channelizer.hip no longer has exactly one {old!r}: update this self-test"
    (tmp_path / "channelizer.hip").write_text(text.replace(old, new))
    return build_emulator(out=str(tmp_path / "channelizer_emu_test"), override_dir=str(tmp_path))


def test_checker_sees_a_dropped_rotation(tmp_path):
    """(a) the first tap of a column taken as (-p) mod M, without the frame's m D: wrong bits, and only in the shapes whose hop
    is no multiple of M (the program marks them rot=1) -- where D mod M = 0 the rotation is the identity"""
    rc, out = run(mutated(tmp_path, "r0[i] = in ? (af >= p ? af - p : af + m - p) : 0;", "r0[i] = in ? (p ? m - p : 0) : 0;"))
    assert rc != 0, out[-4000:]
    fails = [line for line in out.splitlines() if line.startswith("FAIL ")]
    assert fails and all(re.search(r"rot=1 .*column \d+ = .* must be exactly", line) for line in fails), out[-4000:]
    assert re.search(r"channelizer: FAILED \([1-9]\d* failures, 0 of them at D mod M = 0\)", out), out[-4000:]
    for needle in SANITIZER:
        assert needle not in out, out[-4000:]


def test_checker_sees_a_dropped_zero_fill(tmp_path):
    """(b) the samples outside [0, L) are loaded instead of zero-filled: a read in front of or behind a buffer of exactly L
    samples (AddressSanitizer), or, between the signals of a batch, a neighbour's sample in place of a zero (wrong bits)"""
    rc, out = run(mutated(tmp_path, "sig[e] = s >= 0 && s < (long long)a.len ? x[s] : T(0);", "sig[e] = x[s];"))
    assert rc != 0, out[-4000:]
    assert "ERROR: AddressSanitizer" in out or re.search(r"FAIL chan_fold \[.*\]: plane \d frame \d+ of signal \d+ column \d+ = ", out), out[-4000:]
