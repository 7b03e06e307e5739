"""The kernels of sample-rate conversion (csrc/resample.hip), run thread by thread ON THE HOST under AddressSanitizer and
UndefinedBehaviorSanitizer -- no GPU, no HIP runtime.

tests/cpp/resample_emu_test.cpp is a stand-alone program: it #includes resample.hip as it stands over tests/emu/block_shim.hpp
(the polyphase kernel stages taps and samples through LDS between barriers, so a workgroup's threads are fibers), drives both
kernels through their launchers with arguments built as the planners build them, aligned and one element off, whole and in
chunks of one signal, on buffers of exactly the contract's elements, in both fiber orders.  The polyphase outputs are compared
bit for bit with the documented order -- acc = fma(row[j], x[q - j], acc), j ascending -- on data whose sums round.

The last two tests turn the checker on itself: one textual change in a copy of resample.hip, first on the include path, must
fail the program."""
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
SRC = os.path.join(CPP, "resample_emu_test.cpp")
HIP = os.path.join(_b.SRC, "resample.hip")
HPP = os.path.join(_b.SRC, "resample.hpp")
SANITIZER = ("ERROR: AddressSanitizer", "runtime error:", "LeakSanitizer")


def build_emulator(out: str | None = None, override_dir: str | None = None) -> str:
    """the program, or (override_dir) one whose resample.hip and resample.hpp are the copies in that directory"""
    exe = out or os.path.join(EMU, "build", "resample_emu_test")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    deps = [SRC, BLOCK_SHIM, os.path.join(CPP, "sanitizer_exit.hpp"), os.path.abspath(__file__), HIP] + _b._deps(HIP)
    if override_dir or _b._stale(exe, deps):
        obj = exe + ".o"
        cmd = [_b.hipcc(), *BLOCK_FLAGS, *(["-I", override_dir] if override_dir else []), "-I", _b.SRC, "-I", _b.INCLUDE, "-I", EMU,
               "-I", CPP, "-c", SRC, "-o", obj]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed for the resample emulator:\n{r.stdout}\n{r.stderr}")
        r = subprocess.run([_host_linker(), "-fsanitize=address,undefined", obj, "-o", exe], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"link failed for the resample emulator:\n{r.stdout}\n{r.stderr}")
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
    assert "resample: ok (0 failures)" in out
    assert re.search(r"launches [1-9]\d{2,}", out) and re.search(r"barriers [1-9]\d{2,}", out)  # kernels ran, through barriers


def mutated(tmp_path, old, new):
    """the program with `old` -> `new` in a copy of resample.hip; the copies precede the product's files on the include path
    (resample.hip names resample.hpp in quotes: its own directory is searched first)"""
    for p in (HIP, HPP):
        shutil.copy(p, tmp_path / os.path.basename(p))
    text = open(HIP).read()
    assert text.count(old) == 1, f"resample.hip no longer has exactly one {old!r}: update this self-test"
    (tmp_path / "resample.hip").write_text(text.replace(old, new))
    return build_emulator(out=str(tmp_path / "resample_emu_test"), override_dir=str(tmp_path))


def test_checker_sees_a_run_of_the_signal_one_sample_short(tmp_path):
    """(a) the run of the signal a tile stages ends one sample early: the outputs that meet the last sample read what LDS held
    before -- wrong bits, and only in the polyphase kernel"""
    rc, out = run(mutated(tmp_path, "const unsigned span = (p0 + (n - 1) * down) / up + g.jc;", "const unsigned span = (p0 + (n - 1) * down) / up + g.jc - 1;"))
    assert rc != 0, out[-4000:]
    assert re.search(r"FAIL upfirdn \[.*\]: output \d+ of signal \d+ = .* must be exactly", out), out[-4000:]
    assert "FAIL resample_spectrum" not in out


def test_checker_sees_a_dropped_zero_fill(tmp_path):
    """(b) the samples outside [0, L) are loaded instead of zero-filled: a read in front of or behind a buffer of exactly L
    samples (AddressSanitizer), or, between the signals of a batch, a neighbour's sample in place of a zero (wrong bits)"""
    rc, out = run(mutated(tmp_path, "sig[u] = s >= 0 && s < (long long)a.len ? x[s] : T(0);", "sig[u] = x[s];"))
    assert rc != 0, out[-4000:]
    assert "ERROR: AddressSanitizer" in out or re.search(r"FAIL upfirdn \[.*\]: output \d+ of signal \d+ = ", out), out[-4000:]
