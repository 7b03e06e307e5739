"""The tile and save sweeps of N-d overlap-save convolution (csrc/convnd.hip), run thread by thread ON THE HOST under
AddressSanitizer and UndefinedBehaviorSanitizer -- no GPU, no HIP runtime.

tests/cpp/convnd_emu_test.cpp is a stand-alone program: it #includes convnd.hip as it stands over tests/emu/sweep_shim.hpp, drives
both kernels through launch_convnd with arguments built as ConvNdPlanner::dev builds them, whole and in chunks of 1 and 2 tiles,
aligned and one element off, on buffers of exactly the contract's bytes, and compares every workspace element and every output
sample bit for bit with the definition (integer data: every sum is exact).

The last two tests turn the checker on itself: one textual change in a copy of convnd.hip, first on the include path, must fail
the program."""
import os
import re
import subprocess
import sys

import pytest

from phastft_amd import build as _b
from tests.emu import HERE as EMU, SWEEP_FLAGS, SWEEP_SHIM, _host_linker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
SRC = os.path.join(CPP, "convnd_emu_test.cpp")
CONVND = os.path.join(_b.SRC, "convnd.hip")
SANITIZER = ("ERROR: AddressSanitizer", "runtime error:", "LeakSanitizer")


def build_emulator(out: str | None = None, override_dir: str | None = None) -> str:
    """the program, or (override_dir) one whose convnd.hip is the copy in that directory"""
    exe = out or os.path.join(EMU, "build", "convnd_emu_test")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    deps = [SRC, SWEEP_SHIM, os.path.join(CPP, "sanitizer_exit.hpp"), os.path.abspath(__file__), CONVND] + _b._deps(CONVND)
    if override_dir or _b._stale(exe, deps):
        obj = exe + ".o"
        cmd = [_b.hipcc(), *SWEEP_FLAGS, *(["-I", override_dir] if override_dir else []), "-I", _b.SRC, "-I", _b.INCLUDE, "-I", EMU,
               "-I", CPP, "-c", SRC, "-o", obj]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed for the convnd emulator:\n{r.stdout}\n{r.stderr}")
        r = subprocess.run([_host_linker(), "-fsanitize=address,undefined", obj, "-o", exe], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"link failed for the convnd emulator:\n{r.stdout}\n{r.stderr}")
    return exe


def run(program, *args):
    # the environment as it is, but for settings that would change what the sanitizers report
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "UBSAN_OPTIONS")}
    r = subprocess.run([program, *args], capture_output=True, text=True, env=env)
    return r.returncode, r.stdout + r.stderr


def test_tile_and_save_sweeps():
    """both kernels: in bounds, aligned as promised, every named element written and right to the bit, nothing else touched"""
    rc, out = run(build_emulator())
    sys.stdout.write(out[-3000:])
    failures = [line for line in out.splitlines() if line.startswith("FAIL ")]
    assert not failures, "\n".join(failures[:12])
    for needle in SANITIZER:
        assert needle not in out, out[-4000:]
    assert rc == 0, out[-4000:]
    assert "convnd: ok (0 failures)" in out
    assert re.search(r"launches [1-9]\d{2,}", out)  # kernels ran


def mutated(tmp_path, old, new):
    """the program with `old` -> `new` in a copy of convnd.hip that precedes the product's on the include path"""
    text = open(CONVND).read()
    assert text.count(old) == 1, f"convnd.hip no longer has exactly one {old!r}: update this self-test"
    (tmp_path / "convnd.hip").write_text(text.replace(old, new))
    return build_emulator(out=str(tmp_path / "convnd_emu_test"), override_dir=str(tmp_path))


def test_checker_sees_a_broken_zero_fill(tmp_path):
    """(a) the element path's zero-fill condition forgets the tile's end: the padding between prod B and fd is filled from the
    array wherever the rows behind the tile's last lie inside it"""
    rc, out = run(mutated(tmp_path, "const bool inside = f0 + e < a.pts && c0 >= 0", "const bool inside = c0 >= 0"), "quick")
    assert rc == 1, out[-4000:]
    assert re.search(r"FAIL convnd_tile_kernel \[.*\]: tile \d+ element \d+ = .* must be exactly 0\n", out), out[-4000:]
    assert "FAIL convnd_save_kernel" not in out  # nothing else is blamed: the padding is never saved
    assert not any(needle in out for needle in SANITIZER), out[-4000:]


def test_checker_sees_a_broken_straddle_path(tmp_path):
    """(b) a group that straddles two tile rows (B_last no multiple of the group) does not carry into the next row"""
    rc, out = run(mutated(tmp_path, "if (++j2 == a.b[2]) {  // the next tile row", "if (++j2 == a.b[2] + 1) {"), "quick")
    assert rc == 1, out[-4000:]
    assert re.search(r"FAIL convnd_tile_kernel \[.* B=\d+,\d+,(17|7) .*\]: tile \d+ element \d+ = .* must be exactly", out), out[-4000:]
    assert not any(needle in out for needle in SANITIZER), out[-4000:]
