"""The four sweeps of the MDCT and its inverse (csrc/mdct.hip), run thread by thread ON THE HOST under AddressSanitizer and
UndefinedBehaviorSanitizer -- no GPU, no HIP runtime.

tests/cpp/mdct_emu_test.cpp is a stand-alone program: it #includes mdct.hip as it stands over tests/emu/sweep_shim.hpp, drives all
four kernels through launch_mdct with arguments built as MdctPlanner builds them, whole and in chunks of one frame (forward) or
one signal (inverse), aligned and one element off, on buffers of exactly the contract's bytes.  Integer data and a window of ones
make the fold, the de-interleave, the unfold and the overlap-add exact: those are compared bit for bit, the twiddled elements
against the same expression on the host.

The last two tests turn the checker on itself: one textual change in a copy of mdct.hip, first on the include path, must fail
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
SRC = os.path.join(CPP, "mdct_emu_test.cpp")
MDCT = os.path.join(_b.SRC, "mdct.hip")
SANITIZER = ("ERROR: AddressSanitizer", "runtime error:", "LeakSanitizer")


def build_emulator(out: str | None = None, override_dir: str | None = None) -> str:
    """the program, or (override_dir) one whose mdct.hip is the copy in that directory"""
    exe = out or os.path.join(EMU, "build", "mdct_emu_test")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    deps = [SRC, SWEEP_SHIM, os.path.join(CPP, "sanitizer_exit.hpp"), os.path.abspath(__file__), MDCT] + _b._deps(MDCT)
    if override_dir or _b._stale(exe, deps):
        obj = exe + ".o"
        cmd = [_b.hipcc(), *SWEEP_FLAGS, *(["-I", override_dir] if override_dir else []), "-I", _b.SRC, "-I", _b.INCLUDE, "-I", EMU,
               "-I", CPP, "-c", SRC, "-o", obj]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed for the mdct emulator:\n{r.stdout}\n{r.stderr}")
        r = subprocess.run([_host_linker(), "-fsanitize=address,undefined", obj, "-o", exe], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"link failed for the mdct emulator:\n{r.stdout}\n{r.stderr}")
    return exe


def run(program, *args):
    # the environment as it is, but for settings that would change what the sanitizers report
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "UBSAN_OPTIONS")}
    r = subprocess.run([program, *args], capture_output=True, text=True, env=env)
    return r.returncode, r.stdout + r.stderr


def test_the_four_sweeps():
    """all kernels: in bounds, aligned as promised, every named element written and right, nothing else touched"""
    rc, out = run(build_emulator())
    sys.stdout.write(out[-3000:])
    failures = [line for line in out.splitlines() if line.startswith("FAIL ")]
    assert not failures, "\n".join(failures[:12])
    for needle in SANITIZER:
        assert needle not in out, out[-4000:]
    assert rc == 0, out[-4000:]
    assert "mdct: ok (0 failures)" in out
    assert re.search(r"launches [1-9]\d{2,}", out)  # kernels ran


def mutated(tmp_path, old, new):
    """the program with `old` -> `new` in a copy of mdct.hip that precedes the product's on the include path"""
    text = open(MDCT).read()
    assert text.count(old) == 1, f"mdct.hip no longer has exactly one {old!r}: update this self-test"
    (tmp_path / "mdct.hip").write_text(text.replace(old, new))
    return build_emulator(out=str(tmp_path / "mdct_emu_test"), override_dir=str(tmp_path))


def test_checker_sees_a_broken_zero_fill(tmp_path):
    """(a) the zero-fill condition at the signal's end starts one sample early: the last sample of a signal is folded as 0"""
    rc, out = run(mutated(tmp_path, "(sa >= 0 && sa < len) ?", "(sa >= 0 && sa < len - 1) ?"))
    assert rc == 1, out[-4000:]
    assert re.search(r"FAIL mdct_pre_kernel<signal> \[.*\]: row \d+ element \d+ \((re|im)\) = .* must be exactly", out), out[-4000:]
    assert "FAIL imdct_ola_kernel" not in out and "FAIL dct4_post_kernel" not in out  # nothing else is blamed
    assert not any(needle in out for needle in SANITIZER), out[-4000:]


def test_checker_sees_a_flipped_unfold_sign(tmp_path):
    """(b) the second half of a frame is added with the wrong sign"""
    rc, out = run(mutated(tmp_path, "acc = sg < 0 ? -y : y;", "acc = sg < 0 ? y : -y;"))
    assert rc == 1, out[-4000:]
    assert re.search(r"FAIL imdct_ola_kernel \[.*\]: sample \d+ of signal \d+ = .* must be exactly", out), out[-4000:]
    assert "FAIL mdct_pre_kernel" not in out and "FAIL dct4_post_kernel" not in out
    assert not any(needle in out for needle in SANITIZER), out[-4000:]
