"""The streaming sweep kernels of the composite transforms (any_len, any_real, dct, stft, conv, czt, complex_nums, r2c .hip), run
thread by thread ON THE HOST under AddressSanitizer and UndefinedBehaviorSanitizer -- no GPU, no HIP runtime.

tests/emu/sweep_shim.hpp turns a kernel launch into a serial loop; tests/cpp/sweep_emu_test.cpp #includes the product files as
they stand, drives every kernel through the product's own launch_* function with arguments built as the planners build them,
on buffers of exactly the bytes the contract covers, and compares every output element with a long double statement of the
contract.  What the GPU suite cannot see shows here: a load one element past the caller's buffer whose value is then
discarded (ASan), a 16-byte access through a pointer that only promised element alignment (UBSan, or the host's own
alignment fault), a workspace element left unwritten (it keeps its NaN), an element outside the contract written (it loses
its sentinel bits).

The last four tests turn the checker on itself: one textual change in a copy of any_len.hip, first on the include path, must
fail the program for the stated reason."""
import os
import re
import subprocess
import sys

import pytest

from tests.emu import SWEEP_PARTS, build_sweep_emulator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANY_LEN = os.path.join(ROOT, "phastft_amd", "csrc", "any_len.hip")
SANITIZER = ("ERROR: AddressSanitizer", "runtime error:", "LeakSanitizer")


@pytest.fixture(scope="module")
def exe():
    return build_sweep_emulator()


def run(program, part):
    # the environment as it is, but for settings that would change what the sanitizers report
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "UBSAN_OPTIONS")}
    r = subprocess.run([program, part], capture_output=True, text=True, env=env)
    return r.returncode, r.stdout + r.stderr


@pytest.mark.parametrize("part", SWEEP_PARTS[1:])
def test_sweeps_of(exe, part):
    """every kernel of <part>.hip: in bounds, aligned as promised, every named element written and right, nothing else touched"""
    rc, out = run(exe, part)
    sys.stdout.write(out)
    failures = [line for line in out.splitlines() if line.startswith("FAIL ")]
    assert not failures, "\n".join(failures[:12])
    for needle in SANITIZER:
        assert needle not in out, out[-4000:]
    assert rc == 0, out[-4000:]
    assert f"{part}: ok (0 failures)" in out
    assert re.search(r"launches +[1-9]", out)  # kernels ran


def mutated(tmp_path, old, new):
    """the program with `old` -> `new` in a copy of any_len.hip that precedes the product's on the include path"""
    text = open(ANY_LEN).read()
    assert text.count(old) == 1, f"any_len.hip no longer has exactly one {old!r}: update this self-test"
    (tmp_path / "any_len.hip").write_text(text.replace(old, new))
    return build_sweep_emulator(override_dir=str(tmp_path), parts=("any_len",), out=str(tmp_path / "sweep_emu_test"))


def test_checker_sees_a_load_past_the_end(exe, tmp_path):
    """(a) the 16-byte load of the pad sweep guarded by its first element only: one group reads past the caller's plane, and the
    values are discarded -- the result is right, only AddressSanitizer can tell"""
    old = "if (VEC && k0 + L <= a.n) {\n        vr = __builtin_nontemporal_load"
    rc, out = run(mutated(tmp_path, old, old.replace("k0 + L <= a.n", "k0 < a.n")), "any_len")
    assert rc != 0
    assert "ERROR: AddressSanitizer: heap-buffer-overflow" in out and re.search(r"READ of size (16|8)", out), out[-4000:]
    assert "any_pre_kernel" in out, out[-4000:]


def test_checker_sees_a_wrong_sign(exe, tmp_path):
    """(b) the sign of the s term of the post sweep's real part: the numeric gate, naming the kernel and the case"""
    rc, out = run(mutated(tmp_path, "vr[j] = (T)(x * c - y * s);", "vr[j] = (T)(x * c + y * s);"), "any_len")
    assert rc == 1, out[-4000:]
    assert re.search(r"FAIL any_post_kernel\S* \[f\d\d N=\d+ .*\]: re\[\d+\] = .* > gate", out), out[-4000:]
    assert "any_len: FAILED" in out
    assert not any(needle in out for needle in SANITIZER), out[-4000:]
    assert "FAIL any_pre_kernel" not in out and "FAIL any_spectrum_kernel" not in out  # nothing else is blamed


def test_checker_sees_a_missing_zero_fill(exe, tmp_path):
    """(c) the pad sweep's zero fill left uninitialised (an uninitialised local is a NaN pattern in this build): the elements
    between N and M must be exact zeros"""
    rc, out = run(mutated(tmp_path, "T orr = 0, oi = 0;", "T orr, oi;"), "any_len")
    assert rc == 1, out[-4000:]
    assert re.search(r"FAIL any_pre_kernel\S* \[.*\]: workspace\[\d+\] = .*must be exactly 0", out), out[-4000:]
    assert "FAIL any_post_kernel" not in out


def test_checker_sees_a_broken_alignment_promise(exe, tmp_path):
    """(d) the launcher picks the 16-byte variant of the pad sweep whatever `vec` says: the first plane at element alignment
    (`buf[1:]`) is read with a 16-byte access the hardware under test tolerates -- the host does not"""
    rc, out = run(mutated(tmp_path, "if (kind == 0 && vec)", "if (kind == 0)"), "any_len")
    assert rc != 0
    # UBSan does not instrument the non-temporal builtins, so for them this rests on the host compiler emitting an ALIGNED
    # 16-byte move (x86-64: movntdq / movaps), which faults.  Should a compiler start to emit unaligned moves here, this test
    # fails (the program exits 0): then the promise on those accesses is unchecked and needs a check of its own in the shim.
    assert "misaligned address" in out or "ERROR: AddressSanitizer: SEGV" in out, out[-4000:]
    assert "any_pre_kernel<" in out and "true>" in out, out[-4000:]
