"""The sweeps of Welch spectral estimation (csrc/psd.hip), run thread by thread ON THE HOST under AddressSanitizer and
UndefinedBehaviorSanitizer -- no GPU, no HIP runtime.

tests/cpp/psd_emu_test.cpp is a stand-alone program: it #includes psd.hip as it stands over tests/emu/block_shim.hpp (the mean
sweep reduces through LDS between barriers, so a workgroup's threads are fibers), drives all kernels through launch_psd with
arguments built as PsdPlanner builds them, whole and in chunks of one frame, aligned and one element off, on buffers of exactly
the contract's elements.  Integer data and a window of ones make every value exact: everything is compared bit for bit.

The last two tests turn the checker on itself: one textual change in a copy of psd.hip, first on the include path, must fail
the program and blame only the changed kernel."""
import os
import re
import subprocess
import sys

from phastft_amd import build as _b
from tests.emu import BLOCK_FLAGS, BLOCK_SHIM, _host_linker
from tests.emu import HERE as EMU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
SRC = os.path.join(CPP, "psd_emu_test.cpp")
PSD = os.path.join(_b.SRC, "psd.hip")
SANITIZER = ("ERROR: AddressSanitizer", "runtime error:", "LeakSanitizer")
KERNELS = ("psd_mean_kernel", "psd_frame_kernel", "psd_accum_kernel", "psd_final_kernel", "psd_point_kernel")


def build_emulator(out: str | None = None, override_dir: str | None = None) -> str:
    """the program, or (override_dir) one whose psd.hip is the copy in that directory"""
    exe = out or os.path.join(EMU, "build", "psd_emu_test")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    deps = [SRC, BLOCK_SHIM, os.path.join(CPP, "sanitizer_exit.hpp"), os.path.abspath(__file__), PSD] + _b._deps(PSD)
    if override_dir or _b._stale(exe, deps):
        obj = exe + ".o"
        cmd = [_b.hipcc(), *BLOCK_FLAGS, *(["-I", override_dir] if override_dir else []), "-I", _b.SRC, "-I", _b.INCLUDE, "-I", EMU,
               "-I", CPP, "-c", SRC, "-o", obj]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed for the psd emulator:\n{r.stdout}\n{r.stderr}")
        r = subprocess.run([_host_linker(), "-fsanitize=address,undefined", obj, "-o", exe], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"link failed for the psd emulator:\n{r.stdout}\n{r.stderr}")
    return exe


def run(program, *args):
    # the environment as it is, but for settings that would change what the sanitizers report
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "UBSAN_OPTIONS")}
    r = subprocess.run([program, *args], capture_output=True, text=True, env=env)
    return r.returncode, r.stdout + r.stderr


def test_the_sweeps():
    """all kernels: in bounds, aligned as promised, every named element written and right, nothing else touched"""
    rc, out = run(build_emulator())
    sys.stdout.write(out[-3000:])
    failures = [line for line in out.splitlines() if line.startswith("FAIL ")]
    assert not failures, "\n".join(failures[:12])
    for needle in SANITIZER:
        assert needle not in out, out[-4000:]
    assert rc == 0, out[-4000:]
    assert "psd: ok (0 failures)" in out
    assert re.search(r"launches [1-9]\d{3,}", out) and re.search(r"barriers [1-9]\d{2,}", out)  # kernels ran, through barriers


def mutated(tmp_path, old, new):
    """the program with `old` -> `new` in a copy of psd.hip that precedes the product's on the include path"""
    text = open(PSD).read()
    assert text.count(old) == 1, f"psd.hip no longer has exactly one {old!r}: update this self-test"
    (tmp_path / "psd.hip").write_text(text.replace(old, new))
    return build_emulator(out=str(tmp_path / "psd_emu_test"), override_dir=str(tmp_path))


def blamed(out):
    return {k for k in KERNELS if f"FAIL {k}" in out}


def test_checker_sees_a_zero_fill_that_starts_early(tmp_path):
    """(a) the frame sweep's zero fill starts at P - 1: the last sample of a segment is written as 0"""
    rc, out = run(mutated(tmp_path, "v[j] = j0 + j < a.p ?", "v[j] = j0 + j < a.p - 1 ?"))
    assert rc == 1, out[-4000:]
    assert re.search(r"FAIL psd_frame_kernel \[.*\]: row \d+ element \d+ = .* must be exactly", out), out[-4000:]
    assert blamed(out) == {"psd_frame_kernel"}, blamed(out)  # nothing else is blamed
    assert not any(needle in out for needle in SANITIZER), out[-4000:]


def test_checker_sees_a_dropped_frame(tmp_path):
    """(b) the accumulate sweep drops the last frame of a slab"""
    rc, out = run(mutated(tmp_path, "for (unsigned long long f = lo; f < hi; ++f) {", "for (unsigned long long f = lo; f + 1 < hi; ++f) {"))
    assert rc == 1, out[-4000:]
    assert re.search(r"FAIL psd_accum_kernel \[.*\]: partial row of signal \d+ plane \d slab \d+ bin \d+ = .* must be exactly", out), out[-4000:]
    assert blamed(out) == {"psd_accum_kernel"}, blamed(out)
    assert not any(needle in out for needle in SANITIZER), out[-4000:]
