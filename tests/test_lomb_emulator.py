"""The sweeps of the Lomb-Scargle periodogram (csrc/lomb.hip), run thread by thread ON THE HOST under AddressSanitizer and
UndefinedBehaviorSanitizer -- no GPU, no HIP runtime.

tests/cpp/lomb_emu_test.cpp is a stand-alone program: it #includes lomb.hip as it stands over tests/emu/block_shim.hpp (the
slab sweeps reduce through LDS between barriers, so a workgroup's threads are fibers), drives all kernels through launch_lomb
with arguments built as LombPlanner builds them, whole and in chunks of one signal, aligned and one element off, on buffers of
exactly the contract's elements.  Sums that round are compared bit for bit with the same sums in the documented order; exact
data make everything else exact.

The last two tests turn the checker on itself: one textual change in a copy of lomb.hip or lomb.hpp, first on the include
path, must fail the program and blame only the changed sweeps."""
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
SRC = os.path.join(CPP, "lomb_emu_test.cpp")
HIP = os.path.join(_b.SRC, "lomb.hip")
HPP = os.path.join(_b.SRC, "lomb.hpp")
SANITIZER = ("ERROR: AddressSanitizer", "runtime error:", "LeakSanitizer")
KERNELS = ("lomb_partial", "lomb_final", "lomb_strength", "lomb_post")


def build_emulator(out: str | None = None, override_dir: str | None = None) -> str:
    """the program, or (override_dir) one whose lomb.hip and lomb.hpp are the copies in that directory"""
    exe = out or os.path.join(EMU, "build", "lomb_emu_test")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    deps = [SRC, BLOCK_SHIM, os.path.join(CPP, "sanitizer_exit.hpp"), os.path.abspath(__file__), HIP] + _b._deps(HIP)
    if override_dir or _b._stale(exe, deps):
        obj = exe + ".o"
        cmd = [_b.hipcc(), *BLOCK_FLAGS, *(["-I", override_dir] if override_dir else []), "-I", _b.SRC, "-I", _b.INCLUDE, "-I", EMU,
               "-I", CPP, "-c", SRC, "-o", obj]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed for the lomb emulator:\n{r.stdout}\n{r.stderr}")
        r = subprocess.run([_host_linker(), "-fsanitize=address,undefined", obj, "-o", exe], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"link failed for the lomb emulator:\n{r.stdout}\n{r.stderr}")
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
    assert "lomb: ok (0 failures)" in out
    assert re.search(r"launches [1-9]\d{2,}", out) and re.search(r"barriers [1-9]\d{2,}", out)  # kernels ran, through barriers


def mutated(tmp_path, path, old, new):
    """the program with `old` -> `new` in a copy of `path`; copies of lomb.hip and lomb.hpp precede the product's on the
    include path (lomb.hip names lomb.hpp in quotes: its own directory is searched first)"""
    for p in (HIP, HPP):
        shutil.copy(p, tmp_path / os.path.basename(p))
    text = open(path).read()
    assert text.count(old) == 1, f"{os.path.basename(path)} no longer has exactly one {old!r}: update this self-test"
    (tmp_path / os.path.basename(path)).write_text(text.replace(old, new))
    return build_emulator(out=str(tmp_path / "lomb_emu_test"), override_dir=str(tmp_path))


def blamed(out):
    return {k for k in KERNELS if f"FAIL {k} " in out}


def test_checker_sees_a_slab_summed_in_another_order(tmp_path):
    """(a) the tree folds thread t onto thread 2 step - 1 - t instead of t + step: every point is still added, in another
    order -- the partials of both passes change in their last bits, and nothing else does.  (Handing thread t the groups of
    thread 255 - t, t + 1 or 3 t is no such change: the tree adds cosets of 128, 64, ..., which those maps keep.)"""
    rc, out = run(mutated(tmp_path, HIP, "if (t < step) part[t] += part[t + step];", "if (t < step) part[t] += part[2 * step - 1 - t];"))
    assert rc == 1, out[-4000:]
    assert re.search(r"FAIL lomb_partial \[.*\]: partial of signal \d+ slab \d+ = .* must be exactly", out), out[-4000:]
    assert blamed(out) == {"lomb_partial", "lomb_strength"}, blamed(out)  # the two instances of the one slab sweep
    assert not re.search(r"FAIL lomb_strength \[.*\]: strength \d+", out), out[-4000:]  # the strengths themselves are right
    assert not any(needle in out for needle in SANITIZER), out[-4000:]


def test_checker_sees_a_post_sweep_without_the_rotation(tmp_path):
    """(b) YC is taken as Re A1: the rotation by tau is skipped"""
    rc, out = run(mutated(tmp_path, HPP, "const double yc = ar * ct + ai * st;", "const double yc = ar;"))
    assert rc == 1, out[-4000:]
    assert re.search(r"FAIL lomb_post \[.*\]: output \d+ of signal \d+ = .* must be exactly", out), out[-4000:]
    assert blamed(out) == {"lomb_post"}, blamed(out)
    assert not any(needle in out for needle in SANITIZER), out[-4000:]
