"""The kernels that build the NUFFT planners' point tables on the device (csrc/nufft_sort.hip: keys, histogram, scan, scatter,
tables) run thread by thread ON THE HOST under AddressSanitizer and UndefinedBehaviorSanitizer -- no GPU, no HIP runtime -- and
must give perm, cell_start and xs / ys / zs EQUAL to the host path's (nufft_bin, nufft_nd_bin), bit for bit.

tests/cpp/nufft_sort_emu_test.cpp is a stand-alone program on tests/emu/block_shim.hpp (a workgroup's threads are fibers that
meet at __syncthreads()), built with tests.emu.BLOCK_FLAGS and linked by the toolchain's clang++ without the HIP runtime.  It
drives every kernel through the product's launchers in BOTH thread orders, on heap buffers of exactly the contract's bytes, in one,
two and three dimensions, at M = 1, 2, B - 1, B, B + 1, 3 B + 17 and one M that gives the scan of the counts more than one workgroup
at both levels below its top (B and S are read from csrc/nufft_sort.hpp and the program prints the ones it was built with), on
grids of one, two and three digit passes, on a 1-D grid of 2^20 cells and on a 3-D grid with a different number of bits per axis,
for uniform, clumped, duplicate and edge-case points.  It reports the launches per kernel and fails if one was never reached.

The last three tests turn the checker on itself: one textual change in a copy of nufft_sort.hip, first on the include path, must
fail the program for the stated reason."""
import os
import re
import subprocess
import sys

import pytest

from phastft_amd import build as B
from tests import emu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "nufft_sort_emu_test.cpp")
HIP = os.path.join(B.SRC, "nufft_sort.hip")
SANITIZER = ("ERROR: AddressSanitizer", "runtime error:", "LeakSanitizer")


def build(out_dir, override_dir=None):
    os.makedirs(out_dir, exist_ok=True)
    obj, prog = os.path.join(out_dir, "nufft_sort_emu_test.o"), os.path.join(out_dir, "nufft_sort_emu_test")
    deps = [SRC, emu.BLOCK_SHIM, os.path.join(ROOT, "tests", "cpp", "sanitizer_exit.hpp"), HIP] + B._deps()
    if override_dir or B._stale(prog, deps):
        inc = [*(["-I", override_dir] if override_dir else []), "-I", B.SRC, "-I", B.INCLUDE, "-I", emu.HERE, "-I", os.path.dirname(SRC)]
        r = subprocess.run([B.hipcc(), *emu.BLOCK_FLAGS, *inc, "-c", SRC, "-o", obj], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        r = subprocess.run([emu._host_linker(), "-fsanitize=address,undefined", obj, "-o", prog], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
    return prog


def run(program, *args):
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "UBSAN_OPTIONS")}
    r = subprocess.run([program, *args], capture_output=True, text=True, env=env)
    return r.returncode, r.stdout + r.stderr


def fail_lines(out):
    return [line for line in out.splitlines() if line.startswith("FAIL ")]


def constant(name):
    text = open(os.path.join(B.SRC, "nufft_sort.hpp")).read()
    m = re.search(rf"\b{name} = ([^;,]+)[;,]", text)
    assert m, name
    return m.group(1).strip()


@pytest.fixture(scope="module")
def exe():
    return build(os.path.join(emu.HERE, "build"))


def test_the_sort_kernels_under_the_host_sanitizers(exe):
    """in bounds, every table equal to the host path's in both thread orders, every kernel reached"""
    rc, out = run(exe, "all")
    sys.stdout.write(out)
    failures = fail_lines(out)
    assert not failures, "\n".join(failures[:12])
    for needle in SANITIZER:
        assert needle not in out, out[-4000:]
    assert rc == 0, out[-4000:]
    assert "nufft_sort: ok (0 failures)" in out
    assert re.search(r"launches [1-9]\d* threads [1-9]\d* barriers [1-9]\d* elements [1-9]", out)
    # the program was built with the header's constants
    threads, per, scan, bits = (int(constant(n)) for n in ("kNufftSortThreads", "kNufftSortPerThread", "kNufftSortScan", "kNufftSortBits"))
    assert f"block {threads * per} scan {scan} bits {bits}\n" in out
    m = re.search(r"scan: (\d+) counts, (\d+) and (\d+) partials", out)
    assert m and int(m.group(2)) > scan and int(m.group(3)) > 1, out[-2000:]  # more than one workgroup at both levels below the top
    for kernel in ("key_kernel", "hist_kernel", "scatter_kernel<true>", "scatter_kernel<false>", "reduce_kernel", "scan_kernel",
                   "table_kernel", "cell_kernel"):
        assert re.search(rf"^  ran nufft_sort_{re.escape(kernel)} +[1-9]", out, re.M), (kernel, out[-2000:])


def mutated(tmp_path, old, new):
    """the program with `old` -> `new` in a copy of csrc/nufft_sort.hip that precedes the product's on the include path"""
    text = open(HIP).read()
    assert text.count(old) == 1, f"nufft_sort.hip no longer has exactly one {old!r}: update this self-test"
    (tmp_path / "nufft_sort.hip").write_text(text.replace(old, new))
    return build(str(tmp_path), override_dir=str(tmp_path))


def test_checker_sees_a_ranking_without_its_tie_break(exe, tmp_path):
    """(1) the scatter hands a thread's keys of one digit their slots in DESCENDING order of position: still a sort by cell, so
    cell_start and the set of positions per cell stay right, but equal keys no longer keep the order of their original indices --
    perm differs from the host's counting sort wherever a thread holds two points of one cell (the clumped and duplicate sets)"""
    old = "const unsigned j = k;  // ascending: equal digits keep the order of their positions (the tie-break)"
    rc, out = run(mutated(tmp_path, old, "const unsigned j = kSortP - 1 - k;"), "small")
    assert rc == 1, out[-4000:]
    failures = fail_lines(out)
    assert failures and any(line.startswith("FAIL perm [") for line in failures), out[-4000:]
    assert not any(line.startswith("FAIL cell_start") for line in failures), "\n".join(failures[:12])
    assert any(" set c " in line or " set d " in line for line in failures)
    assert "nufft_sort: FAILED" in out
    assert not any(needle in out for needle in SANITIZER), out[-4000:]


def test_checker_sees_a_missing_barrier_between_count_and_rank(exe, tmp_path):
    """(2) the barrier between the LDS count and the scan that turns the counts into ranks removed: a thread sums columns that
    their owners have not counted yet (they hold the previous workgroup's ranks), so the slots are wrong.  A wrong slot inside
    the arrays is wrong bits in the tables; one outside them is a store that the device would carry out silently and
    AddressSanitizer stops here, in the scatter kernel -- whichever the first workgroup with stale counts meets first"""
    old = "    __syncthreads();  // every column is counted before the scan reads across the columns\n"
    rc, out = run(mutated(tmp_path, old, ""), "small")
    assert rc != 0, out[-4000:]
    failures = fail_lines(out)
    if "ERROR: AddressSanitizer" in out:
        assert re.search(r"#0 .* in void phast::nufft_sort_scatter_kernel<(true|false)>", out), out[-4000:]
        assert re.search(r"The signal is caused by a WRITE|WRITE of size 4", out), out[-4000:]
    else:
        assert failures and "nufft_sort: FAILED" in out, out[-4000:]


def test_checker_sees_a_rounded_position(exe, tmp_path):
    """(3) the position formed by a rounding conversion of the fraction's top word instead of nufft_turns' truncation: the order
    (perm, cell_start) is untouched, the positions differ in the last bit, and -2^-60 becomes 1.0"""
    old = "return nufft_turns(czt_frac(v, 0));"
    rc, out = run(mutated(tmp_path, old, "return (double)czt_frac(v, 0).hi * 0x1p-64;"), "small")
    assert rc == 1, out[-4000:]
    failures = fail_lines(out)
    assert failures and all(re.match(r"FAIL [xyz]s \[", line) for line in failures), "\n".join(failures[:12])
    assert "nufft_sort: FAILED" in out
    assert not any(needle in out for needle in SANITIZER), out[-4000:]
