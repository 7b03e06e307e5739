"""The kernels that move data through LDS between barriers -- the transposes of nd.hip, the bit reversals of bitrev.hip, the twiddle
sweep of twiddle.hip and the digest of fill.hip -- run ON THE HOST under AddressSanitizer and UndefinedBehaviorSanitizer: no GPU,
no HIP runtime.

tests/emu/block_shim.hpp runs a workgroup as fibers that meet at __syncthreads(), the threads between two barriers in ascending
or in descending order; static LDS is a global object and dynamic LDS a heap block, so an LDS index past the allocation, silent on
the device, is an AddressSanitizer report.  tests/cpp/block_emu_test.cpp #includes the product files as they stand and drives
every kernel through the product's own launcher, on buffers of exactly the bytes the contract covers, in both orders, and compares
bits with exact index arithmetic (a long double statement for the two kernels that compute).  It also records which kernel
instantiation every launch reached and fails if one of the 24 transposes or of the bit-reversal kernels was never launched.

What this cannot see: cross-lane operations, timing, a race that both serial orders survive, the device's own arithmetic (the
f32 reciprocal of the narrow transposes is checked on the device by tests/test_gpu_nd.py::test_every_narrow_side_matches_numpy).

The last five tests turn the checker on itself: one textual change in a copy of a product file, first on the include path, must
fail the program for the stated reason."""
import os
import re
import subprocess
import sys

import pytest

from tests.emu import BLOCK_PARTS, build_block_emulator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "phastft_amd", "csrc")
SANITIZER = ("ERROR: AddressSanitizer", "runtime error:", "LeakSanitizer")


@pytest.fixture(scope="module")
def exe():
    return build_block_emulator()


def run(program, *args):
    # the environment as it is, but for settings that would change what the sanitizers report
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "UBSAN_OPTIONS")}
    r = subprocess.run([program, *args], capture_output=True, text=True, env=env)
    return r.returncode, r.stdout + r.stderr


def fail_lines(out):
    return [line for line in out.splitlines() if line.startswith("FAIL ")]


@pytest.mark.parametrize("part", BLOCK_PARTS[1:])
def test_block_kernels_of(exe, part):
    """every kernel of the part, in both thread orders: LDS and global accesses in bounds, every named element right to the bit (or
    within the derived gate), gaps and sources untouched, every instantiation reached"""
    rc, out = run(exe, part)
    sys.stdout.write(out)
    failures = fail_lines(out)
    assert not failures, "\n".join(failures[:12])
    for needle in SANITIZER:
        assert needle not in out, out[-4000:]
    assert rc == 0, out[-4000:]
    assert f"{part}: ok (0 failures)" in out
    assert re.search(r"launches [1-9]\d*  workgroups [1-9]\d*  threads [1-9]\d*  barriers [1-9]", out), out[-2000:]  # kernels ran
    if part == "nd":
        assert len(re.findall(r"^  ran nd_transpose_(?:square|narrow)<", out, re.M)) == 24, out[-4000:]


def mutated(tmp_path, name, part, old, new):
    """the program with `old` -> `new` in a copy of csrc/<name> that precedes the product's on the include path"""
    text = open(os.path.join(CSRC, name)).read()
    assert text.count(old) == 1, f"{name} no longer has exactly one {old!r}: update this self-test"
    (tmp_path / name).write_text(text.replace(old, new))
    return build_block_emulator(override_dir=str(tmp_path), parts=(part,), out=str(tmp_path / "block_emu_test"))


def test_checker_sees_a_missing_barrier_in_the_square_transpose(exe, tmp_path):
    """(1) the barrier between the LDS writes and the LDS reads of nd_transpose_square removed: a thread reads what another has not
    yet written, and the bits are wrong in at least one thread order; no sanitizer can tell"""
    old = ("    __syncthreads();\n    for (int p = 0; p < 2; ++p) {\n"
           "        T *dst = reinterpret_cast<T *>(p ? a.dst_im : a.dst_re) + b * a.dst_dist + c0 * a.rows + r0;")
    rc, out = run(mutated(tmp_path, "nd.hip", "nd", old, old.replace("    __syncthreads();\n", "")), "nd", "f64")
    assert rc == 1, out[-4000:]
    failures = fail_lines(out)
    assert failures and all(line.startswith("FAIL nd_transpose_square<double, ") for line in failures), "\n".join(failures[:12])
    assert any("ascending]" in line for line in failures) or any("descending]" in line for line in failures)
    assert "nd: FAILED" in out
    assert not any(needle in out for needle in SANITIZER), out[-4000:]


def test_checker_needs_the_shrunken_grid_for_the_persistent_barrier(exe, tmp_path):
    """(2) the "previous pair's readers are done" barrier of bitrev_persistent_kernel removed: wrong bits, and only where a
    workgroup walks several pairs -- at the sizes a host run can afford that is the shrunken grid alone, which is why it exists"""
    old = ("        U *x = data + (size_t)(w / pe.pairs) * dist;\n        __syncthreads();  // the previous pair's readers are done\n"
           "#pragma unroll\n        for (int i = 0; i < PER; ++i) {\n            const int idx = i * NTH + threadIdx.x;\n"
           "            sa[idx >> BETA]")
    new = old.replace("        __syncthreads();  // the previous pair's readers are done\n", "")
    rc, out = run(mutated(tmp_path, "bitrev.hip", "bitrev", old, new), "bitrev", "persistent1")
    assert rc == 1, out[-4000:]
    failures = fail_lines(out)
    assert failures, out[-4000:]
    for line in failures:
        assert line.startswith("FAIL bitrev_persistent_kernel<") and "[persistent1 grid=3 " in line, line
    assert re.search(r"ran bitrev_persistent_kernel<unsigned long long, 6, 512> +[1-9]", out)  # the launcher's cases ran, and passed
    assert not any(needle in out for needle in SANITIZER), out[-4000:]


def test_checker_sees_a_span_that_overflows_the_lds_image(exe, tmp_path):
    """(3) the span of a vectorised wide side computed as for the element-wise one (E / pitch, without the skew of one element per V
    entries): the LDS image w * pitch + n + w / V runs past the E elements of a plane's half of the LDS array.  This build gives
    UndefinedBehaviorSanitizer's bounds report on the kernel's static LDS array (index 1024 of double[1024], in the first plane:
    AddressSanitizer's redzone would only see the second plane's overflow, the first's lands in the second's half), at S = 1, the
    first narrow side the program runs."""
    old = "unsigned long long span = vw ? E * V / (V * pitch + 1) : E / pitch;"
    rc, out = run(mutated(tmp_path, "nd.hip", "nd", old, "unsigned long long span = E / pitch;"), "nd", "f64")
    assert rc != 0
    assert re.search(r"nd\.hip:\d+:\d+: runtime error: index \d+ out of bounds for type 'double\[1024\]'", out), out[-4000:]
    assert not fail_lines(out), out[-4000:]


def test_checker_sees_a_quotient_without_its_half(exe, tmp_path):
    """(4) fdiv without its + 0.5f: the exhaustive quotient check names the first (x, d)"""
    old = "return (unsigned)(((float)x + 0.5f) * inv);"
    rc, out = run(mutated(tmp_path, "nd.hip", "nd", old, "return (unsigned)((float)x * inv);"), "nd", "fdiv")
    assert rc == 1, out[-4000:]
    assert re.search(r"^FAIL fdiv \[x=\d+ d=\d+\]: fdiv\(x, 1.0f / d\) = \d+, x / d = \d+", out, re.M), out[-4000:]
    assert not any(needle in out for needle in SANITIZER), out[-4000:]


def test_checker_sees_a_flat_read_past_the_plane(exe, tmp_path):
    """(5) the ragged-tail guard of the narrow kernel's 16-byte flat read weakened to its first element: the last group of the last
    tile reads past the caller's plane and the extra value is discarded -- the result stays right (no FAIL line up to the report),
    only AddressSanitizer can tell"""
    old = ("if (f0 + FV <= flat) {\n                    if constexpr (VF) {\n"
           "                        const vt x = *reinterpret_cast<const vt *>(src + f0);")
    rc, out = run(mutated(tmp_path, "nd.hip", "nd", old, old.replace("f0 + FV <= flat", "f0 < flat")), "nd", "f64")
    assert rc != 0
    assert "ERROR: AddressSanitizer: heap-buffer-overflow" in out and re.search(r"READ of size (16|8)", out), out[-4000:]
    assert "nd_transpose_narrow<double, true, " in out, out[-4000:]
    assert not fail_lines(out), out[-4000:]
