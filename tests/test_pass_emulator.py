"""The FFT pass kernels themselves -- tile_fft_kernel, row_fft_kernel, r2c_last_pass_kernel, c2r_first_pass_kernel, wave_fft_kernel and
quad_fft_kernel -- run ON THE HOST under AddressSanitizer and UndefinedBehaviorSanitizer: no GPU, no HIP runtime.

The other host tests of these passes (tests/test_emulator.py) run emulate_tile_pass, emulate_row_fft, emulate_wave_pass ...: second,
hand-written schedules of the same phase functions.  What makes a kernel a kernel they skip: the barriers, the LDS carve-up against the
launcher's lds_bytes, the table staging, the persistent loop with the next tile's prefetch and its guard, the kernel's own pre-twiddle
branch, readfirstlane's claim of uniformity.  tests/emu/block_shim.hpp runs a workgroup as fibers that meet at __syncthreads() and, wave
by wave, at the cross-lane swaps, wave_barrier and readfirstlane, in ascending and in descending thread order; tests/cpp/pass_emu_test.cpp
#includes the fifteen product units as they stand, launches every pass through the product's own launcher on heap blocks of exactly
the planner's sizes, and requires the bits of the matching emulate_* function on the same arguments -- output, scratch, batch gaps and
all.  It fails unless every instantiation the dispatchers can reach was launched in both orders and unless the kernel-only branches
ran (all but tw_global, which needs the tables of a 2^28-point transform and is reported as not run).

What this cannot see: timing, a race that both serial orders survive, the device's own arithmetic, what the hardware does in a
swap's inactive lanes.

The self-tests turn the checker on itself: one textual change in a copy of a product header, first on the include path of the one
part that is rebuilt, must fail the program for the stated reason."""
import concurrent.futures as cf
import os
import re
import shutil
import subprocess
import sys

import pytest

from tests.emu import PASS_PARTS, build_pass_emulator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "phastft_amd", "csrc")
SANITIZER = ("ERROR: AddressSanitizer", "runtime error:", "LeakSanitizer")
FILTER = {"tile_f64_bc_wide": "10,4,5", "tile_f32_bc_wide": "10,5,5"}  # the one instantiation each of these units holds


def run(program, *args, env_extra=None):
    # the environment as it is, but for settings that would change what the sanitizers report or the wave kernels' stagger
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "UBSAN_OPTIONS", "PHAST_WAVE_STAGGER")}
    env.update(env_extra or {})
    r = subprocess.run([program, *args], capture_output=True, text=True, env=env)
    return r.returncode, r.stdout + r.stderr


def fail_lines(out):
    return [line for line in out.splitlines() if line.startswith("FAIL ")]


@pytest.fixture(scope="module")
def exe():
    return build_pass_emulator()


@pytest.fixture(scope="module")
def results(exe):
    """every part's run, started together: the parts are independent processes of a few seconds each"""
    jobs = {part: (part,) for part in PASS_PARTS[1:]}
    jobs.update({part + " stagger 0": (part,) for part in ("wave_f64", "wave_f32")})
    with cf.ThreadPoolExecutor(min(len(jobs), os.cpu_count() or 4, 16)) as ex:
        futures = {name: ex.submit(run, exe, *args, env_extra={"PHAST_WAVE_STAGGER": "0,0"} if name.endswith(" stagger 0") else None)
                   for name, args in jobs.items()}
        return {name: f.result() for name, f in futures.items()}


def check_green(part, rc, out):
    sys.stdout.write(out)
    failures = fail_lines(out)
    assert not failures, "\n".join(failures[:12])
    for needle in SANITIZER:
        assert needle not in out, out[-4000:]
    assert "block_shim:" not in out, out[-4000:]  # a divergence or uniformity abort of the shim
    assert rc == 0, out[-4000:]
    assert f"{part}: ok (0 failures)" in out
    assert re.search(r"launches [1-9]\d*  workgroups [1-9]\d*  threads [1-9]\d*  barriers \d+  wave operations \d+", out), out[-2000:]
    m = re.search(r"instantiations of \S+ launched: (\d+) \(required: (\d+), each in both orders\)", out)
    assert m and int(m.group(1)) >= int(m.group(2)) >= 1, out[-2000:]


@pytest.mark.parametrize("part", PASS_PARTS[1:])
def test_pass_kernels_of(results, part):
    """every kernel of the unit through its launcher, in both thread orders: LDS and global accesses in bounds, the bits of the
    emulator, gaps untouched, every instantiation reached, the kernel-only branches run"""
    rc, out = results[part]
    check_green(part, rc, out)
    if part.startswith("tile_") and part not in FILTER:
        assert "branch second loop iteration: ran" in out and "branch prefetch guard false: ran" in out
    if part in ("tile_f64_bc", "tile_f32_bc"):
        assert "branch PROG with the table in LDS: ran" in out
    if part.startswith("wave_"):
        assert "branch early-returning waves: ran" in out and "stagger setting 0x308" in out
        rc0, out0 = results[part + " stagger 0"]
        check_green(part, rc0, out0)
        assert "stagger setting 0\n" in out0
    if part.startswith("quad_"):
        assert re.search(r"ran kern in .*launch_quad_inst.* +[1-9]\d* launches", out) and re.search(r"ran kern#1 in .*launch_quad_inst", out)
    assert "branch tw_global: did not run" in out  # said, not faked: DESIGN.md


# ---- the checker turned on itself ----
QUAD_WAVE = "const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform: row bases"
MUTANTS = {
    # name: (header, part, old, new, arguments of the run)
    "two_barrier_middle": ("tile_fft.hpp", "tile_f64_a",
                           "            __syncthreads();\n            Body::template ex_read<E>(sh, tid, r, 0);\n"
                           "            Body::template ex_read<E>(sh, tid, r, 1);\n",
                           "            Body::template ex_read<E>(sh, tid, r, 0);\n            Body::template ex_read<E>(sh, tid, r, 1);\n",
                           ("tile_f64_a", "6,6,3")),
    "plane_seq_third": ("tile_fft.hpp", "tile_f64_a",
                        "            Body::template ex_read<E>(sh, tid, r, 0);\n            __syncthreads();\n"
                        "            Body::template ex_write<E>(sh, tid, r, 1);\n",
                        "            Body::template ex_read<E>(sh, tid, r, 0);\n            Body::template ex_write<E>(sh, tid, r, 1);\n",
                        ("tile_f64_a", "6,6,4")),
    "leading_barrier": ("tile_fft.hpp", "tile_f64_a",
                        "        if constexpr (!Body::PLANE_SEQ) {\n            __syncthreads();\n"
                        "            Body::template ex_write<E>(sh, tid, r, 0);\n",
                        "        if constexpr (!Body::PLANE_SEQ) {\n            Body::template ex_write<E>(sh, tid, r, 0);\n",
                        ("tile_f64_a", "6,6,3")),
    "lds_bytes_short": ("tile_fft.hpp", "tile_f64_bc", "        return exch + tw3 + TWR * sizeof(cx);\n",
                        "        return exch + tw3 + (TWR - 1) * sizeof(cx);\n", ("tile_f64_bc", "6,6,4")),
    "row_top_barrier": ("row_fft.hpp", "small_fft",
                        "        __syncthreads();               // the previous tile's readers are done with the LDS buffer (and the tables are in)\n",
                        "", ("small_fft", "f64")),
    "wave_barrier": ("wave_fft.hpp", "wave_f64",
                     "        Body::xp_park(xp, lane, r);\n        __builtin_amdgcn_fence(__ATOMIC_RELEASE, \"wavefront\");\n"
                     "        __builtin_amdgcn_wave_barrier();\n",
                     "        Body::xp_park(xp, lane, r);\n        __builtin_amdgcn_fence(__ATOMIC_RELEASE, \"wavefront\");\n", ("wave_f64",)),
    "quad_second_barrier": ("quad_fft.hpp", "quad_f64", "        PHAST_STAMP(true);   // 5: exchange written\n        __syncthreads();\n",
                            "        PHAST_STAMP(true);   // 5: exchange written\n", ("quad_f64",)),
    "prefetch_guard": ("tile_fft.hpp", "tile_f64_a", "        if (t < a.tiles_total) {  // next tile's loads go out right behind the stores\n",
                       "        if (true) {  // next tile's loads go out right behind the stores\n", ("tile_f64_a", "6,6,3")),
    "quad_not_uniform": ("quad_fft.hpp", "quad_f64", QUAD_WAVE, QUAD_WAVE.replace("tid >> 6", "tid >> 5"), ("quad_f64",)),
}


@pytest.fixture(scope="module")
def mutants(exe, tmp_path_factory):
    """every mutant built (its one part, at -O0) and run, together: name -> (exit code, output)"""
    dirs = {name: tmp_path_factory.mktemp(name) for name in MUTANTS}

    def one(name):
        header, part, old, new, args = MUTANTS[name]
        text = open(os.path.join(CSRC, header)).read()
        assert text.count(old) == 1, f"{header} no longer has exactly one {old!r}: update this self-test"
        d = dirs[name]
        # a copy of the whole directory: a quoted #include looks beside the including file first, so the unit and every header on
        # the way to the mutated one must come from the copy
        for f in os.listdir(CSRC):
            if f.endswith((".hpp", ".hip", ".inc")):
                shutil.copy(os.path.join(CSRC, f), d / f)
        (d / header).write_text(text.replace(old, new))
        program = build_pass_emulator(override_dir=str(d), parts=(part,), out=str(d / "pass_emu_test"))
        return run(program, *args)

    with cf.ThreadPoolExecutor(min(len(MUTANTS), os.cpu_count() or 4, 16)) as ex:
        return dict(zip(MUTANTS, ex.map(one, MUTANTS)))


def wrong_bits(rc, out, kernel, part):
    """the program failed by comparing bits, in at least one thread order, in this kernel alone, and no sanitizer spoke"""
    assert rc == 1, out[-4000:]
    failures = fail_lines(out)
    assert failures, out[-4000:]
    for line in failures:
        assert kernel in line and ("the kernel gives bits" in line), line
    assert any(" ascending]" in line for line in failures) or any(" descending]" in line for line in failures)
    assert f"{part}: FAILED" in out
    assert not any(needle in out for needle in SANITIZER) and "block_shim:" not in out, out[-4000:]
    return failures


def test_checker_sees_the_missing_barrier_between_write_and_read(mutants):
    """(1) tile_fft_kernel without the barrier between ex_write and ex_read of the two-barrier exchange: a thread reads what another
    has not yet written"""
    wrong_bits(*mutants["two_barrier_middle"], "launch_tile_inst", "tile_f64_a")


def test_checker_sees_the_missing_third_barrier_of_the_plane_sequential_exchange(mutants):
    """(1) ... and, where re and im go through one LDS plane one after the other, without the barrier between the readers of the real
    parts and the writers of the imaginary parts"""
    wrong_bits(*mutants["plane_seq_third"], "launch_tile_inst", "tile_f64_a")


def test_checker_sees_the_missing_leading_barrier_of_an_exchange(mutants):
    """(2) tile_fft_kernel without "previous readers done": the transposing exchange overwrites what exchange 1's readers still want"""
    wrong_bits(*mutants["leading_barrier"], "launch_tile_inst", "tile_f64_a")


def test_checker_sees_an_lds_request_one_entry_short(mutants):
    """(3) TileBody::lds_bytes one complex entry short: the staging of the W_rows table writes past the launch's dynamic LDS, a heap
    block of exactly the bytes asked for"""
    rc, out = mutants["lds_bytes_short"]
    assert rc != 0
    assert "ERROR: AddressSanitizer: heap-buffer-overflow" in out and re.search(r"(WRITE|READ) of size (16|8)", out), out[-4000:]
    assert "tile_fft_kernel" in out, out[-4000:]  # the frame of the report
    assert not fail_lines(out), out[-4000:]


def test_checker_needs_the_shrunken_grid_for_the_row_kernels_loop_barrier(mutants):
    """(4) row_fft_kernel without the barrier at the top of its tile loop: wrong bits.  In the complex and the R2C mode only where a
    workgroup walks several tiles -- the launcher gives every tile of these batches a workgroup of its own, so only the shrunken grid
    can show it.  In the C2R mode the same barrier is also the one behind the staging of the W_2N tables ("and the tables are in"),
    which c2r_park reads at once: there the first tile is already wrong, in any grid."""
    rc, out = mutants["row_top_barrier"]
    failures = wrong_bits(rc, out, "launch_row_inst", "small_fft")
    walked = [line for line in failures if " mode 2 " not in line]
    assert walked, failures[:4]
    for line in walked:
        m = re.search(r"tiles (\d+) grid=(\d+) ", line)
        assert m and int(m.group(2)) < int(m.group(1)), line


def test_checker_sees_the_missing_wave_barrier(mutants):
    """(5) wave_fft_kernel without the wave_barrier between xp_park and xp_pick: a lane picks what the other lanes have not parked"""
    failures = wrong_bits(*mutants["wave_barrier"], "launch_wave_inst", "wave_f64")
    assert all("TRANSPOSE = true" in line for line in failures), failures[:4]  # the pre-twiddle pass has no such buffer


def test_checker_sees_the_missing_second_barrier_of_the_quad_kernel(mutants):
    """(6) quad_fft_kernel without the barrier between the exchange's writes and reads"""
    wrong_bits(*mutants["quad_second_barrier"], "launch_quad_inst", "quad_f64")


def test_checker_sees_a_prefetch_without_its_guard(mutants):
    """(7) the next tile's load_raw issued unconditionally: past the last tile it reads past the caller's plane, the values are never
    used -- only AddressSanitizer can tell"""
    rc, out = mutants["prefetch_guard"]
    assert rc != 0
    assert "ERROR: AddressSanitizer: heap-buffer-overflow" in out and re.search(r"READ of size 8", out), out[-4000:]
    assert "tile_fft_kernel" in out, out[-4000:]
    assert not fail_lines(out), out[-4000:]


def test_checker_sees_a_false_uniformity_claim(mutants):
    """(8) readfirstlane(tid >> 5) in quad_fft_kernel: the device would silently take lane 0's value for the whole wave"""
    rc, out = mutants["quad_not_uniform"]
    assert rc != 0
    assert re.search(r"block_shim: kern.*launch_quad_inst.*workgroup \(0, 0, 0\), wave \d: readfirstlane of a value that is not wave-uniform", out), out[-4000:]
    assert not fail_lines(out), out[-4000:]
