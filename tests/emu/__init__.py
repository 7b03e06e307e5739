"""CPU emulator of the tile kernels (TEST INFRASTRUCTURE: never imported by the product package).

`emu.hip` includes the product's kernel headers (phastft_amd/csrc/tile_fft.hpp, row_fft.hpp, plan.hpp) and runs
their `__host__ __device__` phase functions thread by thread on the host, so index arithmetic, LDS layouts,
twiddle tables and plans are checked against the oracle in the GPU-less build container (tests/test_emulator.py).

`sweep_shim.hpp` does the same for the streaming sweep kernels around the engine, whose bodies are plain `__global__`
functions: it turns a launch into a serial host loop, and `build_sweep_emulator` builds tests/cpp/sweep_emu_test.cpp on it as
a stand-alone program under ASan and UBSan, linked without the HIP runtime (tests/test_sweep_emulator.py).

`block_shim.hpp` is the third emulator, for the kernels that move data through LDS between barriers (nd.hip's transposes, bitrev.hip,
twiddle.hip, the digest of fill.hip): a workgroup's threads are fibers that run, in ascending or in descending order, from one
__syncthreads() to the next; static LDS is a global object and dynamic LDS a heap block, both bounds-checked by ASan.
`build_block_emulator` builds tests/cpp/block_emu_test.cpp on it (tests/test_block_emulator.py).  It checks LDS and global indices,
barriers (a missing one gives wrong bits in one of the two orders) and which kernel instantiation a shape reaches; it cannot check
timing, races that both serial orders survive, or the device's own arithmetic.

The same shim has lanes and waves: a wave-level operation (v_permlane32/16_swap, wave_barrier, readfirstlane, which aborts on a value
that is not wave-uniform) is a second rendezvous of the 64 lanes of a wave.  `build_pass_emulator` builds tests/cpp/pass_emu_test.cpp
on it (tests/test_pass_emulator.py): the six FFT pass kernels (tile, row, fused R2C / C2R, wave, four-wave) as they stand, launched
through the product's launchers on heap blocks of the planner's sizes, bit for bit against the emulate_* functions in both thread
orders.  One run launches 432 / 504 / 480 / 560 tile passes (f64 A, f64 B/C, f32 A, f32 B/C: 36 / 36 / 40 / 40 instantiations), 336 / 504
fused R2C (24 / 36), 420 / 480 fused C2R (35 / 40), 748 small transforms (52 row kernels, 2 one-point), 17 wave (2) and 14 four-wave (2)
passes per type.  It checks barriers, the LDS carve-up against lds_bytes, table staging, the persistent loop and its prefetch guard, the
kernels' own pre-twiddle branch and the uniformity claims; of the optional branches tw_global (tables of a 2^28-point transform) did
NOT run.  It cannot check timing, races that both serial orders survive, the device's own arithmetic, or what the hardware does in a
swap's inactive lanes.
"""
from __future__ import annotations

import concurrent.futures as cf
import os
import subprocess

from phastft_amd import build as _b

HERE = os.path.dirname(os.path.abspath(__file__))
EMU_LIB = os.path.join(HERE, "libphastft_emu.so")

# The sweep emulator (tests/test_sweep_emulator.py): sweep_shim.hpp turns a launch of a streaming sweep kernel into a serial
# loop on the host; tests/cpp/sweep_emu_test.cpp #includes the product's .hip files as they stand, one per translation unit.
SWEEP_SRC = os.path.join(os.path.dirname(HERE), "cpp", "sweep_emu_test.cpp")
SWEEP_SHIM = os.path.join(HERE, "sweep_shim.hpp")
SWEEP_EXE = os.path.join(HERE, "build", "sweep_emu_test")
SWEEP_PARTS = ["main", "any_len", "any_real", "dct", "stft", "conv", "czt", "complex_nums", "r2c"]  # SWEEP_PART = index
# host code only, under AddressSanitizer and UndefinedBehaviorSanitizer; an uninitialised local is a NaN pattern, not luck
SWEEP_FLAGS = ["--cuda-host-only", "-x", "hip", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
               "-fno-sanitize-recover=undefined", "-ftrivial-auto-var-init=pattern", "-Wall", "-Wno-unused-function",
               "-Wno-duplicate-decl-specifier"]

# The block emulator (tests/test_block_emulator.py): block_shim.hpp runs a workgroup as fibers that meet at __syncthreads();
# tests/cpp/block_emu_test.cpp #includes nd.hip, bitrev.hip, twiddle.hip and fill.hip as they stand, one per translation unit.
BLOCK_SRC = os.path.join(os.path.dirname(HERE), "cpp", "block_emu_test.cpp")
BLOCK_SHIM = os.path.join(HERE, "block_shim.hpp")
BLOCK_EXE = os.path.join(HERE, "build", "block_emu_test")
BLOCK_PARTS = ["main", "nd", "bitrev", "twiddle", "digest"]  # BLOCK_PART = index
# as SWEEP_FLAGS, without AddressSanitizer's fake stacks (use-after-return): one per fiber, mapped and unmapped for each of the
# millions of GPU threads a run emulates, they multiply its time; the frames stay on the fibers' own stacks
BLOCK_FLAGS = SWEEP_FLAGS + ["-fsanitize-address-use-after-return=never"]

# The pass emulator (tests/test_pass_emulator.py): block_shim.hpp with its lanes and waves; tests/cpp/pass_emu_test.cpp #includes
# the fifteen product units of the FFT pass kernels as they stand, one per translation unit, and launches every pass through the
# product's own launcher.  PASS_PART = index; the two *_wide units hold one instantiation each and run through their dispatcher's part.
PASS_SRC = os.path.join(os.path.dirname(HERE), "cpp", "pass_emu_test.cpp")
PASS_EXE = os.path.join(HERE, "build", "pass_emu_test")
PASS_PARTS = ["main", "tile_f64_a", "tile_f64_bc", "tile_f64_bc_wide", "tile_f32_a", "tile_f32_bc", "tile_f32_bc_wide", "tile_f64_r2c",
              "tile_f32_r2c", "tile_f64_c2r", "tile_f32_c2r", "wave_f64", "wave_f32", "quad_f64", "quad_f32", "small_fft"]


def build_emulator(force: bool = False) -> str:
    src = os.path.join(HERE, "emu.hip")
    if force or _b._stale(EMU_LIB, [src] + _b._deps()):
        # host code only (--cuda-host-only: the kernels are never launched), in four parts compiled in parallel at -O1:
        # the template instantiations of every tile shape make one -O3 translation unit a four-minute compile
        flags = [f for f in _b.FLAGS if f != "-O3"] + ["-O1", "--cuda-host-only"]
        os.makedirs(os.path.join(HERE, "build"), exist_ok=True)

        def part(k: int) -> str:
            obj = os.path.join(HERE, "build", f"emu_part{k}.o")
            cmd = [_b.hipcc(), *flags, f"-DEMU_PART={k}", "-I", _b.INCLUDE, "-I", _b.SRC, "-c", src, "-o", obj]
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:
                raise RuntimeError(f"hipcc failed for emu part {k}:\n{r.stdout}\n{r.stderr}")
            return obj

        with cf.ThreadPoolExecutor(4) as ex:
            objs = list(ex.map(part, (1, 2, 3, 4)))
        r = subprocess.run([_b.hipcc(), "-shared", "-fPIC", "-o", EMU_LIB, *objs], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"link failed for emu:\n{r.stdout}\n{r.stderr}")
    return EMU_LIB


def _host_linker() -> str:
    """clang++ of the ROCm toolchain: the program is linked WITHOUT the HIP runtime, so a call into it would be a link error"""
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(_b.hipcc())))
    for cand in (os.path.join(rocm, "llvm", "bin", "clang++"), os.path.join(rocm, "lib", "llvm", "bin", "clang++")):
        if os.path.exists(cand):
            return cand
    raise RuntimeError("clang++ of the ROCm toolchain not found next to hipcc")


def build_sweep_emulator(force: bool = False, override_dir: str | None = None, parts: tuple = (), out: str | None = None) -> str:
    """Builds the sweep emulator program and returns its path.  For the checker's self-test: the translation units named in
    `parts` are compiled with `override_dir` (a mutated copy of a product file) first on the include path, into the directory
    of `out`; every other object is the regular build's."""
    exe = out or SWEEP_EXE
    objdir = os.path.join(HERE, "build")
    os.makedirs(objdir, exist_ok=True)
    cpp = os.path.dirname(SWEEP_SRC)
    hips = [os.path.join(_b.SRC, f) for f in os.listdir(_b.SRC) if f.endswith(".hip")]
    deps = [SWEEP_SRC, SWEEP_SHIM, os.path.join(cpp, "sanitizer_exit.hpp"), os.path.abspath(__file__)] + hips + _b._deps()
    inc = ["-I", _b.SRC, "-I", _b.INCLUDE, "-I", HERE, "-I", cpp]

    def part(name: str) -> str:
        k = SWEEP_PARTS.index(name)
        mutated = override_dir is not None and name in parts
        obj = os.path.join(os.path.dirname(exe) if mutated else objdir, f"sweep_part{k}.o")
        if force or mutated or _b._stale(obj, deps):
            cmd = [_b.hipcc(), *SWEEP_FLAGS, f"-DSWEEP_PART={k}", *(["-I", override_dir] if mutated else []), *inc, "-c", SWEEP_SRC, "-o", obj]
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:
                raise RuntimeError(f"hipcc failed for sweep part {name}:\n{r.stdout}\n{r.stderr}")
        return obj

    with cf.ThreadPoolExecutor(len(SWEEP_PARTS)) as ex:
        objs = list(ex.map(part, SWEEP_PARTS))
    if force or override_dir or _b._stale(exe, objs):
        r = subprocess.run([_host_linker(), "-fsanitize=address,undefined", *objs, "-o", exe], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"link failed for the sweep emulator:\n{r.stdout}\n{r.stderr}")
    return exe


def build_block_emulator(force: bool = False, override_dir: str | None = None, parts: tuple = (), out: str | None = None) -> str:
    """Builds the block emulator program and returns its path; `override_dir`, `parts` and `out` as build_sweep_emulator's."""
    exe = out or BLOCK_EXE
    objdir = os.path.join(HERE, "build")
    os.makedirs(objdir, exist_ok=True)
    cpp = os.path.dirname(BLOCK_SRC)
    hips = [os.path.join(_b.SRC, f) for f in os.listdir(_b.SRC) if f.endswith(".hip")]
    deps = [BLOCK_SRC, BLOCK_SHIM, os.path.join(cpp, "sanitizer_exit.hpp"), os.path.abspath(__file__)] + hips + _b._deps()
    inc = ["-I", _b.SRC, "-I", _b.INCLUDE, "-I", HERE, "-I", cpp]

    def part(name: str) -> str:
        k = BLOCK_PARTS.index(name)
        mutated = override_dir is not None and name in parts
        obj = os.path.join(os.path.dirname(exe) if mutated else objdir, f"block_part{k}.o")
        if force or mutated or _b._stale(obj, deps):
            cmd = [_b.hipcc(), *BLOCK_FLAGS, f"-DBLOCK_PART={k}", *(["-I", override_dir] if mutated else []), *inc, "-c", BLOCK_SRC, "-o", obj]
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:
                raise RuntimeError(f"hipcc failed for block part {name}:\n{r.stdout}\n{r.stderr}")
        return obj

    with cf.ThreadPoolExecutor(len(BLOCK_PARTS)) as ex:
        objs = list(ex.map(part, BLOCK_PARTS))
    if force or override_dir or _b._stale(exe, objs):
        r = subprocess.run([_host_linker(), "-fsanitize=address,undefined", *objs, "-o", exe], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"link failed for the block emulator:\n{r.stdout}\n{r.stderr}")
    return exe


def build_pass_emulator(force: bool = False, override_dir: str | None = None, parts: tuple = (), out: str | None = None) -> str:
    """Builds the pass emulator program and returns its path; `override_dir`, `parts` and `out` as build_sweep_emulator's.  A
    mutated part is compiled at -O0 without debug information -- a fifth of the time of the regular -O1 -g build of a tile unit, and
    a self-test runs one shape of it."""
    exe = out or PASS_EXE
    objdir = os.path.join(HERE, "build")
    os.makedirs(objdir, exist_ok=True)
    cpp = os.path.dirname(PASS_SRC)
    hips = [os.path.join(_b.SRC, f) for f in os.listdir(_b.SRC) if f.endswith(".hip")]
    deps = [PASS_SRC, BLOCK_SHIM, os.path.join(cpp, "sanitizer_exit.hpp"), os.path.abspath(__file__)] + hips + _b._deps()
    inc = ["-I", _b.SRC, "-I", _b.INCLUDE, "-I", HERE, "-I", cpp]

    def part(name: str) -> str:
        k = PASS_PARTS.index(name)
        mutated = override_dir is not None and name in parts
        obj = os.path.join(os.path.dirname(exe) if mutated else objdir, f"pass_part{k}.o")
        if force or mutated or _b._stale(obj, deps):
            flags = [f for f in BLOCK_FLAGS if f not in ("-O1", "-g")] + ["-O0"] if mutated else BLOCK_FLAGS
            cmd = [_b.hipcc(), *flags, f"-DPASS_PART={k}", *(["-I", override_dir] if mutated else []), *inc, "-c", PASS_SRC, "-o", obj]
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:
                raise RuntimeError(f"hipcc failed for pass part {name}:\n{r.stdout}\n{r.stderr}")
        return obj

    with cf.ThreadPoolExecutor(min(len(PASS_PARTS), os.cpu_count() or 4, 16)) as ex:
        objs = list(ex.map(part, PASS_PARTS))
    if force or override_dir or _b._stale(exe, objs):
        r = subprocess.run([_host_linker(), "-fsanitize=address,undefined", *objs, "-o", exe], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"link failed for the pass emulator:\n{r.stdout}\n{r.stderr}")
    return exe
