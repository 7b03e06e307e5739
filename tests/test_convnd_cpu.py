"""N-d overlap-save convolution and correlation (csrc/convnd.hpp, csrc/planner_convnd.hpp) without a GPU: convnd.hpp's geometry,
automatic block and argument rules compiled with g++ and checked against Python integers; the tile schedule run in numpy through
those helpers around pocketfft's double rfftn / irfftn, against scipy.signal.convolve / correlate(method="direct") and against
tests/convnd_reference.py (the GPU tests' reference), every output sample written exactly once; the new C ABI exported and
listed, with every argument rule returned before the device is touched; the C++ and Rust mirrors."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.fft as sf
import scipy.signal as ss

from tests import convnd_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = [f"phast_planner_convnd{s}_{w}" for s in ("64", "32")
       for w in ("new", "free", "describe", "device_bytes", "out_len", "out_dims", "block", "tiles", "workspace_len",
                 "workspace_min", "time_stages")]
NEW += [f"phast_convnd_{fs}{suffix}" for fs in ("f64", "f32") for suffix in ("_with_planner", "_dev")]
OK, LEN_MISMATCH, NO_DEVICE, INVALID_ARG = 0, 2, 15, 16
ULL3 = C.c_ulonglong * 3


class Geom(C.Structure):
    """ConvNdGeom of csrc/convnd.hpp"""
    _fields_ = [("rank", C.c_uint), ("axis_of", C.c_uint * 3), ("len", ULL3), ("k", ULL3), ("b", ULL3), ("s", ULL3), ("t0", ULL3),
                ("out", ULL3), ("segs", ULL3), ("sig_pts", C.c_ulonglong), ("out_pts", C.c_ulonglong), ("tile_pts", C.c_ulonglong),
                ("tiles", C.c_ulonglong)]


HELPERS = r"""
#include "convnd.hpp"
extern "C" {
unsigned long long auto_block(unsigned long long len, unsigned long long k, int mode, unsigned rank) {
    return phast::convnd_auto_block(len, k, mode, rank);
}
int bad_args(const size_t *sig, const size_t *taps, size_t rank, int mode, int flip, const size_t *block, unsigned long long vec,
             phast::ConvNdGeom *g) {
    return phast::convnd_bad_args(sig, taps, rank, mode, flip, block, vec, g);
}
long long src0(const phast::ConvNdGeom *g, unsigned i, unsigned long long s) { return phast::convnd_src0(*g, i, s); }
unsigned long long yield(const phast::ConvNdGeom *g, unsigned i, unsigned long long s) { return phast::convnd_yield(*g, i, s); }
unsigned long long save_groups(unsigned long long s, unsigned long long vec) { return phast::convnd_save_groups(s, vec); }
unsigned long long geom_size() { return sizeof(phast::ConvNdGeom); }
}
"""


@pytest.fixture(scope="module")
def helpers(tmp_path_factory):
    d = tmp_path_factory.mktemp("convnd_helpers")
    src, so = d / "helpers.cpp", d / "libconvndhelpers.so"
    src.write_text(HELPERS)
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-shared", "-fPIC", "-I",
                        os.path.join(ROOT, "phastft_amd", "csrc"), str(src), "-o", str(so)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    h = C.CDLL(str(so))
    h.auto_block.restype = C.c_ulonglong
    h.auto_block.argtypes = [C.c_ulonglong, C.c_ulonglong, C.c_int, C.c_uint]
    h.bad_args.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_ulonglong, C.POINTER(Geom)]
    h.src0.restype = C.c_longlong
    h.src0.argtypes = [C.POINTER(Geom), C.c_uint, C.c_ulonglong]
    getattr(h, "yield").restype = C.c_ulonglong
    getattr(h, "yield").argtypes = [C.POINTER(Geom), C.c_uint, C.c_ulonglong]
    h.save_groups.restype = C.c_ulonglong
    h.save_groups.argtypes = [C.c_ulonglong, C.c_ulonglong]
    h.geom_size.restype = C.c_ulonglong
    assert h.geom_size() == C.sizeof(Geom)
    return h


def sz(values):
    return (C.c_size_t * max(1, len(values)))(*values)


def geom_of(h, L, K, mode, flip=0, block=None, vec=2, rank=None):
    """(bad, ConvNdGeom) of convnd_bad_args"""
    g = Geom()
    bad = h.bad_args(sz(L), sz(K), len(L) if rank is None else rank, R.MODE.get(mode, mode), flip,
                     None if block is None else sz(block), vec, C.byref(g))
    return bad, g


def test_geometry_against_python_integers(helpers):
    """per axis t0, out, S and the tile count over a grid with K = 1, B = K (S = 1), K > L, and out a multiple and a non-multiple of
    S; axes with L = K = 1 are dropped (the last stays if nothing else does) and the rest sits behind unit axes"""
    multiples = ragged = 0
    for L in ((1, 1), (7,), (9, 7), (5, 6), (1, 12), (12, 1), (6, 5, 7), (1, 5, 1), (4, 1, 9), (1, 1, 1)):
        for K in itertools.product((1, 2, 5), repeat=len(L)):
            for extra in (0, 1, 6):
                B = tuple(k + extra for k in K)
                for mode in R.MODES:
                    bad, g = geom_of(helpers, L, K, mode, block=B)
                    if not R.has_mode(L, K, mode):
                        assert bad, (L, K, mode)
                        continue
                    assert not bad, (L, K, B, mode)
                    counts = [i for i in range(len(L)) if L[i] > 1 or K[i] > 1] or [len(L) - 1]
                    assert g.rank == len(counts)
                    t0, out = R.geometry(L, K, mode)
                    for e in range(3):
                        if e < 3 - g.rank:
                            assert (g.len[e], g.k[e], g.b[e], g.s[e], g.t0[e], g.out[e], g.segs[e]) == (1, 1, 1, 1, 0, 1, 1)
                            continue
                        ax = counts[e - (3 - g.rank)]
                        assert g.axis_of[e] == ax
                        s = B[ax] - K[ax] + 1
                        assert (g.len[e], g.k[e], g.b[e], g.s[e], g.t0[e], g.out[e]) == (L[ax], K[ax], B[ax], s, t0[ax], out[ax])
                        segs = g.segs[e]
                        assert segs == -(-out[ax] // s) and (segs - 1) * s < out[ax] <= segs * s
                        multiples += out[ax] % s == 0
                        ragged += out[ax] % s != 0
                        for t in range(segs):
                            assert helpers.src0(g, e, t) == t0[ax] + t * s - (K[ax] - 1)
                            y = getattr(helpers, "yield")(g, e, t)
                            assert y == min(s, out[ax] - t * s) and K[ax] - 1 + y - 1 <= B[ax] - 1
                    assert g.sig_pts == int(np.prod(L)) and g.out_pts == int(np.prod(out))
                    assert g.tile_pts == int(np.prod([g.b[e] for e in range(3)]))
                    assert g.tiles == int(np.prod([g.segs[e] for e in range(3)]))
    assert multiples > 100 and ragged > 100
    # the groups of an output row that one tile's run can touch, wherever the row starts in a 16-byte group
    for s in range(1, 40):
        for vec in (2, 4):
            worst = max(-(-(p + s) // vec) for p in range(vec))
            assert worst <= helpers.save_groups(s, vec) <= worst + 1


def test_automatic_block(helpers):
    """the smallest power of two >= max(4 (K - 1), floor), floor 1024 for one axis that counts and 64 for two or three; the
    smallest power of two >= out + K - 1 where that is smaller; an explicit block wins"""
    for L, K in (((1, 1), (1, 1)), ((4096, 4096), (5, 5)), ((4096, 4096), (31, 31)), ((4096, 4096), (129, 129)),
                 ((256, 256, 256), (7, 7, 7)), ((100, 130), (9, 9)), ((300, 260), (31, 31)), ((5, 6), (7, 9)), ((1 << 20,), (33,)),
                 ((1 << 20,), (1000,)), ((1, 1 << 20), (1, 33)), ((40, 1, 50), (3, 1, 3)), ((12, 10), (1, 4))):
        for mode in R.MODES:
            if not R.has_mode(L, K, mode):
                continue
            bad, g = geom_of(helpers, L, K, mode)
            assert not bad
            want = R.auto_block(L, K, mode)
            got = [1] * len(L)
            for e in range(3 - g.rank, 3):
                got[g.axis_of[e]] = g.b[e]
            assert tuple(got) == want, (L, K, mode, got, want)
            assert all(b >= k and b & (b - 1) == 0 for b, k in zip(got, K))
            bad, g = geom_of(helpers, L, K, mode, block=tuple(k + 1 for k in K))   # an explicit block always wins
            assert not bad and all(g.b[e] == g.k[e] + 1 for e in range(3 - g.rank, 3))
    assert R.auto_block((4096, 4096), (31, 31), "same") == (128, 128) and R.auto_block((4096, 4096), (5, 5), "same") == (64, 64)
    assert R.auto_block((4096, 4096), (129, 129), "same") == (512, 512) and R.auto_block((256,) * 3, (7,) * 3, "same") == (64,) * 3
    assert R.auto_block((300, 260), (31, 31), "full") == (128, 128) and R.auto_block((1, 1), (1, 1), "full") == (1, 1)
    assert R.auto_block((1, 1 << 20), (1, 33), "full") == (1, 1024) and R.auto_block((100, 130), (9, 9), "valid") == (64, 64)
    assert helpers.auto_block(4096, 31, 1, 2) == 128 and helpers.auto_block(4096, 31, 1, 1) == 1024


def test_argument_rules_of_the_helper(helpers):
    big = 1 << 29
    for (L, K, mode, flip, block, vec), bad in (
            (((9, 7), (3, 4), 0, 0, (4, 4), 2), 0), (((9, 7), (3, 4), 2, 1, None, 4), 0), (((9, 7), (3, 4), 1, 0, (0, 6), 2), 0),
            (((9, 3), (3, 4), 2, 0, (4, 4), 2), 1),            # valid with L < K on one axis only
            (((9, 3), (3, 4), 1, 0, (4, 4), 2), 0),            # ... same and full take K > L
            (((9, 7), (3, 4), 0, 0, (4, 3), 2), 1),            # B < K on one axis
            (((9, 0), (3, 4), 0, 0, None, 2), 1), (((9, 7), (0, 4), 0, 0, None, 2), 1),   # a zero dimension
            (((big + 1, 1), (3, 4), 1, 0, None, 2), 1), (((9, 7), (3, big + 1), 1, 0, None, 2), 1),
            (((9, 7), (3, 4), 0, 0, (big + 1, 4), 2), 1),      # B > 2^29
            (((1 << 15, 1 << 15), (3, 3), 1, 0, (4, 4), 2), 0),        # prod L = 2^30 exactly
            (((1 << 15, (1 << 15) + 1), (3, 3), 1, 0, (4, 4), 2), 1),  # prod L > 2^30
            (((1 << 15, 1 << 15), (3, 3), 0, 0, (4, 4), 2), 1),        # prod out > 2^30
            (((9, 7), (3, 4), 1, 0, (1 << 14, 1 << 14), 2), 0),        # prod B = 2^28 exactly
            (((9, 7), (3, 4), 1, 0, (1 << 15, 1 << 14), 2), 1),        # prod B > 2^28
            (((9, 7, 2), (3, 4, 1), 1, 0, (1 << 10, 1 << 10, 1 << 9), 4), 1),
            (((9, 7), (3, 4), 3, 0, None, 2), 1), (((9, 7), (3, 4), -1, 0, None, 2), 1),   # the mode
            (((9, 7), (3, 4), 0, 2, None, 2), 1),              # flip is 0 or 1
            (((9, 7), (3, 4), 0, 0, None, 3), 1)):             # 16 bytes hold 2 or 4 elements
        assert bool(geom_of(helpers, L, K, mode, flip, block, vec)[0]) == bool(bad), (L, K, mode, flip, block, vec)
    assert geom_of(helpers, (), (), 0)[0] and geom_of(helpers, (2, 2, 2, 2), (1, 1, 1, 1), 0)[0]   # rank 0 and 4
    g = Geom()
    assert helpers.bad_args(None, sz((1,)), 1, 0, 0, None, 2, C.byref(g)) and helpers.bad_args(sz((1,)), None, 1, 0, 0, None, 2, C.byref(g))


def tiled(h, x, taps, block, mode, flip, dtype=np.float64):
    """the sweeps of convnd.hip restated in numpy on convnd.hpp's helpers, around pocketfft's rfftn / irfftn per tile; returns the
    output and how often each of its samples was written"""
    bad, g = geom_of(h, x.shape, taps.shape, mode, int(flip), block)
    assert not bad
    x3 = np.asarray(x, dtype).reshape([g.len[e] for e in range(3)])
    k3 = np.asarray(taps, np.float64).reshape([g.k[e] for e in range(3)])
    if flip:
        k3 = k3[::-1, ::-1, ::-1]
    B = [g.b[e] for e in range(3)]
    gp = np.zeros(B)
    gp[:k3.shape[0], :k3.shape[1], :k3.shape[2]] = k3
    spec = sf.rfftn(gp).astype(np.complex64 if dtype == np.float32 else np.complex128)
    out = np.zeros([g.out[e] for e in range(3)], dtype)
    written = np.zeros(out.shape, np.int64)
    for s in itertools.product(*(range(g.segs[e]) for e in range(3))):
        idx = [h.src0(g, e, s[e]) + np.arange(B[e]) for e in range(3)]                            # tile sweep
        ok = [(i >= 0) & (i < g.len[e]) for e, i in enumerate(idx)]
        tile = np.where(ok[0][:, None, None] & ok[1][None, :, None] & ok[2][None, None, :], x3[np.ix_(*[np.clip(i, 0, g.len[e] - 1) for e, i in enumerate(idx)])], dtype(0))
        y = sf.irfftn(sf.rfftn(tile) * spec, s=B)                                                 # R2C, spectrum sweep, C2R
        assert y.dtype == dtype
        n = [getattr(h, "yield")(g, e, s[e]) for e in range(3)]                                   # save sweep
        dst = tuple(slice(s[e] * g.s[e], s[e] * g.s[e] + n[e]) for e in range(3))
        out[dst] = y[tuple(slice(g.k[e] - 1, g.k[e] - 1 + n[e]) for e in range(3))]
        written[dst] += 1
    return out, written, g


def test_schedule_against_scipy_and_the_reference(helpers):
    """every mode and both flips over all shapes, in double and in single: against scipy's direct sums and against
    tests/convnd_reference.py; each output sample is written exactly once; the worst rel-L2 is printed (DESIGN.md §23 quotes it)"""
    worst = {"float64": 0.0, "float32": 0.0}
    ref_vs_scipy = 0.0
    for L, K, B in R.SHAPES:
        for mode in R.MODES:
            if not R.has_mode(L, K, mode):
                assert geom_of(helpers, L, K, mode, block=B)[0]
                continue
            for flip in (False, True):
                for dt in (np.float64, np.float32):
                    x, taps, want = R.expected(L, K, np.dtype(dt).name, mode, flip)
                    got, written, g = tiled(helpers, x, taps, B, mode, flip, dt)
                    assert got.size == want.size and tuple(got.reshape(want.shape).shape) == R.geometry(L, K, mode)[1]
                    assert np.all(written == 1), (L, K, B, mode, flip)
                    got = got.reshape(want.shape).astype(np.longdouble)
                    den = float(np.sqrt((want ** 2).sum())) or 1.0
                    worst[np.dtype(dt).name] = max(worst[np.dtype(dt).name], float(np.sqrt(((got - want) ** 2).sum())) / den)
                    if dt is np.float64:
                        direct = (ss.correlate if flip else ss.convolve)(x, taps, mode=mode, method="direct")
                        assert direct.shape == want.shape, (L, K, mode, flip)
                        ref_vs_scipy = max(ref_vs_scipy, float(np.abs(direct - want).max()))
    print(f"tiled overlap-save around pocketfft, worst rel-L2 vs the long double sum: f64 {worst['float64']:.3e}, f32 "
          f"{worst['float32']:.3e}; the reference vs scipy direct, worst |difference| {ref_vs_scipy:.3e}")
    # a direct sum of <= 961 products in double, and transforms of <= 2^14 points in the working precision, stay far below these
    assert worst["float64"] < 1e-14 and worst["float32"] < 5e-6 and ref_vs_scipy < 1e-12


@pytest.fixture(scope="module")
def lib():
    from phastft_amd import _lib

    return _lib.lib()


def test_new_symbols_are_exported_and_listed(lib):
    from phastft_amd import _lib

    header = open(os.path.join(ROOT, "include", "phastft_hip.h")).read()
    assert len(NEW) == 26
    for name in NEW:
        getattr(lib, name)
        assert name in _lib.SYMBOLS and re.search(r"\b" + name + r"\s*\(", header), name
    import phastft_amd as P

    for name in ("PlannerConvNd64", "PlannerConvNd32", "convnd_batched", "convnd_f64_with_planner", "convnd_f32_with_planner",
                 "fftconvolve_nd", "correlate_nd"):
        assert name in P.__all__ and callable(getattr(P, name)), name
    assert "PlannerConvNd64/32" in P.__doc__


def test_argument_codes(lib):
    """every rule of _new, null planners and null pointers come back before the device is touched"""
    big = 1 << 29
    for sfx, fs, dt in (("64", "f64", np.float64), ("32", "f32", np.float32)):
        new = getattr(lib, f"phast_planner_convnd{sfx}_new")
        taps = np.ones(12, dt)
        tp = taps.ctypes.data_as(C.c_void_p)

        def make(L, K, mode=0, flip=0, block=None, out=True, h=tp, rank=None, dims=True):
            p = C.c_void_p(1)
            rc = new(sz(L) if dims else None, sz(K), len(L) if rank is None else rank, h, mode, flip,
                     None if block is None else sz(block), C.byref(p) if out else None)
            assert rc == OK or not p.value or not out
            return rc

        assert make((), (), rank=0) == INVALID_ARG                          # rank 0
        assert make((2, 2, 2, 2), (1, 1, 3, 4)) == INVALID_ARG              # rank 4
        assert make((9, 0), (3, 4)) == INVALID_ARG                          # a zero dimension
        assert make((9, 7), (3, 0)) == INVALID_ARG
        assert make((9, 3), (3, 4), mode=2) == INVALID_ARG                  # valid with L_i < K_i on one axis only
        assert make((9, 7), (3, 4), block=(4, 3)) == INVALID_ARG            # B_i < K_i
        assert make((9, 7), (3, 4), block=(1 << 15, 1 << 14)) == INVALID_ARG   # prod B > 2^28
        assert make((big + 1, 7), (3, 4), mode=1) == INVALID_ARG            # L_i > 2^29
        assert make((1 << 15, 1 << 15), (3, 4), block=(4, 4)) == INVALID_ARG   # prod out > 2^30
        assert make((9, 7), (3, 4), mode=3) == INVALID_ARG                  # the mode
        assert make((9, 7), (3, 4), flip=2) == INVALID_ARG                  # flip is 0 or 1
        assert make((9, 7), (3, 4), h=None) == INVALID_ARG                  # no taps
        assert make((9, 7), (3, 4), dims=False) == INVALID_ARG              # no shape
        assert make((9, 7), (3, 4), out=False) == INVALID_ARG
        assert getattr(lib, f"phast_planner_convnd{sfx}_workspace_len")(None, 1) == 0
        for name in ("device_bytes", "out_len", "tiles", "workspace_min"):
            assert getattr(lib, f"phast_planner_convnd{sfx}_{name}")(None) == 0
        d = sz((0, 0))
        for name in ("out_dims", "block"):
            assert getattr(lib, f"phast_planner_convnd{sfx}_{name}")(None, d, 2) == INVALID_ARG
        assert getattr(lib, f"phast_planner_convnd{sfx}_describe")(None, C.create_string_buffer(8), 8) == INVALID_ARG
        ms = (C.c_float * 5)()
        assert getattr(lib, f"phast_planner_convnd{sfx}_time_stages")(None, None, None, 1, None, 0, 1, ms, None) == INVALID_ARG
        x, y = np.zeros(63, dt), np.zeros(110, dt)
        p = lambda v: v.ctypes.data_as(C.c_void_p)  # noqa: E731
        assert getattr(lib, f"phast_convnd_{fs}_with_planner")(p(x), 63, p(y), 110, None) == INVALID_ARG
        assert getattr(lib, f"phast_convnd_{fs}_dev")(p(x), p(y), 63, 1, 63, 110, None, None, 0, None) == INVALID_ARG


def test_calls_without_a_gpu_fail_loudly(lib):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present: tests/test_gpu_convnd.py covers the device side")
    h = C.c_void_p()
    taps = np.ones((3, 4))
    assert lib.phast_planner_convnd64_new(sz((9, 7)), sz((3, 4)), 2, taps.ctypes.data_as(C.c_void_p), 0, 0, None, C.byref(h)) == NO_DEVICE
    assert not h.value
    taps32 = np.ones((7, 9), np.float32)
    assert lib.phast_planner_convnd32_new(sz((5, 6)), sz((7, 9)), 2, taps32.ctypes.data_as(C.c_void_p), 1, 1, sz((8, 16)),
                                          C.byref(h)) == NO_DEVICE
    import phastft_amd as P

    with pytest.raises(P.PhastHipError):
        P.PlannerConvNd64((9, 7), taps)


def test_python_argument_errors():
    import phastft_amd as P

    with pytest.raises(ValueError):
        P.PlannerConvNd64((9, 7), np.ones((3, 4)), mode="wrap")
    with pytest.raises(ValueError):
        P.PlannerConvNd64((9, 7), np.ones(12))                         # the taps' rank is not the arrays'
    with pytest.raises(ValueError):
        P.PlannerConvNd64((9, 7), np.ones((3, 4)), block=(4,))         # one block for two axes
    with pytest.raises(P.PhastPanic):
        P.PlannerConvNd64((9, 3), np.ones((3, 4)), mode="valid")       # L_1 < K_1: INVALID_ARG before the device is touched
    with pytest.raises(P.PhastPanic):
        P.PlannerConvNd32((9, 7), np.ones((3, 4)), block=(4, 3))       # B_1 < K_1
    with pytest.raises(P.PhastPanic):
        P.PlannerConvNd32((9, 7), np.ones((3, 0)))                     # no taps
    with pytest.raises(P.PhastPanic):
        P.PlannerConvNd64((2, 2, 2, 2), np.ones((1, 1, 1, 1)))         # rank 4


def test_cpp_mirror_without_gpu(tmp_path):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present: tests/test_gpu_convnd.py runs the mirror there")
    from phastft_amd import build

    lib = build.build()
    exe = str(tmp_path / "convnd_test")
    libdir = os.path.dirname(lib)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "convnd_test.cpp"), "-o", exe, "-L", libdir, "-lphastft_hip",
                        f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "convnd: ok" in r.stdout, r.stdout + r.stderr


def test_rust_mirror():
    """Parsed textually, as tests/test_rust_shim.py does (no Rust toolchain here)"""
    src = os.path.join(ROOT, "rust", "phastft-hip", "src")
    ffi = open(os.path.join(src, "ffi.rs")).read()
    for name in NEW:
        assert re.search(r"fn " + name + r"\s*\(", ffi), name
    planner = open(os.path.join(src, "planner.rs")).read()
    assert "PlannerConvNd64" in planner and "PlannerConvNd32" in planner
    conv = open(os.path.join(src, "algorithms", "convnd.rs")).read()
    for f in ("convnd_f64_with_planner", "convnd_f32_with_planner", "convnd_f64_dev", "convnd_f32_dev"):
        assert re.search(r"\b" + f + r"\b", conv), f
    assert "pub mod convnd;" in open(os.path.join(src, "algorithms", "mod.rs")).read()
    lib = open(os.path.join(src, "lib.rs")).read()
    assert "PlannerConvNd64" in lib and "convnd_f64_with_planner" in lib
