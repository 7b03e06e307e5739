"""phastft_amd -- MI355X (gfx950) drop-in for PhastFT's planar power-of-two FFT path.

Host-side mirror of the reference's public Rust API (QuState/PhastFT 0.3.0; citations are relative to
the reference tree) over the C ABI of ``include/phastft_hip.h``:

    ==============================================  ==========================================
    reference (Rust)                                here
    ==============================================  ==========================================
    Direction, PlannerMode            planner.rs:10  Direction, PlannerMode
    Options, Options::guess_options   options.rs:10  Options, Options.guess_options
    PlannerDit64/32::{new,with_mode}  planner.rs:55  PlannerDit64/32(n), .with_mode(n, mode)
    PlannerR2c64/32::new              planner.rs:194 PlannerR2c64/32(n)
    fft_64_dit / fft_32_dit           lib.rs:180,223 fft_64_dit / fft_32_dit
    fft_*_dit_with_planner[_and_opts] lib.rs:143,186 same names
    r2c_fft_f32/f64[_with_planner]    r2c.rs:521-662 same names
    c2r_fft_*[_with_planner[_and_scratch]] r2c.rs:695 same names
    bit_rev_bravo_f32/f64             bravo.rs:303   bit_rev_bravo_f32/f64(data, n)
    deinterleave[_complex64/32]       complex_nums.rs:11   deinterleave(data) -> (a, b)
    combine_re_im                     complex_nums.rs:47   combine_re_im(reals, imags) -> Complex<T> array
    (none: powers of two only)                      PlannerAny64/32, fft_64/32_any[_with_planner], fft_any_batched
    (none: r2c.rs takes powers of two >= 4)         PlannerR2cAny64/32, r2c_fft_f64/f32_any[_with_planner],
                                                    c2r_fft_f64/f32_any[_with_planner], r2c_any_batched, c2r_any_batched
    (none: no real-to-real transforms)              PlannerDct64/32, dct_f64/f32[_with_planner], dst_f64/f32[_with_planner],
                                                    dct_batched, dst_batched, idct, idst
    (none: no short-time transforms)                PlannerStft64/32, stft_batched, istft_batched,
                                                    stft_f64/f32_with_planner, istft_f64/f32_with_planner
    (none: no lapped transforms)                    PlannerMdct64/32, mdct_batched, imdct_batched,
                                                    mdct_f64/f32_with_planner, imdct_f64/f32_with_planner, mdct, imdct,
                                                    mdct_window
    (none: no spectral estimation)                  PlannerPsd64/32, psd_batched, csd_batched,
                                                    psd_f64/f32_with_planner, csd_f64/f32_with_planner, welch, csd,
                                                    spectrogram, periodogram, coherence
    (none: no spectra of uneven samples)            PlannerLomb64/32, lombscargle_batched,
                                                    lombscargle_f64/f32_with_planner, lombscargle
    (none: no sample-rate conversion)               PlannerUpfirdn64/32, PlannerResample64/32, upfirdn_batched,
                                                    resample_batched, upfirdn_64/32_with_planner,
                                                    resample_64/32_with_planner, upfirdn, resample_poly, decimate,
                                                    resample, firwin_lowpass
    (none: no filter banks)                         PlannerChannelizer64/32, channelize_batched,
                                                    channelize_64/32_with_planner, channelize_poly, pfb_prototype
    (none: no filter banks)                         PlannerSynthesizer64/32, synthesize_batched,
                                                    synthesize_64/32_with_planner, synthesize_poly
    (none: no wavelets)                             PlannerCwt64/32, cwt_batched, cwt_64/32_with_planner, cwt, hilbert,
                                                    cwt_scales, cwt_fourier_period
    (none: no wavelets)                             PlannerDwt64/32, wavedec_batched, waverec_batched,
                                                    wavedec_64/32_with_planner, waverec_64/32_with_planner, dwt, idwt,
                                                    wavedec, waverec, wavelet_filters, dwt_max_level, dwt_coeff_lens
    (none: no convolution)                          PlannerConv64/32, conv_batched, conv_f64/f32_with_planner,
                                                    fftconvolve, correlate
    (none: no convolution)                          PlannerConvNd64/32, convnd_batched, convnd_f64/f32_with_planner,
                                                    fftconvolve_nd, correlate_nd
    (none: whole spectra only)                      PlannerCzt64/32, czt_batched, czt_64/32[_with_planner], czt, zoom_fft
    (none: samples on a grid only)                  PlannerNufft64/32, nufft1_batched, nufft2_batched,
                                                    nufft1_64/32[_with_planner], nufft2_64/32[_with_planner], nufft1, nufft2
    (none: samples on a grid only)                  PlannerNufft2d64/32, nufft2d1_batched, nufft2d2_batched,
                                                    nufft2d1_64/32[_with_planner], nufft2d2_64/32[_with_planner],
                                                    nufft2d1, nufft2d2
    (none: samples on a grid only)                  PlannerNufft3d64/32, nufft3d1_batched, nufft3d2_batched,
                                                    nufft3d1_64/32[_with_planner], nufft3d2_64/32[_with_planner],
                                                    nufft3d1, nufft3d2
    (none: samples on a grid only)                  PlannerNufftT3_64/32, nufft3_batched, nufft3_64/32[_with_planner], nufft3
    (none: one axis only)                           PlannerNd64/32, fft_64/32_nd[_with_planner], fft_nd_batched,
                                                    PlannerR2cNd64/32, r2c_fft_f64/f32_nd[_with_planner],
                                                    c2r_fft_f64/f32_nd[_with_planner], r2c_nd_batched, c2r_nd_batched
    ==============================================  ==========================================

Slices are 1-D contiguous arrays: ``numpy.ndarray`` (host slices -- staged through device memory, the
Rust drop-in semantics) or ``torch.Tensor`` on ``cuda`` (device-resident, asynchronous on torch's current
stream; this is the measured path).  All transforms are in place on planar ``reals`` / ``imags``; forward is
unnormalised and ``Direction.Reverse`` scales by 1/N, as in the reference (README.md:167-172).

The reference signals misuse by panicking; here every reference ``assert!`` raises :class:`PhastPanic`
carrying the reference's message.  There is NO CPU fallback: without the HIP library or a GPU the calls
raise.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import enum
import functools
import math
from dataclasses import dataclass

import numpy as np

from . import _lib

__all__ = [
    "Direction", "PlannerMode", "TuneKind", "wisdom_export", "wisdom_import", "wisdom_forget", "wisdom_builtin", "wisdom_count", "Options", "PhastPanic", "PhastHipError",
    "PlannerDit64", "PlannerDit32", "PlannerR2c64", "PlannerR2c32",
    "fft_64_dit", "fft_32_dit", "fft_64_dit_with_planner", "fft_32_dit_with_planner",
    "fft_64_dit_with_planner_and_opts", "fft_32_dit_with_planner_and_opts",
    "r2c_fft_f64", "r2c_fft_f32", "r2c_fft_f64_with_planner", "r2c_fft_f32_with_planner",
    "c2r_fft_f64", "c2r_fft_f32", "c2r_fft_f64_with_planner", "c2r_fft_f32_with_planner",
    "c2r_fft_f64_with_planner_and_scratch", "c2r_fft_f32_with_planner_and_scratch",
    "fft_dit_strided", "fft_64_interleaved", "fft_32_interleaved", "fft_64_interleaved_with_planner", "fft_32_interleaved_with_planner",
    "fft_64_interleaved_with_planner_and_opts", "fft_32_interleaved_with_planner_and_opts",
    "bit_rev_bravo_f64", "bit_rev_bravo_f32", "deinterleave", "deinterleave_complex64", "deinterleave_complex32", "combine_re_im", "fft_dit_batched", "r2c_fft_batched", "c2r_fft_batched", "fill_uniform", "digest", "device_info",
    "TwiddleGrid64", "TwiddleGrid32",
    "PlannerAny64", "PlannerAny32", "fft_64_any", "fft_32_any", "fft_64_any_with_planner", "fft_32_any_with_planner",
    "fft_any_batched",
    "PlannerR2cAny64", "PlannerR2cAny32", "r2c_fft_f64_any", "r2c_fft_f32_any", "r2c_fft_f64_any_with_planner",
    "r2c_fft_f32_any_with_planner", "c2r_fft_f64_any", "c2r_fft_f32_any", "c2r_fft_f64_any_with_planner",
    "c2r_fft_f32_any_with_planner", "r2c_any_batched", "c2r_any_batched",
    "PlannerDct64", "PlannerDct32", "dct_f64", "dct_f32", "dst_f64", "dst_f32", "dct_f64_with_planner", "dct_f32_with_planner",
    "dst_f64_with_planner", "dst_f32_with_planner", "dct_batched", "dst_batched", "idct", "idst",
    "PlannerStft64", "PlannerStft32", "stft_batched", "istft_batched", "stft_f64_with_planner", "stft_f32_with_planner",
    "istft_f64_with_planner", "istft_f32_with_planner",
    "PlannerMdct64", "PlannerMdct32", "mdct_batched", "imdct_batched", "mdct_f64_with_planner", "mdct_f32_with_planner",
    "imdct_f64_with_planner", "imdct_f32_with_planner", "mdct", "imdct", "mdct_window",
    "PlannerPsd64", "PlannerPsd32", "psd_batched", "csd_batched", "psd_f64_with_planner", "psd_f32_with_planner",
    "csd_f64_with_planner", "csd_f32_with_planner", "welch", "csd", "spectrogram", "periodogram", "coherence",
    "PlannerLomb64", "PlannerLomb32", "lombscargle_batched", "lombscargle_f64_with_planner", "lombscargle_f32_with_planner",
    "lombscargle",
    "PlannerUpfirdn64", "PlannerUpfirdn32", "PlannerResample64", "PlannerResample32", "upfirdn_batched", "resample_batched",
    "upfirdn_64_with_planner", "upfirdn_32_with_planner", "resample_64_with_planner", "resample_32_with_planner", "upfirdn",
    "resample_poly", "decimate", "resample", "firwin_lowpass",
    "PlannerChannelizer64", "PlannerChannelizer32", "channelize_batched", "channelize_64_with_planner",
    "channelize_32_with_planner", "channelize_poly", "pfb_prototype",
    "PlannerSynthesizer64", "PlannerSynthesizer32", "synthesize_batched", "synthesize_64_with_planner",
    "synthesize_32_with_planner", "synthesize_poly",
    "PlannerCwt64", "PlannerCwt32", "cwt_batched", "cwt_64_with_planner", "cwt_32_with_planner", "cwt", "hilbert",
    "cwt_scales", "cwt_fourier_period",
    "PlannerDwt64", "PlannerDwt32", "wavedec_batched", "waverec_batched", "wavedec_64_with_planner", "wavedec_32_with_planner",
    "waverec_64_with_planner", "waverec_32_with_planner", "dwt", "idwt", "wavedec", "waverec", "wavelet_filters",
    "dwt_max_level", "dwt_coeff_lens",
    "PlannerConv64", "PlannerConv32", "conv_batched", "conv_f64_with_planner", "conv_f32_with_planner", "fftconvolve",
    "correlate",
    "PlannerConvNd64", "PlannerConvNd32", "convnd_batched", "convnd_f64_with_planner", "convnd_f32_with_planner",
    "fftconvolve_nd", "correlate_nd",
    "PlannerCzt64", "PlannerCzt32", "czt_batched", "czt_64", "czt_32", "czt_64_with_planner", "czt_32_with_planner", "czt",
    "zoom_fft",
    "PlannerNufft64", "PlannerNufft32", "nufft1_batched", "nufft2_batched", "nufft1_64", "nufft1_32", "nufft2_64", "nufft2_32",
    "nufft1_64_with_planner", "nufft1_32_with_planner", "nufft2_64_with_planner", "nufft2_32_with_planner", "nufft1", "nufft2",
    "PlannerNufft2d64", "PlannerNufft2d32", "nufft2d1_batched", "nufft2d2_batched", "nufft2d1_64", "nufft2d1_32", "nufft2d2_64",
    "nufft2d2_32", "nufft2d1_64_with_planner", "nufft2d1_32_with_planner", "nufft2d2_64_with_planner", "nufft2d2_32_with_planner",
    "nufft2d1", "nufft2d2",
    "PlannerNufft3d64", "PlannerNufft3d32", "nufft3d1_batched", "nufft3d2_batched", "nufft3d1_64", "nufft3d1_32", "nufft3d2_64",
    "nufft3d2_32", "nufft3d1_64_with_planner", "nufft3d1_32_with_planner", "nufft3d2_64_with_planner", "nufft3d2_32_with_planner",
    "nufft3d1", "nufft3d2",
    "PlannerNufftT3_64", "PlannerNufftT3_32", "nufft3_batched", "nufft3_64", "nufft3_32", "nufft3_64_with_planner",
    "nufft3_32_with_planner", "nufft3",
    "PlannerNd64", "PlannerNd32", "fft_64_nd", "fft_32_nd", "fft_64_nd_with_planner", "fft_32_nd_with_planner", "fft_nd_batched",
    "PlannerR2cNd64", "PlannerR2cNd32", "r2c_fft_f64_nd", "r2c_fft_f32_nd", "r2c_fft_f64_nd_with_planner",
    "r2c_fft_f32_nd_with_planner", "c2r_fft_f64_nd", "c2r_fft_f32_nd", "c2r_fft_f64_nd_with_planner",
    "c2r_fft_f32_nd_with_planner", "r2c_nd_batched", "c2r_nd_batched",
]


class Direction(enum.IntEnum):
    """planner.rs:10-16"""

    Forward = 1
    Reverse = -1


class PlannerMode(enum.IntEnum):
    """planner.rs:24-32.  ``Tune``: the planner times the plans that exist for its length on the device at plan time and
    keeps the fastest (one transform per call; :meth:`PlannerDit64.tune` for other batch sizes and call kinds)."""

    Heuristic = 0
    Tune = 1


class TuneKind(enum.IntEnum):
    """PHAST_TUNE_* (include/phastft_hip.h): which call a tuning run measures."""

    C2C = 0
    C2CInterleaved = 1
    R2C = 2
    C2R = 3


def _tune(planner, batch: int, kind: "TuneKind") -> dict:
    rep = _lib.PhastTuneReport()
    _check(planner._fn("tune")(planner._h, batch, int(kind), C.byref(rep)))
    return {"adopted": bool(rep.adopted), "candidates": int(rep.candidates), "us_heuristic": float(rep.us_heuristic),
            "us_best": float(rep.us_best), "seconds": float(rep.seconds), "plan": rep.plan.decode()}


def wisdom_count(layer: int = -1) -> int:
    """Entries of a wisdom layer: 0 built-in, 1 PHAST_WISDOM file, 2 imported, 3 measured by this process; -1 all."""
    return int(_call("phast_wisdom_count", layer))


def wisdom_export() -> str:
    """What this process measured, imported or read from PHAST_WISDOM, as text (csrc/wisdom.hpp) -- without the built-in layer."""
    need = C.c_size_t(0)
    _check(_call("phast_wisdom_export", None, 0, C.byref(need)))
    buf = C.create_string_buffer(need.value)
    _check(_call("phast_wisdom_export", buf, need.value, None))
    return buf.value.decode()


def wisdom_import(text: str) -> None:
    """Planners created afterwards start with the plans the text names."""
    _check(_call("phast_wisdom_import", text.encode()))


def wisdom_forget() -> None:
    _call("phast_wisdom_forget")


def wisdom_builtin(enable: bool) -> bool:
    """The wisdom compiled into the library (csrc/builtin_wisdom.inc) off / on for planners made afterwards.  Returns what it
    was before (PHAST_BUILTIN_WISDOM=0 starts it off): `was = wisdom_builtin(False) ... wisdom_builtin(was)` puts it back."""
    return bool(_call("phast_wisdom_builtin", 1 if enable else 0))


ERR_INVALID_ARG = 16  # PHAST_ERR_INVALID_ARG (include/phastft_hip.h): e.g. a shape the strided kernels do not cover


class PhastPanic(AssertionError):
    """A reference ``assert!`` / ``assert_eq!`` would have fired; ``str(e)`` is the reference's message."""

    def __init__(self, code: int, message: str):
        super().__init__(message)
        self.code = code


class PhastHipError(RuntimeError):
    """The HIP runtime failed or no GPU is visible (codes 14/15 of phastft_hip.h)."""

    def __init__(self, code: int, message: str):
        super().__init__(message)
        self.code = code


def _check(rc: int) -> None:
    if rc == 0:
        return
    l = _lib.lib()
    msg = l.phast_strerror(rc).decode()
    if rc in (13, 14, 15):
        raise PhastHipError(rc, f"{msg}: {l.phast_last_hip_error().decode()}")
    raise PhastPanic(rc, msg)


def _call(name: str, *args):
    """The library's function ``name`` on ``args``, converted by the signature _lib took from the header.  An argument ctypes
    cannot convert (a float or ``None`` where a count belongs) is a :class:`TypeError`, as from the scalar types themselves."""
    try:
        return getattr(_lib.lib(), name)(*args)
    except C.ArgumentError as e:
        raise TypeError(str(e)) from None


@dataclass
class Options:
    """options.rs:8-43.  CPU threading knobs: carried for source compatibility, ignored on the GPU."""

    multithreaded_bit_reversal: bool = False
    smallest_parallel_chunk_size: int = 16384

    @staticmethod
    def guess_options(input_size: int) -> "Options":
        o = _lib.PhastOptions()
        _check(_call("phast_options_guess", input_size, C.byref(o)))
        return Options(bool(o.multithreaded_bit_reversal), int(o.smallest_parallel_chunk_size))

    def _c(self) -> _lib.PhastOptions:
        return _lib.PhastOptions(int(self.multithreaded_bit_reversal), self.smallest_parallel_chunk_size)


# ---------------------------------------------------------------------------------------------
# slices
# ---------------------------------------------------------------------------------------------
def _is_torch(x) -> bool:
    return type(x).__module__.split(".")[0] == "torch"


class _Slice:
    """pointer + length + where it lives, for a numpy array or a torch tensor"""

    __slots__ = ("ptr", "len", "dev", "keep")

    def __init__(self, x, dtype, what: str):
        if _is_torch(x):
            import torch

            want = torch.float64 if dtype == np.float64 else torch.float32
            if x.dtype != want or x.dim() != 1 or not x.is_contiguous():
                raise TypeError(f"{what}: need a contiguous 1-D {want} tensor")
            self.dev = x.device.type == "cuda"
            if not self.dev:
                raise TypeError(f"{what}: torch tensors must live on the GPU (use numpy arrays for host slices)")
            self.ptr = C.c_void_p(x.data_ptr())
            self.len = x.numel()
        elif isinstance(x, np.ndarray):
            if x.dtype != dtype or x.ndim != 1 or not x.flags.c_contiguous:
                raise TypeError(f"{what}: need a contiguous 1-D {np.dtype(dtype).name} ndarray")
            self.dev = False
            self.ptr = x.ctypes.data_as(C.c_void_p)
            self.len = x.size
        else:
            raise TypeError(f"{what}: need a numpy.ndarray (host) or a torch cuda tensor (device)")
        self.keep = x


def _stream() -> C.c_void_p:
    import torch

    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _same_place(*slices: _Slice) -> bool:
    dev = slices[0].dev
    if any(s.dev != dev for s in slices):
        raise TypeError("all slices of one call must be host arrays or all device tensors")
    return dev


# ---------------------------------------------------------------------------------------------
# planners
# ---------------------------------------------------------------------------------------------
class _Handle:
    """an object of the library behind an opaque pointer: {_stem}{_prefix}{_sfx}_* of include/phastft_hip.h"""
    _stem = "phast_planner_"
    _sfx = "64"
    _dtype = np.float64

    def _new(self, *args, ctor: str = "new") -> None:
        self._h = C.c_void_p()
        _check(self._fn(ctor)(*args, C.byref(self._h)))

    def _fn(self, name: str):
        return functools.partial(_call, f"{self._stem}{self._prefix}{self._sfx}_{name}")

    def __del__(self):
        try:
            if getattr(self, "_h", None) is not None and self._h.value and _lib is not None and _lib._lib is not None:
                getattr(_lib._lib, f"{self._stem}{self._prefix}{self._sfx}_free")(self._h)
                self._h.value = None
        except Exception:  # interpreter shutdown: modules may already be gone
            pass

    def describe(self) -> str:
        buf = C.create_string_buffer(16384)   # (a planner may carry a dozen wisdom plans besides its static ones)
        _check(self._fn("describe")(self._h, buf, 16384))
        return buf.value.decode()

    def device_bytes(self) -> int:
        return int(self._fn("device_bytes")(self._h))

    def _workspace_len(self, batch: int) -> int:
        return int(self._fn("workspace_len")(self._h, batch))


class _PlannerDit(_Handle):
    _prefix = "dit"

    def __init__(self, num_points: int, mode: PlannerMode = PlannerMode.Heuristic):
        self._new(num_points, int(mode), ctor="with_mode")
        self.num_points = num_points

    @classmethod
    def new(cls, num_points: int):
        """planner.rs:55"""
        return cls(num_points)

    @classmethod
    def with_mode(cls, num_points: int, mode: PlannerMode):
        """planner.rs:65"""
        return cls(num_points, mode)

    # ---- MI355X-side extras (no reference counterpart) ----
    def describe_call(self, batch: int = 1, kind: "TuneKind" = 0) -> str:
        """The plan a call with ``batch`` transforms runs: ``"<which> [rows x cols ...]..."`` (the library's own answer)."""
        buf = C.create_string_buffer(512)
        _check(self._fn("describe_call")(self._h, batch, int(kind), buf, 512))
        return buf.value.decode()

    def check_guards(self) -> int:
        """debug: bytes of the scratch's guard bands overwritten since allocation (see :func:`debug_set_guard_bytes`)"""
        bad = C.c_size_t(0)
        _check(self._fn("debug_check_guards")(self._h, C.byref(bad)))
        return int(bad.value)

    def reserve_batch(self, max_batch: int) -> None:
        _check(self._fn("reserve_batch")(self._h, max_batch))

    def release_graph_workspaces(self) -> int:
        """Hand back the workspaces captured graphs worked in (every graph captured on this planner must be gone)."""
        return int(self._fn("release_graph_workspaces")(self._h))

    def tune(self, batch: int = 1, kind: TuneKind = TuneKind.C2C) -> dict:
        """PlannerMode::Tune for ``batch`` transforms per call (covers batches in (2^(b-1), 2^b]) and the call kind
        ``TuneKind.C2C`` / ``C2CInterleaved``: measures on the device, installs the winner, returns the report."""
        return _tune(self, batch, kind)

    def set_plan(self, log_rows=(), tile_log=12, points_log=4) -> None:
        """Force the pass factorisation (tuning hook); ``()`` restores the heuristic.  ``tile_log`` is
        log2(points per tile): one int for all passes or one per pass; ``points_log`` = log2(points per thread)."""
        n = len(log_rows)
        tls = [tile_log] * n if isinstance(tile_log, int) else list(tile_log)
        arr = (C.c_uint * max(1, n))(*log_rows)
        tarr = (C.c_uint * max(1, n))(*tls)
        _check(self._fn("set_plan")(self._h, arr, tarr, n, points_log))


    def time_passes(self, reals, imags, n: int, reps: int = 10):
        """Average HIP-event duration (ms) of every pass kernel over ``reps`` forward transforms of the
        device tensors (``len/n`` transforms, transformed in place).  Measurement hook for bench.py."""
        re, im = _Slice(reals, self._dtype, "reals"), _Slice(imags, self._dtype, "imags")
        ms = (C.c_float * 3)()
        npass = C.c_int()
        _check(self._fn("time_passes")(self._h, re.ptr, im.ptr, re.len // n, n, reps, ms, C.byref(npass), _stream()))
        return [float(ms[i]) for i in range(npass.value)]


class PlannerDit64(_PlannerDit):
    """planner.rs:34-114 (f64)"""


class PlannerDit32(_PlannerDit):
    """planner.rs:34-114 (f32)"""

    _sfx = "32"
    _dtype = np.float32


class _PlannerR2c(_Handle):
    _prefix = "r2c"

    def __init__(self, n: int, mode: PlannerMode = PlannerMode.Heuristic):
        self._new(n, int(mode), ctor="with_mode")
        self.n = n

    @classmethod
    def new(cls, n: int):
        """planner.rs:194"""
        return cls(n)

    @classmethod
    def with_mode(cls, n: int, mode: PlannerMode):
        """(no reference counterpart: the PlannerDit*::with_mode switch for the real transforms)"""
        return cls(n, mode)

    def describe_call(self, batch: int = 1, kind: "TuneKind" = 2) -> str:
        """The plan of the inner transform an ``r2c_fft`` / ``c2r_fft`` call with ``batch`` transforms runs."""
        buf = C.create_string_buffer(512)
        _check(self._fn("describe_call")(self._h, batch, int(kind), buf, 512))
        return buf.value.decode()

    def check_guards(self) -> int:
        """debug: bytes of the guard bands around the inner planner's scratches overwritten since allocation (see
        :func:`debug_set_guard_bytes`)"""
        bad = C.c_size_t(0)
        _check(self._fn("debug_check_guards")(self._h, C.byref(bad)))
        return int(bad.value)

    def tune(self, batch: int = 1, kind: TuneKind = TuneKind.R2C) -> dict:
        """PlannerMode::Tune for ``batch`` real transforms per call, ``TuneKind.R2C`` or ``TuneKind.C2R``."""
        return _tune(self, batch, kind)

    def describe(self) -> str:
        """Plan of the inner N/2-point complex transform."""
        return super().describe()

    def set_plan(self, log_rows=(), tile_log=12, points_log=4) -> None:
        """Force the pass factorisation of the inner N/2-point transform (tuning hook, as ``PlannerDit*.set_plan``);
        ``()`` restores the library's own plans."""
        n = len(log_rows)
        tls = [tile_log] * n if isinstance(tile_log, int) else list(tile_log)
        arr = (C.c_uint * max(1, n))(*log_rows)
        tarr = (C.c_uint * max(1, n))(*tls)
        _check(self._fn("set_inner_plan")(self._h, arr, tarr, n, points_log))

    def time_passes(self, input_re, output_re, output_im, reps: int = 10):
        """Average HIP-event duration (ms) of every kernel of one R2C transform of the device tensors: the passes of the
        inner N/2-point transform, then the untangle sweep.  Measurement hook for bench.py."""
        i, ore, oim = (_Slice(x, self._dtype, w) for x, w in ((input_re, "input_re"), (output_re, "output_re"),
                                                              (output_im, "output_im")))
        ms = (C.c_float * 4)()
        npass = C.c_int()
        _check(self._fn("time_passes")(self._h, i.ptr, ore.ptr, oim.ptr, 1, self.n, self.n // 2 + 1, reps, ms,
                                       C.byref(npass), _stream()))
        return [float(ms[k]) for k in range(npass.value)]


    def time_c2r_passes(self, input_re, input_im, output, reps: int = 10):
        """The same for one C2R transform: the passes of the inner transform (the first one forms z on load where its
        fused form exists), then the preprocess sweep where it does not."""
        ire, iim, out = (_Slice(x, self._dtype, w) for x, w in ((input_re, "input_re"), (input_im, "input_im"), (output, "output")))
        ms = (C.c_float * 4)()
        npass = C.c_int()
        _check(self._fn("time_c2r_passes")(self._h, ire.ptr, iim.ptr, out.ptr, 1, self.n // 2 + 1, self.n, reps, ms,
                                           C.byref(npass), _stream()))
        return [float(ms[k]) for k in range(npass.value)]


class PlannerR2c64(_PlannerR2c):
    """planner.rs:164-212 (f64)"""


class PlannerR2c32(_PlannerR2c):
    """planner.rs:164-212 (f32)"""

    _sfx = "32"
    _dtype = np.float32


# ---------------------------------------------------------------------------------------------
# C2C  (lib.rs:143-226, algorithms/dit.rs:263,338)
# ---------------------------------------------------------------------------------------------
def _fft(sfx, dtype, reals, imags, direction, planner=None, opts=None, need_opts=False):
    re, im = _Slice(reals, dtype, "reals"), _Slice(imags, dtype, "imags")
    direction = int(direction)
    if _same_place(re, im):
        # device-resident: the Rust asserts are re-checked here, then the batched _dev entry point is used
        own = planner is None
        if own:
            planner = (PlannerDit64 if sfx == "64" else PlannerDit32)(re.len)  # lib.rs:181: planner from reals.len()
        if re.len != im.len:
            _check(2)
        _check(_call(f"phast_fft_{sfx}_dit_dev", re.ptr, im.ptr, re.len, 1, re.len, direction, planner._h, _stream()))
        if own:
            import torch

            torch.cuda.current_stream().synchronize()  # the temporary planner's scratch dies with it
        return
    args = [re.ptr, re.len, im.ptr, im.len, direction]
    if planner is None:
        _check(_call(f"phast_fft_{sfx}_dit", *args))
    elif need_opts:
        _check(_call(f"phast_fft_{sfx}_dit_with_planner_and_opts", *args, planner._h, C.byref(opts._c())))
    else:
        _check(_call(f"phast_fft_{sfx}_dit_with_planner", *args, planner._h))


def fft_64_dit(reals, imags, direction: Direction) -> None:
    """lib.rs:180"""
    _fft("64", np.float64, reals, imags, direction)


def fft_32_dit(reals, imags, direction: Direction) -> None:
    """lib.rs:223"""
    _fft("32", np.float32, reals, imags, direction)


def fft_64_dit_with_planner(reals, imags, direction: Direction, planner: PlannerDit64) -> None:
    """lib.rs:143"""
    _fft("64", np.float64, reals, imags, direction, planner)


def fft_32_dit_with_planner(reals, imags, direction: Direction, planner: PlannerDit32) -> None:
    """lib.rs:186"""
    _fft("32", np.float32, reals, imags, direction, planner)


def fft_64_dit_with_planner_and_opts(reals, imags, direction: Direction, planner: PlannerDit64, opts: Options) -> None:
    """algorithms/dit.rs:263"""
    _fft("64", np.float64, reals, imags, direction, planner, opts, True)


def fft_32_dit_with_planner_and_opts(reals, imags, direction: Direction, planner: PlannerDit32, opts: Options) -> None:
    """algorithms/dit.rs:338"""
    _fft("32", np.float32, reals, imags, direction, planner, opts, True)


# ---------------------------------------------------------------------------------------------
# interleaved Complex<T> signals  (lib.rs:41-140, feature `complex-nums`)
# ---------------------------------------------------------------------------------------------
def _fft_interleaved(sfx, cdtype, signal, direction, planner=None, opts=None, need_opts=False):
    fdtype = np.float64 if sfx == "64" else np.float32
    if _is_torch(signal):
        import torch

        want = torch.complex128 if sfx == "64" else torch.complex64
        if signal.dtype != want or signal.dim() != 1 or not signal.is_contiguous() or signal.device.type != "cuda":
            raise TypeError(f"signal: need a contiguous 1-D {want} cuda tensor")
        n = signal.numel()
        own = planner is None
        if own:
            planner = (PlannerDit64 if sfx == "64" else PlannerDit32)(n)
        _check(_call(f"phast_fft_{sfx}_interleaved_dev", signal.data_ptr(), n, 1, n, int(direction), planner._h, _stream()))
        if own:
            torch.cuda.current_stream().synchronize()
        return
    if not (isinstance(signal, np.ndarray) and signal.dtype == cdtype and signal.ndim == 1 and signal.flags.c_contiguous):
        raise TypeError(f"signal: need a contiguous 1-D {np.dtype(cdtype).name} ndarray or a cuda tensor")
    flat = signal.view(fdtype)
    args = [flat.ctypes.data_as(C.c_void_p), signal.size, int(direction)]
    if planner is None:
        _check(_call(f"phast_fft_{sfx}_interleaved", *args))
    elif need_opts:
        _check(_call(f"phast_fft_{sfx}_interleaved_with_planner_and_opts", *args, planner._h, C.byref(opts._c())))
    else:
        _check(_call(f"phast_fft_{sfx}_interleaved_with_planner", *args, planner._h))


def fft_64_interleaved(signal, direction: Direction) -> None:
    """lib.rs:120 (macro impl_fft_interleaved)"""
    _fft_interleaved("64", np.complex128, signal, direction)


def fft_32_interleaved(signal, direction: Direction) -> None:
    """lib.rs:120"""
    _fft_interleaved("32", np.complex64, signal, direction)


def fft_64_interleaved_with_planner(signal, direction: Direction, planner: PlannerDit64) -> None:
    """lib.rs:87"""
    _fft_interleaved("64", np.complex128, signal, direction, planner)


def fft_32_interleaved_with_planner(signal, direction: Direction, planner: PlannerDit32) -> None:
    """lib.rs:87"""
    _fft_interleaved("32", np.complex64, signal, direction, planner)


def fft_64_interleaved_with_planner_and_opts(signal, direction: Direction, planner: PlannerDit64, opts: Options) -> None:
    """lib.rs:50"""
    _fft_interleaved("64", np.complex128, signal, direction, planner, opts, True)


def fft_32_interleaved_with_planner_and_opts(signal, direction: Direction, planner: PlannerDit32, opts: Options) -> None:
    """lib.rs:50"""
    _fft_interleaved("32", np.complex64, signal, direction, planner, opts, True)


def fft_dit_batched(reals, imags, n: int, direction: Direction, planner, dist: int | None = None) -> None:
    """Device-resident batch: transform b lives at ``[b*dist, b*dist + n)`` of ``reals``/``imags`` (``dist`` defaults
    to ``n``: transforms back to back).  No reference counterpart -- the reference loops over transforms on the CPU."""
    dtype, sfx = planner._dtype, planner._sfx
    re, im = _Slice(reals, dtype, "reals"), _Slice(imags, dtype, "imags")
    if not _same_place(re, im):
        raise TypeError("fft_dit_batched needs device tensors")
    if re.len != im.len:
        _check(2)
    dist = n if dist is None else dist
    if n == 0 or dist < n or re.len < n or (re.len - n) % dist:
        raise ValueError("length must be (batch-1)*dist + n")
    batch = (re.len - n) // dist + 1
    _check(_call(f"phast_fft_{sfx}_dit_dev", re.ptr, im.ptr, n, batch, dist, int(direction), planner._h, _stream()))



# ---------------------------------------------------------------------------------------------
# any length N >= 1 (Bluestein on the power-of-two engine; no reference counterpart -- the reference takes powers of two only)
# ---------------------------------------------------------------------------------------------
class _AnyHandle(_Handle):
    """the handle of an any-length planner: phast_planner_{_prefix}{_sfx}_*"""
    _prefix = "any"

    def __init__(self, n: int):
        self._new(n)
        self.n = n

    def _time(self, name: str, bufs, counts, batch: int, workspace, reps: int):
        """the five stage times of a *_time_*stages call: (handle, buffers, counts, workspace, reps, ms, stream)"""
        ws = _any_workspace(self, batch, workspace)
        ms = (C.c_float * 5)()
        _check(self._fn(name)(self._h, *(b.ptr for b in bufs), *counts, ws.ptr, ws.len, reps, ms, _stream()))
        return [float(x) for x in ms]


class _PlannerAny(_AnyHandle):
    def __init__(self, n: int):
        super().__init__(n)
        # the convolution length: the smallest power of two >= 2N - 1 (N itself for a power of two)
        self.m = n if n & (n - 1) == 0 else 1 << (2 * n - 2).bit_length()

    def workspace_len(self, batch: int = 1) -> int:
        """Elements of T a device call of ``batch`` transforms works in: 2 M batch (0 for a power of two).  A smaller
        workspace of at least 2 M runs the batch in chunks."""
        return self._workspace_len(batch)

    def time_stages(self, reals, imags, batch: int = 1, dist: int | None = None, workspace=None, reps: int = 10):
        """Average HIP-event milliseconds of the five stages of a forward call on device tensors -- chirp-pad sweep, forward
        M-point transform, spectrum sweep, inverse M-point transform, chirp-post sweep (measurement hook)."""
        re, im = _Slice(reals, self._dtype, "reals"), _Slice(imags, self._dtype, "imags")
        return self._time("time_stages", (re, im), (batch, self.n if dist is None else dist), batch, workspace, reps)


class PlannerAny64(_PlannerAny):
    """f64 transforms of any length 1 <= N <= 2^29"""


class PlannerAny32(_PlannerAny):
    """f32 transforms of any length 1 <= N <= 2^29 (the table is built in f64 and rounded)"""

    _sfx = "32"
    _dtype = np.float32


def _any_workspace(planner, batch: int, workspace=None) -> _Slice:
    """the caller's device workspace, or one from torch's allocator on the current stream (stream-ordered: free to reuse
    once the call's work is done)"""
    if workspace is None:
        import torch

        workspace = torch.empty(max(1, planner.workspace_len(batch)),
                                dtype=torch.float64 if planner._dtype == np.float64 else torch.float32, device="cuda")
    ws = _Slice(workspace, planner._dtype, "workspace")
    if not ws.dev:
        raise TypeError("workspace: need a device tensor")
    return ws


def _fft_any(sfx, dtype, reals, imags, direction, planner=None):
    re, im = _Slice(reals, dtype, "reals"), _Slice(imags, dtype, "imags")
    direction = int(direction)
    if _same_place(re, im):
        if re.len != im.len:
            _check(2)
        own = planner is None
        if own:
            planner = (PlannerAny64 if sfx == "64" else PlannerAny32)(re.len)
        ws = _any_workspace(planner, 1)
        _check(_call(f"phast_fft_{sfx}_any_dev", re.ptr, im.ptr, re.len, 1, re.len, direction, planner._h, ws.ptr, ws.len,
                     _stream()))
        if own:
            import torch

            torch.cuda.current_stream().synchronize()  # the temporary planner's tables die with it
        return
    args = [re.ptr, re.len, im.ptr, im.len, direction]
    if planner is None:
        _check(_call(f"phast_fft_{sfx}_any", *args))
    else:
        _check(_call(f"phast_fft_{sfx}_any_with_planner", *args, planner._h))


def fft_64_any(reals, imags, direction: Direction) -> None:
    """In-place f64 DFT of any length N = len(reals) (Reverse scales by 1/N), as fft_64_dit for powers of two"""
    _fft_any("64", np.float64, reals, imags, direction)


def fft_32_any(reals, imags, direction: Direction) -> None:
    """f32 twin of :func:`fft_64_any`"""
    _fft_any("32", np.float32, reals, imags, direction)


def fft_64_any_with_planner(reals, imags, direction: Direction, planner: PlannerAny64) -> None:
    _fft_any("64", np.float64, reals, imags, direction, planner)


def fft_32_any_with_planner(reals, imags, direction: Direction, planner: PlannerAny32) -> None:
    _fft_any("32", np.float32, reals, imags, direction, planner)


def fft_any_batched(reals, imags, n: int, direction: Direction, planner, dist: int | None = None, workspace=None) -> None:
    """Device-resident batch of any-length transforms: transform b at ``[b*dist, b*dist + n)`` (``dist`` defaults to ``n``).
    ``workspace``: a device tensor of the planner's type, at least ``planner.workspace_len(1)`` elements (fewer than
    ``planner.workspace_len(batch)`` runs the batch in chunks); by default one from torch's allocator."""
    dtype, sfx = planner._dtype, planner._sfx
    re, im = _Slice(reals, dtype, "reals"), _Slice(imags, dtype, "imags")
    if not _same_place(re, im):
        raise TypeError("fft_any_batched needs device tensors")
    if re.len != im.len:
        _check(2)
    dist = n if dist is None else dist
    if n == 0 or dist < n or re.len < n or (re.len - n) % dist:
        raise ValueError("length must be (batch-1)*dist + n")
    batch = (re.len - n) // dist + 1
    ws = _any_workspace(planner, batch, workspace)
    _check(_call(f"phast_fft_{sfx}_any_dev", re.ptr, im.ptr, n, batch, dist, int(direction), planner._h, ws.ptr, ws.len,
                 _stream()))


# ---------------------------------------------------------------------------------------------
# real transforms of any length N >= 1 (no reference counterpart: r2c.rs takes powers of two >= 4)
# ---------------------------------------------------------------------------------------------
class _PlannerR2cAny(_AnyHandle):
    _prefix = "r2c_any"

    def __init__(self, n: int):
        super().__init__(n)
        self.half = n // 2
        self.m = self.workspace_len(1) // 2  # the inner convolution length (0: a power of two >= 4, N = 1, 2)

    def workspace_len(self, batch: int = 1) -> int:
        """Elements of T a device call of ``batch`` transforms works in: 2 M batch (0 for a power of two, N = 1 or 2).  A
        smaller workspace of at least 2 M runs the batch in chunks."""
        return self._workspace_len(batch)

    def time_stages(self, input_re, output_re, output_im, batch: int = 1, workspace=None, reps: int = 10):
        """Average HIP-event milliseconds of the five stages of an R2C call on device tensors -- pad sweep, forward M-point
        transform, spectrum sweep, inverse M-point transform, post sweep (measurement hook)"""
        i, ore, oim = (_Slice(x, self._dtype, w) for x, w in ((input_re, "input_re"), (output_re, "output_re"),
                                                               (output_im, "output_im")))
        return self._time("time_stages", (i, ore, oim), (batch,), batch, workspace, reps)

    def time_c2r_stages(self, input_re, input_im, output, batch: int = 1, workspace=None, reps: int = 10):
        """:meth:`time_stages` of a C2R call"""
        ire, iim, out = (_Slice(x, self._dtype, w) for x, w in ((input_re, "input_re"), (input_im, "input_im"),
                                                                 (output, "output")))
        return self._time("time_c2r_stages", (ire, iim, out), (batch,), batch, workspace, reps)


class PlannerR2cAny64(_PlannerR2cAny):
    """f64 real transforms (R2C / C2R) of any length 1 <= N <= 2^29"""


class PlannerR2cAny32(_PlannerR2cAny):
    """f32 real transforms (R2C / C2R) of any length 1 <= N <= 2^29"""

    _sfx = "32"
    _dtype = np.float32


def _r2c_any(fs, dtype, input_re, output_re, output_im, planner=None):
    i, ore, oim = _Slice(input_re, dtype, "input_re"), _Slice(output_re, dtype, "output_re"), _Slice(
        output_im, dtype, "output_im")
    sfx = fs[1:]
    if _same_place(i, ore, oim):
        own = planner is None
        if own:
            planner = (PlannerR2cAny64 if fs == "f64" else PlannerR2cAny32)(i.len)
        n, half = planner.n, planner.n // 2
        for code, got, want in ((5, i.len, n), (6, ore.len, half + 1), (7, oim.len, half + 1)):
            if got != want:
                _check(code)
        ws = _any_workspace(planner, 1)
        _check(_call(f"phast_r2c_fft_{fs}_any_dev", i.ptr, ore.ptr, oim.ptr, n, 1, n, half + 1, planner._h, ws.ptr, ws.len,
                     _stream()))
        if own:
            import torch

            torch.cuda.current_stream().synchronize()  # the temporary planner's tables die with it
        return
    args = [i.ptr, i.len, ore.ptr, ore.len, oim.ptr, oim.len]
    if planner is None:
        _check(_call(f"phast_r2c_fft_{fs}_any", *args))
    else:
        _check(_call(f"phast_r2c_fft_{fs}_any_with_planner", *args, planner._h))


def _c2r_any(fs, dtype, input_re, input_im, output, planner=None):
    ire, iim, out = _Slice(input_re, dtype, "input_re"), _Slice(input_im, dtype, "input_im"), _Slice(
        output, dtype, "output")
    if _same_place(ire, iim, out):
        own = planner is None
        if own:
            planner = (PlannerR2cAny64 if fs == "f64" else PlannerR2cAny32)(out.len)
        n, half = planner.n, planner.n // 2
        for code, got, want in ((8, out.len, n), (9, ire.len, half + 1), (10, iim.len, half + 1)):
            if got != want:
                _check(code)
        ws = _any_workspace(planner, 1)
        _check(_call(f"phast_c2r_fft_{fs}_any_dev", ire.ptr, iim.ptr, out.ptr, n, 1, half + 1, n, planner._h, ws.ptr,
                     ws.len, _stream()))
        if own:
            import torch

            torch.cuda.current_stream().synchronize()
        return
    args = [ire.ptr, ire.len, iim.ptr, iim.len, out.ptr, out.len]
    if planner is None:
        _check(_call(f"phast_c2r_fft_{fs}_any", *args))
    else:
        _check(_call(f"phast_c2r_fft_{fs}_any_with_planner", *args, planner._h))


def r2c_fft_f64_any(input_re, output_re, output_im) -> None:
    """f64 R2C of any length N = len(input_re): X[k], k = 0 .. N // 2, into planes of N // 2 + 1 (numpy.fft.rfft)"""
    _r2c_any("f64", np.float64, input_re, output_re, output_im)


def r2c_fft_f32_any(input_re, output_re, output_im) -> None:
    """f32 twin of :func:`r2c_fft_f64_any`"""
    _r2c_any("f32", np.float32, input_re, output_re, output_im)


def r2c_fft_f64_any_with_planner(input_re, output_re, output_im, planner: PlannerR2cAny64) -> None:
    _r2c_any("f64", np.float64, input_re, output_re, output_im, planner)


def r2c_fft_f32_any_with_planner(input_re, output_re, output_im, planner: PlannerR2cAny32) -> None:
    _r2c_any("f32", np.float32, input_re, output_re, output_im, planner)


def c2r_fft_f64_any(input_re, input_im, output) -> None:
    """f64 C2R of any length N = len(output), scaled by 1/N (numpy.fft.irfft(X, N) for a Hermitian spectrum)"""
    _c2r_any("f64", np.float64, input_re, input_im, output)


def c2r_fft_f32_any(input_re, input_im, output) -> None:
    """f32 twin of :func:`c2r_fft_f64_any`"""
    _c2r_any("f32", np.float32, input_re, input_im, output)


def c2r_fft_f64_any_with_planner(input_re, input_im, output, planner: PlannerR2cAny64) -> None:
    _c2r_any("f64", np.float64, input_re, input_im, output, planner)


def c2r_fft_f32_any_with_planner(input_re, input_im, output, planner: PlannerR2cAny32) -> None:
    _c2r_any("f32", np.float32, input_re, input_im, output, planner)


def _need(what: str, got: int, batch: int, dist: int, per: int) -> None:
    if batch and got < (batch - 1) * dist + per:
        raise ValueError(f"{what}: {got} elements, need (batch-1)*dist + {per} = {(batch - 1) * dist + per}")


def r2c_any_batched(input_re, output_re, output_im, planner, batch: int, in_dist: int | None = None,
                    out_dist: int | None = None, workspace=None) -> None:
    """Device-resident batch of any-length R2C transforms: input b at ``b*in_dist`` (default N), its half spectrum at
    ``b*out_dist`` (default N // 2 + 1); for N a power of two >= 4, ``in_dist`` must be even when ``batch > 1`` (the
    power-of-two path reads the input as pairs).  ``workspace``: a device tensor of the planner's type, at least
    ``planner.workspace_len(1)`` elements (fewer than ``planner.workspace_len(batch)`` runs the batch in chunks); by default
    one from torch's allocator."""
    dtype, fs = planner._dtype, "f64" if planner._dtype == np.float64 else "f32"
    i, ore, oim = (_Slice(x, dtype, w) for x, w in ((input_re, "input_re"), (output_re, "output_re"), (output_im, "output_im")))
    if not _same_place(i, ore, oim):
        raise TypeError("r2c_any_batched needs device tensors")
    n, h1 = planner.n, planner.n // 2 + 1
    in_dist = n if in_dist is None else in_dist
    out_dist = h1 if out_dist is None else out_dist
    _need("input_re", i.len, batch, in_dist, n)
    _need("output_re", ore.len, batch, out_dist, h1)
    _need("output_im", oim.len, batch, out_dist, h1)
    ws = _any_workspace(planner, batch, workspace)
    _check(_call(f"phast_r2c_fft_{fs}_any_dev", i.ptr, ore.ptr, oim.ptr, n, batch, in_dist, out_dist, planner._h, ws.ptr,
                 ws.len, _stream()))


def c2r_any_batched(input_re, input_im, output, planner, batch: int, in_dist: int | None = None,
                    out_dist: int | None = None, workspace=None) -> None:
    """Device-resident batch of any-length C2R transforms: half spectrum b at ``b*in_dist`` (default N // 2 + 1), its real
    signal at ``b*out_dist`` (default N; even when ``batch > 1`` for N a power of two >= 4); ``workspace`` as for
    :func:`r2c_any_batched`."""
    dtype, fs = planner._dtype, "f64" if planner._dtype == np.float64 else "f32"
    ire, iim, out = (_Slice(x, dtype, w) for x, w in ((input_re, "input_re"), (input_im, "input_im"), (output, "output")))
    if not _same_place(ire, iim, out):
        raise TypeError("c2r_any_batched needs device tensors")
    n, h1 = planner.n, planner.n // 2 + 1
    in_dist = h1 if in_dist is None else in_dist
    out_dist = n if out_dist is None else out_dist
    _need("input_re", ire.len, batch, in_dist, h1)
    _need("input_im", iim.len, batch, in_dist, h1)
    _need("output", out.len, batch, out_dist, n)
    ws = _any_workspace(planner, batch, workspace)
    _check(_call(f"phast_c2r_fft_{fs}_any_dev", ire.ptr, iim.ptr, out.ptr, n, batch, in_dist, out_dist, planner._h, ws.ptr,
                 ws.len, _stream()))


# ---------------------------------------------------------------------------------------------
# DCT / DST of types II and III, any length N >= 1 (no reference counterpart; scipy.fft.dct / dst / idct / idst)
# ---------------------------------------------------------------------------------------------
_NORMS = {None: 0, "backward": 0, "ortho": 1, "forward": 2}


def _norm_code(norm) -> int:
    if norm not in _NORMS:
        raise ValueError(f"norm must be None, 'backward', 'ortho' or 'forward', not {norm!r}")
    return _NORMS[norm]


class PlannerDct64(_AnyHandle):
    """f64 DCT / DST of types II and III of any length 1 <= N <= 2^29 (one planner serves all four and every norm)"""

    _prefix = "dct"

    def workspace_len(self, batch: int = 1) -> int:
        """Elements of T a device call of ``batch`` transforms works in.  Any workspace of at least ``workspace_len(1)``
        elements is legal: a smaller one than ``workspace_len(batch)`` runs the batch in chunks."""
        return self._workspace_len(batch)

    def time_stages(self, input, output, kind: str = "dct", type: int = 2, norm=None, batch: int = 1, workspace=None,
                    reps: int = 10):
        """Average HIP-event milliseconds of the pre sweep, the real transform and the post sweep of ``batch`` transforms at
        distance N on device tensors (measurement hook); ``kind`` is ``"dct"`` or ``"dst"``"""
        i, o = _Slice(input, self._dtype, "input"), _Slice(output, self._dtype, "output")
        ws = _any_workspace(self, batch, workspace)
        ms = (C.c_float * 3)()
        _check(self._fn("time_stages")(self._h, kind == "dst", type, _norm_code(norm), i.ptr, o.ptr, batch, ws.ptr, ws.len,
                                       reps, ms, _stream()))
        return [float(x) for x in ms]


class PlannerDct32(PlannerDct64):
    """f32 twin of :class:`PlannerDct64`"""

    _sfx = "32"
    _dtype = np.float32


def _r2r(kind, fs, dtype, input, output, type, norm, planner=None):
    i, o = _Slice(input, dtype, "input"), _Slice(output, dtype, "output")
    code = _norm_code(norm)
    if _same_place(i, o):
        if i.len != o.len:
            _check(2)
        own = planner is None
        if own:
            planner = (PlannerDct64 if fs == "f64" else PlannerDct32)(i.len)
        ws = _any_workspace(planner, 1)
        _check(_call(f"phast_{kind}_{fs}_dev", i.ptr, o.ptr, i.len, 1, i.len, o.len, type, code, planner._h, ws.ptr, ws.len,
                     _stream()))
        if own:
            import torch

            torch.cuda.current_stream().synchronize()
        return
    args = [i.ptr, i.len, o.ptr, o.len, type, code]
    if planner is None:
        _check(_call(f"phast_{kind}_{fs}", *args))
    else:
        _check(_call(f"phast_{kind}_{fs}_with_planner", *args, planner._h))


def dct_f64(input, output, type: int = 2, norm=None) -> None:
    """f64 DCT of ``type`` 2 or 3 of any length N = len(input) into ``output`` (scipy.fft.dct(input, type, norm=norm))"""
    _r2r("dct", "f64", np.float64, input, output, type, norm)


def dct_f32(input, output, type: int = 2, norm=None) -> None:
    """f32 twin of :func:`dct_f64`"""
    _r2r("dct", "f32", np.float32, input, output, type, norm)


def dst_f64(input, output, type: int = 2, norm=None) -> None:
    """f64 DST of ``type`` 2 or 3 of any length N = len(input) into ``output`` (scipy.fft.dst(input, type, norm=norm))"""
    _r2r("dst", "f64", np.float64, input, output, type, norm)


def dst_f32(input, output, type: int = 2, norm=None) -> None:
    """f32 twin of :func:`dst_f64`"""
    _r2r("dst", "f32", np.float32, input, output, type, norm)


def dct_f64_with_planner(input, output, planner: PlannerDct64, type: int = 2, norm=None) -> None:
    _r2r("dct", "f64", np.float64, input, output, type, norm, planner)


def dct_f32_with_planner(input, output, planner: PlannerDct32, type: int = 2, norm=None) -> None:
    _r2r("dct", "f32", np.float32, input, output, type, norm, planner)


def dst_f64_with_planner(input, output, planner: PlannerDct64, type: int = 2, norm=None) -> None:
    _r2r("dst", "f64", np.float64, input, output, type, norm, planner)


def dst_f32_with_planner(input, output, planner: PlannerDct32, type: int = 2, norm=None) -> None:
    _r2r("dst", "f32", np.float32, input, output, type, norm, planner)


def _r2r_batched(kind, input, output, planner, batch, type, norm, in_dist, out_dist, workspace):
    dtype = planner._dtype
    fs = "f64" if dtype == np.float64 else "f32"
    i, o = _Slice(input, dtype, "input"), _Slice(output, dtype, "output")
    if not _same_place(i, o):
        raise TypeError(f"{kind}_batched needs device tensors")
    n = planner.n
    in_dist = n if in_dist is None else in_dist
    out_dist = n if out_dist is None else out_dist
    _need("input", i.len, batch, in_dist, n)
    _need("output", o.len, batch, out_dist, n)
    ws = _any_workspace(planner, batch, workspace)
    _check(_call(f"phast_{kind}_{fs}_dev", i.ptr, o.ptr, n, batch, in_dist, out_dist, type, _norm_code(norm), planner._h,
                 ws.ptr, ws.len, _stream()))


def dct_batched(input, output, planner, batch: int, type: int = 2, norm=None, in_dist: int | None = None,
                out_dist: int | None = None, workspace=None) -> None:
    """Device-resident batch of DCTs: input b at ``b*in_dist``, output b at ``b*out_dist`` (both default N, any distance
    >= N).  ``output`` may be ``input`` itself with equal distances (in place).  ``workspace``: a device tensor of the
    planner's type of at least ``planner.workspace_len(1)`` elements (fewer than ``planner.workspace_len(batch)`` runs the
    batch in chunks); by default one from torch's allocator."""
    _r2r_batched("dct", input, output, planner, batch, type, norm, in_dist, out_dist, workspace)


def dst_batched(input, output, planner, batch: int, type: int = 2, norm=None, in_dist: int | None = None,
                out_dist: int | None = None, workspace=None) -> None:
    """:func:`dct_batched` for the DST"""
    _r2r_batched("dst", input, output, planner, batch, type, norm, in_dist, out_dist, workspace)


_INVERSE_NORM = {None: "forward", "backward": "forward", "ortho": "ortho", "forward": "backward"}


def _inverse(type: int, norm):
    """scipy's idct / idst: type t with norm backward / ortho / forward is the transform of type 5 - t with norm forward /
    ortho / backward"""
    _norm_code(norm)
    if type not in (2, 3):
        raise ValueError(f"type must be 2 or 3, not {type!r}")
    return 5 - type, _INVERSE_NORM[norm]


def idct(input, output, type: int = 2, norm=None, planner=None) -> None:
    """scipy.fft.idct of ``type`` 2 or 3: :func:`dct_f64` / :func:`dct_f32` (by the dtype of ``input``) of type 5 - type with
    the norm swapped between backward and forward"""
    t, nm = _inverse(type, norm)
    _r2r_by_dtype("dct", input, output, t, nm, planner)


def idst(input, output, type: int = 2, norm=None, planner=None) -> None:
    """scipy.fft.idst: :func:`idct` for the DST"""
    t, nm = _inverse(type, norm)
    _r2r_by_dtype("dst", input, output, t, nm, planner)


def _r2r_by_dtype(kind, input, output, type, norm, planner):
    if planner is not None:
        dtype = planner._dtype
    elif _is_torch(input):
        import torch

        dtype = np.float64 if input.dtype == torch.float64 else np.float32
    else:
        dtype = np.float64 if np.asarray(input).dtype == np.float64 else np.float32
    fs = "f64" if dtype == np.float64 else "f32"
    _r2r(kind, fs, dtype, input, output, type, norm, planner)


# ---------------------------------------------------------------------------------------------
# the short-time Fourier transform and its inverse (no reference counterpart; torch.stft / torch.istft(length=L))
# ---------------------------------------------------------------------------------------------
_PADS = {"reflect": 0, "zero": 1, "constant": 1}


class PlannerStft64(_AnyHandle):
    """f64 STFT / inverse STFT of signals of ``signal_len`` samples: frames of ``n_fft`` samples ``hop`` apart, times
    ``window`` (``n_fft`` values; a shorter one is zero-padded on both sides as torch does; None: all ones).  ``center``
    pads the signal by ``n_fft // 2`` on both sides, by reflection (``pad_mode="reflect"``) or with zeros (``"zero"``).
    ``torch.stft(x, n_fft, hop, window=w, center=..., pad_mode=..., return_complex=True)`` is the transpose of the
    (frames, bins) planes; the inverse is ``torch.istft(..., length=signal_len)``."""

    _prefix = "stft"

    def __init__(self, signal_len: int, n_fft: int, hop: int, window=None, center: bool = True, pad_mode: str = "reflect"):
        if pad_mode not in _PADS:
            raise ValueError(f"pad_mode must be 'reflect' or 'zero', not {pad_mode!r}")
        wp = None
        if window is not None:
            if _is_torch(window):
                window = window.detach().cpu().numpy()
            w = np.ascontiguousarray(window, dtype=self._dtype).reshape(-1)
            if w.size > n_fft:
                raise ValueError(f"window: {w.size} values for n_fft = {n_fft}")
            if w.size < n_fft:  # win_length < n_fft: centred in the frame
                left = (n_fft - w.size) // 2
                w = np.concatenate([np.zeros(left, self._dtype), w, np.zeros(n_fft - w.size - left, self._dtype)])
            wp = w.ctypes.data_as(C.c_void_p)
        self._new(signal_len, n_fft, hop, wp, bool(center), _PADS[pad_mode])
        self.n = self.signal_len = signal_len
        self.n_fft, self.hop, self.center, self.pad_mode = n_fft, hop, bool(center), pad_mode
        self.frames = int(self._fn("frames")(self._h))
        self.bins = int(self._fn("bins")(self._h))
        self.envelope_min = float(self._fn("envelope_min")(self._h))

    def workspace_len(self, batch: int = 1) -> int:
        """Elements of T a device call of ``batch`` signals works in.  A smaller workspace runs the batch in chunks: of
        whole frames forward (at least ``workspace_min()``), of whole signals for the inverse (``workspace_min(True)``)."""
        return self._workspace_len(batch)

    def workspace_min(self, inverse: bool = False) -> int:
        return int(self._fn("workspace_min")(self._h, bool(inverse)))

    def time_stages(self, signal, re, im, inverse: bool = False, batch: int = 1, workspace=None, reps: int = 10):
        """Average HIP-event milliseconds of (the sweep, the real transform) of a forward or inverse call of ``batch``
        signals at distance L on device tensors (measurement hook)"""
        x, r, i = (_Slice(t, self._dtype, w) for t, w in ((signal, "signal"), (re, "re"), (im, "im")))
        ws = _any_workspace(self, batch, workspace)
        ms = (C.c_float * 2)()
        _check(self._fn("time_stages")(self._h, bool(inverse), x.ptr, r.ptr, i.ptr, batch, ws.ptr, ws.len, reps, ms,
                                       _stream()))
        return [float(v) for v in ms]


class PlannerStft32(PlannerStft64):
    """f32 twin of :class:`PlannerStft64`"""

    _sfx = "32"
    _dtype = np.float32


def _stft_batched(inverse, signal, re, im, planner, batch, sig_dist, workspace):
    dtype, fs = planner._dtype, "f64" if planner._dtype == np.float64 else "f32"
    x, r, i = (_Slice(t, dtype, w) for t, w in ((signal, "signal"), (re, "re"), (im, "im")))
    name = "istft" if inverse else "stft"
    if not _same_place(x, r, i):
        raise TypeError(f"{name}_batched needs device tensors")
    n, pts = planner.signal_len, planner.frames * planner.bins
    sig_dist = n if sig_dist is None else sig_dist
    _need("signal", x.len, batch, sig_dist, n)
    _need("re", r.len, batch, pts, pts)
    _need("im", i.len, batch, pts, pts)
    ws = _any_workspace(planner, batch, workspace)
    args = (r.ptr, i.ptr, x.ptr) if inverse else (x.ptr, r.ptr, i.ptr)
    _check(_call(f"phast_{name}_{fs}_dev", *args, n, batch, sig_dist, planner._h, ws.ptr, ws.len, _stream()))


def stft_batched(signal, out_re, out_im, planner, batch: int, sig_dist: int | None = None, workspace=None) -> None:
    """Device-resident batch of STFTs: signal b at ``b*sig_dist`` (default L, any distance >= L); frame f, bin k of signal b
    at ``(b*frames + f)*bins + k`` of the dense planes.  ``workspace``: a device tensor of the planner's type of at least
    ``planner.workspace_min()`` elements (fewer than ``planner.workspace_len(batch)`` runs the frames in chunks); by default
    one from torch's allocator."""
    _stft_batched(False, signal, out_re, out_im, planner, batch, sig_dist, workspace)


def istft_batched(in_re, in_im, signal, planner, batch: int, sig_dist: int | None = None, workspace=None) -> None:
    """Device-resident batch of inverse STFTs by weighted overlap-add (``torch.istft(..., length=L)``): the inverse of
    :func:`stft_batched`.  ``workspace``: at least ``planner.workspace_min(True)`` elements (one signal's frames).  A planner
    whose ``envelope_min`` is <= 1e-11 refuses (torch's NOLA rule)."""
    _stft_batched(True, signal, in_re, in_im, planner, batch, sig_dist, workspace)


def _stft_host(name, fs, dtype, a, b, c, planner):
    sl = [_Slice(t, dtype, w) for t, w in zip((a, b, c), ("signal", "re", "im") if name == "stft" else ("re", "im", "signal"))]
    if _same_place(*sl):
        raise TypeError(f"{name}_{fs}_with_planner takes host arrays ({name}_batched takes device tensors)")
    _check(_call(f"phast_{name}_{fs}_with_planner", *(v for s in sl for v in (s.ptr, s.len)), planner._h))


def stft_f64_with_planner(signal, out_re, out_im, planner: PlannerStft64) -> None:
    """f64 STFT of one host signal of L samples into host planes of frames * bins (blocking)"""
    _stft_host("stft", "f64", np.float64, signal, out_re, out_im, planner)


def stft_f32_with_planner(signal, out_re, out_im, planner: PlannerStft32) -> None:
    """f32 twin of :func:`stft_f64_with_planner`"""
    _stft_host("stft", "f32", np.float32, signal, out_re, out_im, planner)


def istft_f64_with_planner(in_re, in_im, signal, planner: PlannerStft64) -> None:
    """f64 inverse STFT of host planes of frames * bins into one host signal of L samples (blocking)"""
    _stft_host("istft", "f64", np.float64, in_re, in_im, signal, planner)


def istft_f32_with_planner(in_re, in_im, signal, planner: PlannerStft32) -> None:
    """f32 twin of :func:`istft_f64_with_planner`"""
    _stft_host("istft", "f32", np.float32, in_re, in_im, signal, planner)


# ---------------------------------------------------------------------------------------------
# the modified discrete cosine transform and its inverse (no reference counterpart, and none in torch or scipy)
# ---------------------------------------------------------------------------------------------
def mdct_window(name: str, n: int, dtype=np.float64, alpha: float = 4.0):
    """The 2N values of a window that reconstructs perfectly (w[j]^2 + w[j+N]^2 = 1, symmetric), as a numpy array of ``dtype``:
    ``"sine"`` sin(pi (j + 1/2) / (2N)), ``"vorbis"`` sin(pi/2 sin^2(pi (j + 1/2) / (2N))) or ``"kbd"``, the
    Kaiser-Bessel-derived window of ``alpha`` (the running sum of a Kaiser window of N + 1 points, beta = pi alpha)."""
    if n < 1:
        raise ValueError(f"n must be positive, not {n}")
    pi = np.longdouble("3.14159265358979323846264338327950288")
    t = (np.arange(n, dtype=np.longdouble) + 0.5) / (2 * n)  # the rising half; the other half mirrors it
    if name == "sine":
        half = np.sin(pi * t)
    elif name == "vorbis":
        half = np.sin(pi / 2 * np.sin(pi * t) ** 2)
    elif name == "kbd":
        j = np.arange(n + 1, dtype=np.float64)
        k = np.i0(np.pi * alpha * np.sqrt(1.0 - (2.0 * j / n - 1.0) ** 2)).astype(np.longdouble)
        half = np.sqrt(np.cumsum(k[:n]) / np.sum(k))
    else:
        raise ValueError(f"window must be 'sine', 'vorbis' or 'kbd', not {name!r}")
    return np.concatenate([half, half[::-1]]).astype(dtype)


class PlannerMdct64(_AnyHandle):
    """f64 MDCT / inverse MDCT of signals of ``signal_len`` samples: ``n`` coefficients (even) per frame of ``2 n`` samples,
    hop ``n``, times ``window`` (``2 n`` values; None: the sine window).  ``padded``: the signal is framed from ``-n`` on, so
    that every sample lies in two frames (``ceil(L / n) + 1`` frames) and a window with ``tdac_defect`` 0 reconstructs all of
    it; without, ``floor(L / n) - 1`` frames from sample 0 on reconstruct ``[n, frames * n)``.  Coefficients are (frames, n),
    row-major.  The forward transform is unscaled, the inverse carries 2 / n."""

    _prefix = "mdct"

    def __init__(self, signal_len: int, n: int, window=None, padded: bool = True):
        wp = None
        if window is not None:
            if _is_torch(window):
                window = window.detach().cpu().numpy()
            w = np.ascontiguousarray(window, dtype=self._dtype).reshape(-1)
            if w.size != 2 * n:
                raise ValueError(f"window: {w.size} values for 2 n = {2 * n}")
            wp = w.ctypes.data_as(C.c_void_p)
        self._new(signal_len, n, wp, bool(padded))
        self.signal_len, self.n, self.padded = signal_len, n, bool(padded)
        self.frames = int(self._fn("frames")(self._h))
        self.tdac_defect = float(self._fn("tdac_defect")(self._h))

    def workspace_len(self, batch: int = 1) -> int:
        """Elements of T a device call of ``batch`` signals works in.  A smaller workspace runs the batch in chunks: of
        whole frames forward (at least ``workspace_min()``), of whole signals for the inverse (``workspace_min(True)``)."""
        return self._workspace_len(batch)

    def workspace_min(self, inverse: bool = False) -> int:
        return int(self._fn("workspace_min")(self._h, bool(inverse)))

    def time_stages(self, signal, coefs, inverse: bool = False, batch: int = 1, workspace=None, reps: int = 10):
        """Average HIP-event milliseconds of (the pre sweep, the complex transform, the post sweep -- with the overlap-add
        for the inverse) of a call of ``batch`` signals at distance L on device tensors (measurement hook)"""
        x, c = _Slice(signal, self._dtype, "signal"), _Slice(coefs, self._dtype, "coefs")
        ws = _any_workspace(self, batch, workspace)
        ms = (C.c_float * 3)()
        _check(self._fn("time_stages")(self._h, bool(inverse), x.ptr, c.ptr, batch, ws.ptr, ws.len, reps, ms, _stream()))
        return [float(v) for v in ms]


class PlannerMdct32(PlannerMdct64):
    """f32 twin of :class:`PlannerMdct64`"""

    _sfx = "32"
    _dtype = np.float32


def _mdct_batched(inverse, signal, coefs, planner, batch, sig_dist, workspace):
    dtype, fs = planner._dtype, "f64" if planner._dtype == np.float64 else "f32"
    x, c = _Slice(signal, dtype, "signal"), _Slice(coefs, dtype, "coefs")
    name = "imdct" if inverse else "mdct"
    if not _same_place(x, c):
        raise TypeError(f"{name}_batched needs device tensors")
    n, pts = planner.signal_len, planner.frames * planner.n
    sig_dist = n if sig_dist is None else sig_dist
    _need("signal", x.len, batch, sig_dist, n)
    _need("coefs", c.len, batch, pts, pts)
    ws = _any_workspace(planner, batch, workspace)
    args = (c.ptr, x.ptr) if inverse else (x.ptr, c.ptr)
    _check(_call(f"phast_{name}_{fs}_dev", *args, n, batch, sig_dist, planner._h, ws.ptr, ws.len, _stream()))


def mdct_batched(signal, coefs, planner, batch: int, sig_dist: int | None = None, workspace=None) -> None:
    """Device-resident batch of MDCTs: signal b at ``b*sig_dist`` (default L, any distance >= L); coefficient k of frame t of
    signal b at ``(b*frames + t)*n + k``.  ``workspace``: a device tensor of the planner's type of at least
    ``planner.workspace_min()`` elements (fewer than ``planner.workspace_len(batch)`` runs the frames in chunks); by default
    one from torch's allocator.  The signal is not written."""
    _mdct_batched(False, signal, coefs, planner, batch, sig_dist, workspace)


def imdct_batched(coefs, signal, planner, batch: int, sig_dist: int | None = None, workspace=None) -> None:
    """Device-resident batch of inverse MDCTs by windowed overlap-add: the inverse of :func:`mdct_batched` where the planner's
    window has ``tdac_defect`` 0.  ``workspace``: at least ``planner.workspace_min(True)`` elements (one signal's frames).
    The coefficients are not written; every sample of [0, L) is (0 where no frame holds it)."""
    _mdct_batched(True, signal, coefs, planner, batch, sig_dist, workspace)


def _mdct_host(name, fs, dtype, a, b, planner):
    sl = [_Slice(t, dtype, w) for t, w in zip((a, b), ("signal", "coefs") if name == "mdct" else ("coefs", "signal"))]
    if _same_place(*sl):
        raise TypeError(f"{name}_{fs}_with_planner takes host arrays ({name}_batched takes device tensors)")
    _check(_call(f"phast_{name}_{fs}_with_planner", *(v for s in sl for v in (s.ptr, s.len)), planner._h))


def mdct_f64_with_planner(signal, coefs, planner: PlannerMdct64) -> None:
    """f64 MDCT of one host signal of L samples into a host array of frames * n coefficients (blocking)"""
    _mdct_host("mdct", "f64", np.float64, signal, coefs, planner)


def mdct_f32_with_planner(signal, coefs, planner: PlannerMdct32) -> None:
    """f32 twin of :func:`mdct_f64_with_planner`"""
    _mdct_host("mdct", "f32", np.float32, signal, coefs, planner)


def imdct_f64_with_planner(coefs, signal, planner: PlannerMdct64) -> None:
    """f64 inverse MDCT of a host array of frames * n coefficients into one host signal of L samples (blocking)"""
    _mdct_host("imdct", "f64", np.float64, coefs, signal, planner)


def imdct_f32_with_planner(coefs, signal, planner: PlannerMdct32) -> None:
    """f32 twin of :func:`imdct_f64_with_planner`"""
    _mdct_host("imdct", "f32", np.float32, coefs, signal, planner)


def _mdct_planner(t, length, n, window, padded):
    import torch

    if not _is_torch(t) or t.device.type != "cuda" or t.dtype not in (torch.float64, torch.float32):
        raise TypeError("need a float64 or float32 device tensor")
    dtype = np.float64 if t.dtype == torch.float64 else np.float32
    if isinstance(window, str):
        window = mdct_window(window, n, dtype)
    return (PlannerMdct64 if dtype == np.float64 else PlannerMdct32)(length, n, window, padded)


def mdct(x, n: int, window="sine", padded: bool = True):
    """The MDCT of one real device tensor of L samples with ``n`` coefficients per frame, through a planner of its own: a new
    device tensor of shape (frames, n).  ``window``: a name for :func:`mdct_window` or ``2 n`` values."""
    import torch

    planner = _mdct_planner(x, x.numel(), n, window, padded)
    out = torch.empty(planner.frames * n, dtype=x.dtype, device=x.device)
    mdct_batched(x.contiguous().reshape(-1), out, planner, 1)
    torch.cuda.current_stream().synchronize()  # the temporary planner's tables die with it
    return out.reshape(planner.frames, n)


def imdct(X, length: int, window="sine", padded: bool = True):
    """The inverse MDCT of one (frames, n) device tensor into a new device tensor of ``length`` samples: ``x`` again for
    ``X = mdct(x, n, window, padded)`` and a window of :func:`mdct_window`."""
    import torch

    if X.dim() != 2:
        raise ValueError("imdct needs a (frames, n) tensor")
    n = X.shape[1]
    planner = _mdct_planner(X, length, n, window, padded)
    if planner.frames != X.shape[0]:
        raise ValueError(f"{X.shape[0]} frames, but length = {length} with n = {n} has {planner.frames}")
    out = torch.empty(length, dtype=X.dtype, device=X.device)
    imdct_batched(X.contiguous().reshape(-1), out, planner, 1)
    torch.cuda.current_stream().synchronize()
    return out


# ---------------------------------------------------------------------------------------------
# Welch spectral estimation (no reference counterpart; scipy.signal.welch / csd / spectrogram / periodogram / coherence)
# ---------------------------------------------------------------------------------------------
_DETRENDS = {"constant": 1, "none": 0}
_SCALINGS = {"density": 0, "spectrum": 1}


def _detrend_code(detrend) -> int:
    if detrend is None or detrend is False:
        return 0
    if isinstance(detrend, str) and detrend in _DETRENDS:
        return _DETRENDS[detrend]
    raise ValueError(f"detrend must be 'constant', 'none', False or None, not {detrend!r} (linear detrending is out of scope)")


def _psd_window(window, nperseg: int):
    """the ``nperseg`` window values as float64, or None for the Hann window the library builds itself"""
    if window is None or (isinstance(window, str) and window in ("hann", "hanning")):
        return None
    if isinstance(window, str) and window in ("boxcar", "box", "ones", "rect", "rectangular"):
        return np.ones(nperseg, np.float64)
    if isinstance(window, (str, tuple, float, int)):
        try:
            from scipy.signal import get_window
        except ImportError:
            raise ValueError(f"window {window!r}: without scipy only 'hann', 'boxcar' and arrays are accepted") from None
        return np.ascontiguousarray(get_window(window, nperseg), dtype=np.float64)
    if _is_torch(window):
        window = window.detach().cpu().numpy()
    w = np.ascontiguousarray(window, dtype=np.float64).reshape(-1)
    if w.size != nperseg:
        raise ValueError(f"window: {w.size} values for nperseg = {nperseg}")
    return w


class PlannerPsd64(_AnyHandle):
    """f64 Welch spectral estimation of signals of ``signal_len`` samples, with scipy.signal's definitions: segments of
    ``nperseg`` samples ``hop`` apart (None: ``nperseg - nperseg // 2``, scipy's default overlap), each less its mean
    (``detrend="constant"``; ``"none"``, False or None: as it is), times ``window`` (``nperseg`` values, a torch tensor, or a
    name: any that ``scipy.signal.get_window`` takes if scipy imports, else ``"hann"`` or ``"boxcar"``; None: Hann),
    zero-padded to ``nfft`` (None: ``nperseg``) and transformed.  ``scaling``: ``"density"`` (V^2/Hz at sampling rate ``fs``)
    or ``"spectrum"`` (V^2).  One-sided: ``bins = nfft // 2 + 1``.  ``segments`` frames per signal; the sums over them run
    in slabs of ``slab`` frames."""

    _prefix = "psd"

    def __init__(self, signal_len: int, nperseg: int, hop: int | None = None, nfft: int | None = None, window=None,
                 detrend="constant", scaling: str = "density", fs: float = 1.0):
        det = _detrend_code(detrend)
        if scaling not in _SCALINGS:
            raise ValueError(f"scaling must be 'density' or 'spectrum', not {scaling!r}")
        hop = nperseg - nperseg // 2 if hop is None else hop
        nfft = nperseg if nfft is None else nfft
        w = _psd_window(window, nperseg)
        self._new(signal_len, nperseg, hop, nfft, None if w is None else w.ctypes.data_as(C.c_void_p), det, _SCALINGS[scaling],
                  float(fs))
        self.n = self.signal_len = signal_len
        self.nperseg, self.hop, self.nfft, self.fs = nperseg, hop, nfft, float(fs)
        self.detrend, self.scaling = "constant" if det else "none", scaling
        self.segments = int(self._fn("segments")(self._h))
        self.bins = int(self._fn("bins")(self._h))
        self.slab = int(self._fn("slab")(self._h))

    def frequencies(self):
        """the ``bins`` sample frequencies, as numpy.fft.rfftfreq(nfft, 1 / fs)"""
        return np.fft.rfftfreq(self.nfft, 1 / self.fs)

    def times(self):
        """the ``segments`` segment centres, as scipy.signal.spectrogram's"""
        return (np.arange(self.segments, dtype=np.float64) * self.hop + self.nperseg / 2) / self.fs

    def workspace_len(self, batch: int = 1, cross: bool = False) -> int:
        """Elements of T a device call of ``batch`` signals (``cross``: pairs of signals, :func:`csd_batched`) works in.  A
        smaller workspace of at least ``workspace_min(cross)`` runs the frames in chunks, to the same bits."""
        return int(self._fn("workspace_len")(self._h, batch, bool(cross)))

    def workspace_min(self, cross: bool = False) -> int:
        return int(self._fn("workspace_min")(self._h, bool(cross)))

    def time_stages(self, signal, out, batch: int = 1, average: bool = True, workspace=None, reps: int = 10, slab: int = 0):
        """Average HIP-event milliseconds of (the mean and frame sweeps, the real transform, the accumulate and final sweeps)
        of an auto-spectrum call of ``batch`` signals at distance L on device tensors (measurement hook).  ``slab``: the frames
        per slab to sum with instead of the planner's (not fewer; ``segments``: one slab)"""
        x, o = _Slice(signal, self._dtype, "signal"), _Slice(out, self._dtype, "out")
        ws = _any_workspace(self, batch, workspace)
        ms = (C.c_float * 3)()
        _check(self._fn("time_stages")(self._h, x.ptr, o.ptr, batch, bool(average), slab, ws.ptr, ws.len, reps, ms, _stream()))
        return [float(v) for v in ms]


class PlannerPsd32(PlannerPsd64):
    """f32 twin of :class:`PlannerPsd64` (the window, the means and the sums over frames stay in double)"""

    _sfx = "32"
    _dtype = np.float32


def _psd_workspace(planner, batch, cross, workspace):
    if workspace is None:
        import torch

        workspace = torch.empty(max(1, planner.workspace_len(batch, cross)),
                                dtype=torch.float64 if planner._dtype == np.float64 else torch.float32, device="cuda")
    return _any_workspace(planner, batch, workspace)


def psd_batched(signal, out, planner, batch: int, average: bool = True, sig_dist: int | None = None, workspace=None) -> None:
    """Device-resident batch of Welch auto spectra: signal b at ``b*sig_dist`` (default L, any distance >= L); bin k of signal
    b at ``b*bins + k`` of ``out``.  ``average=False`` (the spectrogram): bin k of segment f of signal b at
    ``(b*segments + f)*bins + k``.  ``workspace``: a device tensor of the planner's type of at least
    ``planner.workspace_min()`` elements; by default one of ``planner.workspace_len(batch)`` from torch's allocator.  The
    signal is not written."""
    dtype, fs = planner._dtype, "f64" if planner._dtype == np.float64 else "f32"
    x, o = _Slice(signal, dtype, "signal"), _Slice(out, dtype, "out")
    if not _same_place(x, o):
        raise TypeError("psd_batched needs device tensors")
    n, pts = planner.signal_len, planner.bins * (1 if average else planner.segments)
    sig_dist = n if sig_dist is None else sig_dist
    _need("signal", x.len, batch, sig_dist, n)
    _need("out", o.len, batch, pts, pts)
    ws = _psd_workspace(planner, batch, False, workspace)
    _check(_call(f"phast_psd_{fs}_dev", x.ptr, o.ptr, n, batch, sig_dist, bool(average), planner._h, ws.ptr, ws.len, _stream()))


def csd_batched(x, y, out_re, out_im, planner, batch: int, pxx=None, pyy=None, average: bool = True,
                sig_dist: int | None = None, workspace=None) -> None:
    """Device-resident batch of Welch cross spectra P_xy = <conj(X) Y> (scipy.signal.csd's convention) into the planes
    ``out_re`` and ``out_im``, laid out as :func:`psd_batched`'s ``out``; ``pxx`` and ``pyy``, where given, receive the two auto
    spectra from the same pass.  ``workspace``: at least ``planner.workspace_min(True)`` elements."""
    dtype, fs = planner._dtype, "f64" if planner._dtype == np.float64 else "f32"
    names = ("x", "y", "out_re", "out_im", "pxx", "pyy")
    sl = [None if t is None else _Slice(t, dtype, w) for t, w in zip((x, y, out_re, out_im, pxx, pyy), names)]
    if any(v is None for v in sl[:4]):
        raise TypeError("csd_batched needs x, y, out_re and out_im")
    if not _same_place(*(v for v in sl if v is not None)):
        raise TypeError("csd_batched needs device tensors")
    n, pts = planner.signal_len, planner.bins * (1 if average else planner.segments)
    sig_dist = n if sig_dist is None else sig_dist
    for v, w in zip(sl, names):
        if v is not None:
            _need(w, v.len, batch, *((sig_dist, n) if w in ("x", "y") else (pts, pts)))
    ws = _psd_workspace(planner, batch, True, workspace)
    _check(_call(f"phast_csd_{fs}_dev", *(None if v is None else v.ptr for v in sl), n, batch, sig_dist, bool(average),
                 planner._h, ws.ptr, ws.len, _stream()))


def _psd_host(fs, dtype, arrays, names, average, planner):
    sl = [None if t is None else _Slice(t, dtype, w) for t, w in zip(arrays, names)]
    if _same_place(*(v for v in sl if v is not None)):
        raise TypeError(f"the *_{fs}_with_planner forms take host arrays (psd_batched / csd_batched take device tensors)")
    return [x for v in sl for x in ((None, 0) if v is None else (v.ptr, v.len))]


def psd_f64_with_planner(signal, out, planner: PlannerPsd64, average: bool = True) -> None:
    """f64 Welch auto spectrum of one host signal of L samples into a host array of bins (``average=False``: segments * bins)
    values (blocking)"""
    _check(_call("phast_psd_f64_with_planner", *_psd_host("f64", np.float64, (signal, out), ("signal", "out"), average, planner),
                 bool(average), planner._h))


def psd_f32_with_planner(signal, out, planner: PlannerPsd32, average: bool = True) -> None:
    """f32 twin of :func:`psd_f64_with_planner`"""
    _check(_call("phast_psd_f32_with_planner", *_psd_host("f32", np.float32, (signal, out), ("signal", "out"), average, planner),
                 bool(average), planner._h))


_CSD_NAMES = ("x", "y", "out_re", "out_im", "pxx", "pyy")


def csd_f64_with_planner(x, y, out_re, out_im, planner: PlannerPsd64, pxx=None, pyy=None, average: bool = True) -> None:
    """f64 Welch cross spectrum of one pair of host signals into host planes (blocking); ``pxx``, ``pyy``: the auto spectra"""
    _check(_call("phast_csd_f64_with_planner", *_psd_host("f64", np.float64, (x, y, out_re, out_im, pxx, pyy), _CSD_NAMES, average,
                                                          planner), bool(average), planner._h))


def csd_f32_with_planner(x, y, out_re, out_im, planner: PlannerPsd32, pxx=None, pyy=None, average: bool = True) -> None:
    """f32 twin of :func:`csd_f64_with_planner`"""
    _check(_call("phast_csd_f32_with_planner", *_psd_host("f32", np.float32, (x, y, out_re, out_im, pxx, pyy), _CSD_NAMES, average,
                                                          planner), bool(average), planner._h))


def _psd_setup(x, fs, window, nperseg, noverlap, nfft, detrend, scaling, overlap_div=2):
    """the planner, the batch and the leading shape for a device tensor whose last axis is time"""
    import torch

    if not _is_torch(x) or x.device.type != "cuda" or x.dtype not in (torch.float64, torch.float32) or x.dim() < 1:
        raise TypeError("need a float64 or float32 device tensor")
    length = x.shape[-1]
    nperseg = 256 if nperseg is None else int(nperseg)
    if nperseg > length:
        import warnings

        warnings.warn(f"nperseg = {nperseg} is greater than input length = {length}, using nperseg = {length}", stacklevel=3)
        nperseg = length
    noverlap = nperseg // overlap_div if noverlap is None else int(noverlap)
    if not 0 <= noverlap < nperseg:
        raise ValueError("noverlap must be less than nperseg")
    nfft = nperseg if nfft is None else int(nfft)
    if nfft < nperseg:
        raise ValueError("nfft must be greater than or equal to nperseg")
    cls = PlannerPsd64 if x.dtype == torch.float64 else PlannerPsd32
    planner = cls(length, nperseg, nperseg - noverlap, nfft, window, detrend, scaling, fs)
    batch = x.numel() // length
    return planner, batch, tuple(x.shape[:-1])


def _psd_freqs(planner, x):
    import torch

    return torch.as_tensor(planner.frequencies(), dtype=x.dtype, device=x.device)


def welch(x, fs: float = 1.0, window="hann", nperseg: int | None = 256, noverlap: int | None = None, nfft: int | None = None,
          detrend="constant", scaling: str = "density"):
    """scipy.signal.welch over the last axis of a real device tensor, through a planner of its own: ``(freqs, Pxx)`` as new
    device tensors, ``Pxx`` of shape ``x.shape[:-1] + (bins,)``.  ``nperseg`` greater than the length is clamped to it, with
    scipy's warning."""
    import torch

    planner, batch, lead = _psd_setup(x, fs, window, nperseg, noverlap, nfft, detrend, scaling)
    out = torch.empty(batch * planner.bins, dtype=x.dtype, device=x.device)
    psd_batched(x.contiguous().reshape(-1), out, planner, batch)
    torch.cuda.current_stream().synchronize()  # the temporary planner's tables die with it
    return _psd_freqs(planner, x), out.reshape(lead + (planner.bins,))


def _csd_run(x, y, fs, window, nperseg, noverlap, nfft, detrend, scaling, autos):
    import torch

    if not _is_torch(y) or y.shape != x.shape or y.dtype != x.dtype or y.device != x.device:
        raise TypeError("x and y must be device tensors of one shape and type")
    planner, batch, lead = _psd_setup(x, fs, window, nperseg, noverlap, nfft, detrend, scaling)
    outs = [torch.empty(batch * planner.bins, dtype=x.dtype, device=x.device) for _ in range(4 if autos else 2)]
    csd_batched(x.contiguous().reshape(-1), y.contiguous().reshape(-1), outs[0], outs[1], planner, batch, *outs[2:])
    torch.cuda.current_stream().synchronize()
    return _psd_freqs(planner, x), [o.reshape(lead + (planner.bins,)) for o in outs]


def csd(x, y, fs: float = 1.0, window="hann", nperseg: int | None = 256, noverlap: int | None = None, nfft: int | None = None,
        detrend="constant", scaling: str = "density"):
    """scipy.signal.csd over the last axis of two real device tensors of one shape: ``(freqs, Pxy)``, ``Pxy`` complex"""
    import torch

    freqs, (re, im) = _csd_run(x, y, fs, window, nperseg, noverlap, nfft, detrend, scaling, False)
    return freqs, torch.complex(re, im)


def coherence(x, y, fs: float = 1.0, window="hann", nperseg: int | None = 256, noverlap: int | None = None,
              nfft: int | None = None, detrend="constant"):
    """scipy.signal.coherence: ``(freqs, |Pxy|^2 / (Pxx Pyy))`` from one cross call (the last step is elementwise on bins
    values)"""
    freqs, (re, im, pxx, pyy) = _csd_run(x, y, fs, window, nperseg, noverlap, nfft, detrend, "density", True)
    return freqs, (re * re + im * im) / (pxx * pyy)


def spectrogram(x, fs: float = 1.0, window="hann", nperseg: int | None = 256, noverlap: int | None = None,
                nfft: int | None = None, detrend="constant", scaling: str = "density"):
    """scipy.signal.spectrogram with ``mode="psd"`` over the last axis of a real device tensor: ``(freqs, times, Sxx)``, ``Sxx``
    of shape ``x.shape[:-1] + (bins, segments)`` (a transposed view of the frame-major result).  ``noverlap`` defaults to
    ``nperseg // 8`` as scipy's does; the default window here is Hann, not scipy's Tukey(0.25), which needs scipy."""
    import torch

    planner, batch, lead = _psd_setup(x, fs, window, nperseg, noverlap, nfft, detrend, scaling, overlap_div=8)
    out = torch.empty(batch * planner.segments * planner.bins, dtype=x.dtype, device=x.device)
    psd_batched(x.contiguous().reshape(-1), out, planner, batch, average=False)
    torch.cuda.current_stream().synchronize()
    times = torch.as_tensor(planner.times(), dtype=x.dtype, device=x.device)
    return _psd_freqs(planner, x), times, out.reshape(lead + (planner.segments, planner.bins)).transpose(-1, -2)


def periodogram(x, fs: float = 1.0, window="boxcar", nfft: int | None = None, detrend="constant", scaling: str = "density"):
    """scipy.signal.periodogram over the last axis: one segment of all L samples"""
    if not _is_torch(x) or x.dim() < 1:
        raise TypeError("need a float64 or float32 device tensor")
    return welch(x, fs, window, x.shape[-1], 0, nfft, detrend, scaling)


# ---------------------------------------------------------------------------------------------
# the Lomb-Scargle periodogram of unevenly spaced samples (no reference counterpart; scipy.signal.lombscargle)
# ---------------------------------------------------------------------------------------------
_LOMB_NORMS = {"power": 0, "normalize": 1, "amplitude": 2}


def _lomb_norm(normalize) -> int:
    """scipy's ``normalize``: False / "power", True / "normalize", or "amplitude" """
    if normalize is False or normalize is True:
        return 1 if normalize else 0
    if isinstance(normalize, str) and normalize in _LOMB_NORMS:
        return _LOMB_NORMS[normalize]
    raise ValueError(f"normalize must be False, True, 'power', 'normalize' or 'amplitude', not {normalize!r}")


class PlannerLomb64(_AnyHandle):
    """f64 generalised Lomb-Scargle periodogram (scipy.signal.lombscargle's definitions) of signals sampled at the M
    ``times`` (host doubles, any finite values, in any order) at the K ``freqs`` (host doubles, cycles per unit of time:
    scipy's angular frequencies over 2 pi), with optional ``weights`` (M values >= 0, normalised to sum 1; None: equal) and
    ``floating_mean``.  ``eps`` is the accuracy of the inner type-3 transform ([1e-14, 1e-1]).  Times, frequencies and weights
    are fixed here: the tables that depend on them alone are built once, in double."""

    _prefix = "lomb"
    _eps = 1e-12

    def __init__(self, times, freqs, weights=None, floating_mean: bool = False, eps: float | None = None):
        t, f = _host_doubles(times), _host_doubles(freqs)
        w = None if weights is None else _host_doubles(weights)
        if w is not None and w.size != t.size:
            raise ValueError(f"weights: {w.size} values for {t.size} times")
        eps = self._eps if eps is None else float(eps)
        self._new(t.ctypes.data_as(C.c_void_p), t.size, f.ctypes.data_as(C.c_void_p), f.size,
                  None if w is None else w.ctypes.data_as(C.c_void_p), bool(floating_mean), eps)
        self.n = self.m = self.m_points = t.size
        self.k = self.k_freqs = f.size
        self.eps, self.floating_mean = eps, bool(floating_mean)
        self.slab = int(self._fn("slab")(self._h))
        self.grid_len = int(self._fn("grid_len")(self._h))

    def workspace_len(self, batch: int = 1) -> int:
        """Elements of T a device call of ``batch`` signals works in.  A smaller workspace of at least ``workspace_min()``
        runs the batch in chunks of whole signals, to the same bits."""
        return self._workspace_len(batch)

    def workspace_min(self) -> int:
        return int(self._fn("workspace_min")(self._h))

    def time_stages(self, y, out_re, out_im=None, batch: int = 1, normalize="power", workspace=None, reps: int = 10):
        """Average HIP-event milliseconds of (the sweeps in front of the transform, the type-3 call, the post sweep) of a call
        of ``batch`` signals at the natural distances on device tensors (measurement hook)"""
        bufs = [_Slice(y, self._dtype, "y"), _Slice(out_re, self._dtype, "out_re"),
                _NULL if out_im is None else _Slice(out_im, self._dtype, "out_im")]
        ws = _any_workspace(self, batch, workspace)
        ms = (C.c_float * 3)()
        _check(self._fn("time_stages")(self._h, *(b.ptr for b in bufs), batch, _lomb_norm(normalize), ws.ptr, ws.len, reps, ms,
                                       _stream()))
        return [float(v) for v in ms]


class PlannerLomb32(PlannerLomb64):
    """f32 twin of :class:`PlannerLomb64`: eps in [1e-6, 1e-1]; times, frequencies and weights stay doubles, the tables are
    built in f64 and rounded, the mean and the sums over the points stay in double"""

    _sfx = "32"
    _dtype = np.float32
    _eps = 1e-6


def lombscargle_batched(y, planner, normalize="power", out=None, work=None, stream=None):
    """Device-resident batch of periodograms through one planner: ``y`` is a torch device tensor of shape ``(batch, M)`` or
    ``(M,)`` of the planner's type whose last axis is contiguous; returns a tensor of shape ``(batch, K)`` or ``(K,)`` -- for
    ``normalize="amplitude"`` a pair ``(re, im)`` of them.  ``out``: such a tensor (pair) to write into; ``work``: a device
    tensor of at least ``planner.workspace_min()`` elements, by default one of ``planner.workspace_len(batch)`` from torch's
    allocator; ``stream``: a ``torch.cuda.Stream``, by default the current one.  ``y`` is not written."""
    import torch

    want = torch.float64 if planner._dtype == np.float64 else torch.float32
    norm = _lomb_norm(normalize)
    amp = norm == 2
    fs = "f64" if planner._dtype == np.float64 else "f32"

    def plane(v, what, per):
        if not _is_torch(v) or v.device.type != "cuda" or v.dtype != want:
            raise TypeError(f"{what}: need a {want} device tensor")
        if v.dim() not in (1, 2) or v.shape[-1] != per or (per > 1 and v.stride(-1) != 1):
            raise ValueError(f"{what}: need shape (batch, {per}) or ({per},) with a contiguous last axis, not {tuple(v.shape)}")
        rows = v.shape[0] if v.dim() == 2 else 1
        dist = v.stride(0) if v.dim() == 2 and rows > 1 else per
        if dist < per:
            raise ValueError(f"{what}: rows overlap")
        return rows, dist

    batch, sig_dist = plane(y, "y", planner.m_points)
    k = planner.k_freqs
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        shape = (batch, k) if y.dim() == 2 else (k,)
        if out is None:
            out = tuple(torch.empty(shape, dtype=want, device=y.device) for _ in range(2)) if amp else torch.empty(
                shape, dtype=want, device=y.device)
        outs = tuple(out) if amp else (out,)
        if len(outs) != (2 if amp else 1):
            raise ValueError("out: need a pair (re, im) for amplitude, one tensor otherwise")
        rows, out_dist = plane(outs[0], "out", k)
        if rows != batch or outs[0].dim() != y.dim() or (amp and plane(outs[1], "out_im", k) != (batch, out_dist)):
            raise ValueError("out: need (batch, K) tensors with equal strides")
        ws = _any_workspace(planner, batch, work)
        _check(_call(f"phast_lombscargle_{fs}_dev", y.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr() if amp else None,
                     planner.m_points, batch, sig_dist, out_dist, norm, planner._h, ws.ptr, ws.len, _stream()))
    return out


def _lomb_host(fs, dtype, y, out_re, out_im, normalize, planner):
    norm = _lomb_norm(normalize)
    sy, so = _Slice(y, dtype, "y"), _Slice(out_re, dtype, "out_re")
    si = None if out_im is None else _Slice(out_im, dtype, "out_im")
    if _same_place(*(v for v in (sy, so, si) if v is not None)):
        raise TypeError(f"lombscargle_{fs}_with_planner takes host arrays (lombscargle_batched takes device tensors)")
    _check(_call(f"phast_lombscargle_{fs}_with_planner", sy.ptr, sy.len, so.ptr, so.len, None if si is None else si.ptr,
                 0 if si is None else si.len, norm, planner._h))


def lombscargle_f64_with_planner(y, out_re, planner: PlannerLomb64, normalize="power", out_im=None) -> None:
    """f64 periodogram of one host signal of M values into a host array of K values (``normalize="amplitude"``: the real
    parts, the imaginary parts into ``out_im``); blocking"""
    _lomb_host("f64", np.float64, y, out_re, out_im, normalize, planner)


def lombscargle_f32_with_planner(y, out_re, planner: PlannerLomb32, normalize="power", out_im=None) -> None:
    """f32 twin of :func:`lombscargle_f64_with_planner`"""
    _lomb_host("f32", np.float32, y, out_re, out_im, normalize, planner)


def lombscargle(x, y, freqs, precenter: bool = False, normalize=False, *, weights=None, floating_mean: bool = False,
                eps: float | None = None):
    """scipy.signal.lombscargle over the last axis of a real device tensor ``y`` sampled at the times ``x``, at the ANGULAR
    frequencies ``freqs`` (scipy's argument meanings), through a planner of its own: a new tensor of shape
    ``y.shape[:-1] + (len(freqs),)``, complex for ``normalize="amplitude"``.  ``precenter`` (deprecated in scipy) takes the
    plain mean of every signal off first.  float64 runs in f64 (eps defaults to 1e-12), float32 in f32 (1e-6)."""
    import torch

    if not _is_torch(y) or y.device.type != "cuda" or y.dtype not in (torch.float64, torch.float32) or y.dim() < 1:
        raise TypeError("need a float64 or float32 device tensor of at least one axis")
    norm = _lomb_norm(normalize)
    t = _host_doubles(x)
    f = _host_doubles(freqs) / (2 * np.pi)
    if y.shape[-1] != t.size:
        raise ValueError(f"the last axis holds {y.shape[-1]} values for {t.size} times")
    planner = (PlannerLomb64 if y.dtype == torch.float64 else PlannerLomb32)(t, f, weights, floating_mean, eps)
    rows = y.reshape(-1, t.size)
    if precenter:
        rows = rows - rows.mean(dim=-1, keepdim=True)
    rows = rows.contiguous()
    out = torch.empty((2, rows.shape[0], f.size), dtype=y.dtype, device=y.device)
    if rows.shape[0]:
        lombscargle_batched(rows, planner, ("power", "normalize", "amplitude")[norm], (out[0], out[1]) if norm == 2 else out[0])
        torch.cuda.current_stream().synchronize()  # the temporary planner's tables die with it
    res = torch.complex(out[0], out[1]) if norm == 2 else out[0]
    return res.reshape(y.shape[:-1] + (f.size,))


# ---------------------------------------------------------------------------------------------
# sample-rate conversion (no reference counterpart; scipy.signal.upfirdn / resample_poly / decimate / resample)
# ---------------------------------------------------------------------------------------------
class PlannerUpfirdn64(_AnyHandle):
    """f64 polyphase FIR of signals of ``signal_len`` samples: ``scipy.signal.upfirdn(h, x, up, down)`` (zero-stuff by ``up``,
    filter with the taps ``h``, keep every ``down``-th sample), of which a call yields the ``out_len`` samples from ``first``
    on (``out_len=None``: up to the end, ``full_len - first``).  ``first + out_len`` may pass ``full_len``: zeros there.
    ``up`` and ``down`` are used as given.  One direct kernel; no workspace."""

    _prefix = "upfirdn"

    def __init__(self, signal_len: int, h, up: int = 1, down: int = 1, first: int = 0, out_len: int | None = None):
        if _is_torch(h):
            h = h.detach().cpu().numpy()
        taps = np.ascontiguousarray(h, dtype=self._dtype).reshape(-1)
        self._new(signal_len, taps.ctypes.data_as(C.c_void_p), taps.size, up, down, first, 0 if out_len is None else out_len)
        self.n = self.signal_len = signal_len
        self.num_taps, self.up, self.down, self.first = taps.size, up, down, first
        self.out_len = int(self._fn("out_len")(self._h))
        self.full_len = int(self._fn("full_len")(self._h))
        self.tile = int(self._fn("tile")(self._h))
        self.chunk = int(self._fn("chunk")(self._h))

    def workspace_len(self, batch: int = 1) -> int:
        """0: the kernel works in LDS alone"""
        return self._workspace_len(batch)

    def workspace_min(self) -> int:
        return 0

    def time_stages(self, signal, out, batch: int = 1, reps: int = 10):
        """Average HIP-event milliseconds of the kernel of a call of ``batch`` signals at distances L and out_len on device
        tensors, as a list of one (measurement hook)"""
        x, y = _Slice(signal, self._dtype, "signal"), _Slice(out, self._dtype, "out")
        ms = (C.c_float * 1)()
        _check(self._fn("time_stages")(self._h, x.ptr, y.ptr, batch, reps, ms, _stream()))
        return [float(ms[0])]


class PlannerUpfirdn32(PlannerUpfirdn64):
    """f32 twin of :class:`PlannerUpfirdn64`: taps, products and sums in f32"""

    _sfx = "32"
    _dtype = np.float32


class PlannerResample64(_AnyHandle):
    """f64 Fourier-method resampling of real signals of ``signal_len`` samples to ``num``: ``scipy.signal.resample(x, num)``
    (no window, time domain).  One R2C of L and one C2R of num on the any-length real path around one sweep."""

    _prefix = "resample"

    def __init__(self, signal_len: int, num: int):
        self._new(signal_len, num)
        self.n = self.signal_len = signal_len
        self.num = self.out_len = num

    def workspace_len(self, batch: int = 1) -> int:
        """Elements of T a device call of ``batch`` signals works in.  A smaller workspace of at least ``workspace_min()``
        runs the batch in chunks of whole signals, to the same bits."""
        return self._workspace_len(batch)

    def workspace_min(self) -> int:
        return int(self._fn("workspace_min")(self._h))

    def time_stages(self, signal, out, batch: int = 1, workspace=None, reps: int = 10):
        """Average HIP-event milliseconds of (R2C, spectrum sweep, C2R) of a call of ``batch`` signals at distances L and
        num on device tensors (measurement hook)"""
        x, y = _Slice(signal, self._dtype, "signal"), _Slice(out, self._dtype, "out")
        ws = _any_workspace(self, batch, workspace)
        ms = (C.c_float * 3)()
        _check(self._fn("time_stages")(self._h, x.ptr, y.ptr, batch, ws.ptr, ws.len, reps, ms, _stream()))
        return [float(v) for v in ms]


class PlannerResample32(PlannerResample64):
    """f32 twin of :class:`PlannerResample64`"""

    _sfx = "32"
    _dtype = np.float32


def _rate_batched(name, x, planner, out, work, stream):
    """a batch of rows of ``planner.signal_len`` samples through ``phast_{name}_f*_dev`` into rows of ``planner.out_len``"""
    import torch

    want = torch.float64 if planner._dtype == np.float64 else torch.float32
    fs = "f64" if planner._dtype == np.float64 else "f32"

    def plane(v, what, per):
        if not _is_torch(v) or v.device.type != "cuda" or v.dtype != want:
            raise TypeError(f"{what}: need a {want} device tensor")
        if v.dim() not in (1, 2) or v.shape[-1] != per or (per > 1 and v.stride(-1) != 1):
            raise ValueError(f"{what}: need shape (batch, {per}) or ({per},) with a contiguous last axis, not {tuple(v.shape)}")
        rows = v.shape[0] if v.dim() == 2 else 1
        dist = v.stride(0) if v.dim() == 2 and rows > 1 else per
        if dist < per:
            raise ValueError(f"{what}: rows overlap")
        return rows, dist

    batch, sig_dist = plane(x, "x", planner.signal_len)
    m = planner.out_len
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        if out is None:
            out = torch.empty((batch, m) if x.dim() == 2 else (m,), dtype=want, device=x.device)
        rows, out_dist = plane(out, "out", m)
        if rows != batch or out.dim() != x.dim():
            raise ValueError("out: need one row per signal")
        if work is None and planner.workspace_len(batch) == 0:
            ptr, length = None, 0
        else:
            ws = _any_workspace(planner, batch, work)
            ptr, length = ws.ptr, ws.len
        _check(_call(f"phast_{name}_{fs}_dev", x.data_ptr(), out.data_ptr(), planner.signal_len, batch, sig_dist, out_dist,
                     planner._h, ptr, length, _stream()))
    return out


def upfirdn_batched(x, planner, out=None, work=None, stream=None):
    """Device-resident batch through one polyphase planner: ``x`` is a torch device tensor of shape ``(batch, L)`` or ``(L,)``
    of the planner's type whose last axis is contiguous (rows any distance >= L apart); returns a tensor of shape
    ``(batch, out_len)`` or ``(out_len,)``.  ``out``: such a tensor to write into; ``work`` is accepted and not used (the
    kernel needs no workspace); ``stream``: a ``torch.cuda.Stream``, by default the current one.  ``x`` is not written."""
    return _rate_batched("upfirdn", x, planner, out, work, stream)


def resample_batched(x, planner, out=None, work=None, stream=None):
    """Device-resident batch through one Fourier-method planner: ``x`` of shape ``(batch, L)`` or ``(L,)`` as for
    :func:`upfirdn_batched`; returns ``(batch, num)`` or ``(num,)``.  ``work``: a device tensor of at least
    ``planner.workspace_min()`` elements, by default one of ``planner.workspace_len(batch)`` from torch's allocator."""
    return _rate_batched("resample", x, planner, out, work, stream)


def _rate_host(name, fs, dtype, signal, out, planner):
    x, y = _Slice(signal, dtype, "signal"), _Slice(out, dtype, "out")
    if _same_place(x, y):
        raise TypeError(f"{name}_{fs}_with_planner takes host arrays ({name}_batched takes device tensors)")
    _check(_call(f"phast_{name}_{fs}_with_planner", x.ptr, x.len, y.ptr, y.len, planner._h))


def upfirdn_64_with_planner(signal, out, planner: PlannerUpfirdn64) -> None:
    """f64 polyphase FIR of one host signal of L samples into a host array of ``planner.out_len`` (blocking)"""
    _rate_host("upfirdn", "f64", np.float64, signal, out, planner)


def upfirdn_32_with_planner(signal, out, planner: PlannerUpfirdn32) -> None:
    """f32 twin of :func:`upfirdn_64_with_planner`"""
    _rate_host("upfirdn", "f32", np.float32, signal, out, planner)


def resample_64_with_planner(signal, out, planner: PlannerResample64) -> None:
    """f64 Fourier-method resampling of one host signal of L samples into a host array of ``planner.num`` (blocking)"""
    _rate_host("resample", "f64", np.float64, signal, out, planner)


def resample_32_with_planner(signal, out, planner: PlannerResample32) -> None:
    """f32 twin of :func:`resample_64_with_planner`"""
    _rate_host("resample", "f32", np.float32, signal, out, planner)


def _rate_rows(x):
    import torch

    if not _is_torch(x) or x.device.type != "cuda" or x.dtype not in (torch.float64, torch.float32) or x.dim() < 1:
        raise TypeError("need a float64 or float32 device tensor of at least one axis")
    return x.reshape(-1, x.shape[-1]).contiguous(), x.dtype == torch.float64


def _rate_apply(x, rows, planner, batched):
    import torch

    out = torch.empty((rows.shape[0], planner.out_len), dtype=x.dtype, device=x.device)
    if rows.shape[0]:
        batched(rows, planner, out)
        torch.cuda.current_stream().synchronize()  # the temporary planner's tables die with it
    return out.reshape(x.shape[:-1] + (planner.out_len,))


def upfirdn(h, x, up: int = 1, down: int = 1):
    """``scipy.signal.upfirdn(h, x, up, down)`` (mode "constant") over the last axis of a real device tensor ``x`` with the
    taps ``h`` (an array or a tensor), through a planner of its own: a new tensor whose last axis has
    ``((L - 1) * up + len(h) - 1) // down + 1`` samples"""
    rows, f64 = _rate_rows(x)
    planner = (PlannerUpfirdn64 if f64 else PlannerUpfirdn32)(x.shape[-1], h, up, down)
    return _rate_apply(x, rows, planner, upfirdn_batched)


def _fir_window(window, n: int):
    """the symmetric window of n points of a name or a (name, parameter) pair, in double, from numpy alone"""
    name, args = (window, ()) if isinstance(window, str) else (window[0], tuple(window[1:]))
    plain = {"boxcar": np.ones, "rectangular": np.ones, "hamming": np.hamming, "hann": np.hanning, "blackman": np.blackman,
             "bartlett": np.bartlett}
    if name == "kaiser" and len(args) == 1:
        return np.kaiser(n, float(args[0]))
    if name in plain and not args:
        return np.asarray(plain[name](n), dtype=np.float64)
    raise ValueError(f"window {window!r}: need ('kaiser', beta), 'hamming', 'hann', 'blackman', 'bartlett' or 'boxcar', or an "
                     "array of taps")


def firwin_lowpass(numtaps: int, cutoff: float, window=("kaiser", 5.0)):
    """``scipy.signal.firwin(numtaps, cutoff, window=window)``: the windowed-sinc low-pass of ``numtaps`` taps with the cutoff
    in units of the Nyquist frequency, scaled to unit sum; a host array of doubles"""
    if numtaps < 1 or not 0 < cutoff < 1:
        raise ValueError("need numtaps >= 1 and 0 < cutoff < 1")
    m = np.arange(numtaps) - 0.5 * (numtaps - 1)
    h = cutoff * np.sinc(cutoff * m) * _fir_window(window, numtaps)
    return h / h.sum()


def resample_poly(x, up: int, down: int, window=("kaiser", 5.0), padtype: str = "constant"):
    """``scipy.signal.resample_poly(x, up, down, window=window)`` over the last axis of a real device tensor: the rate times
    ``up / down`` through the polyphase kernel, ``ceil(L up / down)`` samples.  ``window``: a window for the low-pass design
    (``firwin(20 max(up, down) + 1, 1 / max(up, down), window)``) or an array of taps.  Only ``padtype="constant"``."""
    import math

    if padtype != "constant":
        raise ValueError("only padtype='constant' is supported")
    up, down = int(up), int(down)
    if up < 1 or down < 1:
        raise ValueError("up and down must be >= 1")
    g = math.gcd(up, down)
    up, down = up // g, down // g
    rows, f64 = _rate_rows(x)
    if up == 1 and down == 1:
        return x.clone()
    n_in = x.shape[-1]
    n_out = -(-n_in * up // down)
    if isinstance(window, (list, np.ndarray)) or _is_torch(window):
        taps = np.asarray(window.detach().cpu().numpy() if _is_torch(window) else window, dtype=np.float64).reshape(-1)
        half = (taps.size - 1) // 2
    else:
        half = 10 * max(up, down)
        taps = firwin_lowpass(2 * half + 1, 1.0 / max(up, down), window)
    n_pre_pad = down - half % down
    h = np.concatenate((np.zeros(n_pre_pad), taps * up))
    planner = (PlannerUpfirdn64 if f64 else PlannerUpfirdn32)(n_in, h, up, down, (half + n_pre_pad) // down, n_out)
    return _rate_apply(x, rows, planner, upfirdn_batched)


def decimate(x, q: int, n: int | None = None, ftype: str = "fir", zero_phase: bool = True):
    """``scipy.signal.decimate(x, q, n, ftype="fir", zero_phase=True)`` over the last axis of a real device tensor: a Hamming
    low-pass of ``n + 1`` taps (``n = 20 q`` by default) and every ``q``-th sample, without delay.  IIR decimation and
    ``zero_phase=False`` are not supported."""
    if ftype != "fir":
        raise ValueError("only ftype='fir' is supported")
    if not zero_phase:
        raise ValueError("only zero_phase=True is supported")
    q = int(q)
    if q < 1:
        raise ValueError("q must be >= 1")
    n = 20 * q if n is None else int(n)
    b = firwin_lowpass(n + 1, 1.0 / q, "hamming") if q > 1 else np.ones(1)
    return resample_poly(x, 1, q, window=b)


def resample(x, num: int):
    """``scipy.signal.resample(x, num)`` over the last axis of a real device tensor (Fourier method, no window), through a
    planner of its own: a new tensor whose last axis has ``num`` samples"""
    rows, f64 = _rate_rows(x)
    planner = (PlannerResample64 if f64 else PlannerResample32)(x.shape[-1], int(num))
    return _rate_apply(x, rows, planner, resample_batched)


# ---------------------------------------------------------------------------------------------
# polyphase filter-bank channelizer (no reference counterpart; cuSignal's channelize_poly)
# ---------------------------------------------------------------------------------------------
class PlannerChannelizer64(_AnyHandle):
    """f64 polyphase channelizer of signals of ``signal_len`` samples: ``n_chans`` equally spaced channels, each the signal
    times ``exp(-2 pi i k n / n_chans)``, filtered with the real taps ``h`` and decimated by ``hop`` (default ``n_chans``:
    critically sampled), with zero extension: channel k is ``scipy.signal.upfirdn(h, x * exp(-2j pi k n / n_chans), 1, hop)``.
    A call yields the ``out_frames`` frames from ``first_frame`` on (``out_frames=None``: up to the end, ``full_frames -
    first_frame``); the window may pass ``full_frames``: zeros there.  ``complex_input``: the signals are (re, im) plane pairs
    and a frame has ``n_chans`` bins; real signals give the one-sided ``n_chans // 2 + 1``.  One fold kernel, then one
    ``n_chans``-point transform per frame on the any-length path."""

    _prefix = "channelizer"

    def __init__(self, signal_len: int, h, n_chans: int, hop: int | None = None, first_frame: int = 0,
                 out_frames: int | None = None, complex_input: bool = False):
        if _is_torch(h):
            h = h.detach().cpu().numpy()
        taps = np.ascontiguousarray(h, dtype=self._dtype).reshape(-1)
        hop = n_chans if hop is None else hop
        self._new(signal_len, taps.ctypes.data_as(C.c_void_p), taps.size, n_chans, hop, first_frame,
                  0 if out_frames is None else out_frames, 1 if complex_input else 0)
        self.n = self.signal_len = signal_len
        self.num_taps, self.n_chans, self.hop, self.first_frame = taps.size, n_chans, hop, first_frame
        self.complex_input = bool(complex_input)
        self.out_frames = int(self._fn("out_frames")(self._h))
        self.full_frames = int(self._fn("full_frames")(self._h))
        self.bins = int(self._fn("bins")(self._h))
        self.tile_frames = int(self._fn("tile_frames")(self._h))
        self.tile_cols = int(self._fn("tile_cols")(self._h))
        self.chunk = int(self._fn("chunk")(self._h))
        self.periods = int(self._fn("periods")(self._h))

    def workspace_len(self, batch: int = 1) -> int:
        """Elements of T a device call of ``batch`` signals works in (0 for complex signals and a power-of-two ``n_chans``).
        A smaller workspace of at least ``workspace_min()`` runs the frames in chunks, to the same bits."""
        return self._workspace_len(batch)

    def workspace_min(self) -> int:
        return int(self._fn("workspace_min")(self._h))

    def time_stages(self, x_re, x_im, out_re, out_im, batch: int = 1, workspace=None, reps: int = 10):
        """Average HIP-event milliseconds of (fold, transform) of a call of ``batch`` signals at distance L on device
        tensors; ``x_im`` is None for a real planner (measurement hook)"""
        xr = _Slice(x_re, self._dtype, "x_re")
        xi = _NULL if x_im is None else _Slice(x_im, self._dtype, "x_im")
        o_re, o_im = _Slice(out_re, self._dtype, "out_re"), _Slice(out_im, self._dtype, "out_im")
        ws = _any_workspace(self, batch, workspace)
        ms = (C.c_float * 2)()
        _check(self._fn("time_stages")(self._h, xr.ptr, xi.ptr, o_re.ptr, o_im.ptr, batch, ws.ptr, ws.len, reps, ms, _stream()))
        return [float(v) for v in ms]


class PlannerChannelizer32(PlannerChannelizer64):
    """f32 twin of :class:`PlannerChannelizer64`: taps, products and sums in f32"""

    _sfx = "32"
    _dtype = np.float32


def channelize_batched(x, planner, out=None, work=None, stream=None):
    """Device-resident batch through one channelizer planner.  ``x``: a real torch device tensor of shape ``(batch, L)`` or
    ``(L,)`` of the planner's type whose last axis is contiguous (rows any distance >= L apart); for a complex planner a
    complex tensor of such a shape (split into planes here) or a pair ``(x_re, x_im)`` of real planes with equal strides.
    Returns a complex tensor of shape ``(batch, out_frames, bins)`` (``(out_frames, bins)`` for one unbatched signal).  ``out``:
    a pair of contiguous real planes of ``batch * out_frames * bins`` elements to write into, returned in place of the
    complex tensor; ``work``: a device tensor of at least ``planner.workspace_min()`` elements, by default one of
    ``planner.workspace_len(batch)`` from torch's allocator; ``stream``: a ``torch.cuda.Stream``, by default the current one.
    ``x`` is not written."""
    import torch

    want = torch.float64 if planner._dtype == np.float64 else torch.float32
    fs = "f64" if planner._dtype == np.float64 else "f32"
    n = planner.signal_len

    def plane(v, what):
        if not _is_torch(v) or v.device.type != "cuda" or v.dtype != want:
            raise TypeError(f"{what}: need a {want} device tensor")
        if v.dim() not in (1, 2) or v.shape[-1] != n or (n > 1 and v.stride(-1) != 1):
            raise ValueError(f"{what}: need shape (batch, {n}) or ({n},) with a contiguous last axis, not {tuple(v.shape)}")
        rows = v.shape[0] if v.dim() == 2 else 1
        dist = v.stride(0) if v.dim() == 2 and rows > 1 else n
        if dist < n:
            raise ValueError(f"{what}: rows overlap")
        return rows, dist

    if isinstance(x, (tuple, list)):
        x_re, x_im = x
    elif _is_torch(x) and x.is_complex():
        x_re, x_im = x.real.contiguous(), x.imag.contiguous()
    else:
        x_re, x_im = x, None
    if (x_im is not None) != planner.complex_input:
        raise TypeError("a complex planner takes complex signals and a real planner real ones")
    batch, sig_dist = plane(x_re, "x")
    if x_im is not None and (plane(x_im, "x_im") != (batch, sig_dist) or x_im.shape != x_re.shape):
        raise ValueError("x_im: need the shape and the strides of x_re")
    pts = batch * planner.out_frames * planner.bins
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        own = out is None
        if own:
            out = torch.empty((2, pts), dtype=want, device=x_re.device)
        out_re, out_im = out[0], out[1]
        for v, what in ((out_re, "out_re"), (out_im, "out_im")):
            if not _is_torch(v) or v.device.type != "cuda" or v.dtype != want or v.numel() != pts or not v.is_contiguous():
                raise ValueError(f"{what}: need a contiguous {want} device tensor of {pts} elements")
        if work is None and planner.workspace_min() == 0:
            ptr, length = None, 0
        else:
            ws = _any_workspace(planner, batch, work)
            ptr, length = ws.ptr, ws.len
        _check(_call(f"phast_channelize_{fs}_dev", x_re.data_ptr(), None if x_im is None else x_im.data_ptr(), out_re.data_ptr(),
                     out_im.data_ptr(), n, batch, sig_dist, planner._h, ptr, length, _stream()))
        if not own:
            return out
        shape = (planner.out_frames, planner.bins) if x_re.dim() == 1 else (batch, planner.out_frames, planner.bins)
        return torch.complex(out_re, out_im).reshape(shape)


def _channelize_host(fs, dtype, signal, signal_im, out_re, out_im, planner):
    x = _Slice(signal, dtype, "signal")
    xi = _NULL if signal_im is None else _Slice(signal_im, dtype, "signal_im")
    o_re, o_im = _Slice(out_re, dtype, "out_re"), _Slice(out_im, dtype, "out_im")
    if _same_place(x, o_re):
        raise TypeError(f"channelize_{fs}_with_planner takes host arrays (channelize_batched takes device tensors)")
    _check(_call(f"phast_channelize_{fs}_with_planner", x.ptr, xi.ptr, x.len, o_re.ptr, o_im.ptr, o_re.len, planner._h))


def channelize_64_with_planner(signal, out_re, out_im, planner: PlannerChannelizer64, signal_im=None) -> None:
    """f64 channelizer of one host signal of L samples (``signal_im``: its imaginary plane, for a complex planner) into two
    host arrays of ``planner.out_frames * planner.bins`` (blocking)"""
    _channelize_host("f64", np.float64, signal, signal_im, out_re, out_im, planner)


def channelize_32_with_planner(signal, out_re, out_im, planner: PlannerChannelizer32, signal_im=None) -> None:
    """f32 twin of :func:`channelize_64_with_planner`"""
    _channelize_host("f32", np.float32, signal, signal_im, out_re, out_im, planner)


def pfb_prototype(n_chans: int, taps_per_chan: int, window=("kaiser", 5.0)):
    """The usual prototype of a polyphase filter bank: ``firwin_lowpass(n_chans * taps_per_chan, 1 / n_chans, window)``, the
    windowed-sinc low-pass whose cutoff is half a channel spacing; a host array of doubles (``n_chans >= 2``)"""
    n_chans, taps_per_chan = int(n_chans), int(taps_per_chan)
    if n_chans < 2 or taps_per_chan < 1:
        raise ValueError("need n_chans >= 2 and taps_per_chan >= 1")
    return firwin_lowpass(n_chans * taps_per_chan, 1.0 / n_chans, window)


def channelize_poly(x, h, n_chans: int, hop: int | None = None, first_frame: int = 0, out_frames: int | None = None):
    """The polyphase channelizer over the last axis of a real or complex device tensor ``x`` with the real taps ``h`` (an
    array or a tensor), through a planner of its own: a new complex tensor of shape ``x.shape[:-1] + (out_frames, bins)``,
    ``bins = n_chans`` for complex ``x`` and ``n_chans // 2 + 1`` for real.  float64 / complex128 run in f64, float32 /
    complex64 in f32.  See :class:`PlannerChannelizer64` for the definition."""
    import torch

    kinds = {torch.float64: PlannerChannelizer64, torch.complex128: PlannerChannelizer64,
             torch.float32: PlannerChannelizer32, torch.complex64: PlannerChannelizer32}
    if not _is_torch(x) or x.device.type != "cuda" or x.dtype not in kinds or x.dim() < 1:
        raise TypeError("need a float64, float32, complex128 or complex64 device tensor of at least one axis")
    planner = kinds[x.dtype](x.shape[-1], h, n_chans, hop, first_frame, out_frames, x.is_complex())
    rows = x.reshape(-1, x.shape[-1]).contiguous()
    tail = (planner.out_frames, planner.bins)
    if not rows.shape[0]:
        return torch.empty(x.shape[:-1] + tail, dtype=torch.complex128 if planner._dtype == np.float64 else torch.complex64,
                           device=x.device)
    out = channelize_batched(rows, planner)
    torch.cuda.current_stream().synchronize()  # the temporary planner's tables die with it
    return out.reshape(x.shape[:-1] + tail)


# ---------------------------------------------------------------------------------------------
# polyphase synthesis filter bank, the channelizer's inverse (no reference counterpart)
# ---------------------------------------------------------------------------------------------
class PlannerSynthesizer64(_AnyHandle):
    """f64 polyphase synthesis bank of ``frames`` frames of ``n_chans`` channels: channel k is raised by ``hop`` (default
    ``n_chans``: critically sampled), filtered with the real taps ``g``, brought back to its band and the channels are summed,
    ``s = sum_k exp(2j pi k n / n_chans) * scipy.signal.upfirdn(g, Y[:, k], hop, 1)`` -- the phase in absolute sample time, as
    in :class:`PlannerChannelizer64`, the sum unnormalised.  A call yields the ``out_len`` samples from ``first`` on
    (``out_len=None``: up to the end, ``full_len - first`` with ``full_len = (frames - 1) * hop + len(g)``); the window may
    pass ``full_len``: zeros there.  ``complex_output``: a frame has ``n_chans`` bins and the signal is complex; otherwise a
    frame is the one-sided ``n_chans // 2 + 1`` bins, read by ``irfft``'s rules, and the signal is real.  One
    ``n_chans``-point inverse transform per frame on the any-length path, then one gather kernel.

    The phases are in absolute time, so the delay of an analysis / synthesis pair must be a multiple of ``n_chans`` for the
    columns to line up: for analysis taps ``h`` of ``n_chans * T`` points, ``g = concatenate(([0], h[::-1]))`` is the adjoint
    of the channelizer delayed by ``len(h)``; with ``h[j] = sin(pi (j + 1/2) / n_chans)``, ``hop = n_chans / 2`` and that
    ``g / n_chans`` the pair returns the signal delayed by ``n_chans``."""

    _prefix = "synthesizer"

    def __init__(self, frames: int, g, n_chans: int, hop: int | None = None, first: int = 0, out_len: int | None = None,
                 complex_output: bool = False):
        if _is_torch(g):
            g = g.detach().cpu().numpy()
        taps = np.ascontiguousarray(g, dtype=self._dtype).reshape(-1)
        hop = n_chans if hop is None else hop
        self._new(frames, taps.ctypes.data_as(C.c_void_p), taps.size, n_chans, hop, first, 0 if out_len is None else out_len,
                  1 if complex_output else 0)
        self.n = self.frames = frames
        self.num_taps, self.n_chans, self.hop, self.first = taps.size, n_chans, hop, first
        self.complex_output = bool(complex_output)
        self.out_len = int(self._fn("out_len")(self._h))
        self.full_len = int(self._fn("full_len")(self._h))
        self.bins = int(self._fn("bins")(self._h))
        self.tile_samples = int(self._fn("tile_samples")(self._h))
        self.per_thread = int(self._fn("per_thread")(self._h))
        self.max_terms = int(self._fn("max_terms")(self._h))

    def workspace_len(self, batch: int = 1) -> int:
        """Elements of T a device call of ``batch`` signals works in.  A smaller workspace of at least ``workspace_min()``
        (one signal's frames) runs whole signals in chunks, to the same bits."""
        return self._workspace_len(batch)

    def workspace_min(self) -> int:
        return int(self._fn("workspace_min")(self._h))

    def time_stages(self, y_re, y_im, out_re, out_im, batch: int = 1, workspace=None, reps: int = 10):
        """Average HIP-event milliseconds of (transform, unfold) of a call of ``batch`` signals at distance ``out_len`` on
        device tensors; ``out_im`` is None for a real planner (measurement hook)"""
        yr, yi = _Slice(y_re, self._dtype, "y_re"), _Slice(y_im, self._dtype, "y_im")
        o_re = _Slice(out_re, self._dtype, "out_re")
        o_im = _NULL if out_im is None else _Slice(out_im, self._dtype, "out_im")
        ws = _any_workspace(self, batch, workspace)
        ms = (C.c_float * 2)()
        _check(self._fn("time_stages")(self._h, yr.ptr, yi.ptr, o_re.ptr, o_im.ptr, batch, ws.ptr, ws.len, reps, ms, _stream()))
        return [float(v) for v in ms]


class PlannerSynthesizer32(PlannerSynthesizer64):
    """f32 twin of :class:`PlannerSynthesizer64`: taps, products and sums in f32"""

    _sfx = "32"
    _dtype = np.float32


def synthesize_batched(y, planner, out=None, work=None, stream=None):
    """Device-resident batch through one synthesizer planner.  ``y``: a complex torch device tensor of shape
    ``(batch, frames, bins)`` or ``(frames, bins)`` (split into planes here) or a pair ``(y_re, y_im)`` of contiguous real
    planes of such a shape, of the planner's type.  Returns a real tensor of shape ``(batch, out_len)`` (``(out_len,)`` for one
    unbatched signal), complex for a complex planner.  ``out``: a real tensor of that shape to write into whose last axis is
    contiguous (rows any distance >= out_len apart), for a complex planner a pair of such planes with equal strides; it is
    returned in place of a new tensor.  ``work``: a device tensor of at least ``planner.workspace_min()`` elements, by default
    one of ``planner.workspace_len(batch)`` from torch's allocator; ``stream``: a ``torch.cuda.Stream``, by default the current
    one.  ``y`` is not written."""
    import torch

    want = torch.float64 if planner._dtype == np.float64 else torch.float32
    fs = "f64" if planner._dtype == np.float64 else "f32"
    f, bins, n = planner.frames, planner.bins, planner.out_len

    if isinstance(y, (tuple, list)):
        y_re, y_im = y
    elif _is_torch(y) and y.is_complex():
        y_re, y_im = y.real.contiguous(), y.imag.contiguous()
    else:
        raise TypeError("y: need a complex device tensor or a pair of real planes")
    for v, what in ((y_re, "y_re"), (y_im, "y_im")):
        if not _is_torch(v) or v.device.type != "cuda" or v.dtype != want or not v.is_contiguous():
            raise TypeError(f"{what}: need a contiguous {want} device tensor")
        if v.dim() not in (2, 3) or tuple(v.shape[-2:]) != (f, bins) or v.shape != y_re.shape:
            raise ValueError(f"{what}: need shape (batch, {f}, {bins}) or ({f}, {bins}), not {tuple(v.shape)}")
    unbatched = y_re.dim() == 2
    batch = 1 if unbatched else y_re.shape[0]

    def plane(v, what):
        if not _is_torch(v) or v.device.type != "cuda" or v.dtype != want:
            raise TypeError(f"{what}: need a {want} device tensor")
        if v.dim() not in (1, 2) or v.shape[-1] != n or (n > 1 and v.stride(-1) != 1) or (v.shape[0] if v.dim() == 2 else 1) != batch:
            raise ValueError(f"{what}: need shape ({batch}, {n}) or ({n},) with a contiguous last axis, not {tuple(v.shape)}")
        dist = v.stride(0) if v.dim() == 2 and batch > 1 else n
        if dist < n:
            raise ValueError(f"{what}: rows overlap")
        return dist

    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        own = out is None
        if own:
            shape = (n,) if unbatched else (batch, n)
            out = tuple(torch.empty(shape, dtype=want, device=y_re.device) for _ in range(2 if planner.complex_output else 1))
            if not planner.complex_output:
                out = out[0]
        if planner.complex_output:
            if not isinstance(out, (tuple, list)) or len(out) != 2:
                raise TypeError("out: a complex planner writes a pair of real planes")
            out_re, out_im = out
            out_dist = plane(out_re, "out_re")
            if plane(out_im, "out_im") != out_dist:
                raise ValueError("out_im: need the strides of out_re")
        else:
            if isinstance(out, (tuple, list)):
                raise TypeError("out: a real planner writes one real plane")
            out_re, out_im = out, None
            out_dist = plane(out_re, "out")
        if batch == 0:
            return out if not (own and planner.complex_output) else torch.complex(out_re, out_im)
        if work is None and planner.workspace_min() == 0:
            ptr, length = None, 0
        else:
            ws = _any_workspace(planner, batch, work)
            ptr, length = ws.ptr, ws.len
        _check(_call(f"phast_synthesize_{fs}_dev", y_re.data_ptr(), y_im.data_ptr(), out_re.data_ptr(),
                     None if out_im is None else out_im.data_ptr(), f, batch, out_dist, planner._h, ptr, length, _stream()))
        if own and planner.complex_output:
            return torch.complex(out_re, out_im)
        return out


def _synthesize_host(fs, dtype, in_re, in_im, out_re, out_im, planner):
    y_re, y_im = _Slice(in_re, dtype, "in_re"), _Slice(in_im, dtype, "in_im")
    o_re = _Slice(out_re, dtype, "out_re")
    o_im = _NULL if out_im is None else _Slice(out_im, dtype, "out_im")
    if y_re.len != y_im.len:
        raise ValueError("in_re and in_im differ in length")
    if _same_place(y_re, o_re):
        raise TypeError(f"synthesize_{fs}_with_planner takes host arrays (synthesize_batched takes device tensors)")
    _check(_call(f"phast_synthesize_{fs}_with_planner", y_re.ptr, y_im.ptr, y_re.len, o_re.ptr, o_im.ptr, o_re.len, planner._h))


def synthesize_64_with_planner(in_re, in_im, out_re, planner: PlannerSynthesizer64, out_im=None) -> None:
    """f64 synthesis of one signal from host planes of ``planner.frames * planner.bins`` points into a host array of
    ``planner.out_len`` samples (``out_im``: its imaginary plane, for a complex planner); blocking"""
    _synthesize_host("f64", np.float64, in_re, in_im, out_re, out_im, planner)


def synthesize_32_with_planner(in_re, in_im, out_re, planner: PlannerSynthesizer32, out_im=None) -> None:
    """f32 twin of :func:`synthesize_64_with_planner`"""
    _synthesize_host("f32", np.float32, in_re, in_im, out_re, out_im, planner)


def synthesize_poly(y, g, n_chans: int, hop: int | None = None, first: int = 0, out_len: int | None = None, real: bool = False):
    """The polyphase synthesis bank over the last two axes ``(frames, bins)`` of a complex device tensor ``y`` with the real
    taps ``g`` (an array or a tensor), through a planner of its own: a new tensor of shape ``y.shape[:-2] + (out_len,)``.
    ``real=False``: ``bins = n_chans`` and the result is complex; ``real=True``: ``bins = n_chans // 2 + 1``, the one-sided
    frames of a real signal as :func:`channelize_poly` writes them, and the result is real.  complex128 runs in f64, complex64
    in f32.  See :class:`PlannerSynthesizer64` for the definition and for the taps that invert a channelizer."""
    import torch

    kinds = {torch.complex128: PlannerSynthesizer64, torch.complex64: PlannerSynthesizer32}
    if not _is_torch(y) or y.device.type != "cuda" or y.dtype not in kinds or y.dim() < 2:
        raise TypeError("need a complex128 or complex64 device tensor of at least two axes (frames, bins)")
    bins = n_chans // 2 + 1 if real else n_chans
    if y.shape[-1] != bins:
        raise ValueError(f"the last axis must have {bins} bins, not {y.shape[-1]}")
    planner = kinds[y.dtype](y.shape[-2], g, n_chans, hop, first, out_len, not real)
    rows = y.reshape((-1,) + tuple(y.shape[-2:]))
    if not rows.shape[0]:
        dt = y.real.dtype if real else y.dtype
        return torch.empty(y.shape[:-2] + (planner.out_len,), dtype=dt, device=y.device)
    out = synthesize_batched(rows, planner)
    torch.cuda.current_stream().synchronize()  # the temporary planner's tables die with it
    return out.reshape(y.shape[:-2] + (planner.out_len,))


# ---------------------------------------------------------------------------------------------
# continuous wavelet transform and analytic signal (no reference counterpart; Torrence & Compo 1998, scipy.signal.hilbert)
# ---------------------------------------------------------------------------------------------
_CWT_FAMILIES = {"morlet": 0, "paul": 1, "dog": 2, "step": 3}
_CWT_NORMS = {"l2": 0, "peak": 1}
_CWT_DEFAULTS = {"morlet": 6.0, "paul": 4.0, "dog": 2.0, "step": 0.0}


def _cwt_family(wavelet: str, param):
    if wavelet not in _CWT_FAMILIES:
        raise ValueError(f"wavelet: one of {sorted(_CWT_FAMILIES)}, not {wavelet!r}")
    return _CWT_FAMILIES[wavelet], float(_CWT_DEFAULTS[wavelet] if param is None else param)


class PlannerCwt64(_AnyHandle):
    """f64 continuous wavelet transform of signals of ``signal_len`` points at the scales ``scales`` (in samples: finite,
    > 0, any order), through a periodic convolution of ``pad_len`` >= ``signal_len`` points (default ``signal_len``; the
    signal is zero-extended, which pushes the wrap-around out of the window):
    ``W[j, n] = ifft(fft(x, pad_len) * conj(c_j * psi_hat(s_j * w)))[n]``, ``n < signal_len``, with Torrence & Compo's (1998)
    frequency-domain wavelets ``"morlet"`` (``param`` = w0, default 6), ``"paul"`` (integer order m <= 85, default 4),
    ``"dog"`` (integer derivative m <= 170, default 2: the Mexican hat) and ``"step"`` (the analytic-signal filter of
    ``scipy.signal.hilbert``; it ignores scale, ``param`` and ``norm``).  ``norm="l2"``: ``c_j = sqrt(2 pi s_j)`` (unit energy,
    Torrence & Compo eq. 6 at dt = 1); ``norm="peak"``: ``c_j = 2 / max |psi_hat|`` (a unit sinusoid at the centre frequency
    has ``|W| = 1`` for Morlet and Paul).  ``real_input`` is a property of the planner: a real planner takes one plane and keeps
    the one-sided spectrum.  One forward transform per signal, one bank kernel, one inverse transform per row.  Not here:
    the inverse transform, real output for real wavelets, ``|W|**2``, other families, other paddings."""

    _prefix = "cwt"

    def __init__(self, signal_len: int, scales, wavelet: str = "morlet", param=None, norm: str = "l2", pad_len: int | None = None,
                 real_input: bool = True):
        family, par = _cwt_family(wavelet, param)
        if norm not in _CWT_NORMS:
            raise ValueError(f"norm: one of {sorted(_CWT_NORMS)}, not {norm!r}")
        if _is_torch(scales):
            scales = scales.detach().cpu().numpy()
        sc = np.ascontiguousarray(scales, dtype=np.float64).reshape(-1)
        self._new(signal_len, 0 if pad_len is None else pad_len, sc.ctypes.data_as(C.c_void_p), sc.size, family, par,
                  _CWT_NORMS[norm], 1 if real_input else 0)
        self.n = self.signal_len = signal_len
        self.scales, self.wavelet, self.param, self.norm = sc.copy(), wavelet, par, norm
        self.real_input = bool(real_input)
        self.pad_len = int(self._fn("pad_len")(self._h))
        self.num_scales = int(self._fn("num_scales")(self._h))
        self.tile_bins = int(self._fn("tile_bins")(self._h))
        self.scale_group = int(self._fn("scale_group")(self._h))

    def workspace_len(self, batch: int = 1) -> int:
        """Elements of T a device call of ``batch`` signals works in.  A smaller workspace of at least ``workspace_min()`` (one
        signal's spectrum and one row) runs chunks of whole rows, to the same bits."""
        return self._workspace_len(batch)

    def workspace_min(self) -> int:
        return int(self._fn("workspace_min")(self._h))

    def time_stages(self, x_re, x_im, out_re, out_im, batch: int = 1, workspace=None, reps: int = 10):
        """Average HIP-event milliseconds of (forward, bank, inverse, crop) of a call of ``batch`` signals at distances
        ``signal_len`` and ``num_scales * signal_len`` on device tensors; ``x_im`` is None for a real planner (measurement hook)"""
        xr = _Slice(x_re, self._dtype, "x_re")
        xi = _NULL if x_im is None else _Slice(x_im, self._dtype, "x_im")
        o_re, o_im = _Slice(out_re, self._dtype, "out_re"), _Slice(out_im, self._dtype, "out_im")
        ws = _any_workspace(self, batch, workspace)
        ms = (C.c_float * 4)()
        _check(self._fn("time_stages")(self._h, xr.ptr, xi.ptr, o_re.ptr, o_im.ptr, batch, ws.ptr, ws.len, reps, ms, _stream()))
        return [float(v) for v in ms]


class PlannerCwt32(PlannerCwt64):
    """f32 twin of :class:`PlannerCwt64`: the scales and gains stay in f64 and the filter is evaluated in f64 and rounded once;
    the transforms and the product are f32"""

    _sfx = "32"
    _dtype = np.float32


def cwt_batched(x, planner, out=None, work=None, stream=None):
    """Device-resident batch through one CWT planner.  ``x``: for a real planner a real torch device tensor of shape
    ``(batch, signal_len)`` or ``(signal_len,)`` whose last axis is contiguous (rows any distance >= signal_len apart); for a
    complex planner a complex tensor of such a shape (split into planes here) or a pair ``(x_re, x_im)`` of such real planes
    with equal strides.  Returns a complex tensor of shape ``(batch, S, signal_len)`` (``(S, signal_len)`` for one unbatched
    signal).  ``out``: a pair ``(out_re, out_im)`` of real tensors of that shape to write into, their last two axes dense
    (signals any distance >= S * signal_len apart), equal strides; it is returned in place of a new tensor.  ``work``: a device
    tensor of at least ``planner.workspace_min()`` elements, by default one of ``planner.workspace_len(batch)`` from torch's
    allocator; ``stream``: a ``torch.cuda.Stream``, by default the current one.  ``x`` is not written."""
    import torch

    want = torch.float64 if planner._dtype == np.float64 else torch.float32
    l, s = planner.signal_len, planner.num_scales

    if planner.real_input:
        if isinstance(x, (tuple, list)) or not _is_torch(x) or x.is_complex():
            raise TypeError("x: a real planner takes one real device tensor")
        x_re, x_im = x, None
    elif isinstance(x, (tuple, list)):
        x_re, x_im = x
    elif _is_torch(x) and x.is_complex():
        x_re, x_im = x.real.contiguous(), x.imag.contiguous()
    else:
        raise TypeError("x: a complex planner takes a complex device tensor or a pair of real planes")

    def plane(v, what, n, lead):
        """the distance of the leading axis of a plane whose trailing axes are dense"""
        if not _is_torch(v) or v.device.type != "cuda" or v.dtype != want:
            raise TypeError(f"{what}: need a {want} device tensor")
        tail = (s, n) if lead == 2 else (n,)
        if v.dim() not in (lead, lead + 1) or tuple(v.shape[-lead:]) != tail:
            raise ValueError(f"{what}: need shape (batch,) + {tail} or {tail}, not {tuple(v.shape)}")
        dense = 1
        for ax in range(v.dim() - 1, v.dim() - 1 - lead, -1):
            if v.shape[ax] > 1 and v.stride(ax) != dense:
                raise ValueError(f"{what}: the last {lead} axes must be dense")
            dense *= v.shape[ax]
        count = v.shape[0] if v.dim() == lead + 1 else 1
        dist = v.stride(0) if v.dim() == lead + 1 and count > 1 else dense
        if dist < dense:
            raise ValueError(f"{what}: rows overlap")
        return count, dist

    batch, sig_dist = plane(x_re, "x", l, 1)
    if x_im is not None and plane(x_im, "x_im", l, 1) != (batch, sig_dist):
        raise ValueError("x_im: need the shape and strides of x_re")
    unbatched = x_re.dim() == 1

    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        own = out is None
        if own:
            shape = (s, l) if unbatched else (batch, s, l)
            out = tuple(torch.empty(shape, dtype=want, device=x_re.device) for _ in range(2))
        if not isinstance(out, (tuple, list)) or len(out) != 2:
            raise TypeError("out: a pair of real planes (out_re, out_im)")
        out_re, out_im = out
        n_out, out_dist = plane(out_re, "out_re", l, 2)
        if plane(out_im, "out_im", l, 2) != (n_out, out_dist) or n_out != batch:
            raise ValueError("out: need two planes of the batch's shape with equal strides")
        if batch:
            ws = _any_workspace(planner, batch, work)
            _check(_call(f"phast_cwt_{planner._sfx}_dev", x_re.data_ptr(), None if x_im is None else x_im.data_ptr(),
                         out_re.data_ptr(), out_im.data_ptr(), l, batch, sig_dist, out_dist, planner._h, ws.ptr, ws.len, _stream()))
        return torch.complex(out_re, out_im) if own else out


def _cwt_host(sfx, dtype, x_re, x_im, out_re, out_im, planner):
    xr = _Slice(x_re, dtype, "x_re")
    xi = _NULL if x_im is None else _Slice(x_im, dtype, "x_im")
    o_re, o_im = _Slice(out_re, dtype, "out_re"), _Slice(out_im, dtype, "out_im")
    if o_re.len != o_im.len:
        raise ValueError("out_re and out_im differ in length")
    if _same_place(xr, o_re, o_im):
        raise TypeError(f"cwt_{sfx}_with_planner takes host arrays (cwt_batched takes device tensors)")
    _check(_call(f"phast_cwt_{sfx}_with_planner", xr.ptr, xi.ptr, xr.len, o_re.ptr, o_im.ptr, o_re.len, planner._h))


def cwt_64_with_planner(x_re, out_re, out_im, planner: PlannerCwt64, x_im=None) -> None:
    """f64 transform of one signal from a host array of ``planner.signal_len`` points (``x_im``: its imaginary plane, for a
    complex planner) into host planes of ``planner.num_scales * planner.signal_len`` points, scale-major; blocking"""
    _cwt_host("64", np.float64, x_re, x_im, out_re, out_im, planner)


def cwt_32_with_planner(x_re, out_re, out_im, planner: PlannerCwt32, x_im=None) -> None:
    """f32 twin of :func:`cwt_64_with_planner`"""
    _cwt_host("32", np.float32, x_re, x_im, out_re, out_im, planner)


def cwt(x, scales, wavelet: str = "morlet", param=None, norm: str = "l2", pad_len: int | None = None):
    """The continuous wavelet transform over the last axis of a real or complex device tensor ``x`` at the scales ``scales``
    (an array or a tensor, in samples), through a planner of its own: a new complex tensor of shape
    ``x.shape[:-1] + (len(scales), x.shape[-1])``.  float64 / complex128 run in f64, float32 / complex64 in f32.  See
    :class:`PlannerCwt64` for the definition; :func:`cwt_scales` makes the customary dyadic scales and
    :func:`cwt_fourier_period` turns a scale into a Fourier period.  Not here: the inverse transform."""
    import torch

    kinds = {torch.float64: (PlannerCwt64, True), torch.float32: (PlannerCwt32, True),
             torch.complex128: (PlannerCwt64, False), torch.complex64: (PlannerCwt32, False)}
    if not _is_torch(x) or x.device.type != "cuda" or x.dtype not in kinds or x.dim() < 1:
        raise TypeError("need a float64, float32, complex128 or complex64 device tensor of at least one axis")
    kind, real = kinds[x.dtype]
    planner = kind(x.shape[-1], scales, wavelet, param, norm, pad_len, real)
    rows = x.reshape(-1, x.shape[-1]).contiguous()
    tail = (planner.num_scales, x.shape[-1])
    if not rows.shape[0]:
        return torch.empty(x.shape[:-1] + tail, dtype=torch.complex128 if kind is PlannerCwt64 else torch.complex64, device=x.device)
    out = cwt_batched(rows, planner)
    torch.cuda.current_stream().synchronize()  # the temporary planner's tables die with it
    return out.reshape(x.shape[:-1] + tail)


def hilbert(x, pad_len: int | None = None):
    """The analytic signal over the last axis of a real or complex device tensor, ``scipy.signal.hilbert(x, N=pad_len)`` cut
    to the first ``x.shape[-1]`` points: the ``"step"`` filter of :func:`cwt` with one scale.  A complex tensor of ``x``'s shape."""
    return cwt(x, [1.0], "step", pad_len=pad_len).squeeze(-2)


def cwt_scales(L: int, s0: float = 2.0, dj: float = 0.25, J: int | None = None):
    """Torrence & Compo's eqs. 9-10: the scales ``s0 * 2**(j * dj)``, ``j = 0 .. J``, with ``J = floor(log2(L / s0) / dj)`` by
    default, as a float64 array.  A negative default ``J`` (``L < s0``) has no scales and is a :class:`ValueError`."""
    if not (s0 > 0 and dj > 0 and L >= 1):
        raise ValueError("need L >= 1, s0 > 0 and dj > 0")
    if J is None:
        J = int(math.floor(math.log2(L / s0) / dj))
    if J < 0:
        raise ValueError(f"J = {J}: no scales (give J, or an s0 <= L)")
    return s0 * 2.0 ** (dj * np.arange(J + 1, dtype=np.float64))


def cwt_fourier_period(wavelet: str = "morlet", param=None) -> float:
    """The Fourier period of scale 1 (Torrence & Compo's table 1): ``4 pi / (w0 + sqrt(2 + w0**2))`` for Morlet,
    ``4 pi / (2 m + 1)`` for Paul, ``2 pi / sqrt(m + 1/2)`` for DOG; multiply by a scale.  ``"step"`` has no scale."""
    family, par = _cwt_family(wavelet, param)
    if family == 0:
        return 4 * math.pi / (par + math.sqrt(2 + par * par))
    if family == 1:
        return 4 * math.pi / (2 * par + 1)
    if family == 2:
        return 2 * math.pi / math.sqrt(par + 0.5)
    raise ValueError("the step filter has no scale")


# ---------------------------------------------------------------------------------------------
# discrete wavelet transform and its inverse (no reference counterpart; pywt.dwt / idwt / wavedec / waverec)
# ---------------------------------------------------------------------------------------------
_DWT_MODES = {"zero": 0, "constant": 1, "symmetric": 2, "reflect": 3, "periodic": 4, "periodization": 5}
_DWT_REFUSED = ("smooth", "antisymmetric", "antireflect")


def _dwt_mode(mode) -> int:
    if isinstance(mode, str):
        if mode in _DWT_REFUSED:
            raise ValueError(f"mode {mode!r} is out of scope: one of {sorted(_DWT_MODES)}")
        if mode in _DWT_MODES:
            return _DWT_MODES[mode]
    raise ValueError(f"mode: one of {sorted(_DWT_MODES)}, not {mode!r}")


@functools.lru_cache(maxsize=None)
def _daubechies(n: int):
    """rec_lo of dbN, 2N taps, by spectral factorisation: with y = (2 - z - 1/z) / 4 the half-band product filter is
    ((1 + z)(1 + 1/z) / 4)^N P(y), P(y) = sum_{k<N} C(N - 1 + k, k) y^k; each root of P gives a pair (z, 1/z) of which the one
    inside the unit circle is kept (minimum phase); h = (1 + z)^N prod (z - z_k), scaled to sum sqrt(2)"""
    roots = np.roots([math.comb(n - 1 + k, k) for k in range(n - 1, -1, -1)]) if n > 1 else np.zeros(0)
    zs = []
    for y in roots:
        b = 1 - 2 * y
        d = np.sqrt(b * b - 1 + 0j)
        z = b + d
        zs.append(z if abs(z) < 1 else b - d)
    h = np.real(np.poly(zs)) if zs else np.ones(1)
    for _ in range(n):
        h = np.convolve(h, [1.0, 1.0])
    return h * (math.sqrt(2.0) / h.sum())


def wavelet_filters(name: str):
    """``(dec_lo, dec_hi, rec_lo, rec_hi)`` of a built-in orthogonal wavelet as float64 arrays, in PyWavelets' order and sign:
    ``"haar"`` and ``"db1"`` .. ``"db10"``, computed by spectral factorisation (no tables).  ``rec_lo = h``, ``dec_lo`` is
    ``rec_lo`` reversed, ``rec_hi[k] = (-1)**k rec_lo[F - 1 - k]``, ``dec_hi`` is ``rec_hi`` reversed."""
    order = 1 if name == "haar" else int(name[2:]) if isinstance(name, str) and name[:2] == "db" and name[2:].isdigit() else 0
    if not 1 <= order <= 10:
        raise ValueError(f"wavelet {name!r}: 'haar' or 'db1' .. 'db10' (pass the four filters for any other bank)")
    rec_lo = _daubechies(order).copy()
    rec_hi = rec_lo[::-1] * (-1.0) ** np.arange(rec_lo.size)
    return rec_lo[::-1].copy(), rec_hi[::-1].copy(), rec_lo, rec_hi


def _dwt_bank(wavelet):
    """the four filters of a name or a 4-tuple of tap arrays, as float64 arrays of one even length"""
    if isinstance(wavelet, str):
        return wavelet_filters(wavelet)
    bank = tuple(wavelet)
    if len(bank) != 4:
        raise ValueError("wavelet: a name or the 4-tuple (dec_lo, dec_hi, rec_lo, rec_hi)")
    bank = tuple(np.asarray(f.detach().cpu().numpy() if _is_torch(f) else f, dtype=np.float64).reshape(-1) for f in bank)
    f = bank[0].size
    if any(b.size != f for b in bank) or f < 2 or f > 256 or f % 2:
        raise ValueError("wavelet: four filters of one even length 2 .. 256 (pad an odd-length filter with a zero)")
    return bank


def _dwt_filter_len(wavelet) -> int:
    return int(wavelet) if isinstance(wavelet, (int, np.integer)) else _dwt_bank(wavelet)[0].size


def dwt_max_level(signal_len: int, wavelet) -> int:
    """``pywt.dwt_max_level``: ``floor(log2(L / (F - 1)))``, 0 for ``L < F - 1``; ``wavelet``: a name, a filter bank or F"""
    f = _dwt_filter_len(wavelet)
    if signal_len < 1 or f < 2:
        raise ValueError("need L >= 1 and F >= 2")
    j = 0
    while (signal_len >> (j + 1)) >= f - 1:
        j += 1
    return j


def dwt_coeff_lens(signal_len: int, wavelet, level: int = 1, mode="symmetric"):
    """The lengths of ``pywt.wavedec``'s list ``[cA_J, cD_J, .., cD_1]`` for a signal of ``signal_len`` samples"""
    f, m = _dwt_filter_len(wavelet), _dwt_mode(mode)
    if signal_len < 1 or f < 2 or f % 2 or not 1 <= level <= 32:
        raise ValueError("need L >= 1, an even F >= 2 and 1 <= level <= 32")
    lens, n = [], signal_len
    for _ in range(level):
        n = (n + (n & 1)) // 2 if m == 5 else (n + f - 1) // 2
        lens.append(n)
    return [lens[-1]] + lens[::-1]


class PlannerDwt64(_AnyHandle):
    """f64 discrete wavelet transform of real signals of ``signal_len`` samples and its inverse: ``pywt.wavedec`` /
    ``pywt.waverec`` with ``level`` levels (1 .. 32; more than ``dwt_max_level`` is legal) in one of the modes ``zero``,
    ``constant``, ``symmetric``, ``reflect``, ``periodic``, ``periodization``.  ``filters``: a built-in name
    (:func:`wavelet_filters`) or the 4-tuple ``(dec_lo, dec_hi, rec_lo, rec_hi)`` of one even length 2 .. 256.  A signal's
    result is the packed row ``[cA_J | cD_J | .. | cD_1]`` of ``coeff_len`` elements.  One direct kernel launch per level."""

    _prefix = "dwt"

    def __init__(self, signal_len: int, filters, level: int = 1, mode="symmetric"):
        bank = [np.ascontiguousarray(f, dtype=self._dtype) for f in _dwt_bank(filters)]
        self.mode = mode
        self._new(signal_len, *(f.ctypes.data_as(C.c_void_p) for f in bank), bank[0].size, level, _dwt_mode(mode))
        self.n = self.signal_len = signal_len
        self.filter_len, self.level = bank[0].size, level
        self.coeff_len = int(self._fn("coeff_len")(self._h))
        self.tile = int(self._fn("tile")(self._h))
        self.level_lens = [int(self._fn("level_len")(self._h, l)) for l in range(level + 1)]          # n_0 .. n_J
        self.level_offsets = [0] + [int(self._fn("level_offset")(self._h, l)) for l in range(1, level + 1)]  # [0]: cA_J

    def bands(self):
        """``[(offset, length)]`` of ``cA_J, cD_J, .., cD_1`` in a packed row"""
        return [(0, self.level_lens[-1])] + [(self.level_offsets[l], self.level_lens[l]) for l in range(self.level, 0, -1)]

    def workspace_len(self, batch: int = 1) -> int:
        """Elements of T a device call of ``batch`` signals works in (0 for one level).  A smaller workspace of at least
        ``workspace_min()`` runs the batch in chunks of whole signals, to the same bits."""
        return self._workspace_len(batch)

    def workspace_min(self) -> int:
        return int(self._fn("workspace_min")(self._h))

    def time_stages(self, signal, coeffs, batch: int = 1, workspace=None, reps: int = 10):
        """Average HIP-event milliseconds of (wavedec, waverec) of ``batch`` signals at distances L and coeff_len on device
        tensors; the second overwrites ``signal`` with its reconstruction (measurement hook)"""
        x, y = _Slice(signal, self._dtype, "signal"), _Slice(coeffs, self._dtype, "coeffs")
        ws = _any_workspace(self, batch, workspace)
        ms = (C.c_float * 2)()
        _check(self._fn("time_stages")(self._h, x.ptr, y.ptr, batch, ws.ptr, ws.len, reps, ms, _stream()))
        return [float(v) for v in ms]


class PlannerDwt32(PlannerDwt64):
    """f32 twin of :class:`PlannerDwt64`: taps, products and sums in f32"""

    _sfx = "32"
    _dtype = np.float32


def _dwt_batched(name, x, planner, out, work, stream, per_in, per_out):
    """rows of ``per_in`` elements through ``phast_{name}_f*_dev`` into rows of ``per_out``"""
    import torch

    want = torch.float64 if planner._dtype == np.float64 else torch.float32
    fs = "f64" if planner._dtype == np.float64 else "f32"

    def plane(v, what, per):
        if not _is_torch(v) or v.device.type != "cuda" or v.dtype != want:
            raise TypeError(f"{what}: need a {want} device tensor")
        if v.dim() not in (1, 2) or v.shape[-1] != per or (per > 1 and v.stride(-1) != 1):
            raise ValueError(f"{what}: need shape (batch, {per}) or ({per},) with a contiguous last axis, not {tuple(v.shape)}")
        rows = v.shape[0] if v.dim() == 2 else 1
        dist = v.stride(0) if v.dim() == 2 and rows > 1 else per
        if dist < per:
            raise ValueError(f"{what}: rows overlap")
        return rows, dist

    batch, in_dist = plane(x, "input", per_in)
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        if out is None:
            out = torch.empty((batch, per_out) if x.dim() == 2 else (per_out,), dtype=want, device=x.device)
        rows, out_dist = plane(out, "out", per_out)
        if rows != batch or out.dim() != x.dim():
            raise ValueError("out: need one row per signal")
        if work is None and planner.workspace_len(batch) == 0:
            ptr, length = None, 0
        else:
            ws = _any_workspace(planner, batch, work)
            ptr, length = ws.ptr, ws.len
        _check(_call(f"phast_{name}_{fs}_dev", x.data_ptr(), out.data_ptr(), planner.signal_len, batch, in_dist, out_dist,
                     planner._h, ptr, length, _stream()))
    return out


def wavedec_batched(x, planner, out=None, work=None, stream=None):
    """Device-resident batch through one wavelet planner: ``x`` is a torch device tensor of shape ``(batch, L)`` or ``(L,)`` of
    the planner's type whose last axis is contiguous (rows any distance >= L apart); returns the packed rows, shape
    ``(batch, coeff_len)`` or ``(coeff_len,)``.  ``out``: such a tensor to write into; ``work``: a device tensor of at least
    ``planner.workspace_min()`` elements, by default one of ``planner.workspace_len(batch)`` from torch's allocator (none is
    needed for one level); ``stream``: a ``torch.cuda.Stream``, by default the current one.  ``x`` is not written."""
    return _dwt_batched("wavedec", x, planner, out, work, stream, planner.signal_len, planner.coeff_len)


def waverec_batched(coeffs, planner, out=None, work=None, stream=None):
    """The inverse of :func:`wavedec_batched`: packed rows ``(batch, coeff_len)`` or ``(coeff_len,)`` into signals
    ``(batch, L)`` or ``(L,)``.  ``coeffs`` is not written."""
    return _dwt_batched("waverec", coeffs, planner, out, work, stream, planner.coeff_len, planner.signal_len)


def _dwt_host(name, fs, dtype, a, b, planner):
    x, y = _Slice(a, dtype, "input"), _Slice(b, dtype, "out")
    if _same_place(x, y):
        raise TypeError(f"{name}_{fs[1:]}_with_planner takes host arrays ({name}_batched takes device tensors)")
    _check(_call(f"phast_{name}_{fs}_with_planner", x.ptr, x.len, y.ptr, y.len, planner._h))


def wavedec_64_with_planner(signal, coeffs, planner: PlannerDwt64) -> None:
    """f64 transform of one host signal of L samples into a host array of ``planner.coeff_len`` (blocking)"""
    _dwt_host("wavedec", "f64", np.float64, signal, coeffs, planner)


def wavedec_32_with_planner(signal, coeffs, planner: PlannerDwt32) -> None:
    """f32 twin of :func:`wavedec_64_with_planner`"""
    _dwt_host("wavedec", "f32", np.float32, signal, coeffs, planner)


def waverec_64_with_planner(coeffs, signal, planner: PlannerDwt64) -> None:
    """f64 inverse of one host packed row of ``planner.coeff_len`` into a host array of L samples (blocking)"""
    _dwt_host("waverec", "f64", np.float64, coeffs, signal, planner)


def waverec_32_with_planner(coeffs, signal, planner: PlannerDwt32) -> None:
    """f32 twin of :func:`waverec_64_with_planner`"""
    _dwt_host("waverec", "f32", np.float32, coeffs, signal, planner)


def _dwt_planner(f64, signal_len, wavelet, level, mode):
    return (PlannerDwt64 if f64 else PlannerDwt32)(signal_len, wavelet, level, mode)


def _dwt_apply(x, rows, planner, batched, per_out):
    import torch

    out = torch.empty((rows.shape[0], per_out), dtype=x.dtype, device=x.device)
    if rows.shape[0]:
        batched(rows, planner, out)
        torch.cuda.current_stream().synchronize()  # the temporary planner's table dies with it
    return out.reshape(x.shape[:-1] + (per_out,))


def wavedec(x, wavelet, mode="symmetric", level: int | None = None):
    """``pywt.wavedec(x, wavelet, mode, level)`` over the last axis of a real device tensor: the list of views
    ``[cA_J, cD_J, .., cD_1]`` into one new packed tensor.  ``level=None``: ``dwt_max_level`` (at least 1)."""
    rows, f64 = _rate_rows(x)
    if level is None:
        level = max(1, dwt_max_level(x.shape[-1], wavelet))
    planner = _dwt_planner(f64, x.shape[-1], wavelet, level, mode)
    packed = _dwt_apply(x, rows, planner, wavedec_batched, planner.coeff_len)
    return [packed[..., o:o + n] for o, n in planner.bands()]


def waverec(coeffs, wavelet, mode="symmetric"):
    """``pywt.waverec(coeffs, wavelet, mode)`` over the last axis of the real device tensors ``[cA_J, cD_J, .., cD_1]``: a new
    tensor.  As in PyWavelets the lengths of the list fix the signal's length up to one sample, and the longer one is
    returned; lengths that no signal gives are a :class:`ValueError`."""
    import torch

    coeffs = list(coeffs)
    if len(coeffs) < 2 or any(c is None for c in coeffs):
        raise ValueError("coeffs: [cA_J, cD_J, .., cD_1] without missing bands")
    lens = [c.shape[-1] for c in coeffs]
    f, m = _dwt_filter_len(wavelet), _dwt_mode(mode)
    top = 2 * lens[-1] if m == 5 else 2 * lens[-1] - f + 2
    level = len(coeffs) - 1
    for signal_len in (top, top - 1):
        if signal_len >= 1 and dwt_coeff_lens(signal_len, f, level, mode) == lens:
            break
    else:
        raise ValueError(f"coeffs: no signal has bands of the lengths {lens} with F = {f} in mode {mode!r}")
    packed = torch.cat(coeffs, dim=-1)
    rows, f64 = _rate_rows(packed)
    planner = _dwt_planner(f64, signal_len, wavelet, level, mode)
    return _dwt_apply(packed, rows, planner, waverec_batched, signal_len)


def dwt(x, wavelet, mode="symmetric"):
    """``pywt.dwt(x, wavelet, mode)`` over the last axis of a real device tensor: ``(cA, cD)``"""
    cA, cD = wavedec(x, wavelet, mode, 1)
    return cA, cD


def idwt(cA, cD, wavelet, mode="symmetric"):
    """``pywt.idwt(cA, cD, wavelet, mode)`` over the last axis of two real device tensors of one shape (a ``None`` band is
    out of scope): ``2 m - F + 2`` samples, ``2 m`` in periodization"""
    if cA is None or cD is None:
        raise ValueError("idwt: a None band is out of scope")
    if cA.shape != cD.shape:
        raise ValueError("idwt: cA and cD must have one shape")
    return waverec([cA, cD], wavelet, mode)


# ---------------------------------------------------------------------------------------------
# overlap-save FIR convolution and correlation of real signals (no reference counterpart; scipy.signal.convolve / correlate)
# ---------------------------------------------------------------------------------------------
_CONV_MODES = {"full": 0, "same": 1, "valid": 2}


class PlannerConv64(_AnyHandle):
    """f64 convolution (``correlate=True``: cross-correlation) of signals of ``signal_len`` samples with the real ``taps``:
    ``scipy.signal.convolve(x, taps, mode, method="direct")`` / ``scipy.signal.correlate(...)``.  ``mode``: ``"full"``
    (L + K - 1 samples), ``"same"`` (L) or ``"valid"`` (L - K + 1; needs L >= K).  The signal runs in overlapping segments of
    ``block`` samples, each one R2C, one multiply by the filter's spectrum and one C2R; ``block=0`` picks a power of two
    from the number of taps, any other value must be at least ``len(taps)``."""

    _prefix = "conv"

    def __init__(self, signal_len: int, taps, mode: str = "full", correlate: bool = False, block: int = 0):
        if mode not in _CONV_MODES:
            raise ValueError(f"mode must be 'full', 'same' or 'valid', not {mode!r}")
        if _is_torch(taps):
            taps = taps.detach().cpu().numpy()
        h = np.ascontiguousarray(taps, dtype=self._dtype).reshape(-1)
        self._new(signal_len, h.ctypes.data_as(C.c_void_p), h.size, _CONV_MODES[mode], bool(correlate), block)
        self.n = self.signal_len = signal_len
        self.num_taps, self.mode, self.correlate = h.size, mode, bool(correlate)
        self.out_len = int(self._fn("out_len")(self._h))
        self.block = int(self._fn("block")(self._h))
        self.segments = int(self._fn("segments")(self._h))

    def workspace_len(self, batch: int = 1) -> int:
        """Elements of T a device call of ``batch`` signals works in.  A smaller workspace of at least ``workspace_min()``
        (one segment) runs the call in chunks of whole segments."""
        return self._workspace_len(batch)

    def workspace_min(self) -> int:
        return int(self._fn("workspace_min")(self._h))

    def time_stages(self, signal, out, batch: int = 1, workspace=None, reps: int = 10):
        """Average HIP-event milliseconds of (segment sweep, R2C, spectrum sweep, C2R, save sweep) of a call of ``batch``
        signals at distances L and out_len on device tensors (measurement hook)"""
        x, y = _Slice(signal, self._dtype, "signal"), _Slice(out, self._dtype, "out")
        return self._time("time_stages", (x, y), (batch,), batch, workspace, reps)


class PlannerConv32(PlannerConv64):
    """f32 twin of :class:`PlannerConv64` (the filter's spectrum is built in f64 and rounded)"""

    _sfx = "32"
    _dtype = np.float32


def conv_batched(signal, out, planner, batch: int, sig_dist: int | None = None, out_dist: int | None = None,
                 workspace=None) -> None:
    """Device-resident batch of convolutions through one planner's filter: signal b at ``b*sig_dist`` (default L, any distance
    >= L), its output at ``b*out_dist`` (default ``planner.out_len``, any distance >= that).  ``workspace``: a device tensor
    of the planner's type of at least ``planner.workspace_min()`` elements (fewer than ``planner.workspace_len(batch)`` runs
    the segments in chunks); by default one from torch's allocator."""
    dtype, fs = planner._dtype, "f64" if planner._dtype == np.float64 else "f32"
    x, y = _Slice(signal, dtype, "signal"), _Slice(out, dtype, "out")
    if not _same_place(x, y):
        raise TypeError("conv_batched needs device tensors")
    n, m = planner.signal_len, planner.out_len
    sig_dist = n if sig_dist is None else sig_dist
    out_dist = m if out_dist is None else out_dist
    _need("signal", x.len, batch, sig_dist, n)
    _need("out", y.len, batch, out_dist, m)
    ws = _any_workspace(planner, batch, workspace)
    _check(_call(f"phast_conv_{fs}_dev", x.ptr, y.ptr, n, batch, sig_dist, out_dist, planner._h, ws.ptr, ws.len, _stream()))


def _conv_host(fs, dtype, signal, out, planner):
    x, y = _Slice(signal, dtype, "signal"), _Slice(out, dtype, "out")
    if _same_place(x, y):
        raise TypeError(f"conv_{fs}_with_planner takes host arrays (conv_batched takes device tensors)")
    _check(_call(f"phast_conv_{fs}_with_planner", x.ptr, x.len, y.ptr, y.len, planner._h))


def conv_f64_with_planner(signal, out, planner: PlannerConv64) -> None:
    """f64 convolution of one host signal of L samples into a host array of ``planner.out_len`` (blocking)"""
    _conv_host("f64", np.float64, signal, out, planner)


def conv_f32_with_planner(signal, out, planner: PlannerConv32) -> None:
    """f32 twin of :func:`conv_f64_with_planner`"""
    _conv_host("f32", np.float32, signal, out, planner)


def _convolve(x, h, mode, correlate):
    import torch

    if not _is_torch(x) or x.device.type != "cuda" or x.dtype not in (torch.float64, torch.float32):
        raise TypeError("need a float64 or float32 device tensor")
    x = x.contiguous().reshape(-1)
    planner = (PlannerConv64 if x.dtype == torch.float64 else PlannerConv32)(x.numel(), h, mode, correlate)
    out = torch.empty(planner.out_len, dtype=x.dtype, device=x.device)
    conv_batched(x, out, planner, 1)
    torch.cuda.current_stream().synchronize()  # the temporary planner's tables die with it
    return out


def fftconvolve(x, h, mode: str = "full"):
    """``scipy.signal.fftconvolve(x, h, mode)`` of one real device tensor with the taps ``h`` (an array or a tensor), by
    overlap-save through a planner of its own: a new device tensor"""
    return _convolve(x, h, mode, False)


def correlate(x, h, mode: str = "full"):
    """``scipy.signal.correlate(x, h, mode)`` of one real device tensor with the template ``h``: a new device tensor"""
    return _convolve(x, h, mode, True)


# ---------------------------------------------------------------------------------------------
# overlap-save convolution and correlation of real arrays of rank 1 .. 3 (no reference counterpart; scipy.signal.convolve /
# correlate of N-d arrays)
# ---------------------------------------------------------------------------------------------
class PlannerConvNd64(_AnyHandle):
    """f64 convolution (``correlate=True``: cross-correlation) of row-major arrays of ``signal_shape`` (rank 1 .. 3) with the real
    ``taps`` of the same rank: ``scipy.signal.convolve(x, taps, mode, method="direct")`` / ``scipy.signal.correlate(...)``.
    ``mode``: ``"full"``, ``"same"`` or ``"valid"`` (needs L_i >= K_i on every axis).  The array runs in overlapping tiles of
    ``block`` points per axis, each one R2C of the tile shape, one multiply by the filter's spectrum and one C2R; ``block=None``,
    or a 0 in it, picks a power of two per axis from the taps, any other value must be at least the taps' extent."""

    _prefix = "convnd"

    def __init__(self, signal_shape, taps, mode: str = "full", correlate: bool = False, block=None):
        if mode not in _CONV_MODES:
            raise ValueError(f"mode must be 'full', 'same' or 'valid', not {mode!r}")
        if _is_torch(taps):
            taps = taps.detach().cpu().numpy()
        h = np.ascontiguousarray(taps, dtype=self._dtype)
        self.signal_shape = tuple(int(d) for d in signal_shape)
        rank = len(self.signal_shape)
        if h.ndim != rank:
            raise ValueError(f"the taps have rank {h.ndim}, the arrays rank {rank}")
        if block is not None and len(tuple(block)) != rank:
            raise ValueError(f"block needs one entry per axis ({rank}), or None")
        blk = None if block is None else _dims(block)[0]
        self._new(_dims(self.signal_shape)[0], _dims(h.shape)[0], rank, h.ctypes.data_as(C.c_void_p), _CONV_MODES[mode],
                  bool(correlate), blk)
        self.n = self.signal_len = int(np.prod(self.signal_shape, dtype=np.int64))
        self.taps_shape, self.mode, self.correlate = tuple(h.shape), mode, bool(correlate)
        self.out_len = int(self._fn("out_len")(self._h))
        self.out_shape = self._dims_of("out_dims")
        self.block = self._dims_of("block")
        self.tiles = int(self._fn("tiles")(self._h))

    def _dims_of(self, name: str):
        rank = len(self.signal_shape)
        d = (C.c_size_t * rank)()
        _check(self._fn(name)(self._h, d, rank))
        return tuple(int(v) for v in d)

    def workspace_len(self, batch: int = 1) -> int:
        """Elements of T a device call of ``batch`` arrays works in.  A smaller workspace of at least ``workspace_min()``
        (one tile) runs the call in chunks of whole tiles."""
        return self._workspace_len(batch)

    def workspace_min(self) -> int:
        return int(self._fn("workspace_min")(self._h))

    def time_stages(self, signal, out, batch: int = 1, workspace=None, reps: int = 10):
        """Average HIP-event milliseconds of (tile sweep, R2C, spectrum sweep, C2R, save sweep) of a call of ``batch``
        arrays at distances prod L and ``out_len`` on device tensors (measurement hook)"""
        x, y = _Slice(_flat(signal), self._dtype, "signal"), _Slice(_flat(out), self._dtype, "out")
        return self._time("time_stages", (x, y), (batch,), batch, workspace, reps)


class PlannerConvNd32(PlannerConvNd64):
    """f32 twin of :class:`PlannerConvNd64` (the filter's spectrum is built in f64 and rounded)"""

    _sfx = "32"
    _dtype = np.float32


def convnd_batched(signal, out, planner, batch: int, sig_dist: int | None = None, out_dist: int | None = None,
                   workspace=None) -> None:
    """Device-resident batch of N-d convolutions through one planner's filter: array b at ``b*sig_dist`` elements (default
    prod L, any distance >= that), its output at ``b*out_dist`` (default ``planner.out_len``, any distance >= that).
    ``workspace``: a device tensor of the planner's type of at least ``planner.workspace_min()`` elements (fewer than
    ``planner.workspace_len(batch)`` runs the tiles in chunks); by default one from torch's allocator."""
    dtype, fs = planner._dtype, "f64" if planner._dtype == np.float64 else "f32"
    x, y = _Slice(_flat(signal), dtype, "signal"), _Slice(_flat(out), dtype, "out")
    if not _same_place(x, y):
        raise TypeError("convnd_batched needs device tensors")
    n, m = planner.signal_len, planner.out_len
    sig_dist = n if sig_dist is None else sig_dist
    out_dist = m if out_dist is None else out_dist
    _need("signal", x.len, batch, sig_dist, n)
    _need("out", y.len, batch, out_dist, m)
    ws = _any_workspace(planner, batch, workspace)
    _check(_call(f"phast_convnd_{fs}_dev", x.ptr, y.ptr, n, batch, sig_dist, out_dist, planner._h, ws.ptr, ws.len, _stream()))


def _convnd_host(fs, dtype, signal, out, planner):
    x, y = _Slice(_flat(signal), dtype, "signal"), _Slice(_flat(out), dtype, "out")
    if _same_place(x, y):
        raise TypeError(f"convnd_{fs}_with_planner takes host arrays (convnd_batched takes device tensors)")
    _check(_call(f"phast_convnd_{fs}_with_planner", x.ptr, x.len, y.ptr, y.len, planner._h))


def convnd_f64_with_planner(signal, out, planner: PlannerConvNd64) -> None:
    """f64 convolution of one host array of ``signal_shape`` into a host array of ``planner.out_shape`` (blocking)"""
    _convnd_host("f64", np.float64, signal, out, planner)


def convnd_f32_with_planner(signal, out, planner: PlannerConvNd32) -> None:
    """f32 twin of :func:`convnd_f64_with_planner`"""
    _convnd_host("f32", np.float32, signal, out, planner)


def _convolve_nd(x, h, mode, correlate):
    import torch

    if not _is_torch(x) or x.device.type != "cuda" or x.dtype not in (torch.float64, torch.float32):
        raise TypeError("need a float64 or float32 device tensor")
    x = x.contiguous()
    planner = (PlannerConvNd64 if x.dtype == torch.float64 else PlannerConvNd32)(tuple(x.shape), h, mode, correlate)
    out = torch.empty(planner.out_shape, dtype=x.dtype, device=x.device)
    convnd_batched(x, out, planner, 1)
    torch.cuda.current_stream().synchronize()  # the temporary planner's tables die with it
    return out


def fftconvolve_nd(x, h, mode: str = "full"):
    """``scipy.signal.fftconvolve(x, h, mode)`` of one real device tensor of rank 1 .. 3 with the taps ``h`` of the same rank (an
    array or a tensor), by overlap-save along every axis through a planner of its own: a new device tensor of the output's shape"""
    return _convolve_nd(x, h, mode, False)


def correlate_nd(x, h, mode: str = "full"):
    """``scipy.signal.correlate(x, h, mode)`` of one real device tensor of rank 1 .. 3 with the template ``h``: a new device tensor"""
    return _convolve_nd(x, h, mode, True)


# ---------------------------------------------------------------------------------------------
# the chirp-Z transform on the unit circle and the zoom FFT (no reference counterpart; scipy.signal.czt / zoom_fft)
# ---------------------------------------------------------------------------------------------
class PlannerCzt64(_AnyHandle):
    """f64 chirp-Z transform on the unit circle: ``m`` bins of ``n`` points at the frequencies ``start + k*step``, both in
    turns (cycles per sample): ``X[k] = sum_n x[n] exp(-2j pi n (start + k step))``, which is ``scipy.signal.czt(x, m,
    w=exp(-2j pi step), a=exp(2j pi start))``.  1 <= n, 1 <= m, n + m - 1 <= 2^30, finite ``step`` and ``start``."""

    _prefix = "czt"

    def __init__(self, n: int, m: int, step: float, start: float = 0.0):
        self._new(n, m, step, start)
        self.n, self.m, self.step, self.start = n, m, float(step), float(start)
        self.conv_len = int(self._fn("conv_len")(self._h))

    def workspace_len(self, batch: int = 1) -> int:
        """Elements of T a device call of ``batch`` transforms works in: 2 L batch, L = ``conv_len``.  A smaller workspace of
        at least 2 L runs the batch in chunks."""
        return self._workspace_len(batch)

    def time_stages(self, in_re, in_im, out_re, out_im, batch: int = 1, workspace=None, reps: int = 10):
        """Average HIP-event milliseconds of (pre sweep, forward L-point transform, spectrum sweep, inverse L-point transform,
        post sweep) of a call of ``batch`` transforms at distances n and m on device tensors (measurement hook)"""
        bufs = [_Slice(in_re, self._dtype, "in_re"), _NULL if in_im is None else _Slice(in_im, self._dtype, "in_im"),
                _Slice(out_re, self._dtype, "out_re"), _Slice(out_im, self._dtype, "out_im")]
        return self._time("time_stages", bufs, (batch,), batch, workspace, reps)


class PlannerCzt32(PlannerCzt64):
    """f32 twin of :class:`PlannerCzt64` (the phases and the table are built in f64 and rounded)"""

    _sfx = "32"
    _dtype = np.float32


class _Null:
    ptr = None


_NULL = _Null()


def czt_batched(x_re, x_im, planner, out=None, work=None, stream=None):
    """Device-resident batch of chirp-Z transforms through one planner: ``x_re`` (and ``x_im``, or ``None`` for a real
    signal) are torch device tensors of shape ``(batch, n)`` or ``(n,)`` of the planner's type whose last axis is
    contiguous; returns ``(out_re, out_im)`` of shape ``(batch, m)`` or ``(m,)``.  ``out``: such a pair to write into (it must
    not overlap the input or ``work``); ``work``: a device tensor of at least ``planner.workspace_len(1)`` elements (fewer than
    ``planner.workspace_len(batch)`` runs the batch in chunks), by default one from torch's allocator; ``stream``: a
    ``torch.cuda.Stream``, by default the current one."""
    import torch

    want = torch.float64 if planner._dtype == np.float64 else torch.float32
    n, m = planner.n, planner.m

    def plane(t, what, per):
        if not _is_torch(t) or t.device.type != "cuda" or t.dtype != want:
            raise TypeError(f"{what}: need a {want} device tensor")
        if t.dim() not in (1, 2) or t.shape[-1] != per or t.stride(-1) != 1:
            raise ValueError(f"{what}: need shape (batch, {per}) or ({per},) with a contiguous last axis, not {tuple(t.shape)}")
        rows = t.shape[0] if t.dim() == 2 else 1
        dist = t.stride(0) if t.dim() == 2 and rows > 1 else per
        if dist < per:
            raise ValueError(f"{what}: rows overlap")
        return rows, dist

    batch, in_dist = plane(x_re, "x_re", n)
    if x_im is not None and (plane(x_im, "x_im", n) != (batch, in_dist) or x_im.shape != x_re.shape):
        raise ValueError("x_im: need the shape and the strides of x_re")
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        if out is None:
            shape = (batch, m) if x_re.dim() == 2 else (m,)
            out = (torch.empty(shape, dtype=want, device=x_re.device), torch.empty(shape, dtype=want, device=x_re.device))
        out_re, out_im = out
        rows, out_dist = plane(out_re, "out_re", m)
        if rows != batch or plane(out_im, "out_im", m) != (batch, out_dist) or out_re.dim() != x_re.dim():
            raise ValueError("out: need a pair of (batch, m) tensors with equal strides")
        ws = _any_workspace(planner, batch, work)
        _check(_call(f"phast_czt_{planner._sfx}_dev", x_re.data_ptr(), None if x_im is None else x_im.data_ptr(), in_dist,
                     out_re.data_ptr(), out_im.data_ptr(), out_dist, batch, planner._h, ws.ptr, ws.len, _stream()))
    return out_re, out_im


def _czt_host(sfx, dtype, in_re, in_im, out_re, out_im, step, start, planner=None):
    x = _Slice(in_re, dtype, "in_re")
    y = _NULL if in_im is None else _Slice(in_im, dtype, "in_im")
    o_re, o_im = _Slice(out_re, dtype, "out_re"), _Slice(out_im, dtype, "out_im")
    if _same_place(*(s for s in (x, y, o_re, o_im) if s is not _NULL)):
        raise TypeError(f"czt_{sfx} takes host arrays (czt_batched takes device tensors)")
    if (y is not _NULL and y.len != x.len) or o_re.len != o_im.len:
        _check(2)
    args = [x.ptr, y.ptr, x.len, o_re.ptr, o_im.ptr, o_re.len]
    if planner is None:
        _check(_call(f"phast_czt_{sfx}", *args, step, start))
    else:
        _check(_call(f"phast_czt_{sfx}_with_planner", *args, planner._h))


def czt_64(in_re, in_im, out_re, out_im, step: float, start: float = 0.0) -> None:
    """f64 chirp-Z transform of one host signal (``in_im`` may be ``None``: a real signal) into host arrays of m bins, through
    a planner of its own (blocking)"""
    _czt_host("64", np.float64, in_re, in_im, out_re, out_im, step, start)


def czt_32(in_re, in_im, out_re, out_im, step: float, start: float = 0.0) -> None:
    """f32 twin of :func:`czt_64`"""
    _czt_host("32", np.float32, in_re, in_im, out_re, out_im, step, start)


def czt_64_with_planner(in_re, in_im, out_re, out_im, planner: PlannerCzt64) -> None:
    _czt_host("64", np.float64, in_re, in_im, out_re, out_im, 0.0, 0.0, planner)


def czt_32_with_planner(in_re, in_im, out_re, out_im, planner: PlannerCzt32) -> None:
    _czt_host("32", np.float32, in_re, in_im, out_re, out_im, 0.0, 0.0, planner)


def czt(x, m: int | None = None, step: float | None = None, start: float = 0.0):
    """The chirp-Z transform on the unit circle of a real or complex device tensor over its last axis: ``m`` bins (default n)
    at ``start + k*step`` turns (``step`` defaults to 1/m: with ``start = 0`` and ``m = n`` the forward DFT).  float64 /
    complex128 run in f64, float32 / complex64 in f32; returns a new complex tensor of shape ``x.shape[:-1] + (m,)``."""
    import torch

    kinds = {torch.float64: (PlannerCzt64, torch.float64), torch.complex128: (PlannerCzt64, torch.float64),
             torch.float32: (PlannerCzt32, torch.float32), torch.complex64: (PlannerCzt32, torch.float32)}
    if not _is_torch(x) or x.device.type != "cuda" or x.dtype not in kinds or x.dim() < 1:
        raise TypeError("need a float64, float32, complex128 or complex64 device tensor of at least one axis")
    n = x.shape[-1]
    m = n if m is None else int(m)
    if n < 1 or m < 1:
        raise ValueError("need at least one input point and one output point")
    step = 1.0 / m if step is None else float(step)
    cls, real = kinds[x.dtype]
    planner = cls(n, m, step, start)
    rows = x.reshape(-1, n)
    if x.is_complex():
        x_re, x_im = rows.real.contiguous(), rows.imag.contiguous()
    else:
        x_re, x_im = rows.contiguous(), None
    out = torch.empty((2, rows.shape[0], m), dtype=real, device=x.device)
    if rows.shape[0]:
        czt_batched(x_re, x_im, planner, out=(out[0], out[1]))
        torch.cuda.current_stream().synchronize()  # the temporary planner's tables die with it
    return torch.complex(out[0], out[1]).reshape(x.shape[:-1] + (m,))


def zoom_fft(x, fn, m: int | None = None, fs: float = 2.0, endpoint: bool = False):
    """``scipy.signal.zoom_fft(x, fn, m, fs=fs, endpoint=endpoint)`` of a real or complex device tensor over its last axis:
    ``m`` bins (default n) of the band ``fn = [f1, f2]`` (a scalar means ``[0, fn]``) at the sampling rate ``fs``."""
    if np.ndim(fn) == 0:
        f1, f2 = 0.0, float(fn)
    elif np.size(fn) == 2:
        f1, f2 = (float(v) for v in fn)
    else:
        raise ValueError("fn must be a scalar or a pair [f1, f2]")
    if not _is_torch(x) or x.dim() < 1:
        raise TypeError("need a device tensor of at least one axis")
    m = x.shape[-1] if m is None else int(m)
    if m < 1:
        raise ValueError("need at least one output point")
    spans = m - 1 if endpoint else m
    step = (f2 - f1) / (fs * spans) if spans else 0.0
    return czt(x, m, step, f1 / fs)


# ---------------------------------------------------------------------------------------------
# non-uniform FFTs of types 1 and 2 in one dimension (no reference counterpart)
# ---------------------------------------------------------------------------------------------
def _device_points(*coords):
    """``(pointers, M)`` of the coordinate arrays of a point set in device memory: contiguous float64 device tensors of M
    values each.  Anything else is a :class:`TypeError`: nothing is copied or converted behind the caller's back."""
    import torch

    for v in coords:
        if not _is_torch(v) or v.device.type != "cuda" or v.dtype != torch.float64 or not v.is_contiguous():
            raise TypeError("points in device memory: need contiguous float64 device tensors")
    m = coords[0].numel()
    if any(v.numel() != m for v in coords):
        raise ValueError("points in device memory: the coordinate arrays differ in length")
    return [C.c_void_p(v.data_ptr()) for v in coords], m


class _DevicePoints:
    """``from_device`` and ``set_points`` of the NUFFT planners of types 1 and 2: the points stay in device memory and are
    sorted there, into the very tables the host constructor builds, so the transforms give the same bits through either."""

    @classmethod
    def _from_device(cls, n_modes, coords, eps, stream):
        import torch

        ptrs, m = _device_points(*coords)
        self = cls.__new__(cls)
        eps = cls._eps if eps is None else float(eps)
        shape = tuple(int(v) for v in n_modes) if isinstance(n_modes, (tuple, list)) else (int(n_modes),)
        with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
            self._new(*shape, *ptrs, m, eps, _stream(), ctor="new_dev")
        self._describe_points(shape[0] if len(shape) == 1 else shape, m, eps)
        return self

    def _set_points(self, coords, stream) -> None:
        import torch

        ptrs, m = _device_points(*coords)
        with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
            _check(self._fn("set_points_dev")(self._h, *ptrs, m, _stream()))

    def time_set_points(self, *coords):
        """HIP-event milliseconds of the keys, sort and tables stages of one ``set_points`` (measurement hook)"""
        ptrs, m = _device_points(*coords)
        ms = (C.c_float * 3)()
        _check(self._fn("time_set_points")(self._h, *ptrs, m, ms, _stream()))
        return [float(x) for x in ms]


class PlannerNufft64(_DevicePoints, _AnyHandle):
    """f64 non-uniform FFTs of ``points`` (M doubles in turns, any finite value, reduced mod 1) and ``n_modes`` modes in numpy
    ``fftfreq`` order, ``k = fftfreq(n_modes) * n_modes``, to the relative accuracy ``eps``:

        type 1 (points -> modes)   ``F[m] = sum_j c[j] exp(-+2j pi k[m] x[j])``
        type 2 (modes -> points)   ``c[j] = sum_m F[m] exp(-+2j pi k[m] x[j])``

    with ``-`` for ``Direction.Forward`` and ``+`` for ``Direction.Reverse`` and no scaling.  1 <= n_modes <= 2^28,
    1 <= M <= 2^30, eps in [1e-14, 1e-1].  The points are host memory (an array or a sequence) and are sorted once here;
    :meth:`from_device` takes them from device memory, :meth:`set_points` replaces them."""

    _prefix = "nufft"
    _eps = 1e-12

    def __init__(self, n_modes: int, points, eps: float | None = None):
        x = np.ascontiguousarray(points.detach().cpu().numpy() if _is_torch(points) else points, dtype=np.float64).reshape(-1)
        eps = self._eps if eps is None else float(eps)
        self._new(n_modes, x.ctypes.data_as(C.c_void_p), x.size, eps)
        self._describe_points(n_modes, x.size, eps)

    @classmethod
    def from_device(cls, n_modes: int, points, eps: float | None = None, stream=None):
        """The planner for ``points`` given as a contiguous float64 device tensor, sorted on the device.  ``stream``: a
        ``torch.cuda.Stream`` whose earlier work produced the points, by default the current one.  Blocks until the planner is
        built; a point that is not finite is an error and no planner is built.  Any other kind of ``points`` is a
        :class:`TypeError`."""
        return cls._from_device(n_modes, (points,), eps, stream)

    def set_points(self, points, stream=None) -> None:
        """New points for this planner, the same number of them, as a contiguous float64 device tensor: the planner's tables are
        rewritten in place (a captured graph stays valid and, replayed, transforms at the new points).  Orders itself after the
        earlier work of ``stream`` (default: the current stream) ONLY -- work on other streams that uses the planner must have
        finished -- and blocks until done.  A point that is not finite is an error and the planner keeps its old points."""
        self._set_points((points,), stream)

    def _describe_points(self, n_modes, m, eps):
        self.n = self.n_modes = n_modes
        self.m = self.m_points = m
        self.eps = eps
        self.grid_len = int(self._fn("grid_len")(self._h))
        self.width = int(self._fn("width")(self._h))

    def workspace_len(self, batch: int = 1) -> int:
        """Elements of T a device call of ``batch`` transforms works in: 2 n_g batch, n_g = ``grid_len``.  A smaller workspace
        of at least 2 n_g runs the batch in chunks."""
        return self._workspace_len(batch)

    def time_stages(self, type: int, in_re, in_im, out_re, out_im, batch: int = 1, workspace=None, reps: int = 10):
        """Average HIP-event milliseconds of (spread or pre, the n_g-point transform, deconvolve or interpolate) of a Forward
        call of ``type`` 1 or 2 of ``batch`` transforms at the natural distances on device tensors (measurement hook)"""
        bufs = [_Slice(in_re, self._dtype, "in_re"), _NULL if in_im is None else _Slice(in_im, self._dtype, "in_im"),
                _Slice(out_re, self._dtype, "out_re"), _Slice(out_im, self._dtype, "out_im")]
        return self._time("time_stages", bufs, (type, batch), batch, workspace, reps)[:3]


class PlannerNufft32(PlannerNufft64):
    """f32 twin of :class:`PlannerNufft64`: eps in [1e-6, 1e-1]; the points stay doubles and the table of 1 / phi^ is built in
    f64 and rounded"""

    _sfx = "32"
    _dtype = np.float32
    _eps = 1e-6


def _nufft_batched(t, x_re, x_im, planner, direction, out, work, stream):
    import torch

    want = torch.float64 if planner._dtype == np.float64 else torch.float32
    n_in, n_out = (planner.m_points, planner.n_modes) if t == 1 else (planner.n_modes, planner.m_points)

    def plane(v, what, per):
        if not _is_torch(v) or v.device.type != "cuda" or v.dtype != want:
            raise TypeError(f"{what}: need a {want} device tensor")
        if v.dim() not in (1, 2) or v.shape[-1] != per or (per > 1 and v.stride(-1) != 1):  # a single element has no stride
            raise ValueError(f"{what}: need shape (batch, {per}) or ({per},) with a contiguous last axis, not {tuple(v.shape)}")
        rows = v.shape[0] if v.dim() == 2 else 1
        dist = v.stride(0) if v.dim() == 2 and rows > 1 else per
        if dist < per:
            raise ValueError(f"{what}: rows overlap")
        return rows, dist

    batch, in_dist = plane(x_re, "x_re", n_in)
    if x_im is not None and (plane(x_im, "x_im", n_in) != (batch, in_dist) or x_im.shape != x_re.shape):
        raise ValueError("x_im: need the shape and the strides of x_re")
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        if out is None:
            shape = (batch, n_out) if x_re.dim() == 2 else (n_out,)
            out = (torch.empty(shape, dtype=want, device=x_re.device), torch.empty(shape, dtype=want, device=x_re.device))
        out_re, out_im = out
        rows, out_dist = plane(out_re, "out_re", n_out)
        if rows != batch or plane(out_im, "out_im", n_out) != (batch, out_dist) or out_re.dim() != x_re.dim():
            raise ValueError("out: need a pair of (batch, n_out) tensors with equal strides")
        ws = _any_workspace(planner, batch, work)
        _check(_call(f"phast_nufft{t}_{planner._sfx}_dev", x_re.data_ptr(), None if x_im is None else x_im.data_ptr(), in_dist,
                     out_re.data_ptr(), out_im.data_ptr(), out_dist, batch, int(direction), planner._h, ws.ptr, ws.len,
                     _stream()))
    return out_re, out_im


def nufft1_batched(c_re, c_im, planner, direction=Direction.Forward, out=None, work=None, stream=None):
    """Device-resident batch of type 1 transforms (points -> modes) through one planner: ``c_re`` (and ``c_im``, or ``None``
    for real data) are torch device tensors of shape ``(batch, M)`` or ``(M,)`` of the planner's type whose last axis is
    contiguous; returns ``(out_re, out_im)`` of shape ``(batch, n_modes)`` or ``(n_modes,)``.  ``out``: such a pair to write
    into (it must not overlap the input or ``work``); ``work``: a device tensor of at least ``planner.workspace_len(1)``
    elements (fewer than ``planner.workspace_len(batch)`` runs the batch in chunks), by default one from torch's allocator;
    ``stream``: a ``torch.cuda.Stream``, by default the current one."""
    return _nufft_batched(1, c_re, c_im, planner, direction, out, work, stream)


def nufft2_batched(f_re, f_im, planner, direction=Direction.Forward, out=None, work=None, stream=None):
    """Device-resident batch of type 2 transforms (modes -> points): as :func:`nufft1_batched` with inputs of ``n_modes`` and
    outputs of M values per transform"""
    return _nufft_batched(2, f_re, f_im, planner, direction, out, work, stream)


def _nufft_host(t, sfx, dtype, in_re, in_im, out_re, out_im, direction, planner=None, points=None, eps=None):
    x = _Slice(in_re, dtype, "in_re")
    y = _NULL if in_im is None else _Slice(in_im, dtype, "in_im")
    o_re, o_im = _Slice(out_re, dtype, "out_re"), _Slice(out_im, dtype, "out_im")
    if _same_place(*(s for s in (x, y, o_re, o_im) if s is not _NULL)):
        raise TypeError(f"nufft{t}_{sfx} takes host arrays (nufft{t}_batched takes device tensors)")
    if (y is not _NULL and y.len != x.len) or o_re.len != o_im.len:
        _check(2)
    if planner is not None:
        _check(_call(f"phast_nufft{t}_{sfx}_with_planner", x.ptr, y.ptr, x.len, o_re.ptr, o_im.ptr, o_re.len, int(direction),
                     planner._h))
        return
    pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1)
    n_modes, m_points = (o_re.len, x.len) if t == 1 else (x.len, o_re.len)
    if pts.size != m_points:
        _check(2)
    _check(_call(f"phast_nufft{t}_{sfx}", pts.ctypes.data_as(C.c_void_p), pts.size, x.ptr, y.ptr, o_re.ptr, o_im.ptr, n_modes,
                 float(eps), int(direction)))


def nufft1_64(points, c_re, c_im, out_re, out_im, eps: float = 1e-12, direction=Direction.Forward) -> None:
    """f64 type 1 transform of one host vector of M values at ``points`` (``c_im`` may be ``None``: real data) into host arrays
    of n_modes values, through a planner of its own (blocking)"""
    _nufft_host(1, "64", np.float64, c_re, c_im, out_re, out_im, direction, points=points, eps=eps)


def nufft1_32(points, c_re, c_im, out_re, out_im, eps: float = 1e-6, direction=Direction.Forward) -> None:
    """f32 twin of :func:`nufft1_64`"""
    _nufft_host(1, "32", np.float32, c_re, c_im, out_re, out_im, direction, points=points, eps=eps)


def nufft2_64(points, f_re, f_im, out_re, out_im, eps: float = 1e-12, direction=Direction.Forward) -> None:
    """f64 type 2 transform of one host vector of n_modes values into host arrays of M values at ``points`` (blocking)"""
    _nufft_host(2, "64", np.float64, f_re, f_im, out_re, out_im, direction, points=points, eps=eps)


def nufft2_32(points, f_re, f_im, out_re, out_im, eps: float = 1e-6, direction=Direction.Forward) -> None:
    """f32 twin of :func:`nufft2_64`"""
    _nufft_host(2, "32", np.float32, f_re, f_im, out_re, out_im, direction, points=points, eps=eps)


def nufft1_64_with_planner(c_re, c_im, out_re, out_im, planner: PlannerNufft64, direction=Direction.Forward) -> None:
    _nufft_host(1, "64", np.float64, c_re, c_im, out_re, out_im, direction, planner)


def nufft1_32_with_planner(c_re, c_im, out_re, out_im, planner: PlannerNufft32, direction=Direction.Forward) -> None:
    _nufft_host(1, "32", np.float32, c_re, c_im, out_re, out_im, direction, planner)


def nufft2_64_with_planner(f_re, f_im, out_re, out_im, planner: PlannerNufft64, direction=Direction.Forward) -> None:
    _nufft_host(2, "64", np.float64, f_re, f_im, out_re, out_im, direction, planner)


def nufft2_32_with_planner(f_re, f_im, out_re, out_im, planner: PlannerNufft32, direction=Direction.Forward) -> None:
    _nufft_host(2, "32", np.float32, f_re, f_im, out_re, out_im, direction, planner)


def _nufft(t, points, v, n_modes, eps, direction):
    import torch

    kinds = {torch.float64: (PlannerNufft64, torch.float64), torch.complex128: (PlannerNufft64, torch.float64),
             torch.float32: (PlannerNufft32, torch.float32), torch.complex64: (PlannerNufft32, torch.float32)}
    if not _is_torch(v) or v.device.type != "cuda" or v.dtype not in kinds or v.dim() < 1:
        raise TypeError("need a float64, float32, complex128 or complex64 device tensor of at least one axis")
    cls, real = kinds[v.dtype]
    planner = cls(n_modes, points, eps)
    n_in, n_out = (planner.m_points, n_modes) if t == 1 else (n_modes, planner.m_points)
    if v.shape[-1] != n_in:
        raise ValueError(f"the last axis holds {v.shape[-1]} values, the transform takes {n_in}")
    rows = v.reshape(-1, n_in)
    if v.is_complex():
        x_re, x_im = rows.real.contiguous(), rows.imag.contiguous()
    else:
        x_re, x_im = rows.contiguous(), None
    out = torch.empty((2, rows.shape[0], n_out), dtype=real, device=v.device)
    if rows.shape[0]:
        _nufft_batched(t, x_re, x_im, planner, direction, (out[0], out[1]), None, None)
        torch.cuda.current_stream().synchronize()  # the temporary planner's tables die with it
    return torch.complex(out[0], out[1]).reshape(v.shape[:-1] + (n_out,))


def nufft1(points, c, n_modes: int, eps: float | None = None, direction=Direction.Forward):
    """Type 1 non-uniform FFT of a real or complex device tensor ``c`` over its last axis (M values at ``points``, in turns)
    into ``n_modes`` modes in ``fftfreq`` order: a new complex tensor of shape ``c.shape[:-1] + (n_modes,)``.  float64 /
    complex128 run in f64 (eps defaults to 1e-12), float32 / complex64 in f32 (1e-6)."""
    return _nufft(1, points, c, int(n_modes), eps, direction)


def nufft2(points, F, eps: float | None = None, direction=Direction.Forward):
    """Type 2 non-uniform FFT of a real or complex device tensor ``F`` of modes over its last axis, evaluated at ``points``
    (in turns): a new complex tensor of shape ``F.shape[:-1] + (len(points),)``"""
    if not _is_torch(F) or F.dim() < 1:
        raise TypeError("need a device tensor of at least one axis")
    return _nufft(2, points, F, int(F.shape[-1]), eps, direction)


# ---------------------------------------------------------------------------------------------
# the non-uniform FFT of type 3 in one dimension (no reference counterpart)
# ---------------------------------------------------------------------------------------------
def _host_doubles(v):
    return np.ascontiguousarray(v.detach().cpu().numpy() if _is_torch(v) else v, dtype=np.float64).reshape(-1)


class PlannerNufftT3_64(_AnyHandle):
    """f64 non-uniform FFT of type 3: ``sources`` (M doubles x, any finite values, in a unit U) to ``targets`` (K doubles s, any
    finite values, in 1 / U), the product ``s[k] * x[j]`` in turns, to the relative accuracy ``eps``:

        ``f[k] = sum_j c[j] exp(-+2j pi s[k] x[j])``

    with ``-`` for ``Direction.Forward`` and ``+`` for ``Direction.Reverse`` and no scaling.  1 <= M, K <= 2^30, eps in
    [1e-14, 1e-1], and the fine grid ``grid_len`` = the smallest power of two >= max(8 S X + w, 2 w, 8) -- X and S the
    half-widths of the two point sets -- is at most 2^28.  Both point sets are host memory and are fixed here."""

    _prefix = "nufft_t3_"
    _eps = 1e-12

    def __init__(self, sources, targets, eps: float | None = None):
        x, s = _host_doubles(sources), _host_doubles(targets)
        eps = self._eps if eps is None else float(eps)
        self._new(x.ctypes.data_as(C.c_void_p), x.size, s.ctypes.data_as(C.c_void_p), s.size, eps)
        self.m = self.m_points = x.size
        self.k = self.k_targets = s.size
        self.eps = eps
        self.grid_len = int(self._fn("grid_len")(self._h))
        self.width = int(self._fn("width")(self._h))

    def workspace_len(self, batch: int = 1) -> int:
        """Elements of T a device call of ``batch`` transforms works in: 4 n_f batch, n_f = ``grid_len``.  A smaller workspace
        of at least 4 n_f runs the batch in chunks."""
        return self._workspace_len(batch)

    def time_stages(self, in_re, in_im, out_re, out_im, batch: int = 1, workspace=None, reps: int = 10):
        """Average HIP-event milliseconds of (spread, the n_g-point transform, interpolate, post) of a Forward call of ``batch``
        transforms at the natural distances on device tensors (measurement hook)"""
        bufs = [_Slice(in_re, self._dtype, "in_re"), _NULL if in_im is None else _Slice(in_im, self._dtype, "in_im"),
                _Slice(out_re, self._dtype, "out_re"), _Slice(out_im, self._dtype, "out_im")]
        return self._time("time_stages", bufs, (batch,), batch, workspace, reps)[:4]


class PlannerNufftT3_32(PlannerNufftT3_64):
    """f32 twin of :class:`PlannerNufftT3_64`: eps in [1e-6, 1e-1]; the points stay doubles and every table is built in f64
    and rounded"""

    _sfx = "32"
    _dtype = np.float32
    _eps = 1e-6


def nufft3_batched(c_re, c_im, planner, direction=Direction.Forward, out=None, work=None, stream=None):
    """Device-resident batch of type 3 transforms through one planner: ``c_re`` (and ``c_im``, or ``None`` for real data) are
    torch device tensors of shape ``(batch, M)`` or ``(M,)`` of the planner's type whose last axis is contiguous; returns
    ``(out_re, out_im)`` of shape ``(batch, K)`` or ``(K,)``.  ``out``: such a pair to write into (it must not overlap the
    input or ``work``); ``work``: a device tensor of at least ``planner.workspace_len(1)`` elements (fewer than
    ``planner.workspace_len(batch)`` runs the batch in chunks), by default one from torch's allocator; ``stream``: a
    ``torch.cuda.Stream``, by default the current one."""
    import torch

    want = torch.float64 if planner._dtype == np.float64 else torch.float32
    n_in, n_out = planner.m_points, planner.k_targets

    def plane(v, what, per):
        if not _is_torch(v) or v.device.type != "cuda" or v.dtype != want:
            raise TypeError(f"{what}: need a {want} device tensor")
        if v.dim() not in (1, 2) or v.shape[-1] != per or (per > 1 and v.stride(-1) != 1):  # a single element has no stride
            raise ValueError(f"{what}: need shape (batch, {per}) or ({per},) with a contiguous last axis, not {tuple(v.shape)}")
        rows = v.shape[0] if v.dim() == 2 else 1
        dist = v.stride(0) if v.dim() == 2 and rows > 1 else per
        if dist < per:
            raise ValueError(f"{what}: rows overlap")
        return rows, dist

    batch, in_dist = plane(c_re, "c_re", n_in)
    if c_im is not None and (plane(c_im, "c_im", n_in) != (batch, in_dist) or c_im.shape != c_re.shape):
        raise ValueError("c_im: need the shape and the strides of c_re")
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        if out is None:
            shape = (batch, n_out) if c_re.dim() == 2 else (n_out,)
            out = (torch.empty(shape, dtype=want, device=c_re.device), torch.empty(shape, dtype=want, device=c_re.device))
        out_re, out_im = out
        rows, out_dist = plane(out_re, "out_re", n_out)
        if rows != batch or plane(out_im, "out_im", n_out) != (batch, out_dist) or out_re.dim() != c_re.dim():
            raise ValueError("out: need a pair of (batch, K) tensors with equal strides")
        ws = _any_workspace(planner, batch, work)
        _check(_call(f"phast_nufft3_{planner._sfx}_dev", c_re.data_ptr(), None if c_im is None else c_im.data_ptr(), in_dist,
                     out_re.data_ptr(), out_im.data_ptr(), out_dist, batch, int(direction), planner._h, ws.ptr, ws.len,
                     _stream()))
    return out_re, out_im


def _nufft3_host(sfx, dtype, c_re, c_im, out_re, out_im, direction, planner=None, sources=None, targets=None, eps=None):
    x = _Slice(c_re, dtype, "c_re")
    y = _NULL if c_im is None else _Slice(c_im, dtype, "c_im")
    o_re, o_im = _Slice(out_re, dtype, "out_re"), _Slice(out_im, dtype, "out_im")
    if _same_place(*(v for v in (x, y, o_re, o_im) if v is not _NULL)):
        raise TypeError(f"nufft3_{sfx} takes host arrays (nufft3_batched takes device tensors)")
    if (y is not _NULL and y.len != x.len) or o_re.len != o_im.len:
        _check(2)
    if planner is not None:
        _check(_call(f"phast_nufft3_{sfx}_with_planner", x.ptr, y.ptr, x.len, o_re.ptr, o_im.ptr, o_re.len, int(direction),
                     planner._h))
        return
    xs, ss = _host_doubles(sources), _host_doubles(targets)
    if xs.size != x.len or ss.size != o_re.len:
        _check(2)
    _check(_call(f"phast_nufft3_{sfx}", xs.ctypes.data_as(C.c_void_p), xs.size, ss.ctypes.data_as(C.c_void_p), ss.size, x.ptr,
                 y.ptr, o_re.ptr, o_im.ptr, float(eps), int(direction)))


def nufft3_64(sources, targets, c_re, c_im, out_re, out_im, eps: float = 1e-12, direction=Direction.Forward) -> None:
    """f64 type 3 transform of one host vector of M values at ``sources`` (``c_im`` may be ``None``: real data) into host arrays
    of K values at ``targets``, through a planner of its own (blocking)"""
    _nufft3_host("64", np.float64, c_re, c_im, out_re, out_im, direction, sources=sources, targets=targets, eps=eps)


def nufft3_32(sources, targets, c_re, c_im, out_re, out_im, eps: float = 1e-6, direction=Direction.Forward) -> None:
    """f32 twin of :func:`nufft3_64`"""
    _nufft3_host("32", np.float32, c_re, c_im, out_re, out_im, direction, sources=sources, targets=targets, eps=eps)


def nufft3_64_with_planner(c_re, c_im, out_re, out_im, planner: PlannerNufftT3_64, direction=Direction.Forward) -> None:
    _nufft3_host("64", np.float64, c_re, c_im, out_re, out_im, direction, planner)


def nufft3_32_with_planner(c_re, c_im, out_re, out_im, planner: PlannerNufftT3_32, direction=Direction.Forward) -> None:
    _nufft3_host("32", np.float32, c_re, c_im, out_re, out_im, direction, planner)


def nufft3(x, s, c, eps: float | None = None, direction=Direction.Forward):
    """Type 3 non-uniform FFT of a real or complex device tensor ``c`` over its last axis (M values at the sources ``x``) at the
    target frequencies ``s`` (``s[k] * x[j]`` in turns): a new complex tensor of shape ``c.shape[:-1] + (len(s),)``.  float64 /
    complex128 run in f64 (eps defaults to 1e-12), float32 / complex64 in f32 (1e-6)."""
    import torch

    kinds = {torch.float64: (PlannerNufftT3_64, torch.float64), torch.complex128: (PlannerNufftT3_64, torch.float64),
             torch.float32: (PlannerNufftT3_32, torch.float32), torch.complex64: (PlannerNufftT3_32, torch.float32)}
    if not _is_torch(c) or c.device.type != "cuda" or c.dtype not in kinds or c.dim() < 1:
        raise TypeError("need a float64, float32, complex128 or complex64 device tensor of at least one axis")
    cls, real = kinds[c.dtype]
    planner = cls(x, s, eps)
    if c.shape[-1] != planner.m_points:
        raise ValueError(f"the last axis holds {c.shape[-1]} values, the transform takes {planner.m_points}")
    rows = c.reshape(-1, planner.m_points)
    if c.is_complex():
        c_re, c_im = rows.real.contiguous(), rows.imag.contiguous()
    else:
        c_re, c_im = rows.contiguous(), None
    out = torch.empty((2, rows.shape[0], planner.k_targets), dtype=real, device=c.device)
    if rows.shape[0]:
        nufft3_batched(c_re, c_im, planner, direction, (out[0], out[1]))
        torch.cuda.current_stream().synchronize()  # the temporary planner's tables die with it
    return torch.complex(out[0], out[1]).reshape(c.shape[:-1] + (planner.k_targets,))


# ---------------------------------------------------------------------------------------------
# non-uniform FFTs of types 1 and 2 in two and three dimensions (no reference counterpart)
# ---------------------------------------------------------------------------------------------
class _PlannerNufftNd(_DevicePoints, _AnyHandle):
    """what the planners of two and three dimensions share: phast_planner_nufft{_rank}d{_sfx}_*"""

    _eps = 1e-12
    _rank = 0

    def _init(self, n_modes, coords, eps):
        shape = tuple(int(v) for v in n_modes)
        if len(shape) != self._rank:
            raise ValueError(f"n_modes: need {self._rank} mode counts, not {len(shape)}")
        pts = [np.ascontiguousarray(v.detach().cpu().numpy() if _is_torch(v) else v, dtype=np.float64).reshape(-1) for v in coords]
        if any(p.size != pts[0].size for p in pts):
            _check(2)
        eps = self._eps if eps is None else float(eps)
        self._new(*shape, *(p.ctypes.data_as(C.c_void_p) for p in pts), pts[0].size, eps)
        self._describe_points(shape, pts[0].size, eps)

    def _describe_points(self, n_modes, m, eps):
        self.n_modes = tuple(n_modes)
        self.n = int(np.prod(self.n_modes, dtype=np.int64))
        self.m = self.m_points = m
        self.eps = eps
        self.grid_len = int(self._fn("grid_len")(self._h))
        if self._rank == 2:
            self.grid_shape = (int(self._fn("grid_rows")(self._h)), int(self._fn("grid_cols")(self._h)))
        else:
            self.grid_shape = tuple(int(self._fn("grid_dim")(self._h, axis)) for axis in range(self._rank))
        self.width = int(self._fn("width")(self._h))

    def workspace_len(self, batch: int = 1) -> int:
        """Elements of T a device call of ``batch`` transforms works in: 4 G batch, G = ``grid_len``.  A smaller workspace of
        at least ``workspace_len(1)`` runs the batch in chunks."""
        return self._workspace_len(batch)

    def time_stages(self, type: int, in_re, in_im, out_re, out_im, batch: int = 1, workspace=None, reps: int = 10):
        """Average HIP-event milliseconds of (spread or pre, the transform of the grid, deconvolve or interpolate) of a
        Forward call of ``type`` 1 or 2 of ``batch`` transforms at the natural distances on device tensors (measurement hook)"""
        bufs = [_Slice(_flat(in_re), self._dtype, "in_re"), _NULL if in_im is None else _Slice(_flat(in_im), self._dtype, "in_im"),
                _Slice(_flat(out_re), self._dtype, "out_re"), _Slice(_flat(out_im), self._dtype, "out_im")]
        return self._time("time_stages", bufs, (type, batch), batch, workspace, reps)[:3]


class PlannerNufft2d64(_PlannerNufftNd):
    """f64 non-uniform FFTs of the M points ``(x[j], y[j])`` (doubles in turns, any finite value, reduced mod 1 per coordinate)
    and ``n_modes = (n1, n2)`` modes, row-major, each axis in numpy ``fftfreq`` order (``k1`` pairs with x, ``k2`` with y), to
    the relative accuracy ``eps``:

        type 1 (points -> modes)   ``F[m1, m2] = sum_j c[j] exp(-+2j pi (k1[m1] x[j] + k2[m2] y[j]))``
        type 2 (modes -> points)   ``c[j] = sum_{m1, m2} F[m1, m2] exp(-+2j pi (k1[m1] x[j] + k2[m2] y[j]))``

    with ``-`` for ``Direction.Forward`` and ``+`` for ``Direction.Reverse`` and no scaling.  n1, n2 >= 1, the fine grid
    ``grid_len = grid_shape[0] * grid_shape[1] <= 2^28``, 1 <= M <= 2^30, eps in [1e-14, 1e-1].  The points are host memory
    (arrays or sequences) and are sorted once here; :meth:`from_device` takes them from device memory, :meth:`set_points`
    replaces them."""

    _prefix = "nufft2d"
    _rank = 2

    def __init__(self, n_modes, x, y, eps: float | None = None):
        self._init(n_modes, (x, y), eps)

    @classmethod
    def from_device(cls, n_modes, x, y, eps: float | None = None, stream=None):
        """as :meth:`PlannerNufft64.from_device`, the coordinates as two contiguous float64 device tensors of M values"""
        return cls._from_device(tuple(n_modes), (x, y), eps, stream)

    def set_points(self, x, y, stream=None) -> None:
        """as :meth:`PlannerNufft64.set_points`"""
        self._set_points((x, y), stream)


class PlannerNufft2d32(PlannerNufft2d64):
    """f32 twin of :class:`PlannerNufft2d64`: eps in [1e-6, 1e-1]; the points stay doubles and the tables of 1 / phi^ are built
    in f64 and rounded"""

    _sfx = "32"
    _dtype = np.float32
    _eps = 1e-6


class PlannerNufft3d64(_PlannerNufftNd):
    """f64 non-uniform FFTs of the M points ``(x[j], y[j], z[j])`` (doubles in turns, any finite value, reduced mod 1 per coordinate)
    and ``n_modes = (n1, n2, n3)`` modes, row-major, each axis in numpy ``fftfreq`` order (``k1`` pairs with x, ``k2`` with y, ``k3`` with z), to
    the relative accuracy ``eps``:

        type 1 (points -> modes)   ``F[m1, m2, m3] = sum_j c[j] exp(-+2j pi (k1[m1] x[j] + k2[m2] y[j] + k3[m3] z[j]))``
        type 2 (modes -> points)   ``c[j] = sum_m F[m1, m2, m3] exp(-+2j pi (k1[m1] x[j] + k2[m2] y[j] + k3[m3] z[j]))``

    with ``-`` for ``Direction.Forward`` and ``+`` for ``Direction.Reverse`` and no scaling.  n1, n2, n3 >= 1, the fine grid
    ``grid_len = prod(grid_shape) <= 2^28``, 1 <= M <= 2^30, eps in [1e-14, 1e-1].  The points are host memory
    (arrays or sequences) and are sorted once here; :meth:`from_device` takes them from device memory, :meth:`set_points`
    replaces them."""

    _prefix = "nufft3d"
    _rank = 3

    def __init__(self, n_modes, x, y, z, eps: float | None = None):
        self._init(n_modes, (x, y, z), eps)

    @classmethod
    def from_device(cls, n_modes, x, y, z, eps: float | None = None, stream=None):
        """as :meth:`PlannerNufft64.from_device`, the coordinates as three contiguous float64 device tensors of M values"""
        return cls._from_device(tuple(n_modes), (x, y, z), eps, stream)

    def set_points(self, x, y, z, stream=None) -> None:
        """as :meth:`PlannerNufft64.set_points`"""
        self._set_points((x, y, z), stream)


class PlannerNufft3d32(PlannerNufft3d64):
    """f32 twin of :class:`PlannerNufft3d64`: eps in [1e-6, 1e-1]; the points stay doubles and the tables of 1 / phi^ are built
    in f64 and rounded"""

    _sfx = "32"
    _dtype = np.float32
    _eps = 1e-6


def _nufft_nd_batched(rank, t, x_re, x_im, planner, direction, out, work, stream):
    import torch

    want = torch.float64 if planner._dtype == np.float64 else torch.float32
    nm = tuple(planner.n_modes)
    if len(nm) != rank:
        raise ValueError(f"nufft{rank}d{t}_batched: need a planner of {rank} dimensions, not of {len(nm)}")
    row_major = [int(np.prod(nm[i + 1:], dtype=np.int64)) for i in range(rank)]  # the stride of axis i of a mode-side array

    def plane(v, what, modes):
        """(transforms, distance, batched) of a point-side or mode-side plane"""
        if not _is_torch(v) or v.device.type != "cuda" or v.dtype != want:
            raise TypeError(f"{what}: need a {want} device tensor")
        per = planner.n if modes else planner.m_points
        if modes and (v.dim() == rank + 1 or (v.dim() == rank and tuple(v.shape) == nm)):  # (batch, N1, .., ND) or (N1, .., ND)
            ok = tuple(v.shape[-rank:]) == nm and all(nm[i] == 1 or v.stride(i - rank) == row_major[i] for i in range(rank))
            batched = v.dim() == rank + 1
        else:  # (batch, per) or (per,)
            ok = v.dim() in (1, 2) and v.shape[-1] == per and (per == 1 or v.stride(-1) == 1)
            batched = v.dim() == 2
        if not ok:
            dims = ", ".join(str(k) for k in nm)
            shapes = f"(batch, {dims}), ({dims}), (batch, {per}) or ({per},)" if modes else f"(batch, {per}) or ({per},)"
            raise ValueError(f"{what}: need shape {shapes} with a contiguous last axis, not {tuple(v.shape)}")
        rows = v.shape[0] if batched else 1
        dist = v.stride(0) if batched and rows > 1 else per
        if dist < per:
            raise ValueError(f"{what}: rows overlap")
        return rows, dist, batched

    batch, in_dist, batched = plane(x_re, "x_re", t == 2)
    if x_im is not None and (plane(x_im, "x_im", t == 2) != (batch, in_dist, batched) or x_im.shape != x_re.shape):
        raise ValueError("x_im: need the shape and the strides of x_re")
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        if out is None:
            shape = ((batch,) if batched else ()) + (nm if t == 1 else (planner.m_points,))
            out = (torch.empty(shape, dtype=want, device=x_re.device), torch.empty(shape, dtype=want, device=x_re.device))
        out_re, out_im = out
        rows, out_dist, _ = plane(out_re, "out_re", t == 1)
        if rows != batch or plane(out_im, "out_im", t == 1)[:2] != (batch, out_dist) or out_im.shape != out_re.shape:
            raise ValueError("out: need a pair of tensors of one row per transform with equal shapes and strides")
        ws = _any_workspace(planner, batch, work)
        _check(_call(f"phast_nufft{rank}d{t}_{planner._sfx}_dev", x_re.data_ptr(), None if x_im is None else x_im.data_ptr(), in_dist,
                     out_re.data_ptr(), out_im.data_ptr(), out_dist, batch, int(direction), planner._h, ws.ptr, ws.len,
                     _stream()))
    return out_re, out_im


def nufft2d1_batched(c_re, c_im, planner, direction=Direction.Forward, out=None, work=None, stream=None):
    """Device-resident batch of two-dimensional type 1 transforms (points -> modes) through one planner: ``c_re`` (and ``c_im``,
    or ``None`` for real data) are torch device tensors of shape ``(batch, M)`` or ``(M,)`` of the planner's type whose last axis
    is contiguous; returns ``(out_re, out_im)`` of shape ``(batch, n1, n2)`` or ``(n1, n2)``.  ``out``: such a pair to write
    into, of shape ``(batch, n1, n2)``, ``(n1, n2)`` or flat, ``(batch, n1 n2)`` or ``(n1 n2,)``, with a contiguous last axis
    (it must not overlap the input or ``work``); ``work``: a device tensor of at least ``planner.workspace_len(1)`` elements
    (fewer than ``planner.workspace_len(batch)`` runs the batch in chunks), by default one from torch's allocator; ``stream``: a
    ``torch.cuda.Stream``, by default the current one."""
    return _nufft_nd_batched(2, 1, c_re, c_im, planner, direction, out, work, stream)


def nufft2d2_batched(f_re, f_im, planner, direction=Direction.Forward, out=None, work=None, stream=None):
    """Device-resident batch of two-dimensional type 2 transforms (modes -> points): as :func:`nufft2d1_batched` with inputs of
    the mode-side shapes and outputs of M values per transform"""
    return _nufft_nd_batched(2, 2, f_re, f_im, planner, direction, out, work, stream)


def nufft3d1_batched(c_re, c_im, planner, direction=Direction.Forward, out=None, work=None, stream=None):
    """Device-resident batch of three-dimensional type 1 transforms (points -> modes) through one planner: ``c_re`` (and ``c_im``,
    or ``None`` for real data) are torch device tensors of shape ``(batch, M)`` or ``(M,)`` of the planner's type whose last axis
    is contiguous; returns ``(out_re, out_im)`` of shape ``(batch, n1, n2, n3)`` or ``(n1, n2, n3)``.  ``out``: such a pair to write
    into, of shape ``(batch, n1, n2, n3)``, ``(n1, n2, n3)`` or flat, ``(batch, n1 n2 n3)`` or ``(n1 n2 n3,)``, with a contiguous last axis
    (it must not overlap the input or ``work``); ``work``: a device tensor of at least ``planner.workspace_len(1)`` elements
    (fewer than ``planner.workspace_len(batch)`` runs the batch in chunks), by default one from torch's allocator; ``stream``: a
    ``torch.cuda.Stream``, by default the current one."""
    return _nufft_nd_batched(3, 1, c_re, c_im, planner, direction, out, work, stream)


def nufft3d2_batched(f_re, f_im, planner, direction=Direction.Forward, out=None, work=None, stream=None):
    """Device-resident batch of three-dimensional type 2 transforms (modes -> points): as :func:`nufft3d1_batched` with inputs of
    the mode-side shapes and outputs of M values per transform"""
    return _nufft_nd_batched(3, 2, f_re, f_im, planner, direction, out, work, stream)


def _nufft_nd_host(rank, t, sfx, dtype, in_re, in_im, out_re, out_im, direction, planner=None, coords=None, n_modes=None, eps=None):
    a = _Slice(_flat(in_re), dtype, "in_re")
    b = _NULL if in_im is None else _Slice(_flat(in_im), dtype, "in_im")
    o_re, o_im = _Slice(_flat(out_re), dtype, "out_re"), _Slice(_flat(out_im), dtype, "out_im")
    name = f"nufft{rank}d{t}"
    if _same_place(*(s for s in (a, b, o_re, o_im) if s is not _NULL)):
        raise TypeError(f"{name}_{sfx} takes host arrays ({name}_batched takes device tensors)")
    if (b is not _NULL and b.len != a.len) or o_re.len != o_im.len:
        _check(2)
    if planner is not None:
        _check(_call(f"phast_{name}_{sfx}_with_planner", a.ptr, b.ptr, a.len, o_re.ptr, o_im.ptr, o_re.len, int(direction),
                     planner._h))
        return
    pts = [np.ascontiguousarray(v, dtype=np.float64).reshape(-1) for v in coords]
    if len(n_modes) != rank:
        want = ", ".join(f"n{i + 1}" for i in range(rank))
        raise ValueError(f"{name}_{sfx}: the mode-side arrays need shape ({want}), not {tuple(n_modes)}")
    shape = tuple(int(v) for v in n_modes)
    m, n = pts[0].size, int(np.prod(shape, dtype=np.int64))
    n_in, n_out = (m, n) if t == 1 else (n, m)
    if any(p.size != m for p in pts) or a.len != n_in or o_re.len != n_out:
        _check(2)
    _check(_call(f"phast_{name}_{sfx}", *(p.ctypes.data_as(C.c_void_p) for p in pts), m, a.ptr, b.ptr, o_re.ptr, o_im.ptr, *shape,
                 float(eps), int(direction)))


def nufft2d1_64(x, y, c_re, c_im, out_re, out_im, eps: float = 1e-12, direction=Direction.Forward) -> None:
    """f64 two-dimensional type 1 transform of one host vector of M values at the points ``(x, y)`` (``c_im`` may be ``None``:
    real data) into host arrays of shape ``(n1, n2)``, through a planner of its own (blocking)"""
    _nufft_nd_host(2, 1, "64", np.float64, c_re, c_im, out_re, out_im, direction, coords=(x, y), n_modes=np.shape(out_re), eps=eps)


def nufft2d1_32(x, y, c_re, c_im, out_re, out_im, eps: float = 1e-6, direction=Direction.Forward) -> None:
    """f32 twin of :func:`nufft2d1_64`"""
    _nufft_nd_host(2, 1, "32", np.float32, c_re, c_im, out_re, out_im, direction, coords=(x, y), n_modes=np.shape(out_re), eps=eps)


def nufft2d2_64(x, y, f_re, f_im, out_re, out_im, eps: float = 1e-12, direction=Direction.Forward) -> None:
    """f64 two-dimensional type 2 transform of one host array of shape ``(n1, n2)`` into host arrays of M values at the points
    ``(x, y)`` (blocking)"""
    _nufft_nd_host(2, 2, "64", np.float64, f_re, f_im, out_re, out_im, direction, coords=(x, y), n_modes=np.shape(f_re), eps=eps)


def nufft2d2_32(x, y, f_re, f_im, out_re, out_im, eps: float = 1e-6, direction=Direction.Forward) -> None:
    """f32 twin of :func:`nufft2d2_64`"""
    _nufft_nd_host(2, 2, "32", np.float32, f_re, f_im, out_re, out_im, direction, coords=(x, y), n_modes=np.shape(f_re), eps=eps)


def nufft2d1_64_with_planner(c_re, c_im, out_re, out_im, planner: PlannerNufft2d64, direction=Direction.Forward) -> None:
    _nufft_nd_host(2, 1, "64", np.float64, c_re, c_im, out_re, out_im, direction, planner)


def nufft2d1_32_with_planner(c_re, c_im, out_re, out_im, planner: PlannerNufft2d32, direction=Direction.Forward) -> None:
    _nufft_nd_host(2, 1, "32", np.float32, c_re, c_im, out_re, out_im, direction, planner)


def nufft2d2_64_with_planner(f_re, f_im, out_re, out_im, planner: PlannerNufft2d64, direction=Direction.Forward) -> None:
    _nufft_nd_host(2, 2, "64", np.float64, f_re, f_im, out_re, out_im, direction, planner)


def nufft2d2_32_with_planner(f_re, f_im, out_re, out_im, planner: PlannerNufft2d32, direction=Direction.Forward) -> None:
    _nufft_nd_host(2, 2, "32", np.float32, f_re, f_im, out_re, out_im, direction, planner)


def nufft3d1_64(x, y, z, c_re, c_im, out_re, out_im, eps: float = 1e-12, direction=Direction.Forward) -> None:
    """f64 three-dimensional type 1 transform of one host vector of M values at the points ``(x, y, z)`` (``c_im`` may be ``None``:
    real data) into host arrays of shape ``(n1, n2, n3)``, through a planner of its own (blocking)"""
    _nufft_nd_host(3, 1, "64", np.float64, c_re, c_im, out_re, out_im, direction, coords=(x, y, z), n_modes=np.shape(out_re), eps=eps)


def nufft3d1_32(x, y, z, c_re, c_im, out_re, out_im, eps: float = 1e-6, direction=Direction.Forward) -> None:
    """f32 twin of :func:`nufft3d1_64`"""
    _nufft_nd_host(3, 1, "32", np.float32, c_re, c_im, out_re, out_im, direction, coords=(x, y, z), n_modes=np.shape(out_re), eps=eps)


def nufft3d2_64(x, y, z, f_re, f_im, out_re, out_im, eps: float = 1e-12, direction=Direction.Forward) -> None:
    """f64 three-dimensional type 2 transform of one host array of shape ``(n1, n2, n3)`` into host arrays of M values at the points
    ``(x, y)`` (blocking)"""
    _nufft_nd_host(3, 2, "64", np.float64, f_re, f_im, out_re, out_im, direction, coords=(x, y, z), n_modes=np.shape(f_re), eps=eps)


def nufft3d2_32(x, y, z, f_re, f_im, out_re, out_im, eps: float = 1e-6, direction=Direction.Forward) -> None:
    """f32 twin of :func:`nufft3d2_64`"""
    _nufft_nd_host(3, 2, "32", np.float32, f_re, f_im, out_re, out_im, direction, coords=(x, y, z), n_modes=np.shape(f_re), eps=eps)


def nufft3d1_64_with_planner(c_re, c_im, out_re, out_im, planner: PlannerNufft3d64, direction=Direction.Forward) -> None:
    _nufft_nd_host(3, 1, "64", np.float64, c_re, c_im, out_re, out_im, direction, planner)


def nufft3d1_32_with_planner(c_re, c_im, out_re, out_im, planner: PlannerNufft3d32, direction=Direction.Forward) -> None:
    _nufft_nd_host(3, 1, "32", np.float32, c_re, c_im, out_re, out_im, direction, planner)


def nufft3d2_64_with_planner(f_re, f_im, out_re, out_im, planner: PlannerNufft3d64, direction=Direction.Forward) -> None:
    _nufft_nd_host(3, 2, "64", np.float64, f_re, f_im, out_re, out_im, direction, planner)


def nufft3d2_32_with_planner(f_re, f_im, out_re, out_im, planner: PlannerNufft3d32, direction=Direction.Forward) -> None:
    _nufft_nd_host(3, 2, "32", np.float32, f_re, f_im, out_re, out_im, direction, planner)


def _nufft_nd(t, coords, v, n_modes, eps, direction):
    import torch

    rank = len(coords)
    word = {2: "two", 3: "three"}[rank]
    if t == 2:  # the modes are the last `rank` axes of v
        if not _is_torch(v) or v.dim() < rank:
            raise TypeError(f"need a device tensor of at least {word} axes")
        n_modes = tuple(v.shape[-rank:])
    p64, p32 = {2: (PlannerNufft2d64, PlannerNufft2d32), 3: (PlannerNufft3d64, PlannerNufft3d32)}[rank]
    kinds = {torch.float64: (p64, torch.float64), torch.complex128: (p64, torch.float64),
             torch.float32: (p32, torch.float32), torch.complex64: (p32, torch.float32)}
    if not _is_torch(v) or v.device.type != "cuda" or v.dtype not in kinds or v.dim() < (1 if t == 1 else rank):
        raise TypeError(f"need a float64, float32, complex128 or complex64 device tensor of at least one axis (points) or {word} (modes)")
    cls, real = kinds[v.dtype]
    planner = cls(n_modes, *coords, eps)
    tail_in, tail_out = ((planner.m_points,), planner.n_modes) if t == 1 else (planner.n_modes, (planner.m_points,))
    if tuple(v.shape[-len(tail_in):]) != tail_in:
        raise ValueError(f"the last axes are {tuple(v.shape[-len(tail_in):])}, the transform takes {tail_in}")
    lead = tuple(v.shape[:-len(tail_in)])
    n_in, n_out = int(np.prod(tail_in)), int(np.prod(tail_out))
    rows = v.reshape(-1, n_in)
    if v.is_complex():
        x_re, x_im = rows.real.contiguous(), rows.imag.contiguous()
    else:
        x_re, x_im = rows.contiguous(), None
    out = torch.empty((2, rows.shape[0], n_out), dtype=real, device=v.device)
    if rows.shape[0]:
        _nufft_nd_batched(rank, t, x_re, x_im, planner, direction, (out[0], out[1]), None, None)
        torch.cuda.current_stream().synchronize()  # the temporary planner's tables die with it
    return torch.complex(out[0], out[1]).reshape(lead + tail_out)


def nufft2d1(x, y, c, n_modes, eps: float | None = None, direction=Direction.Forward):
    """Two-dimensional type 1 non-uniform FFT of a real or complex device tensor ``c`` over its last axis (M values at the
    points ``(x, y)``, in turns) into ``n_modes = (n1, n2)`` modes in ``fftfreq`` order: a new complex tensor of shape
    ``c.shape[:-1] + (n1, n2)``.  float64 / complex128 run in f64 (eps defaults to 1e-12), float32 / complex64 in f32 (1e-6)."""
    return _nufft_nd(1, (x, y), c, n_modes, eps, direction)


def nufft2d2(x, y, F, eps: float | None = None, direction=Direction.Forward):
    """Two-dimensional type 2 non-uniform FFT of a real or complex device tensor ``F`` of modes over its last two axes, evaluated
    at the points ``(x, y)`` (in turns): a new complex tensor of shape ``F.shape[:-2] + (len(x),)``"""
    return _nufft_nd(2, (x, y), F, None, eps, direction)


def nufft3d1(x, y, z, c, n_modes, eps: float | None = None, direction=Direction.Forward):
    """Three-dimensional type 1 non-uniform FFT of a real or complex device tensor ``c`` over its last axis (M values at the
    points ``(x, y, z)``, in turns) into ``n_modes = (n1, n2, n3)`` modes in ``fftfreq`` order: a new complex tensor of shape
    ``c.shape[:-1] + (n1, n2, n3)``.  float64 / complex128 run in f64 (eps defaults to 1e-12), float32 / complex64 in f32 (1e-6)."""
    return _nufft_nd(1, (x, y, z), c, n_modes, eps, direction)


def nufft3d2(x, y, z, F, eps: float | None = None, direction=Direction.Forward):
    """Three-dimensional type 2 non-uniform FFT of a real or complex device tensor ``F`` of modes over its last three axes, evaluated
    at the points ``(x, y, z)`` (in turns): a new complex tensor of shape ``F.shape[:-3] + (len(x),)``"""
    return _nufft_nd(2, (x, y, z), F, None, eps, direction)


# ---------------------------------------------------------------------------------------------
# multi-dimensional transforms over every axis of a row-major array (numpy fftn / ifftn / rfftn / irfftn; no reference
# counterpart).  Arrays and tensors of any view shape are taken by their contiguous elements.
# ---------------------------------------------------------------------------------------------
def _flat(x):
    """a contiguous array or tensor of any shape as a 1-D view of its elements (anything else goes to _Slice as it is)"""
    if _is_torch(x):
        return x.view(-1) if x.dim() != 1 and x.is_contiguous() else x
    if isinstance(x, np.ndarray) and x.ndim != 1 and x.flags.c_contiguous:
        return x.reshape(-1)
    return x


class _NdHandle(_AnyHandle):
    """the handle of a multi-dimensional planner: phast_planner_{_prefix}{_sfx}_*"""

    _prefix = "nd"

    def __init__(self, shape):
        self.shape = tuple(int(d) for d in shape)
        dims = (C.c_size_t * max(1, len(self.shape)))(*self.shape)
        self._new(dims, len(self.shape))
        self.n = int(np.prod(self.shape, dtype=np.int64))

    def workspace_len(self, batch: int = 1) -> int:
        """Elements of T a device call of ``batch`` arrays works in at full speed; ``workspace_len(1)`` serves any batch, in
        chunks (include/phastft_hip.h gives the smallest legal length)"""
        return self._workspace_len(batch)


class _PlannerNd(_NdHandle):
    def time_steps(self, reals, imags, batch: int = 1, dist: int | None = None, workspace=None, reps: int = 10):
        """Average HIP-event milliseconds of every step of a forward call on device tensors, in the order describe() lists
        them (row transforms and transposes; measurement hook)"""
        re, im = _Slice(_flat(reals), self._dtype, "reals"), _Slice(_flat(imags), self._dtype, "imags")
        ws = _any_workspace(self, batch, workspace)
        ms, ns = (C.c_float * 17)(), C.c_size_t()
        _check(self._fn("time_steps")(self._h, re.ptr, im.ptr, batch, self.n if dist is None else dist, ws.ptr, ws.len,
                                      reps, ms, C.byref(ns), _stream()))
        return [float(ms[i]) for i in range(ns.value)]


class PlannerNd64(_PlannerNd):
    """f64 complex transforms over every axis of a row-major array of rank 1 .. 8 (each axis 1 .. 2^29, <= 2^30 points)"""


class PlannerNd32(_PlannerNd):
    """f32 twin of :class:`PlannerNd64`"""

    _sfx = "32"
    _dtype = np.float32


class _PlannerR2cNd(_NdHandle):
    _prefix = "r2c_nd"

    def __init__(self, shape):
        super().__init__(shape)
        self.half = self.n // self.shape[-1] * (self.shape[-1] // 2 + 1)  # points of the half spectrum


class PlannerR2cNd64(_PlannerR2cNd):
    """f64 real transforms (numpy rfftn / irfftn) over every axis of a row-major array of rank 1 .. 8"""


class PlannerR2cNd32(_PlannerR2cNd):
    """f32 twin of :class:`PlannerR2cNd64`"""

    _sfx = "32"
    _dtype = np.float32


def _dims(shape):
    shape = tuple(int(d) for d in shape)
    return (C.c_size_t * max(1, len(shape)))(*shape), len(shape)


def _fft_nd(sfx, dtype, reals, imags, shape, direction, planner=None):
    re, im = _Slice(_flat(reals), dtype, "reals"), _Slice(_flat(imags), dtype, "imags")
    direction = int(direction)
    if _same_place(re, im):
        if re.len != im.len:
            _check(2)
        own = planner is None
        if own:
            planner = (PlannerNd64 if sfx == "64" else PlannerNd32)(shape)
        ws = _any_workspace(planner, 1)
        _check(_call(f"phast_fft_{sfx}_nd_dev", re.ptr, im.ptr, re.len, 1, re.len, direction, planner._h, ws.ptr, ws.len,
                     _stream()))
        if own:
            import torch

            torch.cuda.current_stream().synchronize()  # the temporary planner's tables die with it
        return
    args = [re.ptr, re.len, im.ptr, im.len]
    if planner is None:
        _check(_call(f"phast_fft_{sfx}_nd", *args, *_dims(shape), direction))
    else:
        _check(_call(f"phast_fft_{sfx}_nd_with_planner", *args, direction, planner._h))


def fft_64_nd(reals, imags, shape, direction: Direction) -> None:
    """In-place f64 DFT over every axis of the row-major array ``shape`` held by (reals, imags) (numpy fftn; Reverse is
    ifftn: scaled by 1 / prod(shape))"""
    _fft_nd("64", np.float64, reals, imags, shape, direction)


def fft_32_nd(reals, imags, shape, direction: Direction) -> None:
    """f32 twin of :func:`fft_64_nd`"""
    _fft_nd("32", np.float32, reals, imags, shape, direction)


def fft_64_nd_with_planner(reals, imags, direction: Direction, planner: PlannerNd64) -> None:
    _fft_nd("64", np.float64, reals, imags, planner.shape, direction, planner)


def fft_32_nd_with_planner(reals, imags, direction: Direction, planner: PlannerNd32) -> None:
    _fft_nd("32", np.float32, reals, imags, planner.shape, direction, planner)


def fft_nd_batched(reals, imags, direction: Direction, planner, batch: int = 1, dist: int | None = None,
                   workspace=None) -> None:
    """Device-resident batch of multi-dimensional transforms: array b at ``b*dist`` (default prod(shape)).  ``workspace``: a
    device tensor of the planner's type of at least ``planner.workspace_len(1)`` elements (fewer than
    ``planner.workspace_len(batch)`` runs the batch in chunks); by default one from torch's allocator."""
    dtype, sfx, n = planner._dtype, planner._sfx, planner.n
    re, im = _Slice(_flat(reals), dtype, "reals"), _Slice(_flat(imags), dtype, "imags")
    if not _same_place(re, im):
        raise TypeError("fft_nd_batched needs device tensors")
    dist = n if dist is None else dist
    _need("reals", re.len, batch, dist, n)
    _need("imags", im.len, batch, dist, n)
    ws = _any_workspace(planner, batch, workspace)
    _check(_call(f"phast_fft_{sfx}_nd_dev", re.ptr, im.ptr, n, batch, dist, int(direction), planner._h, ws.ptr, ws.len,
                 _stream()))


def _real_nd(c2r, fs, dtype, a, b, c, shape, planner=None):
    """R2C: (a = the real array; b, c = the planes); C2R: (a, b = the planes; c = the real array)"""
    names = ("input_re", "input_im", "output") if c2r else ("input_re", "output_re", "output_im")
    sa, sb, sc = (_Slice(_flat(x), dtype, w) for x, w in zip((a, b, c), names))
    sfx, kind = fs[1:], "c2r" if c2r else "r2c"
    if _same_place(sa, sb, sc):
        own = planner is None
        if own:
            planner = (PlannerR2cNd64 if fs == "f64" else PlannerR2cNd32)(shape)
        n, h = planner.n, planner.half
        checks = ((8, sc.len, n), (9, sa.len, h), (10, sb.len, h)) if c2r else ((5, sa.len, n), (6, sb.len, h), (7, sc.len, h))
        for code, got, want in checks:
            if got != want:
                _check(code)
        ws = _any_workspace(planner, 1)
        dists = (h, n) if c2r else (n, h)
        _check(_call(f"phast_{kind}_fft_{fs}_nd_dev", sa.ptr, sb.ptr, sc.ptr, n, 1, *dists, planner._h, ws.ptr, ws.len,
                     _stream()))
        if own:
            import torch

            torch.cuda.current_stream().synchronize()  # the temporary planner's tables die with it
        return
    args = [sa.ptr, sa.len, sb.ptr, sb.len, sc.ptr, sc.len]
    if planner is None:
        _check(_call(f"phast_{kind}_fft_{fs}_nd", *args, *_dims(shape)))
    else:
        _check(_call(f"phast_{kind}_fft_{fs}_nd_with_planner", *args, planner._h))


def r2c_fft_f64_nd(input_re, output_re, output_im, shape) -> None:
    """f64 numpy rfftn of the real row-major array ``shape``: the half spectrum [n_0 .. n_{r-2}][n_{r-1} // 2 + 1] into two
    planes (unnormalised)"""
    _real_nd(False, "f64", np.float64, input_re, output_re, output_im, shape)


def r2c_fft_f32_nd(input_re, output_re, output_im, shape) -> None:
    """f32 twin of :func:`r2c_fft_f64_nd`"""
    _real_nd(False, "f32", np.float32, input_re, output_re, output_im, shape)


def r2c_fft_f64_nd_with_planner(input_re, output_re, output_im, planner: PlannerR2cNd64) -> None:
    _real_nd(False, "f64", np.float64, input_re, output_re, output_im, planner.shape, planner)


def r2c_fft_f32_nd_with_planner(input_re, output_re, output_im, planner: PlannerR2cNd32) -> None:
    _real_nd(False, "f32", np.float32, input_re, output_re, output_im, planner.shape, planner)


def c2r_fft_f64_nd(input_re, input_im, output, shape) -> None:
    """f64 numpy irfftn(X, shape) of the half spectrum planes, scaled by 1 / prod(shape); the input planes stay unchanged"""
    _real_nd(True, "f64", np.float64, input_re, input_im, output, shape)


def c2r_fft_f32_nd(input_re, input_im, output, shape) -> None:
    """f32 twin of :func:`c2r_fft_f64_nd`"""
    _real_nd(True, "f32", np.float32, input_re, input_im, output, shape)


def c2r_fft_f64_nd_with_planner(input_re, input_im, output, planner: PlannerR2cNd64) -> None:
    _real_nd(True, "f64", np.float64, input_re, input_im, output, planner.shape, planner)


def c2r_fft_f32_nd_with_planner(input_re, input_im, output, planner: PlannerR2cNd32) -> None:
    _real_nd(True, "f32", np.float32, input_re, input_im, output, planner.shape, planner)


def _real_nd_batched(c2r, a, b, c, planner, batch, in_dist, out_dist, workspace):
    dtype, fs = planner._dtype, "f64" if planner._dtype == np.float64 else "f32"
    names = ("input_re", "input_im", "output") if c2r else ("input_re", "output_re", "output_im")
    sa, sb, sc = (_Slice(_flat(x), dtype, w) for x, w in zip((a, b, c), names))
    kind = "c2r" if c2r else "r2c"
    if not _same_place(sa, sb, sc):
        raise TypeError(f"{kind}_nd_batched needs device tensors")
    n, h = planner.n, planner.half
    in_dist = (h if c2r else n) if in_dist is None else in_dist
    out_dist = (n if c2r else h) if out_dist is None else out_dist
    if c2r:
        _need("input_re", sa.len, batch, in_dist, h)
        _need("input_im", sb.len, batch, in_dist, h)
        _need("output", sc.len, batch, out_dist, n)
    else:
        _need("input_re", sa.len, batch, in_dist, n)
        _need("output_re", sb.len, batch, out_dist, h)
        _need("output_im", sc.len, batch, out_dist, h)
    ws = _any_workspace(planner, batch, workspace)
    _check(_call(f"phast_{kind}_fft_{fs}_nd_dev", sa.ptr, sb.ptr, sc.ptr, n, batch, in_dist, out_dist, planner._h, ws.ptr,
                 ws.len, _stream()))


def r2c_nd_batched(input_re, output_re, output_im, planner, batch: int = 1, in_dist: int | None = None,
                   out_dist: int | None = None, workspace=None) -> None:
    """Device-resident batch of multi-dimensional R2C transforms: real array b at ``b*in_dist`` (default prod(shape)), its
    half spectrum at ``b*out_dist`` (default ``planner.half``); ``workspace`` as for :func:`fft_nd_batched`"""
    _real_nd_batched(False, input_re, output_re, output_im, planner, batch, in_dist, out_dist, workspace)


def c2r_nd_batched(input_re, input_im, output, planner, batch: int = 1, in_dist: int | None = None,
                   out_dist: int | None = None, workspace=None) -> None:
    """Device-resident batch of multi-dimensional C2R transforms: half spectrum b at ``b*in_dist`` (default
    ``planner.half``), its real array at ``b*out_dist`` (default prod(shape)); ``workspace`` as for :func:`fft_nd_batched`"""
    _real_nd_batched(True, input_re, input_im, output, planner, batch, in_dist, out_dist, workspace)


class TransformList:
    """`count` independent transforms at arbitrary device addresses, prepared once (the pointer arrays) and enqueued by
    ONE call into the library -- each runs exactly as a single-transform call (``phast_fft_*_dit_many_dev``)."""

    def __init__(self, pairs, n: int, planner):
        dtype = planner._dtype
        self._keep = [(_Slice(r, dtype, "reals"), _Slice(m, dtype, "imags")) for r, m in pairs]
        for r, m in self._keep:
            if not (r.dev and m.dev) or r.len != n or m.len != n:
                raise TypeError("TransformList needs device tensors of n elements each")
        k = len(self._keep)
        self._re = (C.c_void_p * k)(*[r.ptr.value for r, _ in self._keep])
        self._im = (C.c_void_p * k)(*[m.ptr.value for _, m in self._keep])
        self.n, self.count, self.planner = n, k, planner

    def run(self, direction: Direction, first: int = 0, count: int | None = None) -> None:
        k = self.count - first if count is None else count
        if first < 0 or k < 0 or first + k > self.count:
            raise ValueError("range outside the list")
        off = first * C.sizeof(C.c_void_p)
        _check(_call(f"phast_fft_{self.planner._sfx}_dit_many_dev", C.addressof(self._re) + off,
                     C.addressof(self._im) + off, k, self.n, int(direction), self.planner._h, _stream()))


def fft_dit_strided(reals, imags, n: int, direction: Direction, planner, batch: int, stride: int,
                    twiddle_n: int = 0, twiddle_col0: int = 0) -> None:
    """Device-resident "column FFTs": the tensors hold a row-major ``[n][stride]`` array whose first ``batch`` columns
    are transformed along the rows' axis, in place (transform ``c`` = elements ``c + j*stride``).  ``stride`` and
    ``batch`` powers of two, ``batch <= stride``, ``n >= 64``; ``batch >= 16`` is always served, 8 columns for every n
    but 2^6 / 2^12 / 2^13, 4 columns for n = 2^10 / 2^20 only -- anything narrower raises :class:`PhastPanic` with code
    ``ERR_INVALID_ARG`` before anything runs (transpose and use :func:`fft_dit_batched`).  With ``twiddle_n`` the first pass multiplies element
    ``j`` of column ``c`` by ``W_twiddle_n^(j*(twiddle_col0 + c))`` on load (the inter-factor twiddle of a four-step
    split).  No reference counterpart."""
    dtype, sfx = planner._dtype, planner._sfx
    re, im = _Slice(reals, dtype, "reals"), _Slice(imags, dtype, "imags")
    if not _same_place(re, im):
        raise TypeError("fft_dit_strided needs device tensors")
    if re.len != im.len:
        _check(2)
    if re.len < n * stride:
        raise ValueError("the tensors must hold n*stride elements")
    if twiddle_n:
        _check(_call(f"phast_fft_{sfx}_dit_strided_tw_dev", re.ptr, im.ptr, n, batch, 1, stride, int(direction), planner._h,
                     twiddle_n, twiddle_col0, _stream()))
        return
    _check(_call(f"phast_fft_{sfx}_dit_strided_dev", re.ptr, im.ptr, n, batch, 1, stride, int(direction), planner._h,
                 _stream()))


def r2c_fft_batched(input_re, output_re, output_im, planner, batch: int) -> None:
    """Device-resident batch of R2C transforms: inputs ``n`` apart, outputs ``n/2 + 1`` apart."""
    fs = "f64" if planner._dtype == np.float64 else "f32"
    i, ore, oim = (_Slice(x, planner._dtype, w) for x, w in ((input_re, "input_re"), (output_re, "output_re"),
                                                              (output_im, "output_im")))
    n, out = planner.n, planner.n // 2 + 1
    if not _same_place(i, ore, oim) or i.len != batch * n or ore.len != batch * out or oim.len != batch * out:
        raise ValueError("need device tensors of batch*n, batch*(n/2+1), batch*(n/2+1) elements")
    _check(_call(f"phast_r2c_fft_{fs}_dev", i.ptr, ore.ptr, oim.ptr, batch, n, out, planner._h, _stream()))


def c2r_fft_batched(input_re, input_im, output, planner, batch: int) -> None:
    """Device-resident batch of C2R transforms: inputs ``n/2 + 1`` apart, outputs ``n`` apart."""
    fs = "f64" if planner._dtype == np.float64 else "f32"
    ire, iim, out = (_Slice(x, planner._dtype, w) for x, w in ((input_re, "input_re"), (input_im, "input_im"),
                                                                (output, "output")))
    n, half1 = planner.n, planner.n // 2 + 1
    if not _same_place(ire, iim, out) or out.len != batch * n or ire.len != batch * half1 or iim.len != batch * half1:
        raise ValueError("need device tensors of batch*(n/2+1), batch*(n/2+1), batch*n elements")
    _check(_call(f"phast_c2r_fft_{fs}_dev", ire.ptr, iim.ptr, out.ptr, batch, half1, n, planner._h, _stream()))


class TwiddleGrid64(_Handle):
    """Device tables of W_N for the inter-factor twiddle of a four-step split (``include/phastft_hip.h``:
    ``phast_twiddle_grid64_*``): ``apply`` multiplies element (r, c) of a row-major device block by
    ``W_N^((row0 + r)*(col0 + c))`` in place.  Used by :mod:`phastft_amd.distributed`."""

    _stem = "phast_twiddle_"
    _prefix = "grid"

    def __init__(self, n: int):
        self._new(n)
        self.n = n

    def apply(self, reals, imags, rows: int, cols: int, row0: int = 0, col0: int = 0, row_pitch: int | None = None):
        re, im = _Slice(reals, self._dtype, "reals"), _Slice(imags, self._dtype, "imags")
        if not _same_place(re, im):
            raise TypeError("TwiddleGrid.apply needs device tensors")
        pitch = cols if row_pitch is None else row_pitch
        if re.len != im.len or (rows and re.len < (rows - 1) * pitch + cols):
            raise ValueError("block does not fit the tensors")
        _check(self._fn("apply_dev")(self._h, re.ptr, im.ptr, rows, cols, pitch, row0, col0, _stream()))


class TwiddleGrid32(TwiddleGrid64):
    _sfx = "32"
    _dtype = np.float32


# ---------------------------------------------------------------------------------------------
# bit reversal  (algorithms/bravo.rs:303,317; public with feature bench-internals)
# ---------------------------------------------------------------------------------------------
def _bit_rev(fs, dtype, data, n):
    d = _Slice(data, dtype, "data")
    if d.len != (1 << n):
        raise PhastPanic(16, "Data length must be 2^n")  # bravo.rs:228
    if d.dev:
        _check(_call(f"phast_bit_rev_{fs}_dev", d.ptr, n, 1, d.len, _stream()))
    else:
        _check(_call(f"phast_bit_rev_{fs}", d.ptr, d.len, n))


def bit_rev_bravo_f64(data, n: int) -> None:
    """bravo.rs:317"""
    _bit_rev("f64", np.float64, data, n)


def bit_rev_bravo_f32(data, n: int) -> None:
    """bravo.rs:303"""
    _bit_rev("f32", np.float32, data, n)


# ---------------------------------------------------------------------------------------------
# Complex<T> <-> planes  (complex_nums.rs:11-56; public with feature bench-internals)
# ---------------------------------------------------------------------------------------------
def _np_dtype(x):
    if _is_torch(x):
        import torch

        return np.float64 if x.dtype == torch.float64 else np.float32
    return np.float64 if x.dtype == np.float64 else np.float32


def _scalars(x):
    """a Complex<T> array as its 2 n scalars (`bytemuck::cast_slice`, complex_nums.rs:26,38); real arrays pass through"""
    if _is_torch(x):
        import torch

        return torch.view_as_real(x).reshape(-1) if x.is_complex() else x
    return x.view(np.float64 if x.dtype == np.complex128 else np.float32) if np.iscomplexobj(x) else x


def _like(x, n, dtype):
    if _is_torch(x):
        import torch

        return torch.empty(n, dtype=torch.float64 if dtype == np.float64 else torch.float32, device=x.device)
    return np.empty(n, dtype)


def deinterleave(data):
    """complex_nums.rs:11-17: ``[1, 2, 3, 4] -> ([1, 3], [2, 4])`` for any length (an odd last element is dropped, as
    `chunks_exact(2)` does).  A numpy array (host slice) or a torch cuda tensor (device, asynchronous on the current stream);
    returns two new arrays of the same kind."""
    data = _scalars(data)
    dtype = _np_dtype(data)
    fs = "f64" if dtype == np.float64 else "f32"
    d = _Slice(data, dtype, "input")
    a, b = _like(data, d.len // 2, dtype), _like(data, d.len // 2, dtype)
    sa, sb = _Slice(a, dtype, "out_a"), _Slice(b, dtype, "out_b")
    if d.dev:
        _check(_call(f"phast_deinterleave_{fs}_dev", d.ptr, d.len, sa.ptr, sb.ptr, _stream()))
    else:
        _check(_call(f"phast_deinterleave_{fs}", d.ptr, d.len, sa.ptr, sa.len, sb.ptr, sb.len))
    return a, b


def deinterleave_complex64(signal):
    """complex_nums.rs:25-28: a `&[Complex<f64>]` (numpy complex128 / torch complex128) into (reals, imags)"""
    return deinterleave(signal)


def deinterleave_complex32(signal):
    """complex_nums.rs:37-40: a `&[Complex<f32>]` (numpy complex64 / torch complex64) into (reals, imags)"""
    return deinterleave(signal)


def combine_re_im(reals, imags):
    """complex_nums.rs:47-56: (reals, imags) -> one Complex<T> array; panics (PhastPanic) unless the lengths agree"""
    dtype = _np_dtype(reals)
    fs = "f64" if dtype == np.float64 else "f32"
    r, m = _Slice(reals, dtype, "reals"), _Slice(imags, dtype, "imags")
    dev = _same_place(r, m)
    if r.len != m.len:
        raise PhastPanic(2, "assertion `left == right` failed")  # complex_nums.rs:48
    out = _like(reals, 2 * r.len, dtype)
    so = _Slice(out, dtype, "out")
    if dev:
        _check(_call(f"phast_combine_re_im_{fs}_dev", r.ptr, m.ptr, r.len, so.ptr, _stream()))
    else:
        _check(_call(f"phast_combine_re_im_{fs}", r.ptr, r.len, m.ptr, m.len, so.ptr, so.len))
    if _is_torch(out):
        import torch

        return torch.view_as_complex(out.reshape(-1, 2))
    return out.view(np.complex128 if dtype == np.float64 else np.complex64)


# ---------------------------------------------------------------------------------------------
# R2C / C2R  (algorithms/r2c.rs:521-895)
# ---------------------------------------------------------------------------------------------
def _r2c(fs, dtype, input_re, output_re, output_im, planner=None):
    i, ore, oim = _Slice(input_re, dtype, "input_re"), _Slice(output_re, dtype, "output_re"), _Slice(
        output_im, dtype, "output_im")
    if _same_place(i, ore, oim):
        own = planner is None
        if own:
            planner = (PlannerR2c64 if fs == "f64" else PlannerR2c32)(i.len)  # r2c.rs:522
        n, half = planner.n, planner.n // 2
        if i.len != n:
            _check(5)
        if ore.len != half + 1:
            _check(6)
        if oim.len != half + 1:
            _check(7)
        _check(_call(f"phast_r2c_fft_{fs}_dev", i.ptr, ore.ptr, oim.ptr, 1, n, half + 1, planner._h, _stream()))
        if own:
            import torch

            torch.cuda.current_stream().synchronize()
        return
    args = [i.ptr, i.len, ore.ptr, ore.len, oim.ptr, oim.len]
    if planner is None:
        _check(_call(f"phast_r2c_fft_{fs}", *args))
    else:
        _check(_call(f"phast_r2c_fft_{fs}_with_planner", *args, planner._h))


def r2c_fft_f64(input_re, output_re, output_im) -> None:
    """r2c.rs:521"""
    _r2c("f64", np.float64, input_re, output_re, output_im)


def r2c_fft_f32(input_re, output_re, output_im) -> None:
    """r2c.rs:598"""
    _r2c("f32", np.float32, input_re, output_re, output_im)


def r2c_fft_f64_with_planner(input_re, output_re, output_im, planner: PlannerR2c64) -> None:
    """r2c.rs:535"""
    _r2c("f64", np.float64, input_re, output_re, output_im, planner)


def r2c_fft_f32_with_planner(input_re, output_re, output_im, planner: PlannerR2c32) -> None:
    """r2c.rs:607"""
    _r2c("f32", np.float32, input_re, output_re, output_im, planner)


def _c2r(fs, dtype, input_re, input_im, output, planner=None, scratch=None):
    ire, iim, out = _Slice(input_re, dtype, "input_re"), _Slice(input_im, dtype, "input_im"), _Slice(
        output, dtype, "output")
    sc = None
    if scratch is not None:
        sc = (_Slice(scratch[0], dtype, "scratch_re"), _Slice(scratch[1], dtype, "scratch_im"))
    if _same_place(ire, iim, out):
        own = planner is None
        if own:
            planner = (PlannerR2c64 if fs == "f64" else PlannerR2c32)(out.len)  # r2c.rs:696
        n, half = planner.n, planner.n // 2
        if out.len != n:
            _check(8)
        if ire.len != half + 1:
            _check(9)
        if iim.len != half + 1:
            _check(10)
        if sc is not None and sc[0].len != half:
            _check(11)
        if sc is not None and sc[1].len != half:
            _check(12)
        _check(_call(f"phast_c2r_fft_{fs}_dev", ire.ptr, iim.ptr, out.ptr, 1, half + 1, n, planner._h, _stream()))
        if own:
            import torch

            torch.cuda.current_stream().synchronize()
        return
    args = [ire.ptr, ire.len, iim.ptr, iim.len, out.ptr, out.len]
    if planner is None:
        _check(_call(f"phast_c2r_fft_{fs}", *args))
    elif sc is None:
        _check(_call(f"phast_c2r_fft_{fs}_with_planner", *args, planner._h))
    else:
        _check(_call(f"phast_c2r_fft_{fs}_with_planner_and_scratch", *args, planner._h, sc[0].ptr, sc[0].len, sc[1].ptr,
                     sc[1].len))


def c2r_fft_f64(input_re, input_im, output) -> None:
    """r2c.rs:695"""
    _c2r("f64", np.float64, input_re, input_im, output)


def c2r_fft_f32(input_re, input_im, output) -> None:
    """r2c.rs:804"""
    _c2r("f32", np.float32, input_re, input_im, output)


def c2r_fft_f64_with_planner(input_re, input_im, output, planner: PlannerR2c64) -> None:
    """r2c.rs:710"""
    _c2r("f64", np.float64, input_re, input_im, output, planner)


def c2r_fft_f32_with_planner(input_re, input_im, output, planner: PlannerR2c32) -> None:
    """r2c.rs:813"""
    _c2r("f32", np.float32, input_re, input_im, output, planner)


def c2r_fft_f64_with_planner_and_scratch(input_re, input_im, output, planner, scratch_re, scratch_im) -> None:
    """r2c.rs:740"""
    _c2r("f64", np.float64, input_re, input_im, output, planner, (scratch_re, scratch_im))


def c2r_fft_f32_with_planner_and_scratch(input_re, input_im, output, planner, scratch_re, scratch_im) -> None:
    """r2c.rs:836"""
    _c2r("f32", np.float32, input_re, input_im, output, planner, (scratch_re, scratch_im))


# ---------------------------------------------------------------------------------------------
# harness helpers
# ---------------------------------------------------------------------------------------------
def fill_uniform(reals, imags, n: int, seed: int = 0xCAFE, first_id: int = 0) -> None:
    """Fill device tensors holding ``len/n`` transforms with the counter-based uniform [-1, 1) input
    (``imags`` may be None for real input)."""
    import torch

    dtype = np.float64 if reals.dtype == torch.float64 else np.float32
    fs = "f64" if dtype == np.float64 else "f32"
    re = _Slice(reals, dtype, "reals")
    im_ptr = _Slice(imags, dtype, "imags").ptr if imags is not None else None
    _check(_call(f"phast_fill_{fs}_dev", re.ptr, im_ptr, n, re.len // n, n, seed, first_id, _stream()))


def digest(reals, imags, n: int, probe: int = 1):
    """Per-transform digest [sum re, sum im, sum |z|^2, re[probe]] as an f64 tensor of shape (batch, 4)."""
    import torch

    dtype = np.float64 if reals.dtype == torch.float64 else np.float32
    fs = "f64" if dtype == np.float64 else "f32"
    re, im = _Slice(reals, dtype, "reals"), _Slice(imags, dtype, "imags")
    batch = re.len // n
    out = torch.empty((batch, 4), dtype=torch.float64, device=reals.device)
    _check(_call(f"phast_digest_{fs}_dev", re.ptr, im.ptr, n, batch, n, probe, out.data_ptr(), _stream()))
    return out


def stream_probe(mib: int = 1024, reps: int = 5) -> dict:
    """This box's HBM streaming ceilings from the library's hand-written probe kernels (csrc/probe.hip): GB/s of a
    read-only, a write-only and a 1:1 copy kernel (read + write counted) over two buffers of ``mib`` MiB -- the figure a
    pass that reads and writes every byte once is to be read against."""
    import torch

    a = torch.empty(mib << 17, dtype=torch.float64, device="cuda").fill_(1.0)
    b = torch.empty_like(a)
    out = (C.c_double * 3)()
    _check(_call("phast_stream_probe_dev", a.data_ptr(), b.data_ptr(), mib << 20, reps, out, _stream()))
    del a, b
    return {"read": out[0], "write": out[1], "copy": out[2], "unit": "GB/s", "MiB": mib}


def debug_set_guard_bytes(nbytes: int) -> None:
    """debug: scratch buffers allocated from now on carry `nbytes` of 0xA5 guard band on either side"""
    _call("phast_debug_set_guard_bytes", nbytes)


def debug_wisdom_lookup(dtype: str, kind: "TuneKind", log_n: int, bucket: int = 0, cus: int = 0, arch: int = 0):
    """debug (no device needed): ``(layer, plan text)`` of the wisdom entry a planner on a device with ``cus`` compute units of
    architecture ``arch`` (0x950 for gfx950; 0 = any) applies for the key, or ``None`` when no entry applies"""
    buf = C.create_string_buffer(96)
    layer = int(_call("phast_debug_wisdom_lookup", 8 if dtype == "f64" else 4, int(kind), log_n, bucket, cus, arch, buf, 96))
    return None if layer < 0 else (layer, buf.value.decode())


def graph_upload(graph, stream=None) -> bool:
    """hipGraphUpload of an instantiated ``torch.cuda.CUDAGraph`` (so that its first replay does not pay the upload);
    False when this torch build does not expose the exec handle."""
    get = getattr(graph, "raw_cuda_graph_exec", None)
    if get is None:
        return False
    try:
        handle = get()
    except Exception:  # handle not kept by this torch version / graph not instantiated yet
        return False
    import torch

    s = stream if stream is not None else torch.cuda.current_stream()
    _check(_call("phast_hip_graph_upload", int(handle), s.cuda_stream))
    return True


def device_info() -> dict:
    name = C.create_string_buffer(256)
    cus, lds, mem = C.c_int(), C.c_size_t(), C.c_size_t()
    _check(_call("phast_device_info", name, 256, C.byref(cus), C.byref(lds), C.byref(mem)))
    return {"name": name.value.decode(), "compute_units": cus.value, "lds_per_block": lds.value,
            "global_mem_bytes": mem.value}
