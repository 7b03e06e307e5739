//! PhastFT's public API (planar slices) on AMD MI355X through `libphastft_hip.so`.
//!
//! The module tree is the reference's (PhastFT 0.3.0 `src/lib.rs:20-38`): `phastft::planner::{Direction,
//! PlannerMode, PlannerDit64, PlannerDit32, PlannerR2c64, PlannerR2c32}`, `phastft::options::Options`, the
//! transforms at the crate root, and -- behind feature `bench-internals`, as upstream --
//! `phastft::algorithms::bravo::{bit_rev_bravo_f64, bit_rev_bravo_f32}`.  Depend on it under the reference's
//! name and existing call sites compile unchanged:
//!
//! ```toml
//! phastft = { package = "phastft-hip", path = "rust/phastft-hip" }
//! ```
//!
//! Every item has the signature, in-place semantics and panics of the item of the same name upstream: the C
//! ABI returns one status per reference `assert!`, `phast_strerror` returns the reference's panic text, and
//! `ffi::check` re-raises it with `panic!`.
//!
//! SOURCE ONLY: written against `include/phastft_hip.h`; the build image has no Rust toolchain, so
//! `tests/test_rust_shim.py` checks the `extern "C"` block against the header instead of `cargo build`.
#![allow(clippy::missing_safety_doc)]

#[cfg(not(feature = "bench-internals"))]
mod algorithms;
#[cfg(feature = "bench-internals")]
pub mod algorithms;
// lib.rs:23-27 of the reference: complex_nums is private with `complex-nums` alone, public with `bench-internals`
#[cfg(all(feature = "complex-nums", not(feature = "bench-internals")))]
mod complex_nums;
#[cfg(feature = "bench-internals")]
pub mod complex_nums;
mod ffi;
pub mod options;
pub mod planner;

pub use algorithms::dit::{fft_32_dit_with_planner_and_opts, fft_64_dit_with_planner_and_opts};
pub use algorithms::r2c::{
    c2r_fft_f32, c2r_fft_f32_with_planner, c2r_fft_f32_with_planner_and_scratch, c2r_fft_f64,
    c2r_fft_f64_with_planner, c2r_fft_f64_with_planner_and_scratch, r2c_fft_f32,
    r2c_fft_f32_with_planner, r2c_fft_f64, r2c_fft_f64_with_planner,
};
// real transforms of any length (an extension beyond PhastFT 0.3.0)
pub use algorithms::r2c::{
    c2r_fft_f32_any, c2r_fft_f32_any_dev, c2r_fft_f32_any_with_planner, c2r_fft_f64_any, c2r_fft_f64_any_dev,
    c2r_fft_f64_any_with_planner, r2c_fft_f32_any, r2c_fft_f32_any_dev, r2c_fft_f32_any_with_planner, r2c_fft_f64_any,
    r2c_fft_f64_any_dev, r2c_fft_f64_any_with_planner,
};
// DCT / DST of types II and III (an extension beyond PhastFT 0.3.0)
pub use algorithms::r2r::{
    dct_f32, dct_f32_dev, dct_f32_with_planner, dct_f64, dct_f64_dev, dct_f64_with_planner, dst_f32, dst_f32_dev,
    dst_f32_with_planner, dst_f64, dst_f64_dev, dst_f64_with_planner, idct_f32, idct_f64, idst_f32, idst_f64, Norm,
};
pub use planner::{PlannerDct32, PlannerDct64};
// the short-time Fourier transform and its inverse (an extension beyond PhastFT 0.3.0)
pub use algorithms::stft::{
    istft_f32_dev, istft_f32_with_planner, istft_f64_dev, istft_f64_with_planner, stft_f32_dev, stft_f32_with_planner,
    stft_f64_dev, stft_f64_with_planner,
};
pub use planner::{PadMode, PlannerStft32, PlannerStft64};
// the modified discrete cosine transform and its inverse (an extension beyond PhastFT 0.3.0)
pub use algorithms::mdct::{
    imdct_f32_dev, imdct_f32_with_planner, imdct_f64_dev, imdct_f64_with_planner, mdct_f32_dev, mdct_f32_with_planner,
    mdct_f64_dev, mdct_f64_with_planner,
};
pub use planner::{PlannerMdct32, PlannerMdct64};
// Welch spectral estimation: welch, csd, spectrogram (an extension beyond PhastFT 0.3.0)
pub use algorithms::psd::{
    csd_f32_dev, csd_f32_with_planner, csd_f64_dev, csd_f64_with_planner, psd_f32_dev, psd_f32_with_planner, psd_f64_dev,
    psd_f64_with_planner,
};
pub use planner::{Detrend, PlannerPsd32, PlannerPsd64, PsdScaling};
// the Lomb-Scargle periodogram of unevenly spaced samples (an extension beyond PhastFT 0.3.0)
pub use algorithms::lomb::{
    lombscargle_f32, lombscargle_f32_dev, lombscargle_f32_with_planner, lombscargle_f64, lombscargle_f64_dev,
    lombscargle_f64_with_planner,
};
pub use planner::{LombNorm, PlannerLomb32, PlannerLomb64};
// sample-rate conversion: the polyphase FIR and the Fourier method (an extension beyond PhastFT 0.3.0)
pub use algorithms::resample::{
    resample_f32_dev, resample_f32_with_planner, resample_f64_dev, resample_f64_with_planner, upfirdn_f32_dev, upfirdn_f32_with_planner,
    upfirdn_f64_dev, upfirdn_f64_with_planner,
};
pub use planner::{PlannerResample32, PlannerResample64, PlannerUpfirdn32, PlannerUpfirdn64};
// the polyphase filter-bank channelizer (an extension beyond PhastFT 0.3.0)
pub use algorithms::channelizer::{channelize_f32_dev, channelize_f32_with_planner, channelize_f64_dev, channelize_f64_with_planner};
pub use planner::{PlannerChannelizer32, PlannerChannelizer64};
// the polyphase synthesis filter bank, the channelizer's inverse (an extension beyond PhastFT 0.3.0)
pub use algorithms::synthesizer::{synthesize_f32_dev, synthesize_f32_with_planner, synthesize_f64_dev, synthesize_f64_with_planner};
pub use planner::{PlannerSynthesizer32, PlannerSynthesizer64};
// the continuous wavelet transform and the analytic signal (an extension beyond PhastFT 0.3.0)
pub use algorithms::cwt::{cwt_32_dev, cwt_32_with_planner, cwt_64_dev, cwt_64_with_planner};
pub use planner::{CwtFamily, CwtNorm, PlannerCwt32, PlannerCwt64};
// the discrete wavelet transform and its inverse (an extension beyond PhastFT 0.3.0)
pub use algorithms::dwt::{
    wavedec_f32_dev, wavedec_f32_with_planner, wavedec_f64_dev, wavedec_f64_with_planner, waverec_f32_dev, waverec_f32_with_planner,
    waverec_f64_dev, waverec_f64_with_planner,
};
pub use planner::{DwtMode, PlannerDwt32, PlannerDwt64};
// overlap-save convolution and correlation of real signals (an extension beyond PhastFT 0.3.0)
pub use algorithms::conv::{conv_f32_dev, conv_f32_with_planner, conv_f64_dev, conv_f64_with_planner};
pub use planner::{ConvMode, PlannerConv32, PlannerConv64};
// ... and of real arrays of rank 1 .. 3, by overlap-save along every axis
pub use algorithms::convnd::{convnd_f32_dev, convnd_f32_with_planner, convnd_f64_dev, convnd_f64_with_planner};
pub use planner::{PlannerConvNd32, PlannerConvNd64};
// the chirp-Z transform on the unit circle and the zoom FFT (an extension beyond PhastFT 0.3.0)
pub use algorithms::czt::{czt_32, czt_32_dev, czt_32_with_planner, czt_64, czt_64_dev, czt_64_with_planner};
pub use planner::{PlannerCzt32, PlannerCzt64};
// non-uniform FFTs of types 1 and 2 (an extension beyond PhastFT 0.3.0)
pub use algorithms::nufft::{
    nufft1_32, nufft1_32_dev, nufft1_32_with_planner, nufft1_64, nufft1_64_dev, nufft1_64_with_planner, nufft2_32, nufft2_32_dev,
    nufft2_32_with_planner, nufft2_64, nufft2_64_dev, nufft2_64_with_planner,
};
pub use planner::{PlannerNufft32, PlannerNufft64};
// the same in two dimensions (an extension beyond PhastFT 0.3.0)
pub use algorithms::nufft2d::{
    nufft2d1_32, nufft2d1_32_dev, nufft2d1_32_with_planner, nufft2d1_64, nufft2d1_64_dev, nufft2d1_64_with_planner, nufft2d2_32,
    nufft2d2_32_dev, nufft2d2_32_with_planner, nufft2d2_64, nufft2d2_64_dev, nufft2d2_64_with_planner,
};
pub use planner::{PlannerNufft2d32, PlannerNufft2d64};
// and in three dimensions (an extension beyond PhastFT 0.3.0)
pub use algorithms::nufft3d::{
    nufft3d1_32, nufft3d1_32_dev, nufft3d1_32_with_planner, nufft3d1_64, nufft3d1_64_dev, nufft3d1_64_with_planner, nufft3d2_32,
    nufft3d2_32_dev, nufft3d2_32_with_planner, nufft3d2_64, nufft3d2_64_dev, nufft3d2_64_with_planner,
};
pub use planner::{PlannerNufft3d32, PlannerNufft3d64};
// the non-uniform FFT of type 3 (an extension beyond PhastFT 0.3.0)
pub use algorithms::nufft_t3::{nufft3_32, nufft3_32_dev, nufft3_32_with_planner, nufft3_64, nufft3_64_dev, nufft3_64_with_planner};
pub use planner::{PlannerNufftT3_32, PlannerNufftT3_64};
// multi-dimensional real transforms (an extension beyond PhastFT 0.3.0)
pub use algorithms::r2c::{
    c2r_fft_f32_nd, c2r_fft_f32_nd_dev, c2r_fft_f32_nd_with_planner, c2r_fft_f64_nd, c2r_fft_f64_nd_dev,
    c2r_fft_f64_nd_with_planner, r2c_fft_f32_nd, r2c_fft_f32_nd_dev, r2c_fft_f32_nd_with_planner, r2c_fft_f64_nd,
    r2c_fft_f64_nd_dev, r2c_fft_f64_nd_with_planner,
};

use crate::options::Options;
use crate::planner::{Direction, PlannerAny32, PlannerAny64, PlannerDit32, PlannerDit64, PlannerNd32, PlannerNd64};
use std::ffi::{c_int, c_void};

macro_rules! impl_fft {
    ($t:ty, $planner:ident, $with_opts:ident, $with_planner:ident, $plain:ident) => {
        /// lib.rs:143 / 186
        pub fn $with_planner(reals: &mut [$t], imags: &mut [$t], direction: Direction, planner: &$planner) {
            let opts = Options::guess_options(reals.len());
            $with_opts(reals, imags, direction, planner, &opts);
        }
        /// lib.rs:180 / 223 -- the planner is built from `reals.len()` first, so a bad length panics there
        pub fn $plain(reals: &mut [$t], imags: &mut [$t], direction: Direction) {
            let planner = <$planner>::new(reals.len());
            $with_planner(reals, imags, direction, &planner);
        }
    };
}
impl_fft!(f64, PlannerDit64, fft_64_dit_with_planner_and_opts, fft_64_dit_with_planner, fft_64_dit);
impl_fft!(f32, PlannerDit32, fft_32_dit_with_planner_and_opts, fft_32_dit_with_planner, fft_32_dit);

/// Device-resident, batched, asynchronous forms (no reference counterpart): `d_reals`/`d_imags` are HIP device
/// pointers to `batch` transforms `dist` elements apart; `stream` is a `hipStream_t`.
pub unsafe fn fft_64_dit_dev(d_reals: *mut f64, d_imags: *mut f64, n: usize, batch: usize, dist: usize,
                             direction: Direction, planner: &PlannerDit64, stream: *mut c_void) {
    ffi::check(ffi::phast_fft_64_dit_dev(d_reals, d_imags, n, batch, dist, direction as c_int, planner.h, stream));
}
/// f32 twin of [`fft_64_dit_dev`]
pub unsafe fn fft_32_dit_dev(d_reals: *mut f32, d_imags: *mut f32, n: usize, batch: usize, dist: usize,
                             direction: Direction, planner: &PlannerDit32, stream: *mut c_void) {
    ffi::check(ffi::phast_fft_32_dit_dev(d_reals, d_imags, n, batch, dist, direction as c_int, planner.h, stream));
}

/// Complex transforms of ANY length N >= 1 -- an extension beyond PhastFT 0.3.0, which takes powers of two only (its README
/// lists other lengths as planned).  Same calling convention as `fft_64_dit`: planar slices, in place, `Reverse` scales by
/// 1/N, panics carry the library's message (`reals.len() != imags.len()`, a planner of another length, N = 0 or > 2^29).
macro_rules! impl_fft_any {
    ($t:ty, $planner:ident, $with_planner:ident, $plain:ident, $c_fn:ident, $dev:ident, $c_dev:ident) => {
        pub fn $with_planner(reals: &mut [$t], imags: &mut [$t], direction: Direction, planner: &$planner) {
            ffi::check(unsafe {
                ffi::$c_fn(reals.as_mut_ptr(), reals.len(), imags.as_mut_ptr(), imags.len(), direction as c_int, planner.h)
            });
        }
        pub fn $plain(reals: &mut [$t], imags: &mut [$t], direction: Direction) {
            let planner = <$planner>::new(reals.len());
            $with_planner(reals, imags, direction, &planner);
        }
        /// Device-resident, batched, asynchronous on `stream`: `d_work` is a device workspace of `work_len >= 2 M` elements
        /// (`planner.workspace_len(batch)` runs the batch in one chunk; unused for a power of two)
        pub unsafe fn $dev(d_reals: *mut $t, d_imags: *mut $t, n: usize, batch: usize, dist: usize, direction: Direction,
                           planner: &$planner, d_work: *mut $t, work_len: usize, stream: *mut c_void) {
            ffi::check(ffi::$c_dev(d_reals, d_imags, n, batch, dist, direction as c_int, planner.h, d_work, work_len, stream));
        }
    };
}
impl_fft_any!(f64, PlannerAny64, fft_64_any_with_planner, fft_64_any, phast_fft_64_any_with_planner, fft_64_any_dev,
              phast_fft_64_any_dev);
impl_fft_any!(f32, PlannerAny32, fft_32_any_with_planner, fft_32_any, phast_fft_32_any_with_planner, fft_32_any_dev,
              phast_fft_32_any_dev);

/// Complex transforms over every axis of a row-major array (numpy fftn / ifftn) -- an extension beyond PhastFT 0.3.0.  Planar
/// slices of prod(shape) points, in place; `Reverse` scales by 1 / prod(shape).
macro_rules! impl_fft_nd {
    ($t:ty, $planner:ident, $with_planner:ident, $plain:ident, $c_fn:ident, $dev:ident, $c_dev:ident) => {
        pub fn $with_planner(reals: &mut [$t], imags: &mut [$t], direction: Direction, planner: &$planner) {
            ffi::check(unsafe {
                ffi::$c_fn(reals.as_mut_ptr(), reals.len(), imags.as_mut_ptr(), imags.len(), direction as c_int, planner.h)
            });
        }
        pub fn $plain(reals: &mut [$t], imags: &mut [$t], shape: &[usize], direction: Direction) {
            let planner = <$planner>::new(shape);
            $with_planner(reals, imags, direction, &planner);
        }
        /// Device-resident, batched, asynchronous on `stream`: `d_work` is a device workspace of at least
        /// `planner.workspace_len(1)` elements (`planner.workspace_len(batch)` runs the batch in one chunk)
        pub unsafe fn $dev(d_reals: *mut $t, d_imags: *mut $t, n_total: usize, batch: usize, dist: usize, direction: Direction,
                           planner: &$planner, d_work: *mut $t, work_len: usize, stream: *mut c_void) {
            ffi::check(ffi::$c_dev(d_reals, d_imags, n_total, batch, dist, direction as c_int, planner.h, d_work, work_len,
                                   stream));
        }
    };
}
impl_fft_nd!(f64, PlannerNd64, fft_64_nd_with_planner, fft_64_nd, phast_fft_64_nd_with_planner, fft_64_nd_dev,
             phast_fft_64_nd_dev);
impl_fft_nd!(f32, PlannerNd32, fft_32_nd_with_planner, fft_32_nd, phast_fft_32_nd_with_planner, fft_32_nd_dev,
             phast_fft_32_nd_dev);

/// Interleaved `Complex<T>` signals (reference: feature `complex-nums`, lib.rs:41-140).  The reference copies into
/// two planar Vecs, runs the planar path and copies back; the library fuses the (de)interleave into the first
/// pass's load and the last pass's store, so there is no extra sweep.  `Complex<T>` is `repr(C)` (re, im).
#[cfg(feature = "complex-nums")]
pub use num_complex::Complex;

#[cfg(feature = "complex-nums")]
macro_rules! impl_interleaved {
    ($t:ty, $planner:ident, $with_opts:ident, $with_planner:ident, $plain:ident, $c_fn:ident) => {
        /// lib.rs:50
        pub fn $with_opts(signal: &mut [Complex<$t>], direction: Direction, planner: &$planner, opts: &Options) {
            let c_opts = opts.to_c();
            ffi::check(unsafe {
                ffi::$c_fn(signal.as_mut_ptr() as *mut $t, signal.len(), direction as c_int, planner.h, &c_opts)
            });
        }
        /// lib.rs:87
        pub fn $with_planner(signal: &mut [Complex<$t>], direction: Direction, planner: &$planner) {
            let opts = Options::guess_options(signal.len());
            $with_opts(signal, direction, planner, &opts);
        }
        /// lib.rs:120
        pub fn $plain(signal: &mut [Complex<$t>], direction: Direction) {
            let planner = <$planner>::new(signal.len());
            $with_planner(signal, direction, &planner);
        }
    };
}
#[cfg(feature = "complex-nums")]
impl_interleaved!(f64, PlannerDit64, fft_64_interleaved_with_planner_and_opts, fft_64_interleaved_with_planner,
                  fft_64_interleaved, phast_fft_64_interleaved_with_planner_and_opts);
#[cfg(feature = "complex-nums")]
impl_interleaved!(f32, PlannerDit32, fft_32_interleaved_with_planner_and_opts, fft_32_interleaved_with_planner,
                  fft_32_interleaved, phast_fft_32_interleaved_with_planner_and_opts);
