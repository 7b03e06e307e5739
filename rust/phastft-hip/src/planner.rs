//! `phastft::planner` (planner.rs:10-212): `Direction`, `PlannerMode` and the four planners.  A planner owns
//! device twiddle tables and device scratch inside `libphastft_hip.so`; like the reference's planners it is an
//! immutable value any number of callers may borrow (`Send + Sync`, planner.rs:38-39) -- inside the library every
//! concurrent caller works in a workspace of its own (scratch, staging, stream), so borrowed planners run side by side.
use crate::ffi::{self, Opaque};
use std::ffi::{c_int, c_void};

/// planner.rs:10-16
#[derive(Copy, Clone)]
pub enum Direction {
    Forward = 1,
    Reverse = -1,
}

/// planner.rs:24-32.  `Tune`: the library times the plans that exist for this length on the device at plan time and keeps
/// the fastest (include/phastft_hip.h, "PlannerMode::Tune"); `Heuristic`: static rules, zero planning overhead.
#[derive(Copy, Clone, Debug, Default)]
pub enum PlannerMode {
    #[default]
    Heuristic,
    Tune,
}

/// PHAST_TUNE_* (include/phastft_hip.h): which call a tuning run measures
#[derive(Copy, Clone, Debug)]
pub enum TuneKind {
    C2C = 0,
    C2CInterleaved = 1,
    R2C = 2,
    C2R = 3,
}

/// What tuning runs found, as text (one line per type / kind / length / batch bucket): carry it to the next process, or set
/// `PHAST_WISDOM=<path>` and the library does.
pub fn wisdom_export() -> String {
    let mut need = 0usize;
    ffi::check(unsafe { ffi::phast_wisdom_export(std::ptr::null_mut(), 0, &mut need) });
    let mut buf = vec![0u8; need];
    ffi::check(unsafe { ffi::phast_wisdom_export(buf.as_mut_ptr() as *mut _, need, std::ptr::null_mut()) });
    buf.pop(); // the NUL
    String::from_utf8(buf).expect("wisdom is ASCII")
}
pub fn wisdom_import(text: &str) {
    let c = std::ffi::CString::new(text).expect("no NUL in wisdom text");
    ffi::check(unsafe { ffi::phast_wisdom_import(c.as_ptr()) });
}
pub fn wisdom_forget() {
    unsafe { ffi::phast_wisdom_forget() }
}

macro_rules! impl_planner_dit {
    ($name:ident, $new:ident, $free:ident, $tune:ident) => {
        /// planner.rs:34-114
        pub struct $name {
            pub(crate) h: *mut Opaque,
        }
        // SAFETY: the handle is immutable after creation; what a call mutates lives in a per-call workspace inside the library
        unsafe impl Send for $name {}
        unsafe impl Sync for $name {}
        impl $name {
            /// planner.rs:55 -- panics unless `num_points` is a power of two > 0 (planner.rs:66)
            pub fn new(num_points: usize) -> Self {
                Self::with_mode(num_points, PlannerMode::Heuristic)
            }
            /// planner.rs:65
            pub fn with_mode(num_points: usize, mode: PlannerMode) -> Self {
                let mut h = std::ptr::null_mut();
                ffi::check(unsafe { ffi::$new(num_points, mode as c_int, &mut h) });
                Self { h }
            }
            /// No reference counterpart: `PlannerMode::Tune` for `batch` transforms per call of `kind` (the reference's
            /// planners only ever see one transform per call, which `with_mode(_, Tune)` covers).
            pub fn tune(&mut self, batch: usize, kind: TuneKind) -> ffi::PhastTuneReport {
                let mut rep = std::mem::MaybeUninit::<ffi::PhastTuneReport>::zeroed();
                ffi::check(unsafe { ffi::$tune(self.h, batch, kind as c_int, rep.as_mut_ptr()) });
                unsafe { rep.assume_init() }
            }
        }
        impl Drop for $name {
            fn drop(&mut self) {
                unsafe { ffi::$free(self.h) }
            }
        }
    };
}
impl_planner_dit!(PlannerDit64, phast_planner_dit64_with_mode, phast_planner_dit64_free, phast_planner_dit64_tune);
impl_planner_dit!(PlannerDit32, phast_planner_dit32_with_mode, phast_planner_dit32_free, phast_planner_dit32_tune);

macro_rules! impl_planner_r2c {
    ($name:ident, $new:ident, $free:ident, $tune:ident) => {
        /// planner.rs:164-212 -- one planner drives both R2C and C2R (planner.rs:171-172)
        pub struct $name {
            pub(crate) h: *mut Opaque,
            pub(crate) n: usize,
        }
        // SAFETY: as for the DIT planners
        unsafe impl Send for $name {}
        unsafe impl Sync for $name {}
        impl $name {
            /// planner.rs:194 -- panics with "n must be a power of 2 >= 4" (planner.rs:195)
            pub fn new(n: usize) -> Self {
                Self::with_mode(n, PlannerMode::Heuristic)
            }
            /// No reference counterpart (PlannerR2c*::new has no mode): the switch of `PlannerDit*::with_mode` for
            /// `r2c_fft_*` and `c2r_fft_*`.
            pub fn with_mode(n: usize, mode: PlannerMode) -> Self {
                let mut h = std::ptr::null_mut();
                ffi::check(unsafe { ffi::$new(n, mode as c_int, &mut h) });
                Self { h, n }
            }
            pub fn tune(&mut self, batch: usize, kind: TuneKind) -> ffi::PhastTuneReport {
                let mut rep = std::mem::MaybeUninit::<ffi::PhastTuneReport>::zeroed();
                ffi::check(unsafe { ffi::$tune(self.h, batch, kind as c_int, rep.as_mut_ptr()) });
                unsafe { rep.assume_init() }
            }
        }
        impl Drop for $name {
            fn drop(&mut self) {
                unsafe { ffi::$free(self.h) }
            }
        }
    };
}
impl_planner_r2c!(PlannerR2c64, phast_planner_r2c64_with_mode, phast_planner_r2c64_free, phast_planner_r2c64_tune);
impl_planner_r2c!(PlannerR2c32, phast_planner_r2c32_with_mode, phast_planner_r2c32_free, phast_planner_r2c32_tune);

macro_rules! impl_planner_any {
    ($any:ident, $new:ident, $free:ident, $ws_len:ident) => {
        /// An extension beyond PhastFT 0.3.0, whose planners take powers of two only: complex transforms of any length
        /// 1 <= N <= 2^29 (Bluestein's algorithm on the power-of-two engine; a power of two runs the `PlannerDit*` path
        /// itself).  Immutable after `new`, like the reference's planners.
        pub struct $any {
            pub(crate) h: *mut Opaque,
            pub(crate) n: usize,
        }
        // SAFETY: the handle is immutable after creation; a call works in the caller's workspace (device calls) or in a
        // workspace of the library's own pool (host-slice calls)
        unsafe impl Send for $any {}
        unsafe impl Sync for $any {}
        impl $any {
            /// panics with "invalid argument" for N = 0 or N > 2^29
            pub fn new(n: usize) -> Self {
                let mut h = std::ptr::null_mut();
                ffi::check(unsafe { ffi::$new(n, &mut h) });
                Self { h, n }
            }
            pub fn num_points(&self) -> usize {
                self.n
            }
            /// elements of the workspace a device call of `batch` transforms works in (0 for a power of two)
            pub fn workspace_len(&self, batch: usize) -> usize {
                unsafe { ffi::$ws_len(self.h, batch) }
            }
        }
        impl Drop for $any {
            fn drop(&mut self) {
                unsafe { ffi::$free(self.h) }
            }
        }
    };
}
impl_planner_any!(PlannerAny64, phast_planner_any64_new, phast_planner_any64_free, phast_planner_any64_workspace_len);
impl_planner_any!(PlannerAny32, phast_planner_any32_new, phast_planner_any32_free, phast_planner_any32_workspace_len);

macro_rules! impl_planner_r2c_any {
    ($any:ident, $new:ident, $free:ident, $ws_len:ident) => {
        /// An extension beyond PhastFT 0.3.0, whose `PlannerR2c*` takes powers of two >= 4 only: real transforms (R2C / C2R)
        /// of any length 1 <= N <= 2^29 (a power of two >= 4 runs the `PlannerR2c*` path itself, an even N packs into an
        /// N/2-point Bluestein transform, an odd N runs an N-point one).  Immutable after `new`, like the reference's planners.
        pub struct $any {
            pub(crate) h: *mut Opaque,
            pub(crate) n: usize,
        }
        // SAFETY: the handle is immutable after creation; a call works in the caller's workspace (device calls) or in a
        // workspace of the library's own pool (host-slice calls)
        unsafe impl Send for $any {}
        unsafe impl Sync for $any {}
        impl $any {
            /// panics with "invalid argument" for N = 0 or N > 2^29
            pub fn new(n: usize) -> Self {
                let mut h = std::ptr::null_mut();
                ffi::check(unsafe { ffi::$new(n, &mut h) });
                Self { h, n }
            }
            pub fn num_points(&self) -> usize {
                self.n
            }
            /// elements of the workspace a device call of `batch` transforms works in (0 for a power of two, N = 1, 2)
            pub fn workspace_len(&self, batch: usize) -> usize {
                unsafe { ffi::$ws_len(self.h, batch) }
            }
        }
        impl Drop for $any {
            fn drop(&mut self) {
                unsafe { ffi::$free(self.h) }
            }
        }
    };
}
impl_planner_r2c_any!(PlannerR2cAny64, phast_planner_r2c_any64_new, phast_planner_r2c_any64_free,
                      phast_planner_r2c_any64_workspace_len);
impl_planner_r2c_any!(PlannerR2cAny32, phast_planner_r2c_any32_new, phast_planner_r2c_any32_free,
                      phast_planner_r2c_any32_workspace_len);

macro_rules! impl_planner_dct {
    ($dct:ident, $new:ident, $free:ident, $ws_len:ident) => {
        /// An extension beyond PhastFT 0.3.0: the DCT and DST of types II and III of any length 1 <= N <= 2^29 (one real
        /// transform of the same N between two sweeps).  One planner serves all four transforms and every norm.  Immutable
        /// after `new`, like the reference's planners.
        pub struct $dct {
            pub(crate) h: *mut Opaque,
            pub(crate) n: usize,
        }
        // SAFETY: the handle is immutable after creation; a call works in the caller's workspace (device calls) or in a
        // workspace of the library's own pool (host-slice calls)
        unsafe impl Send for $dct {}
        unsafe impl Sync for $dct {}
        impl $dct {
            /// panics with "invalid argument" for N = 0 or N > 2^29
            pub fn new(n: usize) -> Self {
                let mut h = std::ptr::null_mut();
                ffi::check(unsafe { ffi::$new(n, &mut h) });
                Self { h, n }
            }
            pub fn num_points(&self) -> usize {
                self.n
            }
            /// elements of the workspace a device call of `batch` transforms works in (any length of at least
            /// `workspace_len(1)` is legal: a shorter one than `workspace_len(batch)` runs the batch in chunks)
            pub fn workspace_len(&self, batch: usize) -> usize {
                unsafe { ffi::$ws_len(self.h, batch) }
            }
        }
        impl Drop for $dct {
            fn drop(&mut self) {
                unsafe { ffi::$free(self.h) }
            }
        }
    };
}
impl_planner_dct!(PlannerDct64, phast_planner_dct64_new, phast_planner_dct64_free, phast_planner_dct64_workspace_len);
impl_planner_dct!(PlannerDct32, phast_planner_dct32_new, phast_planner_dct32_free, phast_planner_dct32_workspace_len);

/// How `center` pads the signal (PHAST_PAD_* of the C ABI)
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum PadMode {
    Reflect = 0,
    Zero = 1,
}

macro_rules! impl_planner_stft {
    ($stft:ident, $t:ty, $new:ident, $free:ident, $frames:ident, $bins:ident, $ws_len:ident, $ws_min:ident, $env:ident) => {
        /// An extension beyond PhastFT 0.3.0: the short-time Fourier transform of signals of `signal_len` samples and its
        /// inverse by weighted overlap-add (torch.stft / torch.istft(length = signal_len) with win_length = n_fft): one real
        /// transform of `n_fft` per frame and one sweep per direction.  Immutable after `new`, like the reference's planners.
        pub struct $stft {
            pub(crate) h: *mut Opaque,
            pub(crate) signal_len: usize,
        }
        // SAFETY: the handle is immutable after creation; a call works in the caller's workspace (device calls) or in
        // device buffers of its own (host-slice calls)
        unsafe impl Send for $stft {}
        unsafe impl Sync for $stft {}
        impl $stft {
            /// `window`: `n_fft` values, or `None` for all ones.  Panics with "invalid argument" unless 1 <= hop <= n_fft
            /// <= 2^29, 1 <= signal_len <= 2^29, n_fft / 2 < signal_len with `center` and `PadMode::Reflect`, signal_len >=
            /// n_fft without `center`, and frames * n_fft <= 2^30
            pub fn new(signal_len: usize, n_fft: usize, hop: usize, window: Option<&[$t]>, center: bool, pad_mode: PadMode) -> Self {
                if let Some(w) = window {
                    assert_eq!(w.len(), n_fft, "invalid argument");
                }
                let mut h = std::ptr::null_mut();
                let w = window.map_or(std::ptr::null(), |w| w.as_ptr());
                ffi::check(unsafe { ffi::$new(signal_len, n_fft, hop, w, center as c_int, pad_mode as c_int, &mut h) });
                Self { h, signal_len }
            }
            pub fn signal_len(&self) -> usize {
                self.signal_len
            }
            pub fn frames(&self) -> usize {
                unsafe { ffi::$frames(self.h) }
            }
            pub fn bins(&self) -> usize {
                unsafe { ffi::$bins(self.h) }
            }
            /// the minimum of the window envelope over the samples some frame holds; the inverse needs more than 1e-11
            pub fn envelope_min(&self) -> f64 {
                unsafe { ffi::$env(self.h) }
            }
            /// elements of the workspace a device call of `batch` signals works in
            pub fn workspace_len(&self, batch: usize) -> usize {
                unsafe { ffi::$ws_len(self.h, batch) }
            }
            /// the least workspace a call runs in: one frame forward, one signal's frames for the inverse
            pub fn workspace_min(&self, inverse: bool) -> usize {
                unsafe { ffi::$ws_min(self.h, inverse as c_int) }
            }
        }
        impl Drop for $stft {
            fn drop(&mut self) {
                unsafe { ffi::$free(self.h) }
            }
        }
    };
}
impl_planner_stft!(PlannerStft64, f64, phast_planner_stft64_new, phast_planner_stft64_free, phast_planner_stft64_frames,
                   phast_planner_stft64_bins, phast_planner_stft64_workspace_len, phast_planner_stft64_workspace_min,
                   phast_planner_stft64_envelope_min);
impl_planner_stft!(PlannerStft32, f32, phast_planner_stft32_new, phast_planner_stft32_free, phast_planner_stft32_frames,
                   phast_planner_stft32_bins, phast_planner_stft32_workspace_len, phast_planner_stft32_workspace_min,
                   phast_planner_stft32_envelope_min);

macro_rules! impl_planner_mdct {
    ($mdct:ident, $t:ty, $new:ident, $free:ident, $frames:ident, $ws_len:ident, $ws_min:ident, $defect:ident) => {
        /// An extension beyond PhastFT 0.3.0: the modified discrete cosine transform of signals of `signal_len` samples and
        /// its inverse by windowed overlap-add: `n` coefficients (even) per frame of `2 n` samples, hop `n`; one complex
        /// transform of `n / 2` per frame between two sweeps.  Immutable after `new`, like the reference's planners.
        pub struct $mdct {
            pub(crate) h: *mut Opaque,
            pub(crate) signal_len: usize,
            pub(crate) n: usize,
        }
        // SAFETY: the handle is immutable after creation; a call works in the caller's workspace (device calls) or in
        // device buffers of its own (host-slice calls)
        unsafe impl Send for $mdct {}
        unsafe impl Sync for $mdct {}
        impl $mdct {
            /// `window`: `2 n` values, or `None` for the sine window.  `padded`: frames from sample `-n` on, so that every
            /// sample lies in two.  Panics with "invalid argument" unless n is even, 2 <= n <= 2^29, 1 <= signal_len <=
            /// 2^29, signal_len >= 2 n without `padded`, and frames * n <= 2^30
            pub fn new(signal_len: usize, n: usize, window: Option<&[$t]>, padded: bool) -> Self {
                if let Some(w) = window {
                    assert_eq!(w.len(), 2 * n, "invalid argument");
                }
                let mut h = std::ptr::null_mut();
                let w = window.map_or(std::ptr::null(), |w| w.as_ptr());
                ffi::check(unsafe { ffi::$new(signal_len, n, w, padded as c_int, &mut h) });
                Self { h, signal_len, n }
            }
            pub fn signal_len(&self) -> usize {
                self.signal_len
            }
            pub fn n(&self) -> usize {
                self.n
            }
            pub fn frames(&self) -> usize {
                unsafe { ffi::$frames(self.h) }
            }
            /// how far the window is from perfect reconstruction (0 for the sine, Vorbis and Kaiser-Bessel-derived windows);
            /// reported, never refused
            pub fn tdac_defect(&self) -> f64 {
                unsafe { ffi::$defect(self.h) }
            }
            /// elements of the workspace a device call of `batch` signals works in
            pub fn workspace_len(&self, batch: usize) -> usize {
                unsafe { ffi::$ws_len(self.h, batch) }
            }
            /// the least workspace a call runs in: one frame forward, one signal's frames for the inverse
            pub fn workspace_min(&self, inverse: bool) -> usize {
                unsafe { ffi::$ws_min(self.h, inverse as c_int) }
            }
        }
        impl Drop for $mdct {
            fn drop(&mut self) {
                unsafe { ffi::$free(self.h) }
            }
        }
    };
}
impl_planner_mdct!(PlannerMdct64, f64, phast_planner_mdct64_new, phast_planner_mdct64_free, phast_planner_mdct64_frames,
                   phast_planner_mdct64_workspace_len, phast_planner_mdct64_workspace_min, phast_planner_mdct64_tdac_defect);
impl_planner_mdct!(PlannerMdct32, f32, phast_planner_mdct32_new, phast_planner_mdct32_free, phast_planner_mdct32_frames,
                   phast_planner_mdct32_workspace_len, phast_planner_mdct32_workspace_min, phast_planner_mdct32_tdac_defect);

/// How a segment is detrended before it is windowed (PHAST_DETREND_* of the C ABI)
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum Detrend {
    None = 0,
    Constant = 1,
}
/// The scale of a spectral estimate (PHAST_PSD_* of the C ABI): V^2 / Hz or V^2
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum PsdScaling {
    Density = 0,
    Spectrum = 1,
}

macro_rules! impl_planner_psd {
    ($psd:ident, $new:ident, $free:ident, $segments:ident, $bins:ident, $slab:ident, $ws_len:ident, $ws_min:ident) => {
        /// An extension beyond PhastFT 0.3.0: Welch spectral estimation of signals of `signal_len` samples with
        /// scipy.signal's definitions (welch, csd, spectrogram): segments of `nperseg` samples `hop` apart, detrended,
        /// windowed, zero-padded to `nfft` and transformed; one-sided, `nfft / 2 + 1` bins.  Immutable after `new`.
        pub struct $psd {
            pub(crate) h: *mut Opaque,
            pub(crate) signal_len: usize,
        }
        // SAFETY: the handle is immutable after creation; a call works in the caller's workspace (device calls) or in
        // device buffers of its own (host-slice calls)
        unsafe impl Send for $psd {}
        unsafe impl Sync for $psd {}
        impl $psd {
            /// `window`: `nperseg` values, or `None` for the periodic Hann window.  Panics with "invalid argument" unless
            /// 1 <= hop <= nperseg <= nfft <= 2^29, nperseg <= signal_len <= 2^29, segments * nfft <= 2^30, fs > 0 and
            /// the window's sum of squares (density) or sum (spectrum) is not zero
            #[allow(clippy::too_many_arguments)]
            pub fn new(signal_len: usize, nperseg: usize, hop: usize, nfft: usize, window: Option<&[f64]>, detrend: Detrend,
                       scaling: PsdScaling, fs: f64) -> Self {
                if let Some(w) = window {
                    assert_eq!(w.len(), nperseg, "invalid argument");
                }
                let mut h = std::ptr::null_mut();
                let w = window.map_or(std::ptr::null(), |w| w.as_ptr());
                ffi::check(unsafe { ffi::$new(signal_len, nperseg, hop, nfft, w, detrend as c_int, scaling as c_int, fs, &mut h) });
                Self { h, signal_len }
            }
            pub fn signal_len(&self) -> usize {
                self.signal_len
            }
            pub fn segments(&self) -> usize {
                unsafe { ffi::$segments(self.h) }
            }
            pub fn bins(&self) -> usize {
                unsafe { ffi::$bins(self.h) }
            }
            /// frames per slab of the sum over frames: a function of `segments()` and `bins()` alone
            pub fn slab(&self) -> usize {
                unsafe { ffi::$slab(self.h) }
            }
            /// elements of the workspace a device call of `batch` signals (`cross`: pairs of signals) works in
            pub fn workspace_len(&self, batch: usize, cross: bool) -> usize {
                unsafe { ffi::$ws_len(self.h, batch, cross as c_int) }
            }
            /// the least workspace a call runs in: one frame (`cross`: one frame of each signal)
            pub fn workspace_min(&self, cross: bool) -> usize {
                unsafe { ffi::$ws_min(self.h, cross as c_int) }
            }
        }
        impl Drop for $psd {
            fn drop(&mut self) {
                unsafe { ffi::$free(self.h) }
            }
        }
    };
}
impl_planner_psd!(PlannerPsd64, phast_planner_psd64_new, phast_planner_psd64_free, phast_planner_psd64_segments,
                  phast_planner_psd64_bins, phast_planner_psd64_slab, phast_planner_psd64_workspace_len,
                  phast_planner_psd64_workspace_min);
impl_planner_psd!(PlannerPsd32, phast_planner_psd32_new, phast_planner_psd32_free, phast_planner_psd32_segments,
                  phast_planner_psd32_bins, phast_planner_psd32_slab, phast_planner_psd32_workspace_len,
                  phast_planner_psd32_workspace_min);

/// What a periodogram returns (PHAST_LOMB_* of the C ABI): scipy's legacy power P M / 4, the power over the signal's own
/// (P / 2 YY, in [0, 1]), or the complex amplitude (a + i b) e^{i tau}
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum LombNorm {
    Power = 0,
    Normalize = 1,
    Amplitude = 2,
}

macro_rules! impl_planner_lomb {
    ($lomb:ident, $new:ident, $free:ident, $slab:ident, $grid:ident, $ws_len:ident, $ws_min:ident) => {
        /// An extension beyond PhastFT 0.3.0: the generalised Lomb-Scargle periodogram (scipy.signal.lombscargle's
        /// definitions) of signals sampled at `times` (any finite values, any order), at `freqs` in cycles per unit of
        /// time, with optional weights and a floating mean.  One type-3 non-uniform transform per signal; the tables that
        /// depend on the times, frequencies and weights alone are built at `new`, in double.  Immutable after `new`.
        pub struct $lomb {
            pub(crate) h: *mut Opaque,
            pub(crate) points: usize,
            pub(crate) freqs: usize,
        }
        // SAFETY: the handle is immutable after creation; a call works in the caller's workspace (device calls) or in
        // device buffers of its own (host-slice calls)
        unsafe impl Send for $lomb {}
        unsafe impl Sync for $lomb {}
        impl $lomb {
            /// `weights`: one value >= 0 per time with a positive sum, or `None` for equal weights.  Panics with "invalid
            /// argument" unless 1 <= M, K <= 2^30, every time, frequency and weight is finite, eps is in the type-3
            /// planner's range for the type and the type-3 grids of (t, f) and of (t, 2 f) are within its limit
            pub fn new(times: &[f64], freqs: &[f64], weights: Option<&[f64]>, floating_mean: bool, eps: f64) -> Self {
                if let Some(w) = weights {
                    assert_eq!(w.len(), times.len(), "invalid argument");
                }
                let mut h = std::ptr::null_mut();
                let w = weights.map_or(std::ptr::null(), |w| w.as_ptr());
                ffi::check(unsafe {
                    ffi::$new(times.as_ptr(), times.len(), freqs.as_ptr(), freqs.len(), w, floating_mean as c_int, eps, &mut h)
                });
                Self { h, points: times.len(), freqs: freqs.len() }
            }
            pub fn points(&self) -> usize {
                self.points
            }
            pub fn freqs(&self) -> usize {
                self.freqs
            }
            /// points per slab of the two reductions: a function of `points()` alone
            pub fn slab(&self) -> usize {
                unsafe { ffi::$slab(self.h) }
            }
            /// n_f of the inner type-3 planner
            pub fn grid_len(&self) -> usize {
                unsafe { ffi::$grid(self.h) }
            }
            /// elements of the workspace a device call of `batch` signals works in
            pub fn workspace_len(&self, batch: usize) -> usize {
                unsafe { ffi::$ws_len(self.h, batch) }
            }
            /// the least workspace a call runs in: one signal
            pub fn workspace_min(&self) -> usize {
                unsafe { ffi::$ws_min(self.h) }
            }
        }
        impl Drop for $lomb {
            fn drop(&mut self) {
                unsafe { ffi::$free(self.h) }
            }
        }
    };
}
impl_planner_lomb!(PlannerLomb64, phast_planner_lomb64_new, phast_planner_lomb64_free, phast_planner_lomb64_slab,
                   phast_planner_lomb64_grid_len, phast_planner_lomb64_workspace_len, phast_planner_lomb64_workspace_min);
impl_planner_lomb!(PlannerLomb32, phast_planner_lomb32_new, phast_planner_lomb32_free, phast_planner_lomb32_slab,
                   phast_planner_lomb32_grid_len, phast_planner_lomb32_workspace_len, phast_planner_lomb32_workspace_min);

macro_rules! impl_planner_upfirdn {
    ($up:ident, $t:ty, $new:ident, $free:ident, $out_len:ident, $full_len:ident, $tile:ident, $chunk:ident) => {
        /// An extension beyond PhastFT 0.3.0: the polyphase FIR of scipy.signal.upfirdn on real signals of `signal_len`
        /// samples -- zero-stuff by `up`, filter with the planner's taps, keep every `down`-th sample -- of which a call
        /// yields the `out_len` samples from `first` on.  One direct kernel, no workspace; the bits of an output depend on the
        /// values alone.  Immutable after `new`.
        pub struct $up {
            pub(crate) h: *mut Opaque,
            pub(crate) signal_len: usize,
        }
        // SAFETY: the handle is immutable after creation; a call works in the caller's buffers (device calls) or in device
        // buffers of its own (host-slice calls)
        unsafe impl Send for $up {}
        unsafe impl Sync for $up {}
        impl $up {
            /// `out_len` = 0 stands for `full_len - first`; `first + out_len` may pass `full_len` (zeros there); `up` and
            /// `down` are used as given.  Panics with "invalid argument" unless 1 <= signal_len, taps.len(), out_len <= 2^29,
            /// 1 <= up, down <= 2^20 and first <= full_len
            pub fn new(signal_len: usize, taps: &[$t], up: usize, down: usize, first: usize, out_len: usize) -> Self {
                let mut h = std::ptr::null_mut();
                ffi::check(unsafe { ffi::$new(signal_len, taps.as_ptr(), taps.len(), up, down, first, out_len, &mut h) });
                Self { h, signal_len }
            }
            pub fn signal_len(&self) -> usize {
                self.signal_len
            }
            pub fn out_len(&self) -> usize {
                unsafe { ffi::$out_len(self.h) }
            }
            /// ((signal_len - 1) up + taps - 1) / down + 1
            pub fn full_len(&self) -> usize {
                unsafe { ffi::$full_len(self.h) }
            }
            /// outputs per workgroup: a function of (taps, up, down) alone
            pub fn tile(&self) -> usize {
                unsafe { ffi::$tile(self.h) }
            }
            /// taps of a phase per LDS chunk
            pub fn chunk(&self) -> usize {
                unsafe { ffi::$chunk(self.h) }
            }
            /// 0: the kernel needs no workspace
            pub fn workspace_min(&self) -> usize {
                0
            }
        }
        impl Drop for $up {
            fn drop(&mut self) {
                unsafe { ffi::$free(self.h) }
            }
        }
    };
}
impl_planner_upfirdn!(PlannerUpfirdn64, f64, phast_planner_upfirdn64_new, phast_planner_upfirdn64_free, phast_planner_upfirdn64_out_len,
                      phast_planner_upfirdn64_full_len, phast_planner_upfirdn64_tile, phast_planner_upfirdn64_chunk);
impl_planner_upfirdn!(PlannerUpfirdn32, f32, phast_planner_upfirdn32_new, phast_planner_upfirdn32_free, phast_planner_upfirdn32_out_len,
                      phast_planner_upfirdn32_full_len, phast_planner_upfirdn32_tile, phast_planner_upfirdn32_chunk);

/// The extension of a discrete wavelet planner (PyWavelets' modes of the same names; `smooth`, `antisymmetric` and
/// `antireflect` are out of scope)
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum DwtMode {
    Zero = 0,
    Constant = 1,
    Symmetric = 2,
    Reflect = 3,
    Periodic = 4,
    Periodization = 5,
}

macro_rules! impl_planner_dwt {
    ($dw:ident, $t:ty, $new:ident, $free:ident, $coeff_len:ident, $level_len:ident, $level_offset:ident, $tile:ident, $ws_len:ident,
     $ws_min:ident) => {
        /// An extension beyond PhastFT 0.3.0: the discrete wavelet transform of real signals of `signal_len` samples and its
        /// inverse (pywt.wavedec / waverec) with `level` levels: four filters of one even length 2 ..= 256, used as given.  A
        /// signal's result is the packed row [cA_J | cD_J | .. | cD_1] of `coeff_len()` elements.  One direct kernel launch per
        /// level; the bits of a coefficient depend on the filters, the mode and the values alone.  Immutable after `new`.
        pub struct $dw {
            pub(crate) h: *mut Opaque,
            pub(crate) signal_len: usize,
        }
        // SAFETY: the handle is immutable after creation; a call works in the caller's buffers (device calls) or in device
        // buffers of its own (host-slice calls)
        unsafe impl Send for $dw {}
        unsafe impl Sync for $dw {}
        impl $dw {
            /// Panics with "invalid argument" unless 1 <= signal_len <= 2^29, the four filters have one even length 2 ..= 256
            /// and 1 <= level <= 32 (more levels than floor(log2(signal_len / (F - 1))) are legal)
            pub fn new(signal_len: usize, dec_lo: &[$t], dec_hi: &[$t], rec_lo: &[$t], rec_hi: &[$t], level: usize, mode: DwtMode) -> Self {
                assert!(dec_hi.len() == dec_lo.len() && rec_lo.len() == dec_lo.len() && rec_hi.len() == dec_lo.len(), "invalid argument");
                let mut h = std::ptr::null_mut();
                ffi::check(unsafe {
                    ffi::$new(signal_len, dec_lo.as_ptr(), dec_hi.as_ptr(), rec_lo.as_ptr(), rec_hi.as_ptr(), dec_lo.len(), level, mode as c_int, &mut h)
                });
                Self { h, signal_len }
            }
            pub fn signal_len(&self) -> usize {
                self.signal_len
            }
            /// elements of a packed row: n_J + the sum of n_l
            pub fn coeff_len(&self) -> usize {
                unsafe { ffi::$coeff_len(self.h) }
            }
            /// n_l for 0 <= l <= J (n_0 = signal_len)
            pub fn level_len(&self, level: usize) -> usize {
                unsafe { ffi::$level_len(self.h, level) }
            }
            /// where cD_l starts in the packed row, 1 <= l <= J (cA_J starts at 0)
            pub fn level_offset(&self, level: usize) -> usize {
                unsafe { ffi::$level_offset(self.h, level) }
            }
            /// coefficient indices / output pairs per workgroup
            pub fn tile(&self) -> usize {
                unsafe { ffi::$tile(self.h) }
            }
            /// elements of T a device call of `batch` signals works in: two ping-pong rows per signal, 0 for one level
            pub fn workspace_len(&self, batch: usize) -> usize {
                unsafe { ffi::$ws_len(self.h, batch) }
            }
            /// the least a device call runs in (one signal's rows)
            pub fn workspace_min(&self) -> usize {
                unsafe { ffi::$ws_min(self.h) }
            }
        }
        impl Drop for $dw {
            fn drop(&mut self) {
                unsafe { ffi::$free(self.h) }
            }
        }
    };
}
impl_planner_dwt!(PlannerDwt64, f64, phast_planner_dwt64_new, phast_planner_dwt64_free, phast_planner_dwt64_coeff_len,
                  phast_planner_dwt64_level_len, phast_planner_dwt64_level_offset, phast_planner_dwt64_tile,
                  phast_planner_dwt64_workspace_len, phast_planner_dwt64_workspace_min);
impl_planner_dwt!(PlannerDwt32, f32, phast_planner_dwt32_new, phast_planner_dwt32_free, phast_planner_dwt32_coeff_len,
                  phast_planner_dwt32_level_len, phast_planner_dwt32_level_offset, phast_planner_dwt32_tile,
                  phast_planner_dwt32_workspace_len, phast_planner_dwt32_workspace_min);

macro_rules! impl_planner_resample {
    ($rs:ident, $new:ident, $free:ident, $ws_len:ident, $ws_min:ident) => {
        /// An extension beyond PhastFT 0.3.0: scipy.signal.resample(x, num) of real signals of `signal_len` samples (Fourier
        /// method, no window): one R2C of `signal_len` and one C2R of `num` on the any-length real path around one sweep.
        /// Immutable after `new`.
        pub struct $rs {
            pub(crate) h: *mut Opaque,
            pub(crate) signal_len: usize,
            num: usize,
        }
        // SAFETY: as for the polyphase planner
        unsafe impl Send for $rs {}
        unsafe impl Sync for $rs {}
        impl $rs {
            /// Panics with "invalid argument" unless 1 <= signal_len, num <= 2^29
            pub fn new(signal_len: usize, num: usize) -> Self {
                let mut h = std::ptr::null_mut();
                ffi::check(unsafe { ffi::$new(signal_len, num, &mut h) });
                Self { h, signal_len, num }
            }
            pub fn signal_len(&self) -> usize {
                self.signal_len
            }
            pub fn out_len(&self) -> usize {
                self.num
            }
            /// elements of the workspace a device call of `batch` signals works in
            pub fn workspace_len(&self, batch: usize) -> usize {
                unsafe { ffi::$ws_len(self.h, batch) }
            }
            /// the least workspace a call runs in: one signal
            pub fn workspace_min(&self) -> usize {
                unsafe { ffi::$ws_min(self.h) }
            }
        }
        impl Drop for $rs {
            fn drop(&mut self) {
                unsafe { ffi::$free(self.h) }
            }
        }
    };
}
impl_planner_resample!(PlannerResample64, phast_planner_resample64_new, phast_planner_resample64_free,
                       phast_planner_resample64_workspace_len, phast_planner_resample64_workspace_min);
impl_planner_resample!(PlannerResample32, phast_planner_resample32_new, phast_planner_resample32_free,
                       phast_planner_resample32_workspace_len, phast_planner_resample32_workspace_min);

macro_rules! impl_planner_channelizer {
    ($ch:ident, $t:ty, $new:ident, $free:ident, $out_frames:ident, $full_frames:ident, $bins:ident, $tile_frames:ident, $tile_cols:ident,
     $chunk:ident, $periods:ident, $ws_len:ident, $ws_min:ident) => {
        /// An extension beyond PhastFT 0.3.0: the polyphase filter-bank channelizer (the analysis side of a uniform DFT filter
        /// bank) of signals of `signal_len` samples -- `channels` equally spaced channels, each the signal times
        /// exp(-2 pi i k n / channels), filtered with the planner's real taps and decimated by `hop`, with zero extension -- of
        /// which a call yields the `out_frames` frames from `first_frame` on.  One fold kernel and one `channels`-point
        /// transform per frame; the bits of an output depend on the values alone.  Immutable after `new`.
        pub struct $ch {
            pub(crate) h: *mut Opaque,
            pub(crate) signal_len: usize,
            complex_input: bool,
        }
        // SAFETY: the handle is immutable after creation; a call works in the caller's buffers (device calls) or in device
        // buffers of its own (host-slice calls)
        unsafe impl Send for $ch {}
        unsafe impl Sync for $ch {}
        impl $ch {
            /// `out_frames` = 0 stands for `full_frames - first_frame`; the window may pass `full_frames` (zeros there);
            /// `complex_input`: the signals are (re, im) planes and a frame has `channels` bins, else `channels / 2 + 1`.
            /// Panics with "invalid argument" unless 1 <= signal_len, taps.len(), channels, hop <= 2^29, first_frame <=
            /// full_frames, out_frames >= 1 and out_frames * channels <= 2^30
            pub fn new(signal_len: usize, taps: &[$t], channels: usize, hop: usize, first_frame: usize, out_frames: usize,
                       complex_input: bool) -> Self {
                let mut h = std::ptr::null_mut();
                ffi::check(unsafe {
                    ffi::$new(signal_len, taps.as_ptr(), taps.len(), channels, hop, first_frame, out_frames, complex_input as c_int, &mut h)
                });
                Self { h, signal_len, complex_input }
            }
            pub fn signal_len(&self) -> usize {
                self.signal_len
            }
            pub fn complex_input(&self) -> bool {
                self.complex_input
            }
            pub fn out_frames(&self) -> usize {
                unsafe { ffi::$out_frames(self.h) }
            }
            /// (signal_len + taps - 2) / hop + 1
            pub fn full_frames(&self) -> usize {
                unsafe { ffi::$full_frames(self.h) }
            }
            /// bins of a frame: channels (complex signals) or channels / 2 + 1 (real signals)
            pub fn bins(&self) -> usize {
                unsafe { ffi::$bins(self.h) }
            }
            /// the fold's tile: (frames, columns) per workgroup, a function of (taps, channels, hop) alone
            pub fn tile(&self) -> (usize, usize) {
                unsafe { (ffi::$tile_frames(self.h), ffi::$tile_cols(self.h)) }
            }
            /// tap rows per LDS chunk
            pub fn chunk(&self) -> usize {
                unsafe { ffi::$chunk(self.h) }
            }
            /// periods of the signal a tile stages in LDS per chunk
            pub fn periods(&self) -> usize {
                unsafe { ffi::$periods(self.h) }
            }
            /// elements of the workspace a device call of `batch` signals works in
            pub fn workspace_len(&self, batch: usize) -> usize {
                unsafe { ffi::$ws_len(self.h, batch) }
            }
            /// the least workspace a call runs in: one frame (0 for complex signals and a power-of-two `channels`)
            pub fn workspace_min(&self) -> usize {
                unsafe { ffi::$ws_min(self.h) }
            }
        }
        impl Drop for $ch {
            fn drop(&mut self) {
                unsafe { ffi::$free(self.h) }
            }
        }
    };
}
impl_planner_channelizer!(PlannerChannelizer64, f64, phast_planner_channelizer64_new, phast_planner_channelizer64_free,
                          phast_planner_channelizer64_out_frames, phast_planner_channelizer64_full_frames, phast_planner_channelizer64_bins,
                          phast_planner_channelizer64_tile_frames, phast_planner_channelizer64_tile_cols, phast_planner_channelizer64_chunk,
                          phast_planner_channelizer64_periods, phast_planner_channelizer64_workspace_len,
                          phast_planner_channelizer64_workspace_min);
impl_planner_channelizer!(PlannerChannelizer32, f32, phast_planner_channelizer32_new, phast_planner_channelizer32_free,
                          phast_planner_channelizer32_out_frames, phast_planner_channelizer32_full_frames, phast_planner_channelizer32_bins,
                          phast_planner_channelizer32_tile_frames, phast_planner_channelizer32_tile_cols, phast_planner_channelizer32_chunk,
                          phast_planner_channelizer32_periods, phast_planner_channelizer32_workspace_len,
                          phast_planner_channelizer32_workspace_min);

macro_rules! impl_planner_synthesizer {
    ($sy:ident, $t:ty, $new:ident, $free:ident, $out_len:ident, $full_len:ident, $bins:ident, $tile:ident, $per:ident, $terms:ident,
     $ws_len:ident, $ws_min:ident) => {
        /// An extension beyond PhastFT 0.3.0: the polyphase synthesis filter bank, the inverse side of the channelizer -- from
        /// `frames` frames of `channels` channels, s[n] = sum_m g[n - m hop] sum_k Y[m][k] exp(2 pi i k n / channels) with the
        /// planner's real taps g and zero extension, of which a call yields the `out_len` samples from `first` on.  One
        /// `channels`-point inverse transform per frame and one gather kernel; the bits of an output depend on the values alone.
        /// The phases are in absolute time, so the delay of an analysis / synthesis pair must be a multiple of `channels`: for
        /// analysis taps h of channels * T points, g = (0, h reversed) is the channelizer's adjoint delayed by h.len().
        /// Immutable after `new`.
        pub struct $sy {
            pub(crate) h: *mut Opaque,
            pub(crate) frames: usize,
            complex_output: bool,
        }
        // SAFETY: the handle is immutable after creation; a call works in the caller's buffers (device calls) or in device
        // buffers of its own (host-slice calls)
        unsafe impl Send for $sy {}
        unsafe impl Sync for $sy {}
        impl $sy {
            /// `out_len` = 0 stands for `full_len - first`; the window may pass `full_len` (zeros there); `complex_output`: a
            /// frame has `channels` bins and the signal is (re, im) planes, else `channels / 2 + 1` bins and one plane.
            /// Panics with "invalid argument" unless 1 <= frames, taps.len(), channels, hop <= 2^29, frames * channels <= 2^30,
            /// first <= full_len and 1 <= out_len <= 2^30
            pub fn new(frames: usize, taps: &[$t], channels: usize, hop: usize, first: usize, out_len: usize, complex_output: bool) -> Self {
                let mut h = std::ptr::null_mut();
                ffi::check(unsafe {
                    ffi::$new(frames, taps.as_ptr(), taps.len(), channels, hop, first, out_len, complex_output as c_int, &mut h)
                });
                Self { h, frames, complex_output }
            }
            pub fn frames(&self) -> usize {
                self.frames
            }
            pub fn complex_output(&self) -> bool {
                self.complex_output
            }
            pub fn out_len(&self) -> usize {
                unsafe { ffi::$out_len(self.h) }
            }
            /// (frames - 1) * hop + taps
            pub fn full_len(&self) -> usize {
                unsafe { ffi::$full_len(self.h) }
            }
            /// bins of a frame: channels (complex output) or channels / 2 + 1 (real output)
            pub fn bins(&self) -> usize {
                unsafe { ffi::$bins(self.h) }
            }
            /// the unfold's tile: (output samples per workgroup, per thread)
            pub fn tile(&self) -> (usize, usize) {
                unsafe { (ffi::$tile(self.h), ffi::$per(self.h)) }
            }
            /// terms of an output sample at most: ceil(taps / hop)
            pub fn max_terms(&self) -> usize {
                unsafe { ffi::$terms(self.h) }
            }
            /// elements of the workspace a device call of `batch` signals works in
            pub fn workspace_len(&self, batch: usize) -> usize {
                unsafe { ffi::$ws_len(self.h, batch) }
            }
            /// the least workspace a call runs in: one signal's frames (0 for complex output of one channel)
            pub fn workspace_min(&self) -> usize {
                unsafe { ffi::$ws_min(self.h) }
            }
        }
        impl Drop for $sy {
            fn drop(&mut self) {
                unsafe { ffi::$free(self.h) }
            }
        }
    };
}
impl_planner_synthesizer!(PlannerSynthesizer64, f64, phast_planner_synthesizer64_new, phast_planner_synthesizer64_free,
                          phast_planner_synthesizer64_out_len, phast_planner_synthesizer64_full_len, phast_planner_synthesizer64_bins,
                          phast_planner_synthesizer64_tile_samples, phast_planner_synthesizer64_per_thread,
                          phast_planner_synthesizer64_max_terms, phast_planner_synthesizer64_workspace_len,
                          phast_planner_synthesizer64_workspace_min);
impl_planner_synthesizer!(PlannerSynthesizer32, f32, phast_planner_synthesizer32_new, phast_planner_synthesizer32_free,
                          phast_planner_synthesizer32_out_len, phast_planner_synthesizer32_full_len, phast_planner_synthesizer32_bins,
                          phast_planner_synthesizer32_tile_samples, phast_planner_synthesizer32_per_thread,
                          phast_planner_synthesizer32_max_terms, phast_planner_synthesizer32_workspace_len,
                          phast_planner_synthesizer32_workspace_min);

/// The wavelet family of a CWT planner (PHAST_CWT_* of the C ABI; Torrence & Compo 1998, table 1); `Step`: the analytic-signal filter
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum CwtFamily {
    Morlet = 0,
    Paul = 1,
    Dog = 2,
    Step = 3,
}

/// The normalisation of a CWT planner: `L2` c = sqrt(2 pi s) (unit energy), `Peak` c = 2 / max |psi^|
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum CwtNorm {
    L2 = 0,
    Peak = 1,
}

macro_rules! impl_planner_cwt {
    ($cw:ident, $t:ty, $new:ident, $free:ident, $pad_len:ident, $scales:ident, $tile:ident, $group:ident, $ws_len:ident, $ws_min:ident) => {
        /// An extension beyond PhastFT 0.3.0: the continuous wavelet transform of signals of `signal_len` points at the given
        /// scales (in samples), W[j][n] = ifft_P(fft_P(x) conj(c_j psi^(s_j w)))[n] for n < signal_len with the signal
        /// zero-extended to `pad_len` points, and with `CwtFamily::Step` and one scale the analytic signal.  One forward
        /// transform per signal, one bank kernel, one inverse transform per scale; the bits of a row depend on its signal and
        /// scale alone.  Immutable after `new`.
        pub struct $cw {
            pub(crate) h: *mut Opaque,
            pub(crate) signal_len: usize,
            real_input: bool,
        }
        // SAFETY: the handle is immutable after creation; a call works in the caller's buffers (device calls) or in device
        // buffers of its own (host-slice calls)
        unsafe impl Send for $cw {}
        unsafe impl Sync for $cw {}
        impl $cw {
            /// `pad_len` = 0 stands for `signal_len`; `param`: w0 of Morlet, the integer m of Paul (<= 85) and DOG (<= 170),
            /// ignored by Step; `real_input`: one input plane, else (re, im) planes.  Panics with "invalid argument" unless
            /// 1 <= signal_len <= pad_len <= 2^29, 1 <= scales.len() <= 2^20, every scale is finite and > 0 and `param` is legal
            pub fn new(signal_len: usize, scales: &[f64], family: CwtFamily, param: f64, norm: CwtNorm, pad_len: usize, real_input: bool) -> Self {
                let mut h = std::ptr::null_mut();
                ffi::check(unsafe {
                    ffi::$new(signal_len, pad_len, scales.as_ptr(), scales.len(), family as c_int, param, norm as c_int, real_input as c_int, &mut h)
                });
                Self { h, signal_len, real_input }
            }
            pub fn signal_len(&self) -> usize {
                self.signal_len
            }
            pub fn real_input(&self) -> bool {
                self.real_input
            }
            pub fn pad_len(&self) -> usize {
                unsafe { ffi::$pad_len(self.h) }
            }
            pub fn num_scales(&self) -> usize {
                unsafe { ffi::$scales(self.h) }
            }
            /// the bank's tile: (bins per workgroup, scales per workgroup at most)
            pub fn tile(&self) -> (usize, usize) {
                unsafe { (ffi::$tile(self.h), ffi::$group(self.h)) }
            }
            /// elements of the workspace a device call of `batch` signals works in
            pub fn workspace_len(&self, batch: usize) -> usize {
                unsafe { ffi::$ws_len(self.h, batch) }
            }
            /// the least workspace a call runs in: one signal's spectrum and one row
            pub fn workspace_min(&self) -> usize {
                unsafe { ffi::$ws_min(self.h) }
            }
        }
        impl Drop for $cw {
            fn drop(&mut self) {
                unsafe { ffi::$free(self.h) }
            }
        }
    };
}
impl_planner_cwt!(PlannerCwt64, f64, phast_planner_cwt64_new, phast_planner_cwt64_free, phast_planner_cwt64_pad_len,
                  phast_planner_cwt64_num_scales, phast_planner_cwt64_tile_bins, phast_planner_cwt64_scale_group,
                  phast_planner_cwt64_workspace_len, phast_planner_cwt64_workspace_min);
impl_planner_cwt!(PlannerCwt32, f32, phast_planner_cwt32_new, phast_planner_cwt32_free, phast_planner_cwt32_pad_len,
                  phast_planner_cwt32_num_scales, phast_planner_cwt32_tile_bins, phast_planner_cwt32_scale_group,
                  phast_planner_cwt32_workspace_len, phast_planner_cwt32_workspace_min);

/// Which part of the full convolution a planner yields (PHAST_CONV_* of the C ABI)
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum ConvMode {
    Full = 0,
    Same = 1,
    Valid = 2,
}

macro_rules! impl_planner_conv {
    ($conv:ident, $t:ty, $new:ident, $free:ident, $out_len:ident, $block:ident, $segments:ident, $ws_len:ident, $ws_min:ident) => {
        /// An extension beyond PhastFT 0.3.0: convolution (`correlate`: cross-correlation) of real signals of `signal_len`
        /// samples with the planner's taps by overlap-save (scipy.signal.convolve / correlate with method = "direct"): one
        /// R2C, one spectrum multiply and one C2R of `block` points per segment.  Immutable after `new`, like the
        /// reference's planners.
        pub struct $conv {
            pub(crate) h: *mut Opaque,
            pub(crate) signal_len: usize,
        }
        // SAFETY: the handle is immutable after creation; a call works in the caller's workspace (device calls) or in
        // device buffers of its own (host-slice calls)
        unsafe impl Send for $conv {}
        unsafe impl Sync for $conv {}
        impl $conv {
            /// `block` = 0 picks the block from the number of taps.  Panics with "invalid argument" unless 1 <= signal_len,
            /// taps.len() <= 2^29, signal_len >= taps.len() with `ConvMode::Valid`, taps.len() <= block <= 2^29, at most
            /// 2^29 output samples and at most 2^30 points in the segments
            pub fn new(signal_len: usize, taps: &[$t], mode: ConvMode, correlate: bool, block: usize) -> Self {
                let mut h = std::ptr::null_mut();
                ffi::check(unsafe { ffi::$new(signal_len, taps.as_ptr(), taps.len(), mode as c_int, correlate as c_int, block, &mut h) });
                Self { h, signal_len }
            }
            pub fn signal_len(&self) -> usize {
                self.signal_len
            }
            pub fn out_len(&self) -> usize {
                unsafe { ffi::$out_len(self.h) }
            }
            pub fn block(&self) -> usize {
                unsafe { ffi::$block(self.h) }
            }
            pub fn segments(&self) -> usize {
                unsafe { ffi::$segments(self.h) }
            }
            /// elements of the workspace a device call of `batch` signals works in
            pub fn workspace_len(&self, batch: usize) -> usize {
                unsafe { ffi::$ws_len(self.h, batch) }
            }
            /// the least workspace a call runs in: one segment
            pub fn workspace_min(&self) -> usize {
                unsafe { ffi::$ws_min(self.h) }
            }
        }
        impl Drop for $conv {
            fn drop(&mut self) {
                unsafe { ffi::$free(self.h) }
            }
        }
    };
}
impl_planner_conv!(PlannerConv64, f64, phast_planner_conv64_new, phast_planner_conv64_free, phast_planner_conv64_out_len,
                   phast_planner_conv64_block, phast_planner_conv64_segments, phast_planner_conv64_workspace_len,
                   phast_planner_conv64_workspace_min);
impl_planner_conv!(PlannerConv32, f32, phast_planner_conv32_new, phast_planner_conv32_free, phast_planner_conv32_out_len,
                   phast_planner_conv32_block, phast_planner_conv32_segments, phast_planner_conv32_workspace_len,
                   phast_planner_conv32_workspace_min);

macro_rules! impl_planner_convnd {
    ($conv:ident, $t:ty, $new:ident, $free:ident, $out_len:ident, $out_dims:ident, $block:ident, $tiles:ident, $ws_len:ident,
     $ws_min:ident) => {
        /// An extension beyond PhastFT 0.3.0: convolution (`correlate`: cross-correlation) of real row-major arrays of rank
        /// 1 .. 3 with the planner's taps of the same rank, by overlap-save along every axis (scipy.signal.convolve /
        /// correlate with method = "direct"): one N-d R2C, one spectrum multiply and one N-d C2R per tile of `block` points
        /// per axis.  Immutable after `new`, like the reference's planners.
        pub struct $conv {
            pub(crate) h: *mut Opaque,
            pub(crate) signal_len: usize,
            rank: usize,
        }
        // SAFETY: the handle is immutable after creation; a call works in the caller's workspace (device calls) or in
        // device buffers of its own (host-slice calls)
        unsafe impl Send for $conv {}
        unsafe impl Sync for $conv {}
        impl $conv {
            /// `taps`: row-major, `taps_shape` of the rank of `signal_shape`; `block`: `None`, or one entry per axis (0 picks
            /// that axis' block from the taps).  Panics with "invalid argument" unless the rank is 1 .. 3, every extent is
            /// 1 ..= 2^29, `signal_shape[i] >= taps_shape[i]` with `ConvMode::Valid`, `taps_shape[i] <= block[i] <= 2^29`, the
            /// array and the output hold at most 2^30 points and a tile at most 2^28
            pub fn new(signal_shape: &[usize], taps_shape: &[usize], taps: &[$t], mode: ConvMode, correlate: bool,
                       block: Option<&[usize]>) -> Self {
                let rank = signal_shape.len();
                assert!(taps_shape.len() == rank && block.map_or(true, |b| b.len() == rank), "invalid argument");
                assert!(taps.len() == taps_shape.iter().product::<usize>(), "invalid argument");
                let mut h = std::ptr::null_mut();
                ffi::check(unsafe {
                    ffi::$new(signal_shape.as_ptr(), taps_shape.as_ptr(), rank, taps.as_ptr(), mode as c_int, correlate as c_int,
                              block.map_or(std::ptr::null(), |b| b.as_ptr()), &mut h)
                });
                Self { h, signal_len: signal_shape.iter().product(), rank }
            }
            pub fn signal_len(&self) -> usize {
                self.signal_len
            }
            pub fn out_len(&self) -> usize {
                unsafe { ffi::$out_len(self.h) }
            }
            pub fn out_shape(&self) -> Vec<usize> {
                let mut d = vec![0usize; self.rank];
                ffi::check(unsafe { ffi::$out_dims(self.h, d.as_mut_ptr(), self.rank) });
                d
            }
            pub fn block(&self) -> Vec<usize> {
                let mut d = vec![0usize; self.rank];
                ffi::check(unsafe { ffi::$block(self.h, d.as_mut_ptr(), self.rank) });
                d
            }
            pub fn tiles(&self) -> usize {
                unsafe { ffi::$tiles(self.h) }
            }
            /// elements of the workspace a device call of `batch` arrays works in
            pub fn workspace_len(&self, batch: usize) -> usize {
                unsafe { ffi::$ws_len(self.h, batch) }
            }
            /// the least workspace a call runs in: one tile
            pub fn workspace_min(&self) -> usize {
                unsafe { ffi::$ws_min(self.h) }
            }
        }
        impl Drop for $conv {
            fn drop(&mut self) {
                unsafe { ffi::$free(self.h) }
            }
        }
    };
}
impl_planner_convnd!(PlannerConvNd64, f64, phast_planner_convnd64_new, phast_planner_convnd64_free, phast_planner_convnd64_out_len,
                     phast_planner_convnd64_out_dims, phast_planner_convnd64_block, phast_planner_convnd64_tiles,
                     phast_planner_convnd64_workspace_len, phast_planner_convnd64_workspace_min);
impl_planner_convnd!(PlannerConvNd32, f32, phast_planner_convnd32_new, phast_planner_convnd32_free, phast_planner_convnd32_out_len,
                     phast_planner_convnd32_out_dims, phast_planner_convnd32_block, phast_planner_convnd32_tiles,
                     phast_planner_convnd32_workspace_len, phast_planner_convnd32_workspace_min);

macro_rules! impl_planner_czt {
    ($czt:ident, $new:ident, $free:ident, $conv_len:ident, $ws_len:ident) => {
        /// An extension beyond PhastFT 0.3.0, whose planners give whole spectra: the chirp-Z transform on the unit circle
        /// (scipy.signal.czt / zoom_fft), `m` bins of `n` points at the frequencies `start + k * step` turns,
        /// X[k] = sum x[n] exp(-2 pi i n (start + k step)).  Immutable after `new`, like the reference's planners.
        pub struct $czt {
            pub(crate) h: *mut Opaque,
            pub(crate) n: usize,
            pub(crate) m: usize,
        }
        // SAFETY: the handle is immutable after creation; a call works in the caller's workspace (device calls) or in
        // device buffers of its own (host-slice calls)
        unsafe impl Send for $czt {}
        unsafe impl Sync for $czt {}
        impl $czt {
            /// Panics with "invalid argument" unless 1 <= n, 1 <= m, n + m - 1 <= 2^30 and `step` and `start` are finite
            pub fn new(n: usize, m: usize, step: f64, start: f64) -> Self {
                let mut h = std::ptr::null_mut();
                ffi::check(unsafe { ffi::$new(n, m, step, start, &mut h) });
                Self { h, n, m }
            }
            pub fn input_len(&self) -> usize {
                self.n
            }
            pub fn output_len(&self) -> usize {
                self.m
            }
            /// the convolution length L: the smallest power of two >= n + m - 1, at least 8
            pub fn conv_len(&self) -> usize {
                unsafe { ffi::$conv_len(self.h) }
            }
            /// elements of the workspace a device call of `batch` transforms works in: 2 L batch
            pub fn workspace_len(&self, batch: usize) -> usize {
                unsafe { ffi::$ws_len(self.h, batch) }
            }
        }
        impl Drop for $czt {
            fn drop(&mut self) {
                unsafe { ffi::$free(self.h) }
            }
        }
    };
}
impl_planner_czt!(PlannerCzt64, phast_planner_czt64_new, phast_planner_czt64_free, phast_planner_czt64_conv_len,
                  phast_planner_czt64_workspace_len);
impl_planner_czt!(PlannerCzt32, phast_planner_czt32_new, phast_planner_czt32_free, phast_planner_czt32_conv_len,
                  phast_planner_czt32_workspace_len);

macro_rules! impl_planner_nufft {
    ($nufft:ident, $new:ident, $new_dev:ident, $set_points:ident, $free:ident, $grid_len:ident, $width:ident, $ws_len:ident) => {
        /// An extension beyond PhastFT 0.3.0, whose planners take samples on a grid: non-uniform FFTs of types 1 and 2 of the
        /// points `x` (turns, reduced mod 1) and `n_modes` modes in numpy fftfreq order, to the relative accuracy `eps`.
        /// Immutable after `new`, like the reference's planners, but for `set_points_dev` (which takes `&mut self`).
        pub struct $nufft {
            pub(crate) h: *mut Opaque,
            pub(crate) n: usize,
            pub(crate) m: usize,
        }
        // SAFETY: the handle is immutable after creation; a call works in the caller's workspace (device calls) or in
        // device buffers of its own (host-slice calls)
        unsafe impl Send for $nufft {}
        unsafe impl Sync for $nufft {}
        impl $nufft {
            /// Panics with "invalid argument" unless 1 <= n_modes <= 2^28, 1 <= x.len() <= 2^30, every x is finite and eps
            /// lies in [1e-14, 1e-1] (f64) or [1e-6, 1e-1] (f32)
            pub fn new(n_modes: usize, x: &[f64], eps: f64) -> Self {
                let mut h = std::ptr::null_mut();
                ffi::check(unsafe { ffi::$new(n_modes, x.as_ptr(), x.len(), eps, &mut h) });
                Self { h, n: n_modes, m: x.len() }
            }
            /// The planner for `m_points` points in DEVICE memory (`d_x`: doubles in turns), sorted on the device into the very
            /// tables `new` builds on the host, ordered after the earlier work of `stream`; blocks until the planner is built.
            /// Panics with "invalid argument" for the sizes `new` refuses, a null pointer, a stream that is capturing or a point
            /// that is not finite.
            ///
            /// # Safety
            /// the pointers must be valid device memory of `m_points` doubles and `stream` a HIP stream or null
            pub unsafe fn from_device(n_modes: usize, d_x: *const f64, m_points: usize, eps: f64, stream: *mut c_void) -> Self {
                let mut h = std::ptr::null_mut();
                ffi::check(ffi::$new_dev(n_modes, d_x, m_points, eps, stream, &mut h));
                Self { h, n: n_modes, m: m_points }
            }
            /// New points for this planner, the same number of them (another `m_points` panics with "planner size"), from device
            /// memory: the tables are rewritten in place, so a HIP graph captured through the planner stays valid and, replayed,
            /// transforms at the new points.  Ordered after the earlier work of `stream` ONLY -- work on other streams that uses
            /// the planner must have finished -- and blocks until done.  A rejected point set leaves the planner as it was.
            ///
            /// # Safety
            /// as `from_device`
            pub unsafe fn set_points_dev(&mut self, d_x: *const f64, m_points: usize, stream: *mut c_void) {
                ffi::check(ffi::$set_points(self.h, d_x, m_points, stream));
            }
            pub fn num_modes(&self) -> usize {
                self.n
            }
            pub fn num_points(&self) -> usize {
                self.m
            }
            /// the fine grid n_g: the smallest power of two >= max(2 n_modes, 2 width, 8)
            pub fn grid_len(&self) -> usize {
                unsafe { ffi::$grid_len(self.h) }
            }
            /// the width of the spreading kernel in grid cells
            pub fn width(&self) -> usize {
                unsafe { ffi::$width(self.h) as usize }
            }
            /// elements of the workspace a device call of `batch` transforms works in: 2 n_g batch
            pub fn workspace_len(&self, batch: usize) -> usize {
                unsafe { ffi::$ws_len(self.h, batch) }
            }
        }
        impl Drop for $nufft {
            fn drop(&mut self) {
                unsafe { ffi::$free(self.h) }
            }
        }
    };
}
impl_planner_nufft!(PlannerNufft64, phast_planner_nufft64_new, phast_planner_nufft64_new_dev,
                    phast_planner_nufft64_set_points_dev, phast_planner_nufft64_free, phast_planner_nufft64_grid_len,
                    phast_planner_nufft64_width, phast_planner_nufft64_workspace_len);
impl_planner_nufft!(PlannerNufft32, phast_planner_nufft32_new, phast_planner_nufft32_new_dev,
                    phast_planner_nufft32_set_points_dev, phast_planner_nufft32_free, phast_planner_nufft32_grid_len,
                    phast_planner_nufft32_width, phast_planner_nufft32_workspace_len);

macro_rules! impl_planner_nufft2d {
    ($nufft:ident, $new:ident, $new_dev:ident, $set_points:ident, $free:ident, $grid_len:ident, $rows:ident, $cols:ident, $width:ident, $ws_len:ident) => {
        /// An extension beyond PhastFT 0.3.0: two-dimensional non-uniform FFTs of types 1 and 2 of the points `(x, y)` (turns,
        /// reduced mod 1 per coordinate) and `n1 x n2` modes, row-major, each axis in numpy fftfreq order (k1 pairs with x, k2
        /// with y), to the relative accuracy `eps`.  Immutable after `new`, like the reference's planners.
        pub struct $nufft {
            pub(crate) h: *mut Opaque,
            pub(crate) n: (usize, usize),
            pub(crate) m: usize,
        }
        // SAFETY: the handle is immutable after creation; a call works in the caller's workspace (device calls) or in
        // a device buffer of its own (host-slice calls)
        unsafe impl Send for $nufft {}
        unsafe impl Sync for $nufft {}
        impl $nufft {
            /// Panics with "invalid argument" unless n1, n2 >= 1, the fine grid g1 g2 <= 2^28, 1 <= x.len() == y.len() <= 2^30,
            /// every coordinate is finite and eps lies in [1e-14, 1e-1] (f64) or [1e-6, 1e-1] (f32)
            pub fn new(n_modes: (usize, usize), x: &[f64], y: &[f64], eps: f64) -> Self {
                assert_eq!(x.len(), y.len());
                let mut h = std::ptr::null_mut();
                ffi::check(unsafe { ffi::$new(n_modes.0, n_modes.1, x.as_ptr(), y.as_ptr(), x.len(), eps, &mut h) });
                Self { h, n: n_modes, m: x.len() }
            }
            /// The planner for `m_points` points in DEVICE memory (`d_x`, `d_y`: doubles in turns), sorted on the device into the very
            /// tables `new` builds on the host, ordered after the earlier work of `stream`; blocks until the planner is built.
            /// Panics with "invalid argument" for the sizes `new` refuses, a null pointer, a stream that is capturing or a point
            /// that is not finite.
            ///
            /// # Safety
            /// the pointers must be valid device memory of `m_points` doubles and `stream` a HIP stream or null
            pub unsafe fn from_device(n_modes: (usize, usize), d_x: *const f64, d_y: *const f64, m_points: usize, eps: f64,
                                      stream: *mut c_void) -> Self {
                let mut h = std::ptr::null_mut();
                ffi::check(ffi::$new_dev(n_modes.0, n_modes.1, d_x, d_y, m_points, eps, stream, &mut h));
                Self { h, n: n_modes, m: m_points }
            }
            /// New points for this planner, the same number of them (another `m_points` panics with "planner size"), from device
            /// memory: the tables are rewritten in place, so a HIP graph captured through the planner stays valid and, replayed,
            /// transforms at the new points.  Ordered after the earlier work of `stream` ONLY -- work on other streams that uses
            /// the planner must have finished -- and blocks until done.  A rejected point set leaves the planner as it was.
            ///
            /// # Safety
            /// as `from_device`
            pub unsafe fn set_points_dev(&mut self, d_x: *const f64, d_y: *const f64, m_points: usize, stream: *mut c_void) {
                ffi::check(ffi::$set_points(self.h, d_x, d_y, m_points, stream));
            }
            pub fn num_modes(&self) -> (usize, usize) {
                self.n
            }
            pub fn num_points(&self) -> usize {
                self.m
            }
            /// the fine grid G = g1 g2
            pub fn grid_len(&self) -> usize {
                unsafe { ffi::$grid_len(self.h) }
            }
            /// (g1, g2): per axis the smallest power of two >= max(2 n, 2 width, 8)
            pub fn grid_shape(&self) -> (usize, usize) {
                unsafe { (ffi::$rows(self.h), ffi::$cols(self.h)) }
            }
            /// the width of the spreading kernel in grid cells
            pub fn width(&self) -> usize {
                unsafe { ffi::$width(self.h) as usize }
            }
            /// elements of the workspace a device call of `batch` transforms works in: 4 G batch
            pub fn workspace_len(&self, batch: usize) -> usize {
                unsafe { ffi::$ws_len(self.h, batch) }
            }
        }
        impl Drop for $nufft {
            fn drop(&mut self) {
                unsafe { ffi::$free(self.h) }
            }
        }
    };
}
impl_planner_nufft2d!(PlannerNufft2d64, phast_planner_nufft2d64_new, phast_planner_nufft2d64_new_dev,
                      phast_planner_nufft2d64_set_points_dev, phast_planner_nufft2d64_free, phast_planner_nufft2d64_grid_len,
                      phast_planner_nufft2d64_grid_rows, phast_planner_nufft2d64_grid_cols, phast_planner_nufft2d64_width,
                      phast_planner_nufft2d64_workspace_len);
impl_planner_nufft2d!(PlannerNufft2d32, phast_planner_nufft2d32_new, phast_planner_nufft2d32_new_dev,
                      phast_planner_nufft2d32_set_points_dev, phast_planner_nufft2d32_free, phast_planner_nufft2d32_grid_len,
                      phast_planner_nufft2d32_grid_rows, phast_planner_nufft2d32_grid_cols, phast_planner_nufft2d32_width,
                      phast_planner_nufft2d32_workspace_len);

macro_rules! impl_planner_nufft3d {
    ($nufft:ident, $new:ident, $new_dev:ident, $set_points:ident, $free:ident, $grid_len:ident, $grid_dim:ident, $width:ident, $ws_len:ident) => {
        /// An extension beyond PhastFT 0.3.0: three-dimensional non-uniform FFTs of types 1 and 2 of the points `(x, y, z)`
        /// (turns, reduced mod 1 per coordinate) and `n1 x n2 x n3` modes, row-major, each axis in numpy fftfreq order (k1 pairs
        /// with x, k2 with y, k3 with z), to the relative accuracy `eps`.  Immutable after `new`, like the reference's planners.
        pub struct $nufft {
            pub(crate) h: *mut Opaque,
            pub(crate) n: (usize, usize, usize),
            pub(crate) m: usize,
        }
        // SAFETY: the handle is immutable after creation; a call works in the caller's workspace (device calls) or in
        // a device buffer of its own (host-slice calls)
        unsafe impl Send for $nufft {}
        unsafe impl Sync for $nufft {}
        impl $nufft {
            /// Panics with "invalid argument" unless n1, n2, n3 >= 1, the fine grid g1 g2 g3 <= 2^28, 1 <= x.len() == y.len() == z.len() <= 2^30,
            /// every coordinate is finite and eps lies in [1e-14, 1e-1] (f64) or [1e-6, 1e-1] (f32)
            pub fn new(n_modes: (usize, usize, usize), x: &[f64], y: &[f64], z: &[f64], eps: f64) -> Self {
                assert_eq!(x.len(), y.len());
                assert_eq!(x.len(), z.len());
                let mut h = std::ptr::null_mut();
                ffi::check(unsafe { ffi::$new(n_modes.0, n_modes.1, n_modes.2, x.as_ptr(), y.as_ptr(), z.as_ptr(), x.len(), eps, &mut h) });
                Self { h, n: n_modes, m: x.len() }
            }
            /// The planner for `m_points` points in DEVICE memory (`d_x`, `d_y`, `d_z`: doubles in turns), sorted on the device into the very
            /// tables `new` builds on the host, ordered after the earlier work of `stream`; blocks until the planner is built.
            /// Panics with "invalid argument" for the sizes `new` refuses, a null pointer, a stream that is capturing or a point
            /// that is not finite.
            ///
            /// # Safety
            /// the pointers must be valid device memory of `m_points` doubles and `stream` a HIP stream or null
            pub unsafe fn from_device(n_modes: (usize, usize, usize), d_x: *const f64, d_y: *const f64, d_z: *const f64, m_points: usize,
                                      eps: f64, stream: *mut c_void) -> Self {
                let mut h = std::ptr::null_mut();
                ffi::check(ffi::$new_dev(n_modes.0, n_modes.1, n_modes.2, d_x, d_y, d_z, m_points, eps, stream, &mut h));
                Self { h, n: n_modes, m: m_points }
            }
            /// New points for this planner, the same number of them (another `m_points` panics with "planner size"), from device
            /// memory: the tables are rewritten in place, so a HIP graph captured through the planner stays valid and, replayed,
            /// transforms at the new points.  Ordered after the earlier work of `stream` ONLY -- work on other streams that uses
            /// the planner must have finished -- and blocks until done.  A rejected point set leaves the planner as it was.
            ///
            /// # Safety
            /// as `from_device`
            pub unsafe fn set_points_dev(&mut self, d_x: *const f64, d_y: *const f64, d_z: *const f64, m_points: usize,
                                         stream: *mut c_void) {
                ffi::check(ffi::$set_points(self.h, d_x, d_y, d_z, m_points, stream));
            }
            pub fn num_modes(&self) -> (usize, usize, usize) {
                self.n
            }
            pub fn num_points(&self) -> usize {
                self.m
            }
            /// the fine grid G = g1 g2 g3
            pub fn grid_len(&self) -> usize {
                unsafe { ffi::$grid_len(self.h) }
            }
            /// (g1, g2, g3): per axis the smallest power of two >= max(2 n, 2 width, 8)
            pub fn grid_shape(&self) -> (usize, usize, usize) {
                unsafe { (ffi::$grid_dim(self.h, 0), ffi::$grid_dim(self.h, 1), ffi::$grid_dim(self.h, 2)) }
            }
            /// the width of the spreading kernel in grid cells
            pub fn width(&self) -> usize {
                unsafe { ffi::$width(self.h) as usize }
            }
            /// elements of the workspace a device call of `batch` transforms works in: 4 G batch
            pub fn workspace_len(&self, batch: usize) -> usize {
                unsafe { ffi::$ws_len(self.h, batch) }
            }
        }
        impl Drop for $nufft {
            fn drop(&mut self) {
                unsafe { ffi::$free(self.h) }
            }
        }
    };
}
impl_planner_nufft3d!(PlannerNufft3d64, phast_planner_nufft3d64_new, phast_planner_nufft3d64_new_dev,
                      phast_planner_nufft3d64_set_points_dev, phast_planner_nufft3d64_free, phast_planner_nufft3d64_grid_len,
                      phast_planner_nufft3d64_grid_dim, phast_planner_nufft3d64_width,
                      phast_planner_nufft3d64_workspace_len);
impl_planner_nufft3d!(PlannerNufft3d32, phast_planner_nufft3d32_new, phast_planner_nufft3d32_new_dev,
                      phast_planner_nufft3d32_set_points_dev, phast_planner_nufft3d32_free, phast_planner_nufft3d32_grid_len,
                      phast_planner_nufft3d32_grid_dim, phast_planner_nufft3d32_width,
                      phast_planner_nufft3d32_workspace_len);

macro_rules! impl_planner_nufft_t3 {
    ($nufft:ident, $new:ident, $free:ident, $grid_len:ident, $width:ident, $ws_len:ident) => {
        /// An extension beyond PhastFT 0.3.0: the non-uniform FFT of type 3 of the sources `x` (any finite values, in a unit U)
        /// at the target frequencies `s` (any finite values, in 1 / U; `s[k] * x[j]` in turns), to the relative accuracy `eps`.
        /// Immutable after `new`, like the reference's planners.
        #[allow(non_camel_case_types)]
        pub struct $nufft {
            pub(crate) h: *mut Opaque,
            pub(crate) m: usize,
            pub(crate) k: usize,
        }
        // SAFETY: the handle is immutable after creation; a call works in the caller's workspace (device calls) or in
        // device buffers of its own (host-slice calls)
        unsafe impl Send for $nufft {}
        unsafe impl Sync for $nufft {}
        impl $nufft {
            /// Panics with "invalid argument" unless 1 <= x.len(), s.len() <= 2^30, every x and s is finite, eps lies in
            /// [1e-14, 1e-1] (f64) or [1e-6, 1e-1] (f32) and the fine grid is at most 2^28 points
            pub fn new(x: &[f64], s: &[f64], eps: f64) -> Self {
                let mut h = std::ptr::null_mut();
                ffi::check(unsafe { ffi::$new(x.as_ptr(), x.len(), s.as_ptr(), s.len(), eps, &mut h) });
                Self { h, m: x.len(), k: s.len() }
            }
            pub fn num_points(&self) -> usize {
                self.m
            }
            pub fn num_targets(&self) -> usize {
                self.k
            }
            /// the fine grid n_f: the smallest power of two >= max(8 S X + width, 2 width, 8), X and S the half-widths
            pub fn grid_len(&self) -> usize {
                unsafe { ffi::$grid_len(self.h) }
            }
            /// the width of the spreading kernel in grid cells
            pub fn width(&self) -> usize {
                unsafe { ffi::$width(self.h) as usize }
            }
            /// elements of the workspace a device call of `batch` transforms works in: 4 n_f batch
            pub fn workspace_len(&self, batch: usize) -> usize {
                unsafe { ffi::$ws_len(self.h, batch) }
            }
        }
        impl Drop for $nufft {
            fn drop(&mut self) {
                unsafe { ffi::$free(self.h) }
            }
        }
    };
}
impl_planner_nufft_t3!(PlannerNufftT3_64, phast_planner_nufft_t3_64_new, phast_planner_nufft_t3_64_free,
                       phast_planner_nufft_t3_64_grid_len, phast_planner_nufft_t3_64_width, phast_planner_nufft_t3_64_workspace_len);
impl_planner_nufft_t3!(PlannerNufftT3_32, phast_planner_nufft_t3_32_new, phast_planner_nufft_t3_32_free,
                       phast_planner_nufft_t3_32_grid_len, phast_planner_nufft_t3_32_width, phast_planner_nufft_t3_32_workspace_len);

macro_rules! impl_planner_nd {
    ($nd:ident, $new:ident, $free:ident, $ws_len:ident, $what:literal) => {
        #[doc = concat!("An extension beyond PhastFT 0.3.0, whose planners transform one axis: ", $what, " over every axis of a ",
                        "row-major array of rank 1 ..= 8 (each axis 1 ..= 2^29, at most 2^30 points; each axis runs the ",
                        "any-length path of its length, rotated to the contiguous end by a batched transpose).  Immutable ",
                        "after `new`, like the reference's planners.")]
        pub struct $nd {
            pub(crate) h: *mut Opaque,
            pub(crate) shape: Vec<usize>,
        }
        // SAFETY: the handle is immutable after creation; a call works in the caller's workspace (device calls) or in a
        // device buffer of its own (host-slice calls)
        unsafe impl Send for $nd {}
        unsafe impl Sync for $nd {}
        impl $nd {
            /// panics with "invalid argument" for rank 0 or > 8, an axis 0 or > 2^29, more than 2^30 points
            pub fn new(shape: &[usize]) -> Self {
                let mut h = std::ptr::null_mut();
                ffi::check(unsafe { ffi::$new(shape.as_ptr(), shape.len(), &mut h) });
                Self { h, shape: shape.to_vec() }
            }
            pub fn shape(&self) -> &[usize] {
                &self.shape
            }
            /// elements of the workspace a device call of `batch` arrays works in at full speed; `workspace_len(1)` serves
            /// any batch, in chunks
            pub fn workspace_len(&self, batch: usize) -> usize {
                unsafe { ffi::$ws_len(self.h, batch) }
            }
        }
        impl Drop for $nd {
            fn drop(&mut self) {
                unsafe { ffi::$free(self.h) }
            }
        }
    };
}
impl_planner_nd!(PlannerNd64, phast_planner_nd64_new, phast_planner_nd64_free, phast_planner_nd64_workspace_len,
                 "f64 complex transforms (numpy fftn / ifftn)");
impl_planner_nd!(PlannerNd32, phast_planner_nd32_new, phast_planner_nd32_free, phast_planner_nd32_workspace_len,
                 "f32 complex transforms (numpy fftn / ifftn)");
impl_planner_nd!(PlannerR2cNd64, phast_planner_r2c_nd64_new, phast_planner_r2c_nd64_free,
                 phast_planner_r2c_nd64_workspace_len, "f64 real transforms (numpy rfftn / irfftn)");
impl_planner_nd!(PlannerR2cNd32, phast_planner_r2c_nd32_new, phast_planner_r2c_nd32_free,
                 phast_planner_r2c_nd32_workspace_len, "f32 real transforms (numpy rfftn / irfftn)");
