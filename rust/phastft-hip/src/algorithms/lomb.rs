//! The generalised Lomb-Scargle periodogram of unevenly spaced samples -- an extension beyond PhastFT 0.3.0:
//! scipy.signal.lombscargle's definitions with the frequencies in cycles per unit of time.  `LombNorm::Power` and
//! `LombNorm::Normalize` give `planner.freqs()` real values per signal; `LombNorm::Amplitude` gives the complex amplitude in
//! two planes and needs `out_im`.  The mean and the sums over the points are carried in double for both types, and the mean is
//! taken off before the transform: an offset of the signal costs nothing.

use crate::ffi;
use crate::planner::{LombNorm, PlannerLomb32, PlannerLomb64};
use std::ffi::c_void;

macro_rules! impl_lomb {
    ($t:ty, $planner:ident, $shot:ident, $host:ident, $dev:ident, $c_shot:ident, $c_host:ident, $c_dev:ident) => {
        /// the periodogram of one host signal through a planner of the call's own; blocking.  `y` holds one value per time,
        /// `out_re` (and `out_im`, required for `Amplitude` only) one per frequency
        #[allow(clippy::too_many_arguments)]
        pub fn $shot(times: &[f64], freqs: &[f64], weights: Option<&[f64]>, floating_mean: bool, eps: f64, y: &[$t], out_re: &mut [$t],
                     out_im: Option<&mut [$t]>, normalize: LombNorm) {
            assert_eq!(y.len(), times.len(), "invalid argument");
            assert_eq!(out_re.len(), freqs.len(), "invalid argument");
            if let Some(w) = weights {
                assert_eq!(w.len(), times.len(), "invalid argument");
            }
            if let Some(im) = &out_im {
                assert_eq!(im.len(), freqs.len(), "invalid argument");
            }
            let w = weights.map_or(std::ptr::null(), |w| w.as_ptr());
            let im_p = out_im.map_or(std::ptr::null_mut(), |s| s.as_mut_ptr());
            ffi::check(unsafe {
                ffi::$c_shot(times.as_ptr(), times.len(), freqs.as_ptr(), freqs.len(), w, floating_mean as i32, eps, y.as_ptr(),
                             out_re.as_mut_ptr(), im_p, normalize as i32)
            });
        }
        /// the periodogram of one host signal of `planner.points()` values into `planner.freqs()` values; blocking
        pub fn $host(y: &[$t], out_re: &mut [$t], out_im: Option<&mut [$t]>, normalize: LombNorm, planner: &$planner) {
            let (im_p, im_n) = out_im.map_or((std::ptr::null_mut(), 0), |s| (s.as_mut_ptr(), s.len()));
            ffi::check(unsafe {
                ffi::$c_host(y.as_ptr(), y.len(), out_re.as_mut_ptr(), out_re.len(), im_p, im_n, normalize as i32, planner.h)
            });
        }
        /// Device-resident, batched, asynchronous on `stream`: signal b at `b * sig_dist`, its results at `b * out_dist`;
        /// `d_out_im` may be null unless `normalize` is `Amplitude`; `d_work` is a device workspace of
        /// `work_len >= planner.workspace_min()` elements
        #[allow(clippy::too_many_arguments)]
        pub unsafe fn $dev(d_y: *const $t, d_out_re: *mut $t, d_out_im: *mut $t, batch: usize, sig_dist: usize, out_dist: usize,
                           normalize: LombNorm, planner: &$planner, d_work: *mut $t, work_len: usize, stream: *mut c_void) {
            ffi::check(ffi::$c_dev(d_y, d_out_re, d_out_im, planner.points, batch, sig_dist, out_dist, normalize as i32, planner.h,
                                   d_work, work_len, stream));
        }
    };
}
impl_lomb!(f64, PlannerLomb64, lombscargle_f64, lombscargle_f64_with_planner, lombscargle_f64_dev, phast_lombscargle_f64,
           phast_lombscargle_f64_with_planner, phast_lombscargle_f64_dev);
impl_lomb!(f32, PlannerLomb32, lombscargle_f32, lombscargle_f32_with_planner, lombscargle_f32_dev, phast_lombscargle_f32,
           phast_lombscargle_f32_with_planner, phast_lombscargle_f32_dev);
