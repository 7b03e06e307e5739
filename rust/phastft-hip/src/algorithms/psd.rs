//! Welch spectral estimation -- an extension beyond PhastFT 0.3.0: scipy.signal's welch, csd and spectrogram (one-sided,
//! `mode = "psd"`) of real signals.  With `average` the result is `planner.bins()` values per signal; without, the spectrogram,
//! `planner.segments() * planner.bins()` values, frame-major.  The cross spectrum is <conj(X) Y> in two planes.  Segment means
//! and the sums over frames are carried in double for both types.

use crate::ffi;
use crate::planner::{PlannerPsd32, PlannerPsd64};
use std::ffi::c_void;

macro_rules! impl_psd {
    ($t:ty, $planner:ident, $psd:ident, $csd:ident, $psd_dev:ident, $csd_dev:ident, $c_psd:ident, $c_csd:ident, $c_psd_dev:ident,
     $c_csd_dev:ident) => {
        /// the auto spectrum of one host signal of `planner.signal_len()` samples; blocking
        pub fn $psd(signal: &[$t], out: &mut [$t], average: bool, planner: &$planner) {
            ffi::check(unsafe { ffi::$c_psd(signal.as_ptr(), signal.len(), out.as_mut_ptr(), out.len(), average as i32, planner.h) });
        }
        /// the cross spectrum of one pair of host signals into two planes, and the two auto spectra where asked for; blocking
        #[allow(clippy::too_many_arguments)]
        pub fn $csd(x: &[$t], y: &[$t], out_re: &mut [$t], out_im: &mut [$t], pxx: Option<&mut [$t]>, pyy: Option<&mut [$t]>,
                    average: bool, planner: &$planner) {
            let (pxx_p, pxx_n) = pxx.map_or((std::ptr::null_mut(), 0), |s| (s.as_mut_ptr(), s.len()));
            let (pyy_p, pyy_n) = pyy.map_or((std::ptr::null_mut(), 0), |s| (s.as_mut_ptr(), s.len()));
            ffi::check(unsafe {
                ffi::$c_csd(x.as_ptr(), x.len(), y.as_ptr(), y.len(), out_re.as_mut_ptr(), out_re.len(), out_im.as_mut_ptr(),
                            out_im.len(), pxx_p, pxx_n, pyy_p, pyy_n, average as i32, planner.h)
            });
        }
        /// Device-resident, batched, asynchronous on `stream`: signal b at `b * sig_dist`, its spectrum at `b * bins` (or at
        /// `b * segments * bins`); `d_work` is a device workspace of `work_len >= planner.workspace_min(false)` elements
        #[allow(clippy::too_many_arguments)]
        pub unsafe fn $psd_dev(d_x: *const $t, d_out: *mut $t, batch: usize, sig_dist: usize, average: bool, planner: &$planner,
                               d_work: *mut $t, work_len: usize, stream: *mut c_void) {
            ffi::check(ffi::$c_psd_dev(d_x, d_out, planner.signal_len, batch, sig_dist, average as i32, planner.h, d_work, work_len,
                                       stream));
        }
        /// the cross spectrum of the above; `d_pxx` and `d_pyy` may be null; `work_len >= planner.workspace_min(true)`
        #[allow(clippy::too_many_arguments)]
        pub unsafe fn $csd_dev(d_x: *const $t, d_y: *const $t, d_out_re: *mut $t, d_out_im: *mut $t, d_pxx: *mut $t, d_pyy: *mut $t,
                               batch: usize, sig_dist: usize, average: bool, planner: &$planner, d_work: *mut $t, work_len: usize,
                               stream: *mut c_void) {
            ffi::check(ffi::$c_csd_dev(d_x, d_y, d_out_re, d_out_im, d_pxx, d_pyy, planner.signal_len, batch, sig_dist, average as i32,
                                       planner.h, d_work, work_len, stream));
        }
    };
}
impl_psd!(f64, PlannerPsd64, psd_f64_with_planner, csd_f64_with_planner, psd_f64_dev, csd_f64_dev, phast_psd_f64_with_planner,
          phast_csd_f64_with_planner, phast_psd_f64_dev, phast_csd_f64_dev);
impl_psd!(f32, PlannerPsd32, psd_f32_with_planner, csd_f32_with_planner, psd_f32_dev, csd_f32_dev, phast_psd_f32_with_planner,
          phast_csd_f32_with_planner, phast_psd_f32_dev, phast_csd_f32_dev);
