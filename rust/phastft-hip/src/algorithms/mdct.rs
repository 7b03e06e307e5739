//! The modified discrete cosine transform and its inverse -- an extension beyond PhastFT 0.3.0, which has neither (nor have
//! torch or scipy): `n` coefficients per frame of `2 n` windowed samples, hop `n`, unscaled forward; the inverse carries 2 / n
//! and overlap-adds without an envelope, so a window with `tdac_defect() == 0` returns the signal.  The coefficients are one
//! dense array of `frames * n` values, frame-major.

use crate::ffi;
use crate::planner::{PlannerMdct32, PlannerMdct64};
use std::ffi::c_void;

macro_rules! impl_mdct {
    ($t:ty, $planner:ident, $fwd:ident, $inv:ident, $fwd_dev:ident, $inv_dev:ident, $c_fwd:ident, $c_inv:ident, $c_fwd_dev:ident,
     $c_inv_dev:ident) => {
        /// one host signal of `planner.signal_len()` samples into `planner.frames() * planner.n()` coefficients; blocking
        pub fn $fwd(signal: &[$t], coefs: &mut [$t], planner: &$planner) {
            ffi::check(unsafe { ffi::$c_fwd(signal.as_ptr(), signal.len(), coefs.as_mut_ptr(), coefs.len(), planner.h) });
        }
        /// the inverse of the above
        pub fn $inv(coefs: &[$t], signal: &mut [$t], planner: &$planner) {
            ffi::check(unsafe { ffi::$c_inv(coefs.as_ptr(), coefs.len(), signal.as_mut_ptr(), signal.len(), planner.h) });
        }
        /// Device-resident, batched, asynchronous on `stream`: signal b at `b * sig_dist`, its coefficients at
        /// `b * frames * n`; `d_work` is a device workspace of `work_len >= planner.workspace_min(false)` elements
        pub unsafe fn $fwd_dev(d_signal: *const $t, d_coefs: *mut $t, batch: usize, sig_dist: usize, planner: &$planner,
                               d_work: *mut $t, work_len: usize, stream: *mut c_void) {
            ffi::check(ffi::$c_fwd_dev(d_signal, d_coefs, planner.signal_len, batch, sig_dist, planner.h, d_work, work_len, stream));
        }
        /// the inverse of the above; `work_len >= planner.workspace_min(true)`
        pub unsafe fn $inv_dev(d_coefs: *const $t, d_signal: *mut $t, batch: usize, sig_dist: usize, planner: &$planner,
                               d_work: *mut $t, work_len: usize, stream: *mut c_void) {
            ffi::check(ffi::$c_inv_dev(d_coefs, d_signal, planner.signal_len, batch, sig_dist, planner.h, d_work, work_len, stream));
        }
    };
}
impl_mdct!(f64, PlannerMdct64, mdct_f64_with_planner, imdct_f64_with_planner, mdct_f64_dev, imdct_f64_dev,
           phast_mdct_f64_with_planner, phast_imdct_f64_with_planner, phast_mdct_f64_dev, phast_imdct_f64_dev);
impl_mdct!(f32, PlannerMdct32, mdct_f32_with_planner, imdct_f32_with_planner, mdct_f32_dev, imdct_f32_dev,
           phast_mdct_f32_with_planner, phast_imdct_f32_with_planner, phast_mdct_f32_dev, phast_imdct_f32_dev);
