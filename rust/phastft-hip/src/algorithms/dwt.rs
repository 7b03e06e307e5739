//! The discrete wavelet transform of real signals and its inverse -- an extension beyond PhastFT 0.3.0, which has none:
//! pywt.wavedec / waverec (`PlannerDwt64/32`) with the extension modes `DwtMode`, as one direct kernel launch per level.  A
//! call takes signals of `planner.signal_len()` samples and yields packed rows [cA_J | cD_J | .. | cD_1] of
//! `planner.coeff_len()` coefficients each, or the other way round.

use crate::ffi;
use crate::planner::{PlannerDwt32, PlannerDwt64};
use std::ffi::c_void;

macro_rules! impl_dwt {
    ($t:ty, $planner:ident, $dec_host:ident, $rec_host:ident, $dec_dev:ident, $rec_dev:ident, $c_dec_host:ident, $c_rec_host:ident,
     $c_dec_dev:ident, $c_rec_dev:ident) => {
        /// one host signal of `planner.signal_len()` samples into its packed row of `planner.coeff_len()`; blocking
        pub fn $dec_host(signal: &[$t], coeffs: &mut [$t], planner: &$planner) {
            ffi::check(unsafe { ffi::$c_dec_host(signal.as_ptr(), signal.len(), coeffs.as_mut_ptr(), coeffs.len(), planner.h) });
        }
        /// one host packed row back into a signal of `planner.signal_len()` samples; blocking
        pub fn $rec_host(coeffs: &[$t], signal: &mut [$t], planner: &$planner) {
            ffi::check(unsafe { ffi::$c_rec_host(coeffs.as_ptr(), coeffs.len(), signal.as_mut_ptr(), signal.len(), planner.h) });
        }
        /// Device-resident, batched, asynchronous on `stream`: signal b at `b * sig_dist`, its packed row at `b * coeff_dist`;
        /// `d_work` is a device workspace of `work_len >= planner.workspace_min()` elements (one level needs none: null and 0
        /// are fine).  The signals are not written.
        pub unsafe fn $dec_dev(d_signal: *const $t, d_coeffs: *mut $t, batch: usize, sig_dist: usize, coeff_dist: usize, planner: &$planner,
                               d_work: *mut $t, work_len: usize, stream: *mut c_void) {
            ffi::check(ffi::$c_dec_dev(d_signal, d_coeffs, planner.signal_len, batch, sig_dist, coeff_dist, planner.h, d_work, work_len, stream));
        }
        /// The inverse of the call above: packed rows into signals.  The coefficients are not written.
        pub unsafe fn $rec_dev(d_coeffs: *const $t, d_signal: *mut $t, batch: usize, coeff_dist: usize, sig_dist: usize, planner: &$planner,
                               d_work: *mut $t, work_len: usize, stream: *mut c_void) {
            ffi::check(ffi::$c_rec_dev(d_coeffs, d_signal, planner.signal_len, batch, coeff_dist, sig_dist, planner.h, d_work, work_len, stream));
        }
    };
}
impl_dwt!(f64, PlannerDwt64, wavedec_f64_with_planner, waverec_f64_with_planner, wavedec_f64_dev, waverec_f64_dev,
          phast_wavedec_f64_with_planner, phast_waverec_f64_with_planner, phast_wavedec_f64_dev, phast_waverec_f64_dev);
impl_dwt!(f32, PlannerDwt32, wavedec_f32_with_planner, waverec_f32_with_planner, wavedec_f32_dev, waverec_f32_dev,
          phast_wavedec_f32_with_planner, phast_waverec_f32_with_planner, phast_wavedec_f32_dev, phast_waverec_f32_dev);
