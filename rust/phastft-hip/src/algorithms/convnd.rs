//! Overlap-save convolution and correlation of real arrays of rank 1 .. 3 -- an extension beyond PhastFT 0.3.0, which has
//! neither: scipy.signal.convolve / correlate(x, h, mode, method = "direct") of N-d arrays.  The planner holds the filter; a
//! call takes row-major arrays of `planner.signal_len()` points and yields `planner.out_len()` points each, of
//! `planner.out_shape()`.

use crate::ffi;
use crate::planner::{PlannerConvNd32, PlannerConvNd64};
use std::ffi::c_void;

macro_rules! impl_convnd {
    ($t:ty, $planner:ident, $host:ident, $dev:ident, $c_host:ident, $c_dev:ident) => {
        /// one host array of `planner.signal_len()` points into `planner.out_len()` output points; blocking
        pub fn $host(signal: &[$t], output: &mut [$t], planner: &$planner) {
            ffi::check(unsafe { ffi::$c_host(signal.as_ptr(), signal.len(), output.as_mut_ptr(), output.len(), planner.h) });
        }
        /// Device-resident, batched, asynchronous on `stream`: array b at `b * sig_dist`, its output at `b * out_dist`;
        /// `d_work` is a device workspace of `work_len >= planner.workspace_min()` elements
        pub unsafe fn $dev(d_signal: *const $t, d_out: *mut $t, batch: usize, sig_dist: usize, out_dist: usize, planner: &$planner,
                           d_work: *mut $t, work_len: usize, stream: *mut c_void) {
            ffi::check(ffi::$c_dev(d_signal, d_out, planner.signal_len, batch, sig_dist, out_dist, planner.h, d_work, work_len, stream));
        }
    };
}
impl_convnd!(f64, PlannerConvNd64, convnd_f64_with_planner, convnd_f64_dev, phast_convnd_f64_with_planner, phast_convnd_f64_dev);
impl_convnd!(f32, PlannerConvNd32, convnd_f32_with_planner, convnd_f32_dev, phast_convnd_f32_with_planner, phast_convnd_f32_dev);
