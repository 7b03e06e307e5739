//! Overlap-save FIR convolution and correlation of real signals -- an extension beyond PhastFT 0.3.0, which has neither:
//! scipy.signal.convolve / correlate(x, h, mode, method = "direct").  The planner holds the filter; a call takes signals of
//! `planner.signal_len()` samples and yields `planner.out_len()` samples each.

use crate::ffi;
use crate::planner::{PlannerConv32, PlannerConv64};
use std::ffi::c_void;

macro_rules! impl_conv {
    ($t:ty, $planner:ident, $host:ident, $dev:ident, $c_host:ident, $c_dev:ident) => {
        /// one host signal of `planner.signal_len()` samples into `planner.out_len()` output samples; blocking
        pub fn $host(signal: &[$t], output: &mut [$t], planner: &$planner) {
            ffi::check(unsafe { ffi::$c_host(signal.as_ptr(), signal.len(), output.as_mut_ptr(), output.len(), planner.h) });
        }
        /// Device-resident, batched, asynchronous on `stream`: signal b at `b * sig_dist`, its output at `b * out_dist`;
        /// `d_work` is a device workspace of `work_len >= planner.workspace_min()` elements
        pub unsafe fn $dev(d_signal: *const $t, d_out: *mut $t, batch: usize, sig_dist: usize, out_dist: usize, planner: &$planner,
                           d_work: *mut $t, work_len: usize, stream: *mut c_void) {
            ffi::check(ffi::$c_dev(d_signal, d_out, planner.signal_len, batch, sig_dist, out_dist, planner.h, d_work, work_len, stream));
        }
    };
}
impl_conv!(f64, PlannerConv64, conv_f64_with_planner, conv_f64_dev, phast_conv_f64_with_planner, phast_conv_f64_dev);
impl_conv!(f32, PlannerConv32, conv_f32_with_planner, conv_f32_dev, phast_conv_f32_with_planner, phast_conv_f32_dev);
