//! Sample-rate conversion of real signals -- an extension beyond PhastFT 0.3.0, which has none.  Two planners: the polyphase
//! FIR of scipy.signal.upfirdn (`PlannerUpfirdn64/32`: zero-stuff by `up`, filter, keep every `down`-th sample, as one direct
//! kernel that needs no workspace) and the Fourier method of scipy.signal.resample (`PlannerResample64/32`: one R2C of the
//! signal length and one C2R of `num` around one sweep).  A call takes signals of `planner.signal_len()` samples and yields
//! `planner.out_len()` samples each.

use crate::ffi;
use crate::planner::{PlannerResample32, PlannerResample64, PlannerUpfirdn32, PlannerUpfirdn64};
use std::ffi::c_void;

macro_rules! impl_rate {
    ($t:ty, $planner:ident, $host:ident, $dev:ident, $c_host:ident, $c_dev:ident) => {
        /// one host signal of `planner.signal_len()` samples into `planner.out_len()` output samples; blocking
        pub fn $host(signal: &[$t], output: &mut [$t], planner: &$planner) {
            ffi::check(unsafe { ffi::$c_host(signal.as_ptr(), signal.len(), output.as_mut_ptr(), output.len(), planner.h) });
        }
        /// Device-resident, batched, asynchronous on `stream`: signal b at `b * sig_dist`, its output at `b * out_dist`;
        /// `d_work` is a device workspace of `work_len >= planner.workspace_min()` elements (the polyphase planner needs
        /// none: null and 0 are fine)
        pub unsafe fn $dev(d_signal: *const $t, d_out: *mut $t, batch: usize, sig_dist: usize, out_dist: usize, planner: &$planner,
                           d_work: *mut $t, work_len: usize, stream: *mut c_void) {
            ffi::check(ffi::$c_dev(d_signal, d_out, planner.signal_len, batch, sig_dist, out_dist, planner.h, d_work, work_len, stream));
        }
    };
}
impl_rate!(f64, PlannerUpfirdn64, upfirdn_f64_with_planner, upfirdn_f64_dev, phast_upfirdn_f64_with_planner, phast_upfirdn_f64_dev);
impl_rate!(f32, PlannerUpfirdn32, upfirdn_f32_with_planner, upfirdn_f32_dev, phast_upfirdn_f32_with_planner, phast_upfirdn_f32_dev);
impl_rate!(f64, PlannerResample64, resample_f64_with_planner, resample_f64_dev, phast_resample_f64_with_planner, phast_resample_f64_dev);
impl_rate!(f32, PlannerResample32, resample_f32_with_planner, resample_f32_dev, phast_resample_f32_with_planner, phast_resample_f32_dev);
