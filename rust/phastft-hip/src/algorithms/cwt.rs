//! The continuous wavelet transform and the analytic signal -- an extension beyond PhastFT 0.3.0, which has none.
//! `PlannerCwt64/32` holds the scales, the wavelet family (Torrence & Compo 1998: Morlet, Paul, DOG; `Step`: the analytic-signal
//! filter of scipy.signal.hilbert) and the norm: one forward transform per signal, one bank kernel that evaluates the filters
//! in registers, one inverse transform per scale.  A call takes `planner.signal_len()` points per signal (one plane for a real
//! planner, two for a complex one) and yields `planner.num_scales() * planner.signal_len()` points per signal in each of the two
//! output planes, scale-major.

use crate::ffi;
use crate::planner::{PlannerCwt32, PlannerCwt64};
use std::ffi::c_void;

macro_rules! impl_cwt {
    ($t:ty, $planner:ident, $host:ident, $dev:ident, $c_host:ident, $c_dev:ident) => {
        /// one signal from a host slice of `planner.signal_len()` points (`x_im`: its imaginary plane for a complex planner,
        /// `None` for a real one) into `out_re` / `out_im` of `planner.num_scales() * planner.signal_len()` points; blocking
        pub fn $host(x: &[$t], x_im: Option<&[$t]>, out_re: &mut [$t], out_im: &mut [$t], planner: &$planner) {
            if let Some(im) = &x_im {
                assert_eq!(im.len(), x.len(), "the signal's planes differ in length");
            }
            assert_eq!(out_re.len(), out_im.len(), "the output planes differ in length");
            let im = x_im.map_or(std::ptr::null(), |s| s.as_ptr());
            ffi::check(unsafe { ffi::$c_host(x.as_ptr(), im, x.len(), out_re.as_mut_ptr(), out_im.as_mut_ptr(), out_re.len(), planner.h) });
        }
        /// Device-resident, batched, asynchronous on `stream`: signal b at `b * sig_dist` of `d_x_re` (and `d_x_im`: null for a
        /// real planner), row (b, j) at `b * out_dist + j * signal_len` of the output planes; `d_work` is a device workspace of
        /// `work_len >= planner.workspace_min()` elements
        pub unsafe fn $dev(d_x_re: *const $t, d_x_im: *const $t, d_out_re: *mut $t, d_out_im: *mut $t, batch: usize, sig_dist: usize,
                           out_dist: usize, planner: &$planner, d_work: *mut $t, work_len: usize, stream: *mut c_void) {
            ffi::check(ffi::$c_dev(d_x_re, d_x_im, d_out_re, d_out_im, planner.signal_len, batch, sig_dist, out_dist, planner.h, d_work,
                                   work_len, stream));
        }
    };
}
impl_cwt!(f64, PlannerCwt64, cwt_64_with_planner, cwt_64_dev, phast_cwt_64_with_planner, phast_cwt_64_dev);
impl_cwt!(f32, PlannerCwt32, cwt_32_with_planner, cwt_32_dev, phast_cwt_32_with_planner, phast_cwt_32_dev);
