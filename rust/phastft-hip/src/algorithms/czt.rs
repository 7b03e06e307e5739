//! The chirp-Z transform on the unit circle and the zoom FFT -- an extension beyond PhastFT 0.3.0, which gives whole spectra
//! only: scipy.signal.czt(x, m, w, a) with w = exp(-2 pi i step), a = exp(2 pi i start), the two parameters in turns.  A call
//! takes `planner.input_len()` points and yields `planner.output_len()` bins; `in_im` = None is a real signal.

use crate::ffi;
use crate::planner::{PlannerCzt32, PlannerCzt64};
use std::ffi::c_void;

macro_rules! impl_czt {
    ($t:ty, $planner:ident, $shot:ident, $host:ident, $dev:ident, $c_shot:ident, $c_host:ident, $c_dev:ident) => {
        /// one host signal into `out_re.len()` bins through a planner of its own; blocking
        pub fn $shot(in_re: &[$t], in_im: Option<&[$t]>, out_re: &mut [$t], out_im: &mut [$t], step: f64, start: f64) {
            assert_eq!(out_re.len(), out_im.len());
            if let Some(im) = in_im {
                assert_eq!(in_re.len(), im.len());
            }
            let im = in_im.map_or(std::ptr::null(), |s| s.as_ptr());
            ffi::check(unsafe {
                ffi::$c_shot(in_re.as_ptr(), im, in_re.len(), out_re.as_mut_ptr(), out_im.as_mut_ptr(), out_re.len(), step, start)
            });
        }
        /// one host signal of `planner.input_len()` points into `planner.output_len()` bins; blocking
        pub fn $host(in_re: &[$t], in_im: Option<&[$t]>, out_re: &mut [$t], out_im: &mut [$t], planner: &$planner) {
            assert_eq!(out_re.len(), out_im.len());
            if let Some(im) = in_im {
                assert_eq!(in_re.len(), im.len());
            }
            let im = in_im.map_or(std::ptr::null(), |s| s.as_ptr());
            ffi::check(unsafe {
                ffi::$c_host(in_re.as_ptr(), im, in_re.len(), out_re.as_mut_ptr(), out_im.as_mut_ptr(), out_re.len(), planner.h)
            });
        }
        /// Device-resident, batched, asynchronous on `stream`: input b at `b * in_dist` (`d_in_im` may be null: real signals),
        /// its bins at `b * out_dist`; `d_work` is a device workspace of `work_len >= planner.workspace_len(1)` elements.  The
        /// output must not overlap the input or the workspace.
        pub unsafe fn $dev(d_in_re: *const $t, d_in_im: *const $t, in_dist: usize, d_out_re: *mut $t, d_out_im: *mut $t,
                           out_dist: usize, batch: usize, planner: &$planner, d_work: *mut $t, work_len: usize, stream: *mut c_void) {
            ffi::check(ffi::$c_dev(d_in_re, d_in_im, in_dist, d_out_re, d_out_im, out_dist, batch, planner.h, d_work, work_len, stream));
        }
    };
}
impl_czt!(f64, PlannerCzt64, czt_64, czt_64_with_planner, czt_64_dev, phast_czt_64, phast_czt_64_with_planner, phast_czt_64_dev);
impl_czt!(f32, PlannerCzt32, czt_32, czt_32_with_planner, czt_32_dev, phast_czt_32, phast_czt_32_with_planner, phast_czt_32_dev);
