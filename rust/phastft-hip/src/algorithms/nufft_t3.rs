//! The non-uniform FFT of type 3 in one dimension -- an extension beyond PhastFT 0.3.0, which transforms samples on a grid only.
//! The planner holds the sources x and the target frequencies s (`s[k] * x[j]` in turns); a transform takes
//! `planner.num_points()` values to `planner.num_targets()` values.  `Direction::Forward` is the - sign, `Reverse` the + sign,
//! neither scales; `c_im` = None is real data.

use crate::ffi;
use crate::planner::{Direction, PlannerNufftT3_32, PlannerNufftT3_64};
use std::ffi::c_void;
use std::os::raw::c_int;

macro_rules! impl_nufft_t3 {
    ($t:ty, $planner:ident, $shot:ident, $host:ident, $dev:ident, $c_shot:ident, $c_host:ident, $c_dev:ident) => {
        /// one host vector at the sources `x` to the targets `s` through a planner of its own; blocking
        pub fn $shot(x: &[f64], s: &[f64], c_re: &[$t], c_im: Option<&[$t]>, out_re: &mut [$t], out_im: &mut [$t], eps: f64,
                     direction: Direction) {
            assert_eq!(out_re.len(), out_im.len());
            if let Some(im) = c_im {
                assert_eq!(c_re.len(), im.len());
            }
            assert_eq!(x.len(), c_re.len());
            assert_eq!(s.len(), out_re.len());
            let im = c_im.map_or(std::ptr::null(), |v| v.as_ptr());
            ffi::check(unsafe {
                ffi::$c_shot(x.as_ptr(), x.len(), s.as_ptr(), s.len(), c_re.as_ptr(), im, out_re.as_mut_ptr(), out_im.as_mut_ptr(), eps,
                             direction as c_int)
            });
        }
        /// one host vector through `planner`; blocking
        pub fn $host(c_re: &[$t], c_im: Option<&[$t]>, out_re: &mut [$t], out_im: &mut [$t], direction: Direction,
                     planner: &$planner) {
            assert_eq!(out_re.len(), out_im.len());
            if let Some(im) = c_im {
                assert_eq!(c_re.len(), im.len());
            }
            let im = c_im.map_or(std::ptr::null(), |v| v.as_ptr());
            ffi::check(unsafe {
                ffi::$c_host(c_re.as_ptr(), im, c_re.len(), out_re.as_mut_ptr(), out_im.as_mut_ptr(), out_re.len(),
                             direction as c_int, planner.h)
            });
        }
        /// Device-resident, batched, asynchronous on `stream`: input b at `b * in_dist` (`d_c_im` may be null: real data), its
        /// output at `b * out_dist`; `d_work` is a device workspace of `work_len >= planner.workspace_len(1)` elements.  The
        /// outputs must not overlap the inputs, the workspace or each other.
        pub unsafe fn $dev(d_c_re: *const $t, d_c_im: *const $t, in_dist: usize, d_out_re: *mut $t, d_out_im: *mut $t,
                           out_dist: usize, batch: usize, direction: Direction, planner: &$planner, d_work: *mut $t,
                           work_len: usize, stream: *mut c_void) {
            ffi::check(ffi::$c_dev(d_c_re, d_c_im, in_dist, d_out_re, d_out_im, out_dist, batch, direction as c_int, planner.h,
                                   d_work, work_len, stream));
        }
    };
}
impl_nufft_t3!(f64, PlannerNufftT3_64, nufft3_64, nufft3_64_with_planner, nufft3_64_dev, phast_nufft3_64, phast_nufft3_64_with_planner,
               phast_nufft3_64_dev);
impl_nufft_t3!(f32, PlannerNufftT3_32, nufft3_32, nufft3_32_with_planner, nufft3_32_dev, phast_nufft3_32, phast_nufft3_32_with_planner,
               phast_nufft3_32_dev);
