//! Non-uniform FFTs of types 1 and 2 in three dimensions -- an extension beyond PhastFT 0.3.0, which transforms samples on a grid
//! only.  The planner holds the points `(x, y, z)` (turns, reduced mod 1 per coordinate) and the mode counts `(n1, n2, n3)`; the
//! modes are row-major (index `(m1 * n2 + m2) * n3 + m3`), each axis in numpy fftfreq order.  Type 1 takes `planner.num_points()` values to
//! `n1 * n2 * n3` modes, type 2 the reverse.  `Direction::Forward` is the - sign, `Reverse` the + sign, neither scales; `in_im` = None
//! is real data.

use crate::ffi;
use crate::planner::{Direction, PlannerNufft3d32, PlannerNufft3d64};
use std::ffi::c_void;
use std::os::raw::c_int;

macro_rules! impl_nufft3d {
    ($t:ty, $planner:ident, $ty:expr, $shot:ident, $host:ident, $dev:ident, $c_shot:ident, $c_host:ident, $c_dev:ident) => {
        /// one host vector at the points `(x, y, z)` and `n_modes = (n1, n2, n3)` through a planner of its own; blocking
        pub fn $shot(x: &[f64], y: &[f64], z: &[f64], in_re: &[$t], in_im: Option<&[$t]>, out_re: &mut [$t], out_im: &mut [$t],
                     n_modes: (usize, usize, usize), eps: f64, direction: Direction) {
            assert_eq!(out_re.len(), out_im.len());
            assert_eq!(x.len(), y.len());
            assert_eq!(x.len(), z.len());
            if let Some(im) = in_im {
                assert_eq!(in_re.len(), im.len());
            }
            let (modes, m_points) = if $ty == 1 { (out_re.len(), in_re.len()) } else { (in_re.len(), out_re.len()) };
            assert_eq!(x.len(), m_points);
            assert_eq!(n_modes.0.checked_mul(n_modes.1).and_then(|v| v.checked_mul(n_modes.2)), Some(modes));
            let im = in_im.map_or(std::ptr::null(), |s| s.as_ptr());
            ffi::check(unsafe {
                ffi::$c_shot(x.as_ptr(), y.as_ptr(), z.as_ptr(), x.len(), in_re.as_ptr(), im, out_re.as_mut_ptr(), out_im.as_mut_ptr(),
                             n_modes.0, n_modes.1, n_modes.2, eps, direction as c_int)
            });
        }
        /// one host vector through `planner`; blocking
        pub fn $host(in_re: &[$t], in_im: Option<&[$t]>, out_re: &mut [$t], out_im: &mut [$t], direction: Direction,
                     planner: &$planner) {
            assert_eq!(out_re.len(), out_im.len());
            if let Some(im) = in_im {
                assert_eq!(in_re.len(), im.len());
            }
            let im = in_im.map_or(std::ptr::null(), |s| s.as_ptr());
            ffi::check(unsafe {
                ffi::$c_host(in_re.as_ptr(), im, in_re.len(), out_re.as_mut_ptr(), out_im.as_mut_ptr(), out_re.len(),
                             direction as c_int, planner.h)
            });
        }
        /// Device-resident, batched, asynchronous on `stream`: input b at `b * in_dist` (`d_in_im` may be null: real data), its
        /// output at `b * out_dist`; `d_work` is a device workspace of `work_len >= planner.workspace_len(1)` elements.  The
        /// outputs must not overlap the inputs, the workspace or each other.
        pub unsafe fn $dev(d_in_re: *const $t, d_in_im: *const $t, in_dist: usize, d_out_re: *mut $t, d_out_im: *mut $t,
                           out_dist: usize, batch: usize, direction: Direction, planner: &$planner, d_work: *mut $t,
                           work_len: usize, stream: *mut c_void) {
            ffi::check(ffi::$c_dev(d_in_re, d_in_im, in_dist, d_out_re, d_out_im, out_dist, batch, direction as c_int, planner.h,
                                   d_work, work_len, stream));
        }
    };
}
impl_nufft3d!(f64, PlannerNufft3d64, 1, nufft3d1_64, nufft3d1_64_with_planner, nufft3d1_64_dev, phast_nufft3d1_64,
              phast_nufft3d1_64_with_planner, phast_nufft3d1_64_dev);
impl_nufft3d!(f32, PlannerNufft3d32, 1, nufft3d1_32, nufft3d1_32_with_planner, nufft3d1_32_dev, phast_nufft3d1_32,
              phast_nufft3d1_32_with_planner, phast_nufft3d1_32_dev);
impl_nufft3d!(f64, PlannerNufft3d64, 2, nufft3d2_64, nufft3d2_64_with_planner, nufft3d2_64_dev, phast_nufft3d2_64,
              phast_nufft3d2_64_with_planner, phast_nufft3d2_64_dev);
impl_nufft3d!(f32, PlannerNufft3d32, 2, nufft3d2_32, nufft3d2_32_with_planner, nufft3d2_32_dev, phast_nufft3d2_32,
              phast_nufft3d2_32_with_planner, phast_nufft3d2_32_dev);
