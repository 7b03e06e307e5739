//! `phastft::algorithms::r2c` (algorithms/r2c.rs:521-895): real-to-complex and complex-to-real transforms.
//! Re-exported at the crate root like the reference does (lib.rs:34-38).
use crate::ffi;
use crate::planner::{PlannerR2c32, PlannerR2c64, PlannerR2cAny32, PlannerR2cAny64, PlannerR2cNd32, PlannerR2cNd64};
use std::ffi::c_void;

macro_rules! impl_r2c {
    ($t:ty, $planner:ident, $r2c:ident, $r2c_p:ident, $c2r:ident, $c2r_p:ident, $c2r_ps:ident, $c_r2c:ident, $c_c2r:ident) => {
        /// r2c.rs:535 / 607 -- the three length panics of r2c.rs:543-553 carry the reference's messages
        pub fn $r2c_p(input_re: &[$t], output_re: &mut [$t], output_im: &mut [$t], planner: &$planner) {
            ffi::check(unsafe {
                ffi::$c_r2c(input_re.as_ptr(), input_re.len(), output_re.as_mut_ptr(), output_re.len(),
                            output_im.as_mut_ptr(), output_im.len(), planner.h)
            });
        }
        /// r2c.rs:521 / 598
        pub fn $r2c(input_re: &[$t], output_re: &mut [$t], output_im: &mut [$t]) {
            let planner = <$planner>::new(input_re.len());
            $r2c_p(input_re, output_re, output_im, &planner);
        }
        /// r2c.rs:740 / 836 -- the scratch slices are length-checked (r2c.rs:760-769) and otherwise unused: the
        /// workspace lives in device memory
        pub fn $c2r_ps(input_re: &[$t], input_im: &[$t], output: &mut [$t], planner: &$planner,
                       scratch_re: &mut [$t], scratch_im: &mut [$t]) {
            ffi::check(unsafe {
                ffi::$c_c2r(input_re.as_ptr(), input_re.len(), input_im.as_ptr(), input_im.len(),
                            output.as_mut_ptr(), output.len(), planner.h, scratch_re.as_mut_ptr(), scratch_re.len(),
                            scratch_im.as_mut_ptr(), scratch_im.len())
            });
        }
        /// r2c.rs:710 / 813
        pub fn $c2r_p(input_re: &[$t], input_im: &[$t], output: &mut [$t], planner: &$planner) {
            let half = planner.n / 2;
            let (mut sre, mut sim) = (vec![0.0 as $t; half], vec![0.0 as $t; half]);
            $c2r_ps(input_re, input_im, output, planner, &mut sre, &mut sim);
        }
        /// r2c.rs:695 / 804
        pub fn $c2r(input_re: &[$t], input_im: &[$t], output: &mut [$t]) {
            let planner = <$planner>::new(output.len());
            $c2r_p(input_re, input_im, output, &planner);
        }
    };
}
impl_r2c!(f64, PlannerR2c64, r2c_fft_f64, r2c_fft_f64_with_planner, c2r_fft_f64, c2r_fft_f64_with_planner,
          c2r_fft_f64_with_planner_and_scratch, phast_r2c_fft_f64_with_planner,
          phast_c2r_fft_f64_with_planner_and_scratch);
impl_r2c!(f32, PlannerR2c32, r2c_fft_f32, r2c_fft_f32_with_planner, c2r_fft_f32, c2r_fft_f32_with_planner,
          c2r_fft_f32_with_planner_and_scratch, phast_r2c_fft_f32_with_planner,
          phast_c2r_fft_f32_with_planner_and_scratch);

/// Real transforms of ANY length N >= 1 -- an extension beyond PhastFT 0.3.0, whose R2C / C2R take powers of two >= 4 only.
/// NumPy rfft / irfft semantics with the conventions above: R2C writes floor(N/2) + 1 bins (unnormalised), C2R reads them
/// and writes N reals scaled by 1/N.  The length panics carry the same messages as r2c.rs:543-553 (with floor(N/2)).
macro_rules! impl_r2c_any {
    ($t:ty, $planner:ident, $r2c:ident, $r2c_p:ident, $r2c_dev:ident, $c2r:ident, $c2r_p:ident, $c2r_dev:ident,
     $c_r2c:ident, $c_r2c_dev:ident, $c_c2r:ident, $c_c2r_dev:ident) => {
        pub fn $r2c_p(input: &[$t], output_re: &mut [$t], output_im: &mut [$t], planner: &$planner) {
            ffi::check(unsafe {
                ffi::$c_r2c(input.as_ptr(), input.len(), output_re.as_mut_ptr(), output_re.len(), output_im.as_mut_ptr(),
                            output_im.len(), planner.h)
            });
        }
        pub fn $r2c(input: &[$t], output_re: &mut [$t], output_im: &mut [$t]) {
            let planner = <$planner>::new(input.len());
            $r2c_p(input, output_re, output_im, &planner);
        }
        /// Device-resident, batched, asynchronous on `stream`: `d_work` is a device workspace of `work_len >= 2 M` elements
        /// (`planner.workspace_len(batch)` runs the batch in one chunk; unused for a power of two, N = 1, 2)
        pub unsafe fn $r2c_dev(d_input: *const $t, d_output_re: *mut $t, d_output_im: *mut $t, n: usize, batch: usize,
                               in_dist: usize, out_dist: usize, planner: &$planner, d_work: *mut $t, work_len: usize,
                               stream: *mut c_void) {
            ffi::check(ffi::$c_r2c_dev(d_input, d_output_re, d_output_im, n, batch, in_dist, out_dist, planner.h, d_work,
                                       work_len, stream));
        }
        pub fn $c2r_p(input_re: &[$t], input_im: &[$t], output: &mut [$t], planner: &$planner) {
            ffi::check(unsafe {
                ffi::$c_c2r(input_re.as_ptr(), input_re.len(), input_im.as_ptr(), input_im.len(), output.as_mut_ptr(),
                            output.len(), planner.h)
            });
        }
        pub fn $c2r(input_re: &[$t], input_im: &[$t], output: &mut [$t]) {
            let planner = <$planner>::new(output.len());
            $c2r_p(input_re, input_im, output, &planner);
        }
        /// Device-resident C2R, as the R2C form above
        pub unsafe fn $c2r_dev(d_input_re: *const $t, d_input_im: *const $t, d_output: *mut $t, n: usize, batch: usize,
                               in_dist: usize, out_dist: usize, planner: &$planner, d_work: *mut $t, work_len: usize,
                               stream: *mut c_void) {
            ffi::check(ffi::$c_c2r_dev(d_input_re, d_input_im, d_output, n, batch, in_dist, out_dist, planner.h, d_work,
                                       work_len, stream));
        }
    };
}
impl_r2c_any!(f64, PlannerR2cAny64, r2c_fft_f64_any, r2c_fft_f64_any_with_planner, r2c_fft_f64_any_dev, c2r_fft_f64_any,
              c2r_fft_f64_any_with_planner, c2r_fft_f64_any_dev, phast_r2c_fft_f64_any_with_planner,
              phast_r2c_fft_f64_any_dev, phast_c2r_fft_f64_any_with_planner, phast_c2r_fft_f64_any_dev);
impl_r2c_any!(f32, PlannerR2cAny32, r2c_fft_f32_any, r2c_fft_f32_any_with_planner, r2c_fft_f32_any_dev, c2r_fft_f32_any,
              c2r_fft_f32_any_with_planner, c2r_fft_f32_any_dev, phast_r2c_fft_f32_any_with_planner,
              phast_r2c_fft_f32_any_dev, phast_c2r_fft_f32_any_with_planner, phast_c2r_fft_f32_any_dev);

/// Real transforms over every axis of a row-major array (numpy rfftn / irfftn) -- an extension beyond PhastFT 0.3.0.  R2C
/// writes the half spectrum [n_0 .. n_{r-2}][n_{r-1} / 2 + 1] to two planes (unnormalised); C2R reads it and writes
/// prod(shape) reals scaled by 1 / prod(shape).  Neither writes its input.
macro_rules! impl_r2c_nd {
    ($t:ty, $planner:ident, $r2c:ident, $r2c_p:ident, $r2c_dev:ident, $c2r:ident, $c2r_p:ident, $c2r_dev:ident,
     $c_r2c:ident, $c_r2c_dev:ident, $c_c2r:ident, $c_c2r_dev:ident) => {
        pub fn $r2c_p(input: &[$t], output_re: &mut [$t], output_im: &mut [$t], planner: &$planner) {
            ffi::check(unsafe {
                ffi::$c_r2c(input.as_ptr(), input.len(), output_re.as_mut_ptr(), output_re.len(), output_im.as_mut_ptr(),
                            output_im.len(), planner.h)
            });
        }
        pub fn $r2c(input: &[$t], output_re: &mut [$t], output_im: &mut [$t], shape: &[usize]) {
            let planner = <$planner>::new(shape);
            $r2c_p(input, output_re, output_im, &planner);
        }
        /// Device-resident, batched, asynchronous on `stream`: `d_work` holds at least `planner.workspace_len(1)` elements
        pub unsafe fn $r2c_dev(d_input: *const $t, d_output_re: *mut $t, d_output_im: *mut $t, n_total: usize, batch: usize,
                               in_dist: usize, out_dist: usize, planner: &$planner, d_work: *mut $t, work_len: usize,
                               stream: *mut c_void) {
            ffi::check(ffi::$c_r2c_dev(d_input, d_output_re, d_output_im, n_total, batch, in_dist, out_dist, planner.h,
                                       d_work, work_len, stream));
        }
        pub fn $c2r_p(input_re: &[$t], input_im: &[$t], output: &mut [$t], planner: &$planner) {
            ffi::check(unsafe {
                ffi::$c_c2r(input_re.as_ptr(), input_re.len(), input_im.as_ptr(), input_im.len(), output.as_mut_ptr(),
                            output.len(), planner.h)
            });
        }
        pub fn $c2r(input_re: &[$t], input_im: &[$t], output: &mut [$t], shape: &[usize]) {
            let planner = <$planner>::new(shape);
            $c2r_p(input_re, input_im, output, &planner);
        }
        /// Device-resident C2R, as the R2C form above
        pub unsafe fn $c2r_dev(d_input_re: *const $t, d_input_im: *const $t, d_output: *mut $t, n_total: usize,
                               batch: usize, in_dist: usize, out_dist: usize, planner: &$planner, d_work: *mut $t,
                               work_len: usize, stream: *mut c_void) {
            ffi::check(ffi::$c_c2r_dev(d_input_re, d_input_im, d_output, n_total, batch, in_dist, out_dist, planner.h,
                                       d_work, work_len, stream));
        }
    };
}
impl_r2c_nd!(f64, PlannerR2cNd64, r2c_fft_f64_nd, r2c_fft_f64_nd_with_planner, r2c_fft_f64_nd_dev, c2r_fft_f64_nd,
             c2r_fft_f64_nd_with_planner, c2r_fft_f64_nd_dev, phast_r2c_fft_f64_nd_with_planner,
             phast_r2c_fft_f64_nd_dev, phast_c2r_fft_f64_nd_with_planner, phast_c2r_fft_f64_nd_dev);
impl_r2c_nd!(f32, PlannerR2cNd32, r2c_fft_f32_nd, r2c_fft_f32_nd_with_planner, r2c_fft_f32_nd_dev, c2r_fft_f32_nd,
             c2r_fft_f32_nd_with_planner, c2r_fft_f32_nd_dev, phast_r2c_fft_f32_nd_with_planner,
             phast_r2c_fft_f32_nd_dev, phast_c2r_fft_f32_nd_with_planner, phast_c2r_fft_f32_nd_dev);
