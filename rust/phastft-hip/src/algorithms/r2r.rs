//! Real-to-real transforms -- an extension beyond PhastFT 0.3.0, which has none: the DCT and DST of types II and III of any
//! length N >= 1, with scipy.fft's definitions and `norm` semantics (`orthogonalize=True`).  `Norm::Backward` is scipy's
//! default: DCT-II y[k] = 2 sum x[n] cos(pi k (2n+1) / (2N)); `Norm::Forward` scales by 1/(2N), `Norm::Ortho` by 1/sqrt(2N)
//! with scipy's sqrt 2 on the first (DCT) / last (DST) point.  `idct` / `idst` of type t and norm n are the transform of
//! type 5 - t with Backward and Forward swapped.  `ty` is 2 or 3; anything else panics with "invalid argument".

use crate::ffi;
use crate::planner::{PlannerDct32, PlannerDct64};
use std::ffi::{c_int, c_void};

/// scipy.fft's `norm` (PHAST_NORM_* of the C ABI)
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum Norm {
    Backward = 0,
    Ortho = 1,
    Forward = 2,
}

impl Norm {
    /// the norm of the inverse transform (scipy's idct / idst)
    pub fn inverse(self) -> Norm {
        match self {
            Norm::Backward => Norm::Forward,
            Norm::Ortho => Norm::Ortho,
            Norm::Forward => Norm::Backward,
        }
    }
}

macro_rules! impl_r2r {
    ($t:ty, $planner:ident, $plain:ident, $with_planner:ident, $dev:ident, $inv:ident, $c_with_planner:ident, $c_dev:ident) => {
        pub fn $with_planner(input: &[$t], output: &mut [$t], ty: u32, norm: Norm, planner: &$planner) {
            ffi::check(unsafe {
                ffi::$c_with_planner(input.as_ptr(), input.len(), output.as_mut_ptr(), output.len(), ty as c_int, norm as c_int,
                                     planner.h)
            });
        }
        pub fn $plain(input: &[$t], output: &mut [$t], ty: u32, norm: Norm) {
            let planner = <$planner>::new(input.len());
            $with_planner(input, output, ty, norm, &planner);
        }
        /// the inverse of type `ty` with `norm`: type 5 - ty with the norm swapped (scipy's idct / idst)
        pub fn $inv(input: &[$t], output: &mut [$t], ty: u32, norm: Norm) {
            if ty != 2 && ty != 3 {
                panic!("invalid argument");
            }
            $plain(input, output, 5 - ty, norm.inverse());
        }
        /// Device-resident, batched, asynchronous on `stream`: `d_work` is a device workspace of `work_len >=
        /// planner.workspace_len(1)` elements (`planner.workspace_len(batch)` runs the batch in one chunk); in place with
        /// `d_output == d_input` and equal distances
        pub unsafe fn $dev(d_input: *const $t, d_output: *mut $t, n: usize, batch: usize, in_dist: usize, out_dist: usize,
                           ty: u32, norm: Norm, planner: &$planner, d_work: *mut $t, work_len: usize, stream: *mut c_void) {
            ffi::check(ffi::$c_dev(d_input, d_output, n, batch, in_dist, out_dist, ty as c_int, norm as c_int, planner.h, d_work,
                                   work_len, stream));
        }
    };
}
impl_r2r!(f64, PlannerDct64, dct_f64, dct_f64_with_planner, dct_f64_dev, idct_f64, phast_dct_f64_with_planner, phast_dct_f64_dev);
impl_r2r!(f32, PlannerDct32, dct_f32, dct_f32_with_planner, dct_f32_dev, idct_f32, phast_dct_f32_with_planner, phast_dct_f32_dev);
impl_r2r!(f64, PlannerDct64, dst_f64, dst_f64_with_planner, dst_f64_dev, idst_f64, phast_dst_f64_with_planner, phast_dst_f64_dev);
impl_r2r!(f32, PlannerDct32, dst_f32, dst_f32_with_planner, dst_f32_dev, idst_f32, phast_dst_f32_with_planner, phast_dst_f32_dev);
