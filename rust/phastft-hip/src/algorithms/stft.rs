//! The short-time Fourier transform and its inverse -- an extension beyond PhastFT 0.3.0, which has neither: torch.stft /
//! torch.istft(length = L) with win_length = n_fft and normalized = False.  The spectrogram is two dense planes of
//! frames * bins values, frame-major (torch's result transposed).  The inverse is the weighted overlap-add; a planner whose
//! window envelope has a minimum <= 1e-11 refuses it with "invalid argument" (torch's NOLA rule).

use crate::ffi;
use crate::planner::{PlannerStft32, PlannerStft64};
use std::ffi::c_void;

macro_rules! impl_stft {
    ($t:ty, $planner:ident, $fwd:ident, $inv:ident, $fwd_dev:ident, $inv_dev:ident, $c_fwd:ident, $c_inv:ident, $c_fwd_dev:ident,
     $c_inv_dev:ident) => {
        /// one host signal of `planner.signal_len()` samples into planes of `planner.frames() * planner.bins()`; blocking
        pub fn $fwd(signal: &[$t], output_re: &mut [$t], output_im: &mut [$t], planner: &$planner) {
            ffi::check(unsafe {
                ffi::$c_fwd(signal.as_ptr(), signal.len(), output_re.as_mut_ptr(), output_re.len(), output_im.as_mut_ptr(),
                            output_im.len(), planner.h)
            });
        }
        /// the inverse of the above
        pub fn $inv(input_re: &[$t], input_im: &[$t], signal: &mut [$t], planner: &$planner) {
            ffi::check(unsafe {
                ffi::$c_inv(input_re.as_ptr(), input_re.len(), input_im.as_ptr(), input_im.len(), signal.as_mut_ptr(), signal.len(),
                            planner.h)
            });
        }
        /// Device-resident, batched, asynchronous on `stream`: signal b at `b * sig_dist`, its planes at `b * frames * bins`;
        /// `d_work` is a device workspace of `work_len >= planner.workspace_min(false)` elements
        pub unsafe fn $fwd_dev(d_signal: *const $t, d_re: *mut $t, d_im: *mut $t, batch: usize, sig_dist: usize, planner: &$planner,
                               d_work: *mut $t, work_len: usize, stream: *mut c_void) {
            ffi::check(ffi::$c_fwd_dev(d_signal, d_re, d_im, planner.signal_len, batch, sig_dist, planner.h, d_work, work_len, stream));
        }
        /// the inverse of the above; `work_len >= planner.workspace_min(true)`
        pub unsafe fn $inv_dev(d_re: *const $t, d_im: *const $t, d_signal: *mut $t, batch: usize, sig_dist: usize, planner: &$planner,
                               d_work: *mut $t, work_len: usize, stream: *mut c_void) {
            ffi::check(ffi::$c_inv_dev(d_re, d_im, d_signal, planner.signal_len, batch, sig_dist, planner.h, d_work, work_len, stream));
        }
    };
}
impl_stft!(f64, PlannerStft64, stft_f64_with_planner, istft_f64_with_planner, stft_f64_dev, istft_f64_dev,
           phast_stft_f64_with_planner, phast_istft_f64_with_planner, phast_stft_f64_dev, phast_istft_f64_dev);
impl_stft!(f32, PlannerStft32, stft_f32_with_planner, istft_f32_with_planner, stft_f32_dev, istft_f32_dev,
           phast_stft_f32_with_planner, phast_istft_f32_with_planner, phast_stft_f32_dev, phast_istft_f32_dev);
