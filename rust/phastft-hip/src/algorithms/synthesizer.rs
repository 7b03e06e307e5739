//! The polyphase synthesis filter bank, the inverse side of the channelizer -- an extension beyond PhastFT 0.3.0, which has none.
//! `PlannerSynthesizer64/32` turns `frames` frames of `channels` channels back into a signal: every channel raised by `hop`,
//! filtered with the planner's real taps, brought back to its band, and the channels summed: one inverse transform per frame
//! and one gather kernel.  A call takes `planner.frames() * planner.bins()` points per signal in each input plane, frame-major
//! as the channelizer writes them, and yields signals of `planner.out_len()` samples (two planes for a complex planner).

use crate::ffi;
use crate::planner::{PlannerSynthesizer32, PlannerSynthesizer64};
use std::ffi::c_void;

macro_rules! impl_synthesize {
    ($t:ty, $planner:ident, $host:ident, $dev:ident, $c_host:ident, $c_dev:ident) => {
        /// one signal's frames from host planes of `planner.frames() * planner.bins()` points into `out` of
        /// `planner.out_len()` samples (`out_im`: its imaginary plane for a complex planner, `None` for a real one); blocking
        pub fn $host(in_re: &[$t], in_im: &[$t], out: &mut [$t], out_im: Option<&mut [$t]>, planner: &$planner) {
            assert_eq!(in_re.len(), in_im.len(), "the input planes differ in length");
            if let Some(im) = &out_im {
                assert_eq!(im.len(), out.len(), "the signal's planes differ in length");
            }
            let im = out_im.map_or(std::ptr::null_mut(), |s| s.as_mut_ptr());
            ffi::check(unsafe { ffi::$c_host(in_re.as_ptr(), in_im.as_ptr(), in_re.len(), out.as_mut_ptr(), im, out.len(), planner.h) });
        }
        /// Device-resident, batched, asynchronous on `stream`: the frames of signal b at `b * frames * bins` of the dense input
        /// planes, signal b at `b * out_dist` of `d_out_re` (and `d_out_im`: null for a real planner); `d_work` is a device
        /// workspace of `work_len >= planner.workspace_min()` elements (null and 0 where that is 0)
        pub unsafe fn $dev(d_in_re: *const $t, d_in_im: *const $t, d_out_re: *mut $t, d_out_im: *mut $t, batch: usize, out_dist: usize,
                           planner: &$planner, d_work: *mut $t, work_len: usize, stream: *mut c_void) {
            ffi::check(ffi::$c_dev(d_in_re, d_in_im, d_out_re, d_out_im, planner.frames, batch, out_dist, planner.h, d_work, work_len, stream));
        }
    };
}
impl_synthesize!(f64, PlannerSynthesizer64, synthesize_f64_with_planner, synthesize_f64_dev, phast_synthesize_f64_with_planner,
                 phast_synthesize_f64_dev);
impl_synthesize!(f32, PlannerSynthesizer32, synthesize_f32_with_planner, synthesize_f32_dev, phast_synthesize_f32_with_planner,
                 phast_synthesize_f32_dev);
