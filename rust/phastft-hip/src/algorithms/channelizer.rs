//! The polyphase filter-bank channelizer -- an extension beyond PhastFT 0.3.0, which has none.  `PlannerChannelizer64/32` splits
//! a real or complex signal into `channels` equally spaced channels, each filtered with the planner's real prototype and
//! decimated by `hop`: one fold kernel and one transform per frame.  A call takes signals of `planner.signal_len()` samples
//! (two planes for a complex planner) and yields `planner.out_frames() * planner.bins()` points per signal in each output
//! plane, frame-major.

use crate::ffi;
use crate::planner::{PlannerChannelizer32, PlannerChannelizer64};
use std::ffi::c_void;

macro_rules! impl_channelize {
    ($t:ty, $planner:ident, $host:ident, $dev:ident, $c_host:ident, $c_dev:ident) => {
        /// one host signal of `planner.signal_len()` samples (`signal_im`: its imaginary plane for a complex planner, `None`
        /// for a real one) into the two output planes of `planner.out_frames() * planner.bins()` points; blocking
        pub fn $host(signal: &[$t], signal_im: Option<&[$t]>, out_re: &mut [$t], out_im: &mut [$t], planner: &$planner) {
            assert_eq!(out_re.len(), out_im.len(), "the output planes differ in length");
            if let Some(im) = signal_im {
                assert_eq!(im.len(), signal.len(), "the signal's planes differ in length");
            }
            let im = signal_im.map_or(std::ptr::null(), |s| s.as_ptr());
            ffi::check(unsafe {
                ffi::$c_host(signal.as_ptr(), im, signal.len(), out_re.as_mut_ptr(), out_im.as_mut_ptr(), out_re.len(), planner.h)
            });
        }
        /// Device-resident, batched, asynchronous on `stream`: signal b at `b * sig_dist` of `d_sig_re` (and `d_sig_im`: null
        /// for a real planner), its frames at `b * out_frames * bins` of the dense output planes; `d_work` is a device
        /// workspace of `work_len >= planner.workspace_min()` elements (null and 0 where that is 0)
        pub unsafe fn $dev(d_sig_re: *const $t, d_sig_im: *const $t, d_out_re: *mut $t, d_out_im: *mut $t, batch: usize, sig_dist: usize,
                           planner: &$planner, d_work: *mut $t, work_len: usize, stream: *mut c_void) {
            ffi::check(ffi::$c_dev(d_sig_re, d_sig_im, d_out_re, d_out_im, planner.signal_len, batch, sig_dist, planner.h, d_work, work_len,
                                   stream));
        }
    };
}
impl_channelize!(f64, PlannerChannelizer64, channelize_f64_with_planner, channelize_f64_dev, phast_channelize_f64_with_planner,
                 phast_channelize_f64_dev);
impl_channelize!(f32, PlannerChannelizer32, channelize_f32_with_planner, channelize_f32_dev, phast_channelize_f32_with_planner,
                 phast_channelize_f32_dev);
