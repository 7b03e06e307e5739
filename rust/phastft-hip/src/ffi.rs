//! Raw bindings to `libphastft_hip.so` -- one declaration per entry point of `include/phastft_hip.h` that the
//! safe wrappers use.  `tests/test_rust_shim.py` parses this block and checks every symbol and its arity
//! against the C header (no Rust toolchain in the build image).
use std::ffi::{c_char, c_int, c_uint, c_void, CStr};

#[repr(C)]
pub(crate) struct PhastOptions {
    pub multithreaded_bit_reversal: c_int,
    pub smallest_parallel_chunk_size: usize,
}

/// `phast_tune_report` (include/phastft_hip.h: PlannerMode::Tune)
#[repr(C)]
pub struct PhastTuneReport {
    pub adopted: c_int,
    pub candidates: c_uint,
    pub us_heuristic: f32,
    pub us_best: f32,
    pub seconds: f64,
    pub plan: [c_char; 96],
}

#[repr(C)]
pub(crate) struct Opaque {
    _private: [u8; 0],
}

extern "C" {
    pub(crate) fn phast_strerror(code: c_int) -> *const c_char;
    pub(crate) fn phast_last_hip_error() -> *const c_char;
    pub(crate) fn phast_options_guess(input_size: usize, out: *mut PhastOptions) -> c_int;
    pub(crate) fn phast_planner_dit64_with_mode(n: usize, mode: c_int, out: *mut *mut Opaque) -> c_int;
    pub(crate) fn phast_planner_dit32_with_mode(n: usize, mode: c_int, out: *mut *mut Opaque) -> c_int;
    pub(crate) fn phast_planner_dit64_free(p: *mut Opaque);
    pub(crate) fn phast_planner_dit32_free(p: *mut Opaque);
    pub(crate) fn phast_planner_r2c64_with_mode(n: usize, mode: c_int, out: *mut *mut Opaque) -> c_int;
    pub(crate) fn phast_planner_r2c32_with_mode(n: usize, mode: c_int, out: *mut *mut Opaque) -> c_int;
    pub(crate) fn phast_planner_dit64_tune(p: *mut Opaque, batch_hint: usize, kind: c_int, report: *mut PhastTuneReport) -> c_int;
    pub(crate) fn phast_planner_dit32_tune(p: *mut Opaque, batch_hint: usize, kind: c_int, report: *mut PhastTuneReport) -> c_int;
    pub(crate) fn phast_planner_r2c64_tune(p: *mut Opaque, batch_hint: usize, kind: c_int, report: *mut PhastTuneReport) -> c_int;
    pub(crate) fn phast_planner_r2c32_tune(p: *mut Opaque, batch_hint: usize, kind: c_int, report: *mut PhastTuneReport) -> c_int;
    pub(crate) fn phast_wisdom_export(buf: *mut c_char, buf_len: usize, needed: *mut usize) -> c_int;
    pub(crate) fn phast_wisdom_import(text: *const c_char) -> c_int;
    pub(crate) fn phast_wisdom_forget();
    pub(crate) fn phast_planner_r2c64_free(p: *mut Opaque);
    pub(crate) fn phast_planner_r2c32_free(p: *mut Opaque);
    pub(crate) fn phast_fft_64_dit_with_planner_and_opts(re: *mut f64, re_len: usize, im: *mut f64, im_len: usize,
        direction: c_int, planner: *const Opaque, opts: *const PhastOptions) -> c_int;
    pub(crate) fn phast_fft_32_dit_with_planner_and_opts(re: *mut f32, re_len: usize, im: *mut f32, im_len: usize,
        direction: c_int, planner: *const Opaque, opts: *const PhastOptions) -> c_int;
    pub(crate) fn phast_r2c_fft_f64_with_planner(input: *const f64, n: usize, ore: *mut f64, ore_len: usize,
        oim: *mut f64, oim_len: usize, planner: *const Opaque) -> c_int;
    pub(crate) fn phast_r2c_fft_f32_with_planner(input: *const f32, n: usize, ore: *mut f32, ore_len: usize,
        oim: *mut f32, oim_len: usize, planner: *const Opaque) -> c_int;
    pub(crate) fn phast_c2r_fft_f64_with_planner_and_scratch(ire: *const f64, ire_len: usize, iim: *const f64,
        iim_len: usize, out: *mut f64, out_len: usize, planner: *const Opaque, sre: *mut f64, sre_len: usize,
        sim: *mut f64, sim_len: usize) -> c_int;
    pub(crate) fn phast_c2r_fft_f32_with_planner_and_scratch(ire: *const f32, ire_len: usize, iim: *const f32,
        iim_len: usize, out: *mut f32, out_len: usize, planner: *const Opaque, sre: *mut f32, sre_len: usize,
        sim: *mut f32, sim_len: usize) -> c_int;
    pub(crate) fn phast_bit_rev_f64(data: *mut f64, len: usize, log_n: c_uint) -> c_int;
    pub(crate) fn phast_bit_rev_f32(data: *mut f32, len: usize, log_n: c_uint) -> c_int;
    pub(crate) fn phast_deinterleave_f64(input: *const f64, len: usize, a: *mut f64, a_len: usize, b: *mut f64,
        b_len: usize) -> c_int;
    pub(crate) fn phast_deinterleave_f32(input: *const f32, len: usize, a: *mut f32, a_len: usize, b: *mut f32,
        b_len: usize) -> c_int;
    pub(crate) fn phast_combine_re_im_f64(re: *const f64, re_len: usize, im: *const f64, im_len: usize, out: *mut f64,
        out_len: usize) -> c_int;
    pub(crate) fn phast_combine_re_im_f32(re: *const f32, re_len: usize, im: *const f32, im_len: usize, out: *mut f32,
        out_len: usize) -> c_int;
    pub(crate) fn phast_fft_64_dit_dev(re: *mut f64, im: *mut f64, n: usize, batch: usize, dist: usize,
        direction: c_int, planner: *const Opaque, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_fft_32_dit_dev(re: *mut f32, im: *mut f32, n: usize, batch: usize, dist: usize,
        direction: c_int, planner: *const Opaque, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_fft_64_interleaved_with_planner_and_opts(signal: *mut f64, n: usize, direction: c_int,
        planner: *const Opaque, opts: *const PhastOptions) -> c_int;
    pub(crate) fn phast_fft_32_interleaved_with_planner_and_opts(signal: *mut f32, n: usize, direction: c_int,
        planner: *const Opaque, opts: *const PhastOptions) -> c_int;
    // any length (an extension beyond PhastFT 0.3.0: planner_any.rs / lib.rs)
    pub(crate) fn phast_planner_any64_new(n: usize, out: *mut *mut Opaque) -> c_int;
    pub(crate) fn phast_planner_any32_new(n: usize, out: *mut *mut Opaque) -> c_int;
    pub(crate) fn phast_planner_any64_free(p: *mut Opaque);
    pub(crate) fn phast_planner_any32_free(p: *mut Opaque);
    pub(crate) fn phast_planner_any64_workspace_len(p: *const Opaque, batch: usize) -> usize;
    pub(crate) fn phast_planner_any32_workspace_len(p: *const Opaque, batch: usize) -> usize;
    pub(crate) fn phast_fft_64_any_with_planner(re: *mut f64, re_len: usize, im: *mut f64, im_len: usize,
        direction: c_int, planner: *const Opaque) -> c_int;
    pub(crate) fn phast_fft_32_any_with_planner(re: *mut f32, re_len: usize, im: *mut f32, im_len: usize,
        direction: c_int, planner: *const Opaque) -> c_int;
    pub(crate) fn phast_fft_64_any_dev(re: *mut f64, im: *mut f64, n: usize, batch: usize, dist: usize,
        direction: c_int, planner: *const Opaque, work: *mut f64, work_len: usize, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_fft_32_any_dev(re: *mut f32, im: *mut f32, n: usize, batch: usize, dist: usize,
        direction: c_int, planner: *const Opaque, work: *mut f32, work_len: usize, stream: *mut c_void) -> c_int;
    // real transforms of any length (an extension beyond PhastFT 0.3.0: planner.rs / algorithms/r2c.rs)
    pub(crate) fn phast_planner_r2c_any64_new(n: usize, out: *mut *mut Opaque) -> c_int;
    pub(crate) fn phast_planner_r2c_any32_new(n: usize, out: *mut *mut Opaque) -> c_int;
    pub(crate) fn phast_planner_r2c_any64_free(p: *mut Opaque);
    pub(crate) fn phast_planner_r2c_any32_free(p: *mut Opaque);
    pub(crate) fn phast_planner_r2c_any64_workspace_len(p: *const Opaque, batch: usize) -> usize;
    pub(crate) fn phast_planner_r2c_any32_workspace_len(p: *const Opaque, batch: usize) -> usize;
    pub(crate) fn phast_r2c_fft_f64_any_with_planner(input: *const f64, n: usize, ore: *mut f64, ore_len: usize,
        oim: *mut f64, oim_len: usize, planner: *const Opaque) -> c_int;
    pub(crate) fn phast_r2c_fft_f32_any_with_planner(input: *const f32, n: usize, ore: *mut f32, ore_len: usize,
        oim: *mut f32, oim_len: usize, planner: *const Opaque) -> c_int;
    pub(crate) fn phast_r2c_fft_f64_any_dev(input: *const f64, ore: *mut f64, oim: *mut f64, n: usize, batch: usize,
        in_dist: usize, out_dist: usize, planner: *const Opaque, work: *mut f64, work_len: usize, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_r2c_fft_f32_any_dev(input: *const f32, ore: *mut f32, oim: *mut f32, n: usize, batch: usize,
        in_dist: usize, out_dist: usize, planner: *const Opaque, work: *mut f32, work_len: usize, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_c2r_fft_f64_any_with_planner(ire: *const f64, ire_len: usize, iim: *const f64, iim_len: usize,
        out: *mut f64, n: usize, planner: *const Opaque) -> c_int;
    pub(crate) fn phast_c2r_fft_f32_any_with_planner(ire: *const f32, ire_len: usize, iim: *const f32, iim_len: usize,
        out: *mut f32, n: usize, planner: *const Opaque) -> c_int;
    pub(crate) fn phast_c2r_fft_f64_any_dev(ire: *const f64, iim: *const f64, out: *mut f64, n: usize, batch: usize,
        in_dist: usize, out_dist: usize, planner: *const Opaque, work: *mut f64, work_len: usize, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_c2r_fft_f32_any_dev(ire: *const f32, iim: *const f32, out: *mut f32, n: usize, batch: usize,
        in_dist: usize, out_dist: usize, planner: *const Opaque, work: *mut f32, work_len: usize, stream: *mut c_void) -> c_int;
    // the STFT and its inverse (an extension beyond PhastFT 0.3.0: planner.rs / algorithms/stft.rs)
    pub(crate) fn phast_planner_stft64_new(signal_len: usize, n_fft: usize, hop: usize, window: *const f64, center: c_int,
        pad_mode: c_int, out: *mut *mut Opaque) -> c_int;
    pub(crate) fn phast_planner_stft64_free(p: *mut Opaque);
    pub(crate) fn phast_planner_stft64_describe(p: *const Opaque, buf: *mut c_char, buf_len: usize) -> c_int;
    pub(crate) fn phast_planner_stft64_device_bytes(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_stft64_frames(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_stft64_bins(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_stft64_workspace_len(p: *const Opaque, batch: usize) -> usize;
    pub(crate) fn phast_planner_stft64_workspace_min(p: *const Opaque, inverse: c_int) -> usize;
    pub(crate) fn phast_planner_stft64_envelope_min(p: *const Opaque) -> f64;
    pub(crate) fn phast_planner_stft64_time_stages(p: *const Opaque, inverse: c_int, signal: *mut f64, re: *mut f64, im: *mut f64,
        batch: usize, work: *mut f64, work_len: usize, reps: c_int, stage_ms: *mut f32, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_stft_f64_with_planner(signal: *const f64, signal_len: usize, ore: *mut f64, ore_len: usize, oim: *mut f64,
        oim_len: usize, planner: *const Opaque) -> c_int;
    pub(crate) fn phast_istft_f64_with_planner(ire: *const f64, ire_len: usize, iim: *const f64, iim_len: usize, signal: *mut f64,
        signal_len: usize, planner: *const Opaque) -> c_int;
    pub(crate) fn phast_stft_f64_dev(signal: *const f64, re: *mut f64, im: *mut f64, signal_len: usize, batch: usize, sig_dist: usize,
        planner: *const Opaque, work: *mut f64, work_len: usize, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_istft_f64_dev(re: *const f64, im: *const f64, signal: *mut f64, signal_len: usize, batch: usize,
        sig_dist: usize, planner: *const Opaque, work: *mut f64, work_len: usize, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_planner_stft32_new(signal_len: usize, n_fft: usize, hop: usize, window: *const f32, center: c_int,
        pad_mode: c_int, out: *mut *mut Opaque) -> c_int;
    pub(crate) fn phast_planner_stft32_free(p: *mut Opaque);
    pub(crate) fn phast_planner_stft32_describe(p: *const Opaque, buf: *mut c_char, buf_len: usize) -> c_int;
    pub(crate) fn phast_planner_stft32_device_bytes(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_stft32_frames(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_stft32_bins(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_stft32_workspace_len(p: *const Opaque, batch: usize) -> usize;
    pub(crate) fn phast_planner_stft32_workspace_min(p: *const Opaque, inverse: c_int) -> usize;
    pub(crate) fn phast_planner_stft32_envelope_min(p: *const Opaque) -> f64;
    pub(crate) fn phast_planner_stft32_time_stages(p: *const Opaque, inverse: c_int, signal: *mut f32, re: *mut f32, im: *mut f32,
        batch: usize, work: *mut f32, work_len: usize, reps: c_int, stage_ms: *mut f32, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_stft_f32_with_planner(signal: *const f32, signal_len: usize, ore: *mut f32, ore_len: usize, oim: *mut f32,
        oim_len: usize, planner: *const Opaque) -> c_int;
    pub(crate) fn phast_istft_f32_with_planner(ire: *const f32, ire_len: usize, iim: *const f32, iim_len: usize, signal: *mut f32,
        signal_len: usize, planner: *const Opaque) -> c_int;
    pub(crate) fn phast_stft_f32_dev(signal: *const f32, re: *mut f32, im: *mut f32, signal_len: usize, batch: usize, sig_dist: usize,
        planner: *const Opaque, work: *mut f32, work_len: usize, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_istft_f32_dev(re: *const f32, im: *const f32, signal: *mut f32, signal_len: usize, batch: usize,
        sig_dist: usize, planner: *const Opaque, work: *mut f32, work_len: usize, stream: *mut c_void) -> c_int;
    // the MDCT and its inverse (an extension beyond PhastFT 0.3.0: planner.rs / algorithms/mdct.rs)
    pub(crate) fn phast_planner_mdct64_new(signal_len: usize, n: usize, window: *const f64, padded: c_int, out: *mut *mut Opaque) -> c_int;
    pub(crate) fn phast_planner_mdct64_free(p: *mut Opaque);
    pub(crate) fn phast_planner_mdct64_describe(p: *const Opaque, buf: *mut c_char, buf_len: usize) -> c_int;
    pub(crate) fn phast_planner_mdct64_device_bytes(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_mdct64_frames(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_mdct64_workspace_len(p: *const Opaque, batch: usize) -> usize;
    pub(crate) fn phast_planner_mdct64_workspace_min(p: *const Opaque, inverse: c_int) -> usize;
    pub(crate) fn phast_planner_mdct64_tdac_defect(p: *const Opaque) -> f64;
    pub(crate) fn phast_planner_mdct64_time_stages(p: *const Opaque, inverse: c_int, signal: *mut f64, coefs: *mut f64, batch: usize,
        work: *mut f64, work_len: usize, reps: c_int, stage_ms: *mut f32, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_mdct_f64_with_planner(signal: *const f64, signal_len: usize, coefs: *mut f64, coefs_len: usize,
        planner: *const Opaque) -> c_int;
    pub(crate) fn phast_imdct_f64_with_planner(coefs: *const f64, coefs_len: usize, signal: *mut f64, signal_len: usize,
        planner: *const Opaque) -> c_int;
    pub(crate) fn phast_mdct_f64_dev(signal: *const f64, coefs: *mut f64, signal_len: usize, batch: usize, sig_dist: usize,
        planner: *const Opaque, work: *mut f64, work_len: usize, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_imdct_f64_dev(coefs: *const f64, signal: *mut f64, signal_len: usize, batch: usize, sig_dist: usize,
        planner: *const Opaque, work: *mut f64, work_len: usize, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_planner_mdct32_new(signal_len: usize, n: usize, window: *const f32, padded: c_int, out: *mut *mut Opaque) -> c_int;
    pub(crate) fn phast_planner_mdct32_free(p: *mut Opaque);
    pub(crate) fn phast_planner_mdct32_describe(p: *const Opaque, buf: *mut c_char, buf_len: usize) -> c_int;
    pub(crate) fn phast_planner_mdct32_device_bytes(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_mdct32_frames(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_mdct32_workspace_len(p: *const Opaque, batch: usize) -> usize;
    pub(crate) fn phast_planner_mdct32_workspace_min(p: *const Opaque, inverse: c_int) -> usize;
    pub(crate) fn phast_planner_mdct32_tdac_defect(p: *const Opaque) -> f64;
    pub(crate) fn phast_planner_mdct32_time_stages(p: *const Opaque, inverse: c_int, signal: *mut f32, coefs: *mut f32, batch: usize,
        work: *mut f32, work_len: usize, reps: c_int, stage_ms: *mut f32, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_mdct_f32_with_planner(signal: *const f32, signal_len: usize, coefs: *mut f32, coefs_len: usize,
        planner: *const Opaque) -> c_int;
    pub(crate) fn phast_imdct_f32_with_planner(coefs: *const f32, coefs_len: usize, signal: *mut f32, signal_len: usize,
        planner: *const Opaque) -> c_int;
    pub(crate) fn phast_mdct_f32_dev(signal: *const f32, coefs: *mut f32, signal_len: usize, batch: usize, sig_dist: usize,
        planner: *const Opaque, work: *mut f32, work_len: usize, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_imdct_f32_dev(coefs: *const f32, signal: *mut f32, signal_len: usize, batch: usize, sig_dist: usize,
        planner: *const Opaque, work: *mut f32, work_len: usize, stream: *mut c_void) -> c_int;
    // Welch spectral estimation (an extension beyond PhastFT 0.3.0: planner.rs / algorithms/psd.rs)
    pub(crate) fn phast_planner_psd64_new(signal_len: usize, nperseg: usize, hop: usize, nfft: usize, window: *const f64, detrend: c_int,
        scaling: c_int, fs: f64, out: *mut *mut Opaque) -> c_int;
    pub(crate) fn phast_planner_psd64_free(p: *mut Opaque);
    pub(crate) fn phast_planner_psd64_describe(p: *const Opaque, buf: *mut c_char, buf_len: usize) -> c_int;
    pub(crate) fn phast_planner_psd64_device_bytes(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_psd64_segments(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_psd64_bins(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_psd64_slab(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_psd64_workspace_len(p: *const Opaque, batch: usize, cross: c_int) -> usize;
    pub(crate) fn phast_planner_psd64_workspace_min(p: *const Opaque, cross: c_int) -> usize;
    pub(crate) fn phast_planner_psd64_time_stages(p: *const Opaque, signal: *mut f64, out: *mut f64, batch: usize, average: c_int,
        slab: usize, work: *mut f64, work_len: usize, reps: c_int, stage_ms: *mut f32, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_psd_f64_with_planner(signal: *const f64, signal_len: usize, out: *mut f64, out_len: usize, average: c_int,
        planner: *const Opaque) -> c_int;
    pub(crate) fn phast_csd_f64_with_planner(x: *const f64, x_len: usize, y: *const f64, y_len: usize, out_re: *mut f64, re_len: usize,
        out_im: *mut f64, im_len: usize, pxx: *mut f64, pxx_len: usize, pyy: *mut f64, pyy_len: usize, average: c_int,
        planner: *const Opaque) -> c_int;
    pub(crate) fn phast_psd_f64_dev(x: *const f64, out: *mut f64, signal_len: usize, batch: usize, sig_dist: usize, average: c_int,
        planner: *const Opaque, work: *mut f64, work_len: usize, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_csd_f64_dev(x: *const f64, y: *const f64, out_re: *mut f64, out_im: *mut f64, pxx: *mut f64, pyy: *mut f64,
        signal_len: usize, batch: usize, sig_dist: usize, average: c_int, planner: *const Opaque, work: *mut f64, work_len: usize,
        stream: *mut c_void) -> c_int;
    pub(crate) fn phast_planner_psd32_new(signal_len: usize, nperseg: usize, hop: usize, nfft: usize, window: *const f64, detrend: c_int,
        scaling: c_int, fs: f64, out: *mut *mut Opaque) -> c_int;
    pub(crate) fn phast_planner_psd32_free(p: *mut Opaque);
    pub(crate) fn phast_planner_psd32_describe(p: *const Opaque, buf: *mut c_char, buf_len: usize) -> c_int;
    pub(crate) fn phast_planner_psd32_device_bytes(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_psd32_segments(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_psd32_bins(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_psd32_slab(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_psd32_workspace_len(p: *const Opaque, batch: usize, cross: c_int) -> usize;
    pub(crate) fn phast_planner_psd32_workspace_min(p: *const Opaque, cross: c_int) -> usize;
    pub(crate) fn phast_planner_psd32_time_stages(p: *const Opaque, signal: *mut f32, out: *mut f32, batch: usize, average: c_int,
        slab: usize, work: *mut f32, work_len: usize, reps: c_int, stage_ms: *mut f32, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_psd_f32_with_planner(signal: *const f32, signal_len: usize, out: *mut f32, out_len: usize, average: c_int,
        planner: *const Opaque) -> c_int;
    pub(crate) fn phast_csd_f32_with_planner(x: *const f32, x_len: usize, y: *const f32, y_len: usize, out_re: *mut f32, re_len: usize,
        out_im: *mut f32, im_len: usize, pxx: *mut f32, pxx_len: usize, pyy: *mut f32, pyy_len: usize, average: c_int,
        planner: *const Opaque) -> c_int;
    pub(crate) fn phast_psd_f32_dev(x: *const f32, out: *mut f32, signal_len: usize, batch: usize, sig_dist: usize, average: c_int,
        planner: *const Opaque, work: *mut f32, work_len: usize, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_csd_f32_dev(x: *const f32, y: *const f32, out_re: *mut f32, out_im: *mut f32, pxx: *mut f32, pyy: *mut f32,
        signal_len: usize, batch: usize, sig_dist: usize, average: c_int, planner: *const Opaque, work: *mut f32, work_len: usize,
        stream: *mut c_void) -> c_int;
    // the Lomb-Scargle periodogram (an extension beyond PhastFT 0.3.0: planner.rs / algorithms/lomb.rs)
    pub(crate) fn phast_planner_lomb64_new(t: *const f64, m: usize, freqs: *const f64, k: usize, weights: *const f64,
        floating_mean: c_int, eps: f64, out: *mut *mut Opaque) -> c_int;
    pub(crate) fn phast_planner_lomb64_free(p: *mut Opaque);
    pub(crate) fn phast_planner_lomb64_describe(p: *const Opaque, buf: *mut c_char, buf_len: usize) -> c_int;
    pub(crate) fn phast_planner_lomb64_device_bytes(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_lomb64_slab(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_lomb64_grid_len(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_lomb64_workspace_len(p: *const Opaque, batch: usize) -> usize;
    pub(crate) fn phast_planner_lomb64_workspace_min(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_lomb64_time_stages(p: *const Opaque, y: *const f64, out_re: *mut f64, out_im: *mut f64, batch: usize,
        normalize: c_int, work: *mut f64, work_len: usize, reps: c_int, stage_ms: *mut f32, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_lombscargle_f64(t: *const f64, m: usize, freqs: *const f64, k: usize, weights: *const f64, floating_mean: c_int,
        eps: f64, y: *const f64, out_re: *mut f64, out_im: *mut f64, normalize: c_int) -> c_int;
    pub(crate) fn phast_lombscargle_f64_with_planner(y: *const f64, m: usize, out_re: *mut f64, re_len: usize, out_im: *mut f64,
        im_len: usize, normalize: c_int, planner: *const Opaque) -> c_int;
    pub(crate) fn phast_lombscargle_f64_dev(y: *const f64, out_re: *mut f64, out_im: *mut f64, m: usize, batch: usize, sig_dist: usize,
        out_dist: usize, normalize: c_int, planner: *const Opaque, work: *mut f64, work_len: usize, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_planner_lomb32_new(t: *const f64, m: usize, freqs: *const f64, k: usize, weights: *const f64,
        floating_mean: c_int, eps: f64, out: *mut *mut Opaque) -> c_int;
    pub(crate) fn phast_planner_lomb32_free(p: *mut Opaque);
    pub(crate) fn phast_planner_lomb32_describe(p: *const Opaque, buf: *mut c_char, buf_len: usize) -> c_int;
    pub(crate) fn phast_planner_lomb32_device_bytes(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_lomb32_slab(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_lomb32_grid_len(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_lomb32_workspace_len(p: *const Opaque, batch: usize) -> usize;
    pub(crate) fn phast_planner_lomb32_workspace_min(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_lomb32_time_stages(p: *const Opaque, y: *const f32, out_re: *mut f32, out_im: *mut f32, batch: usize,
        normalize: c_int, work: *mut f32, work_len: usize, reps: c_int, stage_ms: *mut f32, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_lombscargle_f32(t: *const f64, m: usize, freqs: *const f64, k: usize, weights: *const f64, floating_mean: c_int,
        eps: f64, y: *const f32, out_re: *mut f32, out_im: *mut f32, normalize: c_int) -> c_int;
    pub(crate) fn phast_lombscargle_f32_with_planner(y: *const f32, m: usize, out_re: *mut f32, re_len: usize, out_im: *mut f32,
        im_len: usize, normalize: c_int, planner: *const Opaque) -> c_int;
    pub(crate) fn phast_lombscargle_f32_dev(y: *const f32, out_re: *mut f32, out_im: *mut f32, m: usize, batch: usize, sig_dist: usize,
        out_dist: usize, normalize: c_int, planner: *const Opaque, work: *mut f32, work_len: usize, stream: *mut c_void) -> c_int;
    // sample-rate conversion (an extension beyond PhastFT 0.3.0: planner.rs / algorithms/resample.rs)
    pub(crate) fn phast_planner_upfirdn64_new(signal_len: usize, taps: *const f64, num_taps: usize, up: usize, down: usize, first: usize,
        out_len: usize, out: *mut *mut Opaque) -> c_int;
    pub(crate) fn phast_planner_upfirdn64_free(p: *mut Opaque);
    pub(crate) fn phast_planner_upfirdn64_describe(p: *const Opaque, buf: *mut c_char, buf_len: usize) -> c_int;
    pub(crate) fn phast_planner_upfirdn64_device_bytes(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_upfirdn64_workspace_len(p: *const Opaque, batch: usize) -> usize;
    pub(crate) fn phast_planner_upfirdn64_out_len(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_upfirdn64_full_len(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_upfirdn64_tile(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_upfirdn64_chunk(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_upfirdn64_time_stages(p: *const Opaque, signal: *const f64, out: *mut f64, batch: usize, reps: c_int,
        stage_ms: *mut f32, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_upfirdn_f64_with_planner(signal: *const f64, signal_len: usize, out: *mut f64, out_len: usize,
        planner: *const Opaque) -> c_int;
    pub(crate) fn phast_upfirdn_f64_dev(signal: *const f64, out: *mut f64, signal_len: usize, batch: usize, sig_dist: usize, out_dist: usize,
        planner: *const Opaque, work: *mut f64, work_len: usize, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_planner_resample64_new(signal_len: usize, num: usize, out: *mut *mut Opaque) -> c_int;
    pub(crate) fn phast_planner_resample64_free(p: *mut Opaque);
    pub(crate) fn phast_planner_resample64_describe(p: *const Opaque, buf: *mut c_char, buf_len: usize) -> c_int;
    pub(crate) fn phast_planner_resample64_device_bytes(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_resample64_workspace_len(p: *const Opaque, batch: usize) -> usize;
    pub(crate) fn phast_planner_resample64_workspace_min(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_resample64_time_stages(p: *const Opaque, signal: *const f64, out: *mut f64, batch: usize, work: *mut f64,
        work_len: usize, reps: c_int, stage_ms: *mut f32, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_resample_f64_with_planner(signal: *const f64, signal_len: usize, out: *mut f64, out_len: usize,
        planner: *const Opaque) -> c_int;
    pub(crate) fn phast_resample_f64_dev(signal: *const f64, out: *mut f64, signal_len: usize, batch: usize, sig_dist: usize, out_dist: usize,
        planner: *const Opaque, work: *mut f64, work_len: usize, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_planner_upfirdn32_new(signal_len: usize, taps: *const f32, num_taps: usize, up: usize, down: usize, first: usize,
        out_len: usize, out: *mut *mut Opaque) -> c_int;
    pub(crate) fn phast_planner_upfirdn32_free(p: *mut Opaque);
    pub(crate) fn phast_planner_upfirdn32_describe(p: *const Opaque, buf: *mut c_char, buf_len: usize) -> c_int;
    pub(crate) fn phast_planner_upfirdn32_device_bytes(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_upfirdn32_workspace_len(p: *const Opaque, batch: usize) -> usize;
    pub(crate) fn phast_planner_upfirdn32_out_len(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_upfirdn32_full_len(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_upfirdn32_tile(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_upfirdn32_chunk(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_upfirdn32_time_stages(p: *const Opaque, signal: *const f32, out: *mut f32, batch: usize, reps: c_int,
        stage_ms: *mut f32, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_upfirdn_f32_with_planner(signal: *const f32, signal_len: usize, out: *mut f32, out_len: usize,
        planner: *const Opaque) -> c_int;
    pub(crate) fn phast_upfirdn_f32_dev(signal: *const f32, out: *mut f32, signal_len: usize, batch: usize, sig_dist: usize, out_dist: usize,
        planner: *const Opaque, work: *mut f32, work_len: usize, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_planner_resample32_new(signal_len: usize, num: usize, out: *mut *mut Opaque) -> c_int;
    pub(crate) fn phast_planner_resample32_free(p: *mut Opaque);
    pub(crate) fn phast_planner_resample32_describe(p: *const Opaque, buf: *mut c_char, buf_len: usize) -> c_int;
    pub(crate) fn phast_planner_resample32_device_bytes(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_resample32_workspace_len(p: *const Opaque, batch: usize) -> usize;
    pub(crate) fn phast_planner_resample32_workspace_min(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_resample32_time_stages(p: *const Opaque, signal: *const f32, out: *mut f32, batch: usize, work: *mut f32,
        work_len: usize, reps: c_int, stage_ms: *mut f32, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_resample_f32_with_planner(signal: *const f32, signal_len: usize, out: *mut f32, out_len: usize,
        planner: *const Opaque) -> c_int;
    pub(crate) fn phast_resample_f32_dev(signal: *const f32, out: *mut f32, signal_len: usize, batch: usize, sig_dist: usize, out_dist: usize,
        planner: *const Opaque, work: *mut f32, work_len: usize, stream: *mut c_void) -> c_int;
    // the polyphase channelizer (an extension beyond PhastFT 0.3.0: planner.rs / algorithms/channelizer.rs)
    pub(crate) fn phast_planner_channelizer64_new(signal_len: usize, taps: *const f64, num_taps: usize, channels: usize, hop: usize, first_frame: usize,
        out_frames: usize, complex_input: c_int, out: *mut *mut Opaque) -> c_int;
    pub(crate) fn phast_planner_channelizer64_free(p: *mut Opaque);
    pub(crate) fn phast_planner_channelizer64_describe(p: *const Opaque, buf: *mut c_char, buf_len: usize) -> c_int;
    pub(crate) fn phast_planner_channelizer64_device_bytes(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_channelizer64_workspace_len(p: *const Opaque, batch: usize) -> usize;
    pub(crate) fn phast_planner_channelizer64_workspace_min(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_channelizer64_out_frames(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_channelizer64_full_frames(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_channelizer64_bins(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_channelizer64_tile_frames(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_channelizer64_tile_cols(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_channelizer64_chunk(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_channelizer64_periods(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_channelizer64_time_stages(p: *const Opaque, sig_re: *const f64, sig_im: *const f64, out_re: *mut f64, out_im: *mut f64,
        batch: usize, work: *mut f64, work_len: usize, reps: c_int, stage_ms: *mut f32, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_channelize_f64_with_planner(sig_re: *const f64, sig_im: *const f64, signal_len: usize, out_re: *mut f64,
        out_im: *mut f64, out_len: usize, planner: *const Opaque) -> c_int;
    pub(crate) fn phast_channelize_f64_dev(sig_re: *const f64, sig_im: *const f64, out_re: *mut f64, out_im: *mut f64, signal_len: usize,
        batch: usize, sig_dist: usize, planner: *const Opaque, work: *mut f64, work_len: usize, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_planner_channelizer32_new(signal_len: usize, taps: *const f32, num_taps: usize, channels: usize, hop: usize, first_frame: usize,
        out_frames: usize, complex_input: c_int, out: *mut *mut Opaque) -> c_int;
    pub(crate) fn phast_planner_channelizer32_free(p: *mut Opaque);
    pub(crate) fn phast_planner_channelizer32_describe(p: *const Opaque, buf: *mut c_char, buf_len: usize) -> c_int;
    pub(crate) fn phast_planner_channelizer32_device_bytes(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_channelizer32_workspace_len(p: *const Opaque, batch: usize) -> usize;
    pub(crate) fn phast_planner_channelizer32_workspace_min(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_channelizer32_out_frames(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_channelizer32_full_frames(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_channelizer32_bins(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_channelizer32_tile_frames(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_channelizer32_tile_cols(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_channelizer32_chunk(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_channelizer32_periods(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_channelizer32_time_stages(p: *const Opaque, sig_re: *const f32, sig_im: *const f32, out_re: *mut f32, out_im: *mut f32,
        batch: usize, work: *mut f32, work_len: usize, reps: c_int, stage_ms: *mut f32, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_channelize_f32_with_planner(sig_re: *const f32, sig_im: *const f32, signal_len: usize, out_re: *mut f32,
        out_im: *mut f32, out_len: usize, planner: *const Opaque) -> c_int;
    pub(crate) fn phast_channelize_f32_dev(sig_re: *const f32, sig_im: *const f32, out_re: *mut f32, out_im: *mut f32, signal_len: usize,
        batch: usize, sig_dist: usize, planner: *const Opaque, work: *mut f32, work_len: usize, stream: *mut c_void) -> c_int;
    // the polyphase synthesis bank (an extension beyond PhastFT 0.3.0: planner.rs / algorithms/synthesizer.rs)
    pub(crate) fn phast_planner_synthesizer64_new(frames: usize, taps: *const f64, num_taps: usize, channels: usize, hop: usize, first: usize,
        out_len: usize, complex_output: c_int, out: *mut *mut Opaque) -> c_int;
    pub(crate) fn phast_planner_synthesizer64_free(p: *mut Opaque);
    pub(crate) fn phast_planner_synthesizer64_describe(p: *const Opaque, buf: *mut c_char, buf_len: usize) -> c_int;
    pub(crate) fn phast_planner_synthesizer64_device_bytes(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_synthesizer64_workspace_len(p: *const Opaque, batch: usize) -> usize;
    pub(crate) fn phast_planner_synthesizer64_workspace_min(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_synthesizer64_out_len(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_synthesizer64_full_len(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_synthesizer64_bins(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_synthesizer64_tile_samples(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_synthesizer64_per_thread(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_synthesizer64_max_terms(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_synthesizer64_time_stages(p: *const Opaque, in_re: *const f64, in_im: *const f64, out_re: *mut f64, out_im: *mut f64,
        batch: usize, work: *mut f64, work_len: usize, reps: c_int, stage_ms: *mut f32, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_synthesize_f64_with_planner(in_re: *const f64, in_im: *const f64, in_len: usize, out_re: *mut f64,
        out_im: *mut f64, out_len: usize, planner: *const Opaque) -> c_int;
    pub(crate) fn phast_synthesize_f64_dev(in_re: *const f64, in_im: *const f64, out_re: *mut f64, out_im: *mut f64, frames: usize,
        batch: usize, out_dist: usize, planner: *const Opaque, work: *mut f64, work_len: usize, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_planner_synthesizer32_new(frames: usize, taps: *const f32, num_taps: usize, channels: usize, hop: usize, first: usize,
        out_len: usize, complex_output: c_int, out: *mut *mut Opaque) -> c_int;
    pub(crate) fn phast_planner_synthesizer32_free(p: *mut Opaque);
    pub(crate) fn phast_planner_synthesizer32_describe(p: *const Opaque, buf: *mut c_char, buf_len: usize) -> c_int;
    pub(crate) fn phast_planner_synthesizer32_device_bytes(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_synthesizer32_workspace_len(p: *const Opaque, batch: usize) -> usize;
    pub(crate) fn phast_planner_synthesizer32_workspace_min(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_synthesizer32_out_len(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_synthesizer32_full_len(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_synthesizer32_bins(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_synthesizer32_tile_samples(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_synthesizer32_per_thread(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_synthesizer32_max_terms(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_synthesizer32_time_stages(p: *const Opaque, in_re: *const f32, in_im: *const f32, out_re: *mut f32, out_im: *mut f32,
        batch: usize, work: *mut f32, work_len: usize, reps: c_int, stage_ms: *mut f32, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_synthesize_f32_with_planner(in_re: *const f32, in_im: *const f32, in_len: usize, out_re: *mut f32,
        out_im: *mut f32, out_len: usize, planner: *const Opaque) -> c_int;
    pub(crate) fn phast_synthesize_f32_dev(in_re: *const f32, in_im: *const f32, out_re: *mut f32, out_im: *mut f32, frames: usize,
        batch: usize, out_dist: usize, planner: *const Opaque, work: *mut f32, work_len: usize, stream: *mut c_void) -> c_int;
    // the continuous wavelet transform (an extension beyond PhastFT 0.3.0: planner.rs / algorithms/cwt.rs)
    pub(crate) fn phast_planner_cwt64_new(signal_len: usize, pad_len: usize, scales: *const f64, num_scales: usize, family: c_int, param: f64,
        norm: c_int, real_input: c_int, out: *mut *mut Opaque) -> c_int;
    pub(crate) fn phast_planner_cwt64_free(p: *mut Opaque);
    pub(crate) fn phast_planner_cwt64_describe(p: *const Opaque, buf: *mut c_char, buf_len: usize) -> c_int;
    pub(crate) fn phast_planner_cwt64_device_bytes(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_cwt64_workspace_len(p: *const Opaque, batch: usize) -> usize;
    pub(crate) fn phast_planner_cwt64_workspace_min(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_cwt64_pad_len(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_cwt64_num_scales(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_cwt64_tile_bins(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_cwt64_scale_group(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_cwt64_time_stages(p: *const Opaque, x_re: *const f64, x_im: *const f64, out_re: *mut f64, out_im: *mut f64,
        batch: usize, work: *mut f64, work_len: usize, reps: c_int, stage_ms: *mut f32, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_cwt_64_with_planner(x_re: *const f64, x_im: *const f64, x_len: usize, out_re: *mut f64, out_im: *mut f64,
        out_len: usize, planner: *const Opaque) -> c_int;
    pub(crate) fn phast_cwt_64_dev(x_re: *const f64, x_im: *const f64, out_re: *mut f64, out_im: *mut f64, signal_len: usize, batch: usize,
        sig_dist: usize, out_dist: usize, planner: *const Opaque, work: *mut f64, work_len: usize, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_planner_cwt32_new(signal_len: usize, pad_len: usize, scales: *const f64, num_scales: usize, family: c_int, param: f64,
        norm: c_int, real_input: c_int, out: *mut *mut Opaque) -> c_int;
    pub(crate) fn phast_planner_cwt32_free(p: *mut Opaque);
    pub(crate) fn phast_planner_cwt32_describe(p: *const Opaque, buf: *mut c_char, buf_len: usize) -> c_int;
    pub(crate) fn phast_planner_cwt32_device_bytes(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_cwt32_workspace_len(p: *const Opaque, batch: usize) -> usize;
    pub(crate) fn phast_planner_cwt32_workspace_min(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_cwt32_pad_len(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_cwt32_num_scales(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_cwt32_tile_bins(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_cwt32_scale_group(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_cwt32_time_stages(p: *const Opaque, x_re: *const f32, x_im: *const f32, out_re: *mut f32, out_im: *mut f32,
        batch: usize, work: *mut f32, work_len: usize, reps: c_int, stage_ms: *mut f32, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_cwt_32_with_planner(x_re: *const f32, x_im: *const f32, x_len: usize, out_re: *mut f32, out_im: *mut f32,
        out_len: usize, planner: *const Opaque) -> c_int;
    pub(crate) fn phast_cwt_32_dev(x_re: *const f32, x_im: *const f32, out_re: *mut f32, out_im: *mut f32, signal_len: usize, batch: usize,
        sig_dist: usize, out_dist: usize, planner: *const Opaque, work: *mut f32, work_len: usize, stream: *mut c_void) -> c_int;
    // overlap-save convolution and correlation (an extension beyond PhastFT 0.3.0: planner.rs / algorithms/conv.rs)
    pub(crate) fn phast_planner_conv64_new(signal_len: usize, taps: *const f64, num_taps: usize, mode: c_int, flip: c_int,
        block: usize, out: *mut *mut Opaque) -> c_int;
    pub(crate) fn phast_planner_conv64_free(p: *mut Opaque);
    pub(crate) fn phast_planner_conv64_describe(p: *const Opaque, buf: *mut c_char, buf_len: usize) -> c_int;
    pub(crate) fn phast_planner_conv64_device_bytes(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_conv64_out_len(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_conv64_block(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_conv64_segments(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_conv64_workspace_len(p: *const Opaque, batch: usize) -> usize;
    pub(crate) fn phast_planner_conv64_workspace_min(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_conv64_time_stages(p: *const Opaque, signal: *const f64, out: *mut f64, batch: usize,
        work: *mut f64, work_len: usize, reps: c_int, stage_ms: *mut f32, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_conv_f64_with_planner(signal: *const f64, signal_len: usize, out: *mut f64, out_len: usize,
        planner: *const Opaque) -> c_int;
    pub(crate) fn phast_conv_f64_dev(signal: *const f64, out: *mut f64, signal_len: usize, batch: usize, sig_dist: usize,
        out_dist: usize, planner: *const Opaque, work: *mut f64, work_len: usize, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_planner_conv32_new(signal_len: usize, taps: *const f32, num_taps: usize, mode: c_int, flip: c_int,
        block: usize, out: *mut *mut Opaque) -> c_int;
    pub(crate) fn phast_planner_conv32_free(p: *mut Opaque);
    pub(crate) fn phast_planner_conv32_describe(p: *const Opaque, buf: *mut c_char, buf_len: usize) -> c_int;
    pub(crate) fn phast_planner_conv32_device_bytes(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_conv32_out_len(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_conv32_block(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_conv32_segments(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_conv32_workspace_len(p: *const Opaque, batch: usize) -> usize;
    pub(crate) fn phast_planner_conv32_workspace_min(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_conv32_time_stages(p: *const Opaque, signal: *const f32, out: *mut f32, batch: usize,
        work: *mut f32, work_len: usize, reps: c_int, stage_ms: *mut f32, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_conv_f32_with_planner(signal: *const f32, signal_len: usize, out: *mut f32, out_len: usize,
        planner: *const Opaque) -> c_int;
    pub(crate) fn phast_conv_f32_dev(signal: *const f32, out: *mut f32, signal_len: usize, batch: usize, sig_dist: usize,
        out_dist: usize, planner: *const Opaque, work: *mut f32, work_len: usize, stream: *mut c_void) -> c_int;
    // overlap-save convolution and correlation of arrays of rank 1 .. 3 (an extension: planner.rs / algorithms/convnd.rs)
    pub(crate) fn phast_planner_convnd64_new(signal_dims: *const usize, tap_dims: *const usize, rank: usize, taps: *const f64,
        mode: c_int, flip: c_int, block: *const usize, out: *mut *mut Opaque) -> c_int;
    pub(crate) fn phast_planner_convnd64_free(p: *mut Opaque);
    pub(crate) fn phast_planner_convnd64_describe(p: *const Opaque, buf: *mut c_char, buf_len: usize) -> c_int;
    pub(crate) fn phast_planner_convnd64_device_bytes(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_convnd64_out_len(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_convnd64_out_dims(p: *const Opaque, dims: *mut usize, rank: usize) -> c_int;
    pub(crate) fn phast_planner_convnd64_block(p: *const Opaque, dims: *mut usize, rank: usize) -> c_int;
    pub(crate) fn phast_planner_convnd64_tiles(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_convnd64_workspace_len(p: *const Opaque, batch: usize) -> usize;
    pub(crate) fn phast_planner_convnd64_workspace_min(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_convnd64_time_stages(p: *const Opaque, signal: *const f64, out: *mut f64, batch: usize,
        work: *mut f64, work_len: usize, reps: c_int, stage_ms: *mut f32, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_convnd_f64_with_planner(signal: *const f64, signal_len: usize, out: *mut f64, out_len: usize,
        planner: *const Opaque) -> c_int;
    pub(crate) fn phast_convnd_f64_dev(signal: *const f64, out: *mut f64, signal_len: usize, batch: usize, sig_dist: usize,
        out_dist: usize, planner: *const Opaque, work: *mut f64, work_len: usize, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_planner_convnd32_new(signal_dims: *const usize, tap_dims: *const usize, rank: usize, taps: *const f32,
        mode: c_int, flip: c_int, block: *const usize, out: *mut *mut Opaque) -> c_int;
    pub(crate) fn phast_planner_convnd32_free(p: *mut Opaque);
    pub(crate) fn phast_planner_convnd32_describe(p: *const Opaque, buf: *mut c_char, buf_len: usize) -> c_int;
    pub(crate) fn phast_planner_convnd32_device_bytes(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_convnd32_out_len(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_convnd32_out_dims(p: *const Opaque, dims: *mut usize, rank: usize) -> c_int;
    pub(crate) fn phast_planner_convnd32_block(p: *const Opaque, dims: *mut usize, rank: usize) -> c_int;
    pub(crate) fn phast_planner_convnd32_tiles(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_convnd32_workspace_len(p: *const Opaque, batch: usize) -> usize;
    pub(crate) fn phast_planner_convnd32_workspace_min(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_convnd32_time_stages(p: *const Opaque, signal: *const f32, out: *mut f32, batch: usize,
        work: *mut f32, work_len: usize, reps: c_int, stage_ms: *mut f32, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_convnd_f32_with_planner(signal: *const f32, signal_len: usize, out: *mut f32, out_len: usize,
        planner: *const Opaque) -> c_int;
    pub(crate) fn phast_convnd_f32_dev(signal: *const f32, out: *mut f32, signal_len: usize, batch: usize, sig_dist: usize,
        out_dist: usize, planner: *const Opaque, work: *mut f32, work_len: usize, stream: *mut c_void) -> c_int;
    // the chirp-Z transform on the unit circle (an extension beyond PhastFT 0.3.0: planner.rs / algorithms/czt.rs)
    pub(crate) fn phast_planner_czt64_new(n: usize, m: usize, step: f64, start: f64, out: *mut *mut Opaque) -> c_int;
    pub(crate) fn phast_planner_czt64_free(p: *mut Opaque);
    pub(crate) fn phast_planner_czt64_describe(p: *const Opaque, buf: *mut c_char, buf_len: usize) -> c_int;
    pub(crate) fn phast_planner_czt64_device_bytes(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_czt64_conv_len(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_czt64_workspace_len(p: *const Opaque, batch: usize) -> usize;
    pub(crate) fn phast_planner_czt64_time_stages(p: *const Opaque, in_re: *const f64, in_im: *const f64, out_re: *mut f64,
        out_im: *mut f64, batch: usize, work: *mut f64, work_len: usize, reps: c_int, stage_ms: *mut f32, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_czt_64(in_re: *const f64, in_im: *const f64, n: usize, out_re: *mut f64, out_im: *mut f64, m: usize,
        step: f64, start: f64) -> c_int;
    pub(crate) fn phast_czt_64_with_planner(in_re: *const f64, in_im: *const f64, n: usize, out_re: *mut f64, out_im: *mut f64,
        m: usize, planner: *const Opaque) -> c_int;
    pub(crate) fn phast_czt_64_dev(in_re: *const f64, in_im: *const f64, in_dist: usize, out_re: *mut f64, out_im: *mut f64,
        out_dist: usize, batch: usize, planner: *const Opaque, work: *mut f64, work_len: usize, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_planner_czt32_new(n: usize, m: usize, step: f64, start: f64, out: *mut *mut Opaque) -> c_int;
    pub(crate) fn phast_planner_czt32_free(p: *mut Opaque);
    pub(crate) fn phast_planner_czt32_describe(p: *const Opaque, buf: *mut c_char, buf_len: usize) -> c_int;
    pub(crate) fn phast_planner_czt32_device_bytes(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_czt32_conv_len(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_czt32_workspace_len(p: *const Opaque, batch: usize) -> usize;
    pub(crate) fn phast_planner_czt32_time_stages(p: *const Opaque, in_re: *const f32, in_im: *const f32, out_re: *mut f32,
        out_im: *mut f32, batch: usize, work: *mut f32, work_len: usize, reps: c_int, stage_ms: *mut f32, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_czt_32(in_re: *const f32, in_im: *const f32, n: usize, out_re: *mut f32, out_im: *mut f32, m: usize,
        step: f64, start: f64) -> c_int;
    pub(crate) fn phast_czt_32_with_planner(in_re: *const f32, in_im: *const f32, n: usize, out_re: *mut f32, out_im: *mut f32,
        m: usize, planner: *const Opaque) -> c_int;
    pub(crate) fn phast_czt_32_dev(in_re: *const f32, in_im: *const f32, in_dist: usize, out_re: *mut f32, out_im: *mut f32,
        out_dist: usize, batch: usize, planner: *const Opaque, work: *mut f32, work_len: usize, stream: *mut c_void) -> c_int;
    // non-uniform FFTs of types 1 and 2 (an extension beyond PhastFT 0.3.0: planner.rs / algorithms/nufft.rs)
    pub(crate) fn phast_planner_nufft64_new(n_modes: usize, x_turns: *const f64, m_points: usize, eps: f64, out: *mut *mut Opaque) -> c_int;
    pub(crate) fn phast_planner_nufft64_new_dev(n_modes: usize, d_x_turns: *const f64, m_points: usize, eps: f64, stream: *mut c_void,
        out: *mut *mut Opaque) -> c_int;
    pub(crate) fn phast_planner_nufft64_set_points_dev(p: *mut Opaque, d_x_turns: *const f64, m_points: usize, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_planner_nufft64_free(p: *mut Opaque);
    pub(crate) fn phast_planner_nufft64_describe(p: *const Opaque, buf: *mut c_char, buf_len: usize) -> c_int;
    pub(crate) fn phast_planner_nufft64_device_bytes(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_nufft64_grid_len(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_nufft64_width(p: *const Opaque) -> c_int;
    pub(crate) fn phast_planner_nufft64_workspace_len(p: *const Opaque, batch: usize) -> usize;
    pub(crate) fn phast_planner_nufft64_time_stages(p: *const Opaque, in_re: *const f64, in_im: *const f64, out_re: *mut f64,
        out_im: *mut f64, ty: c_int, batch: usize, work: *mut f64, work_len: usize, reps: c_int, stage_ms: *mut f32, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_nufft1_64(x_turns: *const f64, m_points: usize, in_re: *const f64, in_im: *const f64, out_re: *mut f64,
        out_im: *mut f64, n_modes: usize, eps: f64, direction: c_int) -> c_int;
    pub(crate) fn phast_nufft1_64_with_planner(in_re: *const f64, in_im: *const f64, in_len: usize, out_re: *mut f64, out_im: *mut f64,
        out_len: usize, direction: c_int, planner: *const Opaque) -> c_int;
    pub(crate) fn phast_nufft1_64_dev(in_re: *const f64, in_im: *const f64, in_dist: usize, out_re: *mut f64, out_im: *mut f64,
        out_dist: usize, batch: usize, direction: c_int, planner: *const Opaque, work: *mut f64, work_len: usize, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_nufft2_64(x_turns: *const f64, m_points: usize, in_re: *const f64, in_im: *const f64, out_re: *mut f64,
        out_im: *mut f64, n_modes: usize, eps: f64, direction: c_int) -> c_int;
    pub(crate) fn phast_nufft2_64_with_planner(in_re: *const f64, in_im: *const f64, in_len: usize, out_re: *mut f64, out_im: *mut f64,
        out_len: usize, direction: c_int, planner: *const Opaque) -> c_int;
    pub(crate) fn phast_nufft2_64_dev(in_re: *const f64, in_im: *const f64, in_dist: usize, out_re: *mut f64, out_im: *mut f64,
        out_dist: usize, batch: usize, direction: c_int, planner: *const Opaque, work: *mut f64, work_len: usize, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_planner_nufft32_new(n_modes: usize, x_turns: *const f64, m_points: usize, eps: f64, out: *mut *mut Opaque) -> c_int;
    pub(crate) fn phast_planner_nufft32_new_dev(n_modes: usize, d_x_turns: *const f64, m_points: usize, eps: f64, stream: *mut c_void,
        out: *mut *mut Opaque) -> c_int;
    pub(crate) fn phast_planner_nufft32_set_points_dev(p: *mut Opaque, d_x_turns: *const f64, m_points: usize, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_planner_nufft32_free(p: *mut Opaque);
    pub(crate) fn phast_planner_nufft32_describe(p: *const Opaque, buf: *mut c_char, buf_len: usize) -> c_int;
    pub(crate) fn phast_planner_nufft32_device_bytes(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_nufft32_grid_len(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_nufft32_width(p: *const Opaque) -> c_int;
    pub(crate) fn phast_planner_nufft32_workspace_len(p: *const Opaque, batch: usize) -> usize;
    pub(crate) fn phast_planner_nufft32_time_stages(p: *const Opaque, in_re: *const f32, in_im: *const f32, out_re: *mut f32,
        out_im: *mut f32, ty: c_int, batch: usize, work: *mut f32, work_len: usize, reps: c_int, stage_ms: *mut f32, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_nufft1_32(x_turns: *const f64, m_points: usize, in_re: *const f32, in_im: *const f32, out_re: *mut f32,
        out_im: *mut f32, n_modes: usize, eps: f64, direction: c_int) -> c_int;
    pub(crate) fn phast_nufft1_32_with_planner(in_re: *const f32, in_im: *const f32, in_len: usize, out_re: *mut f32, out_im: *mut f32,
        out_len: usize, direction: c_int, planner: *const Opaque) -> c_int;
    pub(crate) fn phast_nufft1_32_dev(in_re: *const f32, in_im: *const f32, in_dist: usize, out_re: *mut f32, out_im: *mut f32,
        out_dist: usize, batch: usize, direction: c_int, planner: *const Opaque, work: *mut f32, work_len: usize, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_nufft2_32(x_turns: *const f64, m_points: usize, in_re: *const f32, in_im: *const f32, out_re: *mut f32,
        out_im: *mut f32, n_modes: usize, eps: f64, direction: c_int) -> c_int;
    pub(crate) fn phast_nufft2_32_with_planner(in_re: *const f32, in_im: *const f32, in_len: usize, out_re: *mut f32, out_im: *mut f32,
        out_len: usize, direction: c_int, planner: *const Opaque) -> c_int;
    pub(crate) fn phast_nufft2_32_dev(in_re: *const f32, in_im: *const f32, in_dist: usize, out_re: *mut f32, out_im: *mut f32,
        out_dist: usize, batch: usize, direction: c_int, planner: *const Opaque, work: *mut f32, work_len: usize, stream: *mut c_void) -> c_int;
    // the same in two dimensions (planner.rs / algorithms/nufft2d.rs)
    pub(crate) fn phast_planner_nufft2d64_new(n1: usize, n2: usize, x_turns: *const f64, y_turns: *const f64, m_points: usize, eps: f64,
        out: *mut *mut Opaque) -> c_int;
    pub(crate) fn phast_planner_nufft2d64_new_dev(n1: usize, n2: usize, d_x_turns: *const f64, d_y_turns: *const f64, m_points: usize, eps: f64,
        stream: *mut c_void, out: *mut *mut Opaque) -> c_int;
    pub(crate) fn phast_planner_nufft2d64_set_points_dev(p: *mut Opaque, d_x_turns: *const f64, d_y_turns: *const f64, m_points: usize,
        stream: *mut c_void) -> c_int;
    pub(crate) fn phast_planner_nufft2d64_free(p: *mut Opaque);
    pub(crate) fn phast_planner_nufft2d64_describe(p: *const Opaque, buf: *mut c_char, buf_len: usize) -> c_int;
    pub(crate) fn phast_planner_nufft2d64_device_bytes(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_nufft2d64_grid_len(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_nufft2d64_grid_rows(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_nufft2d64_grid_cols(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_nufft2d64_width(p: *const Opaque) -> c_int;
    pub(crate) fn phast_planner_nufft2d64_workspace_len(p: *const Opaque, batch: usize) -> usize;
    pub(crate) fn phast_planner_nufft2d64_time_stages(p: *const Opaque, in_re: *const f64, in_im: *const f64, out_re: *mut f64,
        out_im: *mut f64, ty: c_int, batch: usize, work: *mut f64, work_len: usize, reps: c_int, stage_ms: *mut f32, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_nufft2d1_64(x_turns: *const f64, y_turns: *const f64, m_points: usize, in_re: *const f64, in_im: *const f64,
        out_re: *mut f64, out_im: *mut f64, n1: usize, n2: usize, eps: f64, direction: c_int) -> c_int;
    pub(crate) fn phast_nufft2d1_64_with_planner(in_re: *const f64, in_im: *const f64, in_len: usize, out_re: *mut f64, out_im: *mut f64,
        out_len: usize, direction: c_int, planner: *const Opaque) -> c_int;
    pub(crate) fn phast_nufft2d1_64_dev(in_re: *const f64, in_im: *const f64, in_dist: usize, out_re: *mut f64, out_im: *mut f64,
        out_dist: usize, batch: usize, direction: c_int, planner: *const Opaque, work: *mut f64, work_len: usize, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_nufft2d2_64(x_turns: *const f64, y_turns: *const f64, m_points: usize, in_re: *const f64, in_im: *const f64,
        out_re: *mut f64, out_im: *mut f64, n1: usize, n2: usize, eps: f64, direction: c_int) -> c_int;
    pub(crate) fn phast_nufft2d2_64_with_planner(in_re: *const f64, in_im: *const f64, in_len: usize, out_re: *mut f64, out_im: *mut f64,
        out_len: usize, direction: c_int, planner: *const Opaque) -> c_int;
    pub(crate) fn phast_nufft2d2_64_dev(in_re: *const f64, in_im: *const f64, in_dist: usize, out_re: *mut f64, out_im: *mut f64,
        out_dist: usize, batch: usize, direction: c_int, planner: *const Opaque, work: *mut f64, work_len: usize, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_planner_nufft2d32_new(n1: usize, n2: usize, x_turns: *const f64, y_turns: *const f64, m_points: usize, eps: f64,
        out: *mut *mut Opaque) -> c_int;
    pub(crate) fn phast_planner_nufft2d32_new_dev(n1: usize, n2: usize, d_x_turns: *const f64, d_y_turns: *const f64, m_points: usize, eps: f64,
        stream: *mut c_void, out: *mut *mut Opaque) -> c_int;
    pub(crate) fn phast_planner_nufft2d32_set_points_dev(p: *mut Opaque, d_x_turns: *const f64, d_y_turns: *const f64, m_points: usize,
        stream: *mut c_void) -> c_int;
    pub(crate) fn phast_planner_nufft2d32_free(p: *mut Opaque);
    pub(crate) fn phast_planner_nufft2d32_describe(p: *const Opaque, buf: *mut c_char, buf_len: usize) -> c_int;
    pub(crate) fn phast_planner_nufft2d32_device_bytes(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_nufft2d32_grid_len(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_nufft2d32_grid_rows(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_nufft2d32_grid_cols(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_nufft2d32_width(p: *const Opaque) -> c_int;
    pub(crate) fn phast_planner_nufft2d32_workspace_len(p: *const Opaque, batch: usize) -> usize;
    pub(crate) fn phast_planner_nufft2d32_time_stages(p: *const Opaque, in_re: *const f32, in_im: *const f32, out_re: *mut f32,
        out_im: *mut f32, ty: c_int, batch: usize, work: *mut f32, work_len: usize, reps: c_int, stage_ms: *mut f32, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_nufft2d1_32(x_turns: *const f64, y_turns: *const f64, m_points: usize, in_re: *const f32, in_im: *const f32,
        out_re: *mut f32, out_im: *mut f32, n1: usize, n2: usize, eps: f64, direction: c_int) -> c_int;
    pub(crate) fn phast_nufft2d1_32_with_planner(in_re: *const f32, in_im: *const f32, in_len: usize, out_re: *mut f32, out_im: *mut f32,
        out_len: usize, direction: c_int, planner: *const Opaque) -> c_int;
    pub(crate) fn phast_nufft2d1_32_dev(in_re: *const f32, in_im: *const f32, in_dist: usize, out_re: *mut f32, out_im: *mut f32,
        out_dist: usize, batch: usize, direction: c_int, planner: *const Opaque, work: *mut f32, work_len: usize, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_nufft2d2_32(x_turns: *const f64, y_turns: *const f64, m_points: usize, in_re: *const f32, in_im: *const f32,
        out_re: *mut f32, out_im: *mut f32, n1: usize, n2: usize, eps: f64, direction: c_int) -> c_int;
    pub(crate) fn phast_nufft2d2_32_with_planner(in_re: *const f32, in_im: *const f32, in_len: usize, out_re: *mut f32, out_im: *mut f32,
        out_len: usize, direction: c_int, planner: *const Opaque) -> c_int;
    pub(crate) fn phast_nufft2d2_32_dev(in_re: *const f32, in_im: *const f32, in_dist: usize, out_re: *mut f32, out_im: *mut f32,
        out_dist: usize, batch: usize, direction: c_int, planner: *const Opaque, work: *mut f32, work_len: usize, stream: *mut c_void) -> c_int;
    // the same in three dimensions (planner.rs / algorithms/nufft3d.rs)
    pub(crate) fn phast_planner_nufft3d64_new(n1: usize, n2: usize, n3: usize, x_turns: *const f64, y_turns: *const f64, z_turns: *const f64,
        m_points: usize, eps: f64,
        out: *mut *mut Opaque) -> c_int;
    pub(crate) fn phast_planner_nufft3d64_new_dev(n1: usize, n2: usize, n3: usize, d_x_turns: *const f64, d_y_turns: *const f64, d_z_turns: *const f64, m_points: usize, eps: f64,
        stream: *mut c_void, out: *mut *mut Opaque) -> c_int;
    pub(crate) fn phast_planner_nufft3d64_set_points_dev(p: *mut Opaque, d_x_turns: *const f64, d_y_turns: *const f64, d_z_turns: *const f64, m_points: usize,
        stream: *mut c_void) -> c_int;
    pub(crate) fn phast_planner_nufft3d64_free(p: *mut Opaque);
    pub(crate) fn phast_planner_nufft3d64_describe(p: *const Opaque, buf: *mut c_char, buf_len: usize) -> c_int;
    pub(crate) fn phast_planner_nufft3d64_device_bytes(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_nufft3d64_grid_len(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_nufft3d64_grid_dim(p: *const Opaque, axis: c_int) -> usize;
    pub(crate) fn phast_planner_nufft3d64_width(p: *const Opaque) -> c_int;
    pub(crate) fn phast_planner_nufft3d64_workspace_len(p: *const Opaque, batch: usize) -> usize;
    pub(crate) fn phast_planner_nufft3d64_time_stages(p: *const Opaque, in_re: *const f64, in_im: *const f64, out_re: *mut f64,
        out_im: *mut f64, ty: c_int, batch: usize, work: *mut f64, work_len: usize, reps: c_int, stage_ms: *mut f32, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_nufft3d1_64(x_turns: *const f64, y_turns: *const f64, z_turns: *const f64, m_points: usize, in_re: *const f64, in_im: *const f64,
        out_re: *mut f64, out_im: *mut f64, n1: usize, n2: usize, n3: usize, eps: f64, direction: c_int) -> c_int;
    pub(crate) fn phast_nufft3d1_64_with_planner(in_re: *const f64, in_im: *const f64, in_len: usize, out_re: *mut f64, out_im: *mut f64,
        out_len: usize, direction: c_int, planner: *const Opaque) -> c_int;
    pub(crate) fn phast_nufft3d1_64_dev(in_re: *const f64, in_im: *const f64, in_dist: usize, out_re: *mut f64, out_im: *mut f64,
        out_dist: usize, batch: usize, direction: c_int, planner: *const Opaque, work: *mut f64, work_len: usize, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_nufft3d2_64(x_turns: *const f64, y_turns: *const f64, z_turns: *const f64, m_points: usize, in_re: *const f64, in_im: *const f64,
        out_re: *mut f64, out_im: *mut f64, n1: usize, n2: usize, n3: usize, eps: f64, direction: c_int) -> c_int;
    pub(crate) fn phast_nufft3d2_64_with_planner(in_re: *const f64, in_im: *const f64, in_len: usize, out_re: *mut f64, out_im: *mut f64,
        out_len: usize, direction: c_int, planner: *const Opaque) -> c_int;
    pub(crate) fn phast_nufft3d2_64_dev(in_re: *const f64, in_im: *const f64, in_dist: usize, out_re: *mut f64, out_im: *mut f64,
        out_dist: usize, batch: usize, direction: c_int, planner: *const Opaque, work: *mut f64, work_len: usize, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_planner_nufft3d32_new(n1: usize, n2: usize, n3: usize, x_turns: *const f64, y_turns: *const f64, z_turns: *const f64,
        m_points: usize, eps: f64,
        out: *mut *mut Opaque) -> c_int;
    pub(crate) fn phast_planner_nufft3d32_new_dev(n1: usize, n2: usize, n3: usize, d_x_turns: *const f64, d_y_turns: *const f64, d_z_turns: *const f64, m_points: usize, eps: f64,
        stream: *mut c_void, out: *mut *mut Opaque) -> c_int;
    pub(crate) fn phast_planner_nufft3d32_set_points_dev(p: *mut Opaque, d_x_turns: *const f64, d_y_turns: *const f64, d_z_turns: *const f64, m_points: usize,
        stream: *mut c_void) -> c_int;
    pub(crate) fn phast_planner_nufft3d32_free(p: *mut Opaque);
    pub(crate) fn phast_planner_nufft3d32_describe(p: *const Opaque, buf: *mut c_char, buf_len: usize) -> c_int;
    pub(crate) fn phast_planner_nufft3d32_device_bytes(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_nufft3d32_grid_len(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_nufft3d32_grid_dim(p: *const Opaque, axis: c_int) -> usize;
    pub(crate) fn phast_planner_nufft3d32_width(p: *const Opaque) -> c_int;
    pub(crate) fn phast_planner_nufft3d32_workspace_len(p: *const Opaque, batch: usize) -> usize;
    pub(crate) fn phast_planner_nufft3d32_time_stages(p: *const Opaque, in_re: *const f32, in_im: *const f32, out_re: *mut f32,
        out_im: *mut f32, ty: c_int, batch: usize, work: *mut f32, work_len: usize, reps: c_int, stage_ms: *mut f32, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_nufft3d1_32(x_turns: *const f64, y_turns: *const f64, z_turns: *const f64, m_points: usize, in_re: *const f32, in_im: *const f32,
        out_re: *mut f32, out_im: *mut f32, n1: usize, n2: usize, n3: usize, eps: f64, direction: c_int) -> c_int;
    pub(crate) fn phast_nufft3d1_32_with_planner(in_re: *const f32, in_im: *const f32, in_len: usize, out_re: *mut f32, out_im: *mut f32,
        out_len: usize, direction: c_int, planner: *const Opaque) -> c_int;
    pub(crate) fn phast_nufft3d1_32_dev(in_re: *const f32, in_im: *const f32, in_dist: usize, out_re: *mut f32, out_im: *mut f32,
        out_dist: usize, batch: usize, direction: c_int, planner: *const Opaque, work: *mut f32, work_len: usize, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_nufft3d2_32(x_turns: *const f64, y_turns: *const f64, z_turns: *const f64, m_points: usize, in_re: *const f32, in_im: *const f32,
        out_re: *mut f32, out_im: *mut f32, n1: usize, n2: usize, n3: usize, eps: f64, direction: c_int) -> c_int;
    pub(crate) fn phast_nufft3d2_32_with_planner(in_re: *const f32, in_im: *const f32, in_len: usize, out_re: *mut f32, out_im: *mut f32,
        out_len: usize, direction: c_int, planner: *const Opaque) -> c_int;
    pub(crate) fn phast_nufft3d2_32_dev(in_re: *const f32, in_im: *const f32, in_dist: usize, out_re: *mut f32, out_im: *mut f32,
        out_dist: usize, batch: usize, direction: c_int, planner: *const Opaque, work: *mut f32, work_len: usize, stream: *mut c_void) -> c_int;
    // the non-uniform FFT of type 3
    pub(crate) fn phast_planner_nufft_t3_64_new(x: *const f64, m_points: usize, s: *const f64, k_targets: usize, eps: f64, out: *mut *mut Opaque) -> c_int;
    pub(crate) fn phast_planner_nufft_t3_64_free(p: *mut Opaque);
    pub(crate) fn phast_planner_nufft_t3_64_describe(p: *const Opaque, buf: *mut c_char, buf_len: usize) -> c_int;
    pub(crate) fn phast_planner_nufft_t3_64_device_bytes(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_nufft_t3_64_grid_len(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_nufft_t3_64_width(p: *const Opaque) -> c_int;
    pub(crate) fn phast_planner_nufft_t3_64_workspace_len(p: *const Opaque, batch: usize) -> usize;
    pub(crate) fn phast_planner_nufft_t3_64_time_stages(p: *const Opaque, in_re: *const f64, in_im: *const f64, out_re: *mut f64,
        out_im: *mut f64, batch: usize, work: *mut f64, work_len: usize, reps: c_int, stage_ms: *mut f32, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_nufft3_64(x: *const f64, m_points: usize, s: *const f64, k_targets: usize, c_re: *const f64, c_im: *const f64,
        out_re: *mut f64, out_im: *mut f64, eps: f64, direction: c_int) -> c_int;
    pub(crate) fn phast_nufft3_64_with_planner(c_re: *const f64, c_im: *const f64, m_points: usize, out_re: *mut f64, out_im: *mut f64,
        k_targets: usize, direction: c_int, planner: *const Opaque) -> c_int;
    pub(crate) fn phast_nufft3_64_dev(c_re: *const f64, c_im: *const f64, in_dist: usize, out_re: *mut f64, out_im: *mut f64,
        out_dist: usize, batch: usize, direction: c_int, planner: *const Opaque, work: *mut f64, work_len: usize, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_planner_nufft_t3_32_new(x: *const f64, m_points: usize, s: *const f64, k_targets: usize, eps: f64, out: *mut *mut Opaque) -> c_int;
    pub(crate) fn phast_planner_nufft_t3_32_free(p: *mut Opaque);
    pub(crate) fn phast_planner_nufft_t3_32_describe(p: *const Opaque, buf: *mut c_char, buf_len: usize) -> c_int;
    pub(crate) fn phast_planner_nufft_t3_32_device_bytes(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_nufft_t3_32_grid_len(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_nufft_t3_32_width(p: *const Opaque) -> c_int;
    pub(crate) fn phast_planner_nufft_t3_32_workspace_len(p: *const Opaque, batch: usize) -> usize;
    pub(crate) fn phast_planner_nufft_t3_32_time_stages(p: *const Opaque, in_re: *const f32, in_im: *const f32, out_re: *mut f32,
        out_im: *mut f32, batch: usize, work: *mut f32, work_len: usize, reps: c_int, stage_ms: *mut f32, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_nufft3_32(x: *const f64, m_points: usize, s: *const f64, k_targets: usize, c_re: *const f32, c_im: *const f32,
        out_re: *mut f32, out_im: *mut f32, eps: f64, direction: c_int) -> c_int;
    pub(crate) fn phast_nufft3_32_with_planner(c_re: *const f32, c_im: *const f32, m_points: usize, out_re: *mut f32, out_im: *mut f32,
        k_targets: usize, direction: c_int, planner: *const Opaque) -> c_int;
    pub(crate) fn phast_nufft3_32_dev(c_re: *const f32, c_im: *const f32, in_dist: usize, out_re: *mut f32, out_im: *mut f32,
        out_dist: usize, batch: usize, direction: c_int, planner: *const Opaque, work: *mut f32, work_len: usize, stream: *mut c_void) -> c_int;
    // DCT / DST of types II and III (an extension beyond PhastFT 0.3.0: planner.rs / algorithms/r2r.rs)
    pub(crate) fn phast_planner_dct64_new(n: usize, out: *mut *mut Opaque) -> c_int;
    pub(crate) fn phast_planner_dct32_new(n: usize, out: *mut *mut Opaque) -> c_int;
    pub(crate) fn phast_planner_dct64_free(p: *mut Opaque);
    pub(crate) fn phast_planner_dct32_free(p: *mut Opaque);
    pub(crate) fn phast_planner_dct64_workspace_len(p: *const Opaque, batch: usize) -> usize;
    pub(crate) fn phast_planner_dct32_workspace_len(p: *const Opaque, batch: usize) -> usize;
    pub(crate) fn phast_dct_f64_with_planner(input: *const f64, input_len: usize, output: *mut f64, output_len: usize,
        ty: c_int, norm: c_int, planner: *const Opaque) -> c_int;
    pub(crate) fn phast_dct_f64_dev(input: *const f64, output: *mut f64, n: usize, batch: usize, in_dist: usize, out_dist: usize,
        ty: c_int, norm: c_int, planner: *const Opaque, work: *mut f64, work_len: usize, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_dct_f32_with_planner(input: *const f32, input_len: usize, output: *mut f32, output_len: usize,
        ty: c_int, norm: c_int, planner: *const Opaque) -> c_int;
    pub(crate) fn phast_dct_f32_dev(input: *const f32, output: *mut f32, n: usize, batch: usize, in_dist: usize, out_dist: usize,
        ty: c_int, norm: c_int, planner: *const Opaque, work: *mut f32, work_len: usize, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_dst_f64_with_planner(input: *const f64, input_len: usize, output: *mut f64, output_len: usize,
        ty: c_int, norm: c_int, planner: *const Opaque) -> c_int;
    pub(crate) fn phast_dst_f64_dev(input: *const f64, output: *mut f64, n: usize, batch: usize, in_dist: usize, out_dist: usize,
        ty: c_int, norm: c_int, planner: *const Opaque, work: *mut f64, work_len: usize, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_dst_f32_with_planner(input: *const f32, input_len: usize, output: *mut f32, output_len: usize,
        ty: c_int, norm: c_int, planner: *const Opaque) -> c_int;
    pub(crate) fn phast_dst_f32_dev(input: *const f32, output: *mut f32, n: usize, batch: usize, in_dist: usize, out_dist: usize,
        ty: c_int, norm: c_int, planner: *const Opaque, work: *mut f32, work_len: usize, stream: *mut c_void) -> c_int;
    // multi-dimensional transforms (an extension beyond PhastFT 0.3.0: planner.rs / lib.rs / algorithms/r2c.rs)
    pub(crate) fn phast_planner_nd64_new(dims: *const usize, rank: usize, out: *mut *mut Opaque) -> c_int;
    pub(crate) fn phast_planner_nd32_new(dims: *const usize, rank: usize, out: *mut *mut Opaque) -> c_int;
    pub(crate) fn phast_planner_nd64_free(p: *mut Opaque);
    pub(crate) fn phast_planner_nd32_free(p: *mut Opaque);
    pub(crate) fn phast_planner_nd64_workspace_len(p: *const Opaque, batch: usize) -> usize;
    pub(crate) fn phast_planner_nd32_workspace_len(p: *const Opaque, batch: usize) -> usize;
    pub(crate) fn phast_fft_64_nd_with_planner(re: *mut f64, re_len: usize, im: *mut f64, im_len: usize,
        direction: c_int, planner: *const Opaque) -> c_int;
    pub(crate) fn phast_fft_32_nd_with_planner(re: *mut f32, re_len: usize, im: *mut f32, im_len: usize,
        direction: c_int, planner: *const Opaque) -> c_int;
    pub(crate) fn phast_fft_64_nd_dev(re: *mut f64, im: *mut f64, n_total: usize, batch: usize, dist: usize,
        direction: c_int, planner: *const Opaque, work: *mut f64, work_len: usize, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_fft_32_nd_dev(re: *mut f32, im: *mut f32, n_total: usize, batch: usize, dist: usize,
        direction: c_int, planner: *const Opaque, work: *mut f32, work_len: usize, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_planner_r2c_nd64_new(dims: *const usize, rank: usize, out: *mut *mut Opaque) -> c_int;
    pub(crate) fn phast_planner_r2c_nd32_new(dims: *const usize, rank: usize, out: *mut *mut Opaque) -> c_int;
    pub(crate) fn phast_planner_r2c_nd64_free(p: *mut Opaque);
    pub(crate) fn phast_planner_r2c_nd32_free(p: *mut Opaque);
    pub(crate) fn phast_planner_r2c_nd64_workspace_len(p: *const Opaque, batch: usize) -> usize;
    pub(crate) fn phast_planner_r2c_nd32_workspace_len(p: *const Opaque, batch: usize) -> usize;
    pub(crate) fn phast_r2c_fft_f64_nd_with_planner(input: *const f64, n: usize, ore: *mut f64, ore_len: usize,
        oim: *mut f64, oim_len: usize, planner: *const Opaque) -> c_int;
    pub(crate) fn phast_r2c_fft_f32_nd_with_planner(input: *const f32, n: usize, ore: *mut f32, ore_len: usize,
        oim: *mut f32, oim_len: usize, planner: *const Opaque) -> c_int;
    pub(crate) fn phast_r2c_fft_f64_nd_dev(input: *const f64, ore: *mut f64, oim: *mut f64, n_total: usize, batch: usize,
        in_dist: usize, out_dist: usize, planner: *const Opaque, work: *mut f64, work_len: usize, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_r2c_fft_f32_nd_dev(input: *const f32, ore: *mut f32, oim: *mut f32, n_total: usize, batch: usize,
        in_dist: usize, out_dist: usize, planner: *const Opaque, work: *mut f32, work_len: usize, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_c2r_fft_f64_nd_with_planner(ire: *const f64, ire_len: usize, iim: *const f64, iim_len: usize,
        out: *mut f64, n: usize, planner: *const Opaque) -> c_int;
    pub(crate) fn phast_c2r_fft_f32_nd_with_planner(ire: *const f32, ire_len: usize, iim: *const f32, iim_len: usize,
        out: *mut f32, n: usize, planner: *const Opaque) -> c_int;
    pub(crate) fn phast_c2r_fft_f64_nd_dev(ire: *const f64, iim: *const f64, out: *mut f64, n_total: usize, batch: usize,
        in_dist: usize, out_dist: usize, planner: *const Opaque, work: *mut f64, work_len: usize, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_c2r_fft_f32_nd_dev(ire: *const f32, iim: *const f32, out: *mut f32, n_total: usize, batch: usize,
        in_dist: usize, out_dist: usize, planner: *const Opaque, work: *mut f32, work_len: usize, stream: *mut c_void) -> c_int;
    // the discrete wavelet transform and its inverse
    pub(crate) fn phast_planner_dwt64_new(signal_len: usize, dec_lo: *const f64, dec_hi: *const f64, rec_lo: *const f64, rec_hi: *const f64,
        filter_len: usize, level: usize, mode: c_int, out: *mut *mut Opaque) -> c_int;
    pub(crate) fn phast_planner_dwt64_free(p: *mut Opaque);
    pub(crate) fn phast_planner_dwt64_describe(p: *const Opaque, buf: *mut c_char, buf_len: usize) -> c_int;
    pub(crate) fn phast_planner_dwt64_device_bytes(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_dwt64_workspace_len(p: *const Opaque, batch: usize) -> usize;
    pub(crate) fn phast_planner_dwt64_workspace_min(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_dwt64_coeff_len(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_dwt64_level_len(p: *const Opaque, level: usize) -> usize;
    pub(crate) fn phast_planner_dwt64_level_offset(p: *const Opaque, level: usize) -> usize;
    pub(crate) fn phast_planner_dwt64_tile(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_dwt64_time_stages(p: *const Opaque, signal: *mut f64, coeffs: *mut f64, batch: usize, work: *mut f64, work_len: usize,
        reps: c_int, stage_ms: *mut f32, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_wavedec_f64_with_planner(signal: *const f64, signal_len: usize, coeffs: *mut f64, coeff_len: usize,
        planner: *const Opaque) -> c_int;
    pub(crate) fn phast_waverec_f64_with_planner(coeffs: *const f64, coeff_len: usize, signal: *mut f64, signal_len: usize,
        planner: *const Opaque) -> c_int;
    pub(crate) fn phast_wavedec_f64_dev(signal: *const f64, coeffs: *mut f64, signal_len: usize, batch: usize, sig_dist: usize,
        coeff_dist: usize, planner: *const Opaque, work: *mut f64, work_len: usize, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_waverec_f64_dev(coeffs: *const f64, signal: *mut f64, signal_len: usize, batch: usize, coeff_dist: usize,
        sig_dist: usize, planner: *const Opaque, work: *mut f64, work_len: usize, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_planner_dwt32_new(signal_len: usize, dec_lo: *const f32, dec_hi: *const f32, rec_lo: *const f32, rec_hi: *const f32,
        filter_len: usize, level: usize, mode: c_int, out: *mut *mut Opaque) -> c_int;
    pub(crate) fn phast_planner_dwt32_free(p: *mut Opaque);
    pub(crate) fn phast_planner_dwt32_describe(p: *const Opaque, buf: *mut c_char, buf_len: usize) -> c_int;
    pub(crate) fn phast_planner_dwt32_device_bytes(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_dwt32_workspace_len(p: *const Opaque, batch: usize) -> usize;
    pub(crate) fn phast_planner_dwt32_workspace_min(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_dwt32_coeff_len(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_dwt32_level_len(p: *const Opaque, level: usize) -> usize;
    pub(crate) fn phast_planner_dwt32_level_offset(p: *const Opaque, level: usize) -> usize;
    pub(crate) fn phast_planner_dwt32_tile(p: *const Opaque) -> usize;
    pub(crate) fn phast_planner_dwt32_time_stages(p: *const Opaque, signal: *mut f32, coeffs: *mut f32, batch: usize, work: *mut f32, work_len: usize,
        reps: c_int, stage_ms: *mut f32, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_wavedec_f32_with_planner(signal: *const f32, signal_len: usize, coeffs: *mut f32, coeff_len: usize,
        planner: *const Opaque) -> c_int;
    pub(crate) fn phast_waverec_f32_with_planner(coeffs: *const f32, coeff_len: usize, signal: *mut f32, signal_len: usize,
        planner: *const Opaque) -> c_int;
    pub(crate) fn phast_wavedec_f32_dev(signal: *const f32, coeffs: *mut f32, signal_len: usize, batch: usize, sig_dist: usize,
        coeff_dist: usize, planner: *const Opaque, work: *mut f32, work_len: usize, stream: *mut c_void) -> c_int;
    pub(crate) fn phast_waverec_f32_dev(coeffs: *const f32, signal: *mut f32, signal_len: usize, batch: usize, coeff_dist: usize,
        sig_dist: usize, planner: *const Opaque, work: *mut f32, work_len: usize, stream: *mut c_void) -> c_int;
}

/// Re-raises a library status as the reference's panic: `phast_strerror` returns the exact text of the
/// `assert!` / `assert_eq!` the status stands for (include/phastft_hip.h, enum phast_status).
#[track_caller]
pub(crate) fn check(rc: c_int) {
    if rc != 0 {
        // SAFETY: both functions return static / thread-local NUL-terminated strings
        let msg = unsafe { CStr::from_ptr(phast_strerror(rc)) }.to_string_lossy();
        if rc >= 13 {
            let hip = unsafe { CStr::from_ptr(phast_last_hip_error()) }.to_string_lossy();
            panic!("{msg}: {hip}");
        }
        panic!("{msg}");
    }
}
