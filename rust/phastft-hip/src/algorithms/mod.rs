//! `phastft::algorithms` -- private in the reference unless feature `bench-internals` is on (lib.rs:20-23);
//! the same visibility here, so `phastft::algorithms::bravo::bit_rev_bravo_f64` resolves exactly when it
//! does upstream (benches/bit_reversal.rs:3).
pub mod bravo;
pub mod conv;
pub mod convnd;
pub mod czt;
pub mod dit;
pub mod mdct;
pub mod psd;
pub mod resample;
pub mod channelizer;
pub mod synthesizer;
pub mod cwt;
pub mod dwt;
pub mod lomb;
pub mod nufft;
pub mod nufft2d;
pub mod nufft3d;
pub mod nufft_t3;
pub mod r2c;
pub mod r2r;
pub mod stft;
