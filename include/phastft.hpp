// phastft.hpp -- header-only C++17 host side above the C ABI (phastft_hip.h), mirroring PhastFT 0.3.0's
// public Rust API for the planar FFT path: same names, argument meaning and error behaviour.
//
//   Rust (reference file:line)                               C++ (namespace phastft)
//   ---------------------------------------------------      -------------------------------------------
//   planner::Direction {Forward = 1, Reverse = -1}  planner.rs:10    enum class Direction
//   planner::PlannerMode {Heuristic, Tune}          planner.rs:24    enum class PlannerMode
//   options::Options, Options::guess_options        options.rs:10    struct Options, Options::guess_options
//   PlannerDit64/32::{new, with_mode}               planner.rs:55    class PlannerDit64/32 (ctor, with_mode; + tune, wisdom_*)
//   PlannerR2c64/32::new                            planner.rs:194   class PlannerR2c64/32
//   fft_64_dit, fft_32_dit                          lib.rs:180,223   fft_64_dit, fft_32_dit
//   fft_*_dit_with_planner[_and_opts]               lib.rs:143,186; dit.rs:263,338
//   r2c_fft_f64/f32[_with_planner]                  r2c.rs:521,535,598,607
//   c2r_fft_f64/f32[_with_planner[_and_scratch]]    r2c.rs:695,710,740,804,813,836
//   fft_*_interleaved[_with_planner[_and_opts]]     lib.rs:50,87,120 (feature complex-nums)
//   bit_rev_bravo_f64/f32                           bravo.rs:303,317 (feature bench-internals)
//   deinterleave[_complex64/32], combine_re_im      complex_nums.rs:11,25,37,47 (feature bench-internals)
//   (none: powers of two only upstream)                      class PlannerAny64/32, fft_64/32_any[_with_planner] -- any N >= 1
//   (none: r2c.rs takes powers of two >= 4)                  class PlannerR2cAny64/32, r2c_fft_f64/f32_any[_with_planner],
//                                                            c2r_fft_f64/f32_any[_with_planner] -- any N >= 1
//   (none: no real-to-real transforms upstream)              class PlannerDct64/32, dct_f64/f32[_with_planner],
//                                                            dst_f64/f32[_with_planner], enum Norm -- types II and III, any N >= 1
//   (none: no short-time transforms upstream)                class PlannerStft64/32, stft_f64/f32_with_planner,
//                                                            istft_f64/f32_with_planner, enum PadMode -- torch.stft / istft
//   (none: no lapped transforms upstream)                    class PlannerMdct64/32, mdct_f64/f32_with_planner,
//                                                            imdct_f64/f32_with_planner
//   (none: no spectral estimation upstream)                  class PlannerPsd64/32, psd_f64/f32_with_planner,
//                                                            csd_f64/f32_with_planner
//   (none: no spectra of uneven samples upstream)            class PlannerLomb64/32, lombscargle_f64/f32_with_planner,
//                                                            enum LombNorm -- scipy.signal.lombscargle
//   (none: no filter banks upstream)                         class PlannerChannelizer64/32, channelize_f64/f32_with_planner -- the
//                                                            polyphase channelizer (uniform DFT analysis filter bank)
//   (none: no filter banks upstream)                         class PlannerSynthesizer64/32, synthesize_f64/f32_with_planner -- the
//                                                            polyphase synthesis bank, the channelizer's inverse
//   (none: no wavelets upstream)                             class PlannerCwt64/32, cwt_64/32_with_planner, enum CwtFamily, CwtNorm --
//                                                            the continuous wavelet transform and the analytic signal
//   (none: no wavelets upstream)                             class PlannerDwt64/32, wavedec_f64/f32_with_planner,
//                                                            waverec_f64/f32_with_planner, enum DwtMode -- the discrete wavelet
//                                                            transform and its inverse (pywt.wavedec / waverec)
//   (none: no sample-rate conversion upstream)               class PlannerUpfirdn64/32, upfirdn_f64/f32_with_planner -- the polyphase
//                                                            FIR of scipy.signal.upfirdn; class PlannerResample64/32,
//                                                            resample_f64/f32_with_planner -- scipy.signal.resample
//   (none: no convolution upstream)                          class PlannerConv64/32, conv_f64/f32_with_planner, enum ConvMode --
//                                                            scipy.signal.convolve / correlate by overlap-save
//   (none: no convolution upstream)                          class PlannerConvNd64/32, convnd_f64/f32_with_planner -- the same of
//                                                            arrays of rank 1 .. 3, by overlap-save along every axis
//   (none: whole spectra only upstream)                      class PlannerCzt64/32, czt_64/32[_with_planner] -- the chirp-Z transform
//                                                            on the unit circle (scipy.signal.czt / zoom_fft)
//   (none: samples on a grid only upstream)                  class PlannerNufft64/32, nufft1_64/32[_with_planner],
//                                                            nufft2_64/32[_with_planner] -- non-uniform FFTs of types 1 and 2
//   (none: samples on a grid only upstream)                  class PlannerNufft2d64/32, nufft2d1_64/32[_with_planner],
//                                                            nufft2d2_64/32[_with_planner] -- the same in two dimensions
//   (none: samples on a grid only upstream)                  class PlannerNufft3d64/32, nufft3d1_64/32[_with_planner],
//                                                            nufft3d2_64/32[_with_planner] -- the same in three dimensions;
//                                                            all three: from_device / set_points_dev -- points in device memory
//   (none: samples on a grid only upstream)                  class PlannerNufftT3_64/32, nufft3_64/32[_with_planner] -- the
//                                                            non-uniform FFT of type 3 (points to arbitrary frequencies)
//   (none: one axis only upstream)                           class PlannerNd64/32, PlannerR2cNd64/32, fft_64/32_nd[_with_planner],
//                                                            r2c_fft_f64/f32_nd[...], c2r_fft_f64/f32_nd[...] -- every axis
//
// A Rust `&mut [T]` is a (pointer, length) pair here -- `Slice<T>` converts from std::vector / std::array /
// raw pointer + length.  Where the reference panics (`assert!`), these functions throw `phastft::Panic` whose
// what() is the reference's panic message; HIP failures throw `phastft::HipError`.  There is no CPU fallback.
#ifndef PHASTFT_HPP
#define PHASTFT_HPP

#include <complex>
#include <cstddef>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "phastft_hip.h"

namespace phastft {

struct Panic : std::logic_error {
    int code;
    Panic(int c, const std::string &m) : std::logic_error(m), code(c) {}
};
struct HipError : std::runtime_error {
    int code;
    HipError(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};

inline void check(int rc) {
    if (rc == PHAST_OK) return;
    if (rc == PHAST_ERR_ALLOC || rc == PHAST_ERR_HIP || rc == PHAST_ERR_NO_DEVICE)
        throw HipError(rc, std::string(phast_strerror(rc)) + ": " + phast_last_hip_error());
    throw Panic(rc, phast_strerror(rc));
}

enum class Direction : int { Forward = PHAST_FORWARD, Reverse = PHAST_REVERSE };   // planner.rs:10-16
enum class PlannerMode : int { Heuristic = PHAST_MODE_HEURISTIC, Tune = PHAST_MODE_TUNE };  // planner.rs:24-32

// options.rs:8-43 -- CPU threading knobs, carried for source compatibility, ignored on the GPU
struct Options {
    bool multithreaded_bit_reversal = false;
    std::size_t smallest_parallel_chunk_size = 16384;
    static Options guess_options(std::size_t input_size) {
        phast_options o;
        check(phast_options_guess(input_size, &o));
        return Options{o.multithreaded_bit_reversal != 0, o.smallest_parallel_chunk_size};
    }
    phast_options to_c() const { return phast_options{multithreaded_bit_reversal ? 1 : 0, smallest_parallel_chunk_size}; }
};

// the Rust slice: pointer + length
template <typename T> struct Slice {
    T *ptr;
    std::size_t len;
    Slice(T *p, std::size_t n) : ptr(p), len(n) {}
    template <typename A> Slice(std::vector<T, A> &v) : ptr(v.data()), len(v.size()) {}
    template <typename U, typename A, typename = std::enable_if_t<std::is_same<const U, T>::value>>
    Slice(const std::vector<U, A> &v) : ptr(v.data()), len(v.size()) {}
};

#define PHASTFT_PLANNER(NAME, CT, NEW_EXPR, FREE)                                   \
    class NAME {                                                                    \
      public:                                                                       \
        NAME(const NAME &) = delete;                                                \
        NAME &operator=(const NAME &) = delete;                                     \
        NAME(NAME &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }                      \
        ~NAME() {                                                                   \
            if (h_) FREE(h_);                                                       \
        }                                                                           \
        const CT *get() const { return h_; }                                        \
        CT *get() { return h_; }                                                    \
        NEW_EXPR                                                                    \
      private:                                                                      \
        CT *h_ = nullptr;                                                           \
    };

// planner.rs:34-114
PHASTFT_PLANNER(PlannerDit64, phast_planner_dit64,
                explicit PlannerDit64(std::size_t num_points, PlannerMode mode = PlannerMode::Heuristic) {
                    check(phast_planner_dit64_with_mode(num_points, static_cast<int>(mode), &h_));
                } static PlannerDit64 with_mode(std::size_t n, PlannerMode mode) { return PlannerDit64(n, mode); }
                /* PlannerMode::Tune for another batch size / call kind (PHAST_TUNE_C2C, PHAST_TUNE_C2C_INTERLEAVED) */
                phast_tune_report tune(std::size_t batch = 1, int kind = PHAST_TUNE_C2C) {
                    phast_tune_report r{};
                    check(phast_planner_dit64_tune(h_, batch, kind, &r));
                    return r;
                },
                phast_planner_dit64_free)
PHASTFT_PLANNER(PlannerDit32, phast_planner_dit32,
                explicit PlannerDit32(std::size_t num_points, PlannerMode mode = PlannerMode::Heuristic) {
                    check(phast_planner_dit32_with_mode(num_points, static_cast<int>(mode), &h_));
                } static PlannerDit32 with_mode(std::size_t n, PlannerMode mode) { return PlannerDit32(n, mode); }
                /* PlannerMode::Tune for another batch size / call kind (PHAST_TUNE_C2C, PHAST_TUNE_C2C_INTERLEAVED) */
                phast_tune_report tune(std::size_t batch = 1, int kind = PHAST_TUNE_C2C) {
                    phast_tune_report r{};
                    check(phast_planner_dit32_tune(h_, batch, kind, &r));
                    return r;
                },
                phast_planner_dit32_free)
// planner.rs:164-212
PHASTFT_PLANNER(PlannerR2c64, phast_planner_r2c64,
                explicit PlannerR2c64(std::size_t n, PlannerMode mode = PlannerMode::Heuristic) {
                    check(phast_planner_r2c64_with_mode(n, static_cast<int>(mode), &h_));
                }
                phast_tune_report tune(std::size_t batch = 1, int kind = PHAST_TUNE_R2C) {
                    phast_tune_report r{};
                    check(phast_planner_r2c64_tune(h_, batch, kind, &r));
                    return r;
                },
                phast_planner_r2c64_free)
PHASTFT_PLANNER(PlannerR2c32, phast_planner_r2c32,
                explicit PlannerR2c32(std::size_t n, PlannerMode mode = PlannerMode::Heuristic) {
                    check(phast_planner_r2c32_with_mode(n, static_cast<int>(mode), &h_));
                }
                phast_tune_report tune(std::size_t batch = 1, int kind = PHAST_TUNE_R2C) {
                    phast_tune_report r{};
                    check(phast_planner_r2c32_tune(h_, batch, kind, &r));
                    return r;
                },
                phast_planner_r2c32_free)
#undef PHASTFT_PLANNER

// ---- wisdom: what PlannerMode::Tune measured, as text (csrc/wisdom.hpp; no reference counterpart) ----
inline std::string wisdom_export() {
    std::size_t need = 0;
    check(phast_wisdom_export(nullptr, 0, &need));
    std::string text(need, '\0');
    check(phast_wisdom_export(&text[0], need, nullptr));
    text.resize(need ? need - 1 : 0);
    return text;
}
inline void wisdom_import(const std::string &text) { check(phast_wisdom_import(text.c_str())); }
inline void wisdom_forget() { phast_wisdom_forget(); }

// ---- C2C, planar (lib.rs:143-226, algorithms/dit.rs:263,338) ----
inline void fft_64_dit_with_planner_and_opts(Slice<double> reals, Slice<double> imags, Direction direction,
                                             const PlannerDit64 &planner, const Options &opts) {
    const phast_options o = opts.to_c();
    check(phast_fft_64_dit_with_planner_and_opts(reals.ptr, reals.len, imags.ptr, imags.len, static_cast<int>(direction),
                                                 planner.get(), &o));
}
inline void fft_32_dit_with_planner_and_opts(Slice<float> reals, Slice<float> imags, Direction direction,
                                             const PlannerDit32 &planner, const Options &opts) {
    const phast_options o = opts.to_c();
    check(phast_fft_32_dit_with_planner_and_opts(reals.ptr, reals.len, imags.ptr, imags.len, static_cast<int>(direction),
                                                 planner.get(), &o));
}
inline void fft_64_dit_with_planner(Slice<double> reals, Slice<double> imags, Direction direction, const PlannerDit64 &planner) {
    check(phast_fft_64_dit_with_planner(reals.ptr, reals.len, imags.ptr, imags.len, static_cast<int>(direction), planner.get()));
}
inline void fft_32_dit_with_planner(Slice<float> reals, Slice<float> imags, Direction direction, const PlannerDit32 &planner) {
    check(phast_fft_32_dit_with_planner(reals.ptr, reals.len, imags.ptr, imags.len, static_cast<int>(direction), planner.get()));
}
inline void fft_64_dit(Slice<double> reals, Slice<double> imags, Direction direction) {
    check(phast_fft_64_dit(reals.ptr, reals.len, imags.ptr, imags.len, static_cast<int>(direction)));
}
inline void fft_32_dit(Slice<float> reals, Slice<float> imags, Direction direction) {
    check(phast_fft_32_dit(reals.ptr, reals.len, imags.ptr, imags.len, static_cast<int>(direction)));
}

// ---- C2C, interleaved Complex<T> (lib.rs:41-140) ----
inline void fft_64_interleaved(Slice<std::complex<double>> signal, Direction direction) {
    check(phast_fft_64_interleaved(reinterpret_cast<double *>(signal.ptr), signal.len, static_cast<int>(direction)));
}
inline void fft_32_interleaved(Slice<std::complex<float>> signal, Direction direction) {
    check(phast_fft_32_interleaved(reinterpret_cast<float *>(signal.ptr), signal.len, static_cast<int>(direction)));
}
inline void fft_64_interleaved_with_planner(Slice<std::complex<double>> signal, Direction direction, const PlannerDit64 &planner) {
    check(phast_fft_64_interleaved_with_planner(reinterpret_cast<double *>(signal.ptr), signal.len, static_cast<int>(direction),
                                                planner.get()));
}
inline void fft_32_interleaved_with_planner(Slice<std::complex<float>> signal, Direction direction, const PlannerDit32 &planner) {
    check(phast_fft_32_interleaved_with_planner(reinterpret_cast<float *>(signal.ptr), signal.len, static_cast<int>(direction),
                                                planner.get()));
}

inline void fft_64_interleaved_with_planner_and_opts(Slice<std::complex<double>> signal, Direction direction,
                                                     const PlannerDit64 &planner, const Options &opts) {  // lib.rs:50
    const phast_options o = opts.to_c();
    check(phast_fft_64_interleaved_with_planner_and_opts(reinterpret_cast<double *>(signal.ptr), signal.len,
                                                         static_cast<int>(direction), planner.get(), &o));
}
inline void fft_32_interleaved_with_planner_and_opts(Slice<std::complex<float>> signal, Direction direction,
                                                     const PlannerDit32 &planner, const Options &opts) {
    const phast_options o = opts.to_c();
    check(phast_fft_32_interleaved_with_planner_and_opts(reinterpret_cast<float *>(signal.ptr), signal.len,
                                                         static_cast<int>(direction), planner.get(), &o));
}

// ---- bit reversal (algorithms/bravo.rs:303,317) ----
// `n` is validated BEFORE it is used as a shift count (a shift by >= 64 is undefined; the reference asserts and panics)
inline void bit_rev_bravo_f64(Slice<double> data, unsigned n) {
    if (n >= 8 * sizeof(std::size_t) || data.len != (std::size_t(1) << n))
        throw Panic(PHAST_ERR_INVALID_ARG, "Data length must be 2^n");  // bravo.rs:228
    check(phast_bit_rev_f64(data.ptr, data.len, n));
}
inline void bit_rev_bravo_f32(Slice<float> data, unsigned n) {
    if (n >= 8 * sizeof(std::size_t) || data.len != (std::size_t(1) << n))
        throw Panic(PHAST_ERR_INVALID_ARG, "Data length must be 2^n");
    check(phast_bit_rev_f32(data.ptr, data.len, n));
}

// ---- Complex<T> <-> planes (complex_nums.rs:11-56; feature bench-internals) ----
template <typename T> struct ComplexNumsAbi;
template <> struct ComplexNumsAbi<double> {
    static int deinterleave(const double *in, std::size_t len, double *a, double *b) { return phast_deinterleave_f64(in, len, a, len / 2, b, len / 2); }
    static int combine(const double *re, std::size_t n, const double *im, std::size_t m, double *out) { return phast_combine_re_im_f64(re, n, im, m, out, 2 * n); }
};
template <> struct ComplexNumsAbi<float> {
    static int deinterleave(const float *in, std::size_t len, float *a, float *b) { return phast_deinterleave_f32(in, len, a, len / 2, b, len / 2); }
    static int combine(const float *re, std::size_t n, const float *im, std::size_t m, float *out) { return phast_combine_re_im_f32(re, n, im, m, out, 2 * n); }
};
// complex_nums.rs:11 -- [1, 2, 3, 4] -> ([1, 3], [2, 4]); an odd last element is dropped (chunks_exact(2))
template <typename T> inline std::pair<std::vector<T>, std::vector<T>> deinterleave(Slice<const T> input) {
    std::pair<std::vector<T>, std::vector<T>> out{std::vector<T>(input.len / 2), std::vector<T>(input.len / 2)};
    check(ComplexNumsAbi<T>::deinterleave(input.ptr, input.len, out.first.data(), out.second.data()));
    return out;
}
// complex_nums.rs:25,37 -- std::complex<T> is layout-compatible with T[2] (re, im), as Complex<T> is repr(C)
inline std::pair<std::vector<double>, std::vector<double>> deinterleave_complex64(Slice<const std::complex<double>> signal) {
    return deinterleave<double>(Slice<const double>(reinterpret_cast<const double *>(signal.ptr), 2 * signal.len));
}
inline std::pair<std::vector<float>, std::vector<float>> deinterleave_complex32(Slice<const std::complex<float>> signal) {
    return deinterleave<float>(Slice<const float>(reinterpret_cast<const float *>(signal.ptr), 2 * signal.len));
}
// complex_nums.rs:47 -- panics unless reals.len() == imags.len()
template <typename T> inline std::vector<std::complex<T>> combine_re_im(Slice<const T> reals, Slice<const T> imags) {
    if (reals.len != imags.len) throw Panic(PHAST_ERR_LEN_MISMATCH, "assertion `left == right` failed");  // complex_nums.rs:48
    std::vector<std::complex<T>> out(reals.len);
    check(ComplexNumsAbi<T>::combine(reals.ptr, reals.len, imags.ptr, imags.len, reinterpret_cast<T *>(out.data())));
    return out;
}

// ---- R2C / C2R (algorithms/r2c.rs:521-895) ----
inline void r2c_fft_f64_with_planner(Slice<const double> input_re, Slice<double> output_re, Slice<double> output_im,
                                     const PlannerR2c64 &planner) {
    check(phast_r2c_fft_f64_with_planner(input_re.ptr, input_re.len, output_re.ptr, output_re.len, output_im.ptr, output_im.len,
                                         planner.get()));
}
inline void r2c_fft_f32_with_planner(Slice<const float> input_re, Slice<float> output_re, Slice<float> output_im,
                                     const PlannerR2c32 &planner) {
    check(phast_r2c_fft_f32_with_planner(input_re.ptr, input_re.len, output_re.ptr, output_re.len, output_im.ptr, output_im.len,
                                         planner.get()));
}
inline void r2c_fft_f64(Slice<const double> input_re, Slice<double> output_re, Slice<double> output_im) {
    check(phast_r2c_fft_f64(input_re.ptr, input_re.len, output_re.ptr, output_re.len, output_im.ptr, output_im.len));
}
inline void r2c_fft_f32(Slice<const float> input_re, Slice<float> output_re, Slice<float> output_im) {
    check(phast_r2c_fft_f32(input_re.ptr, input_re.len, output_re.ptr, output_re.len, output_im.ptr, output_im.len));
}
inline void c2r_fft_f64_with_planner_and_scratch(Slice<const double> input_re, Slice<const double> input_im, Slice<double> output,
                                                 const PlannerR2c64 &planner, Slice<double> scratch_re, Slice<double> scratch_im) {
    check(phast_c2r_fft_f64_with_planner_and_scratch(input_re.ptr, input_re.len, input_im.ptr, input_im.len, output.ptr, output.len,
                                                     planner.get(), scratch_re.ptr, scratch_re.len, scratch_im.ptr, scratch_im.len));
}
inline void c2r_fft_f32_with_planner_and_scratch(Slice<const float> input_re, Slice<const float> input_im, Slice<float> output,
                                                 const PlannerR2c32 &planner, Slice<float> scratch_re, Slice<float> scratch_im) {
    check(phast_c2r_fft_f32_with_planner_and_scratch(input_re.ptr, input_re.len, input_im.ptr, input_im.len, output.ptr, output.len,
                                                     planner.get(), scratch_re.ptr, scratch_re.len, scratch_im.ptr, scratch_im.len));
}
inline void c2r_fft_f64_with_planner(Slice<const double> input_re, Slice<const double> input_im, Slice<double> output,
                                     const PlannerR2c64 &planner) {
    check(phast_c2r_fft_f64_with_planner(input_re.ptr, input_re.len, input_im.ptr, input_im.len, output.ptr, output.len, planner.get()));
}
inline void c2r_fft_f32_with_planner(Slice<const float> input_re, Slice<const float> input_im, Slice<float> output,
                                     const PlannerR2c32 &planner) {
    check(phast_c2r_fft_f32_with_planner(input_re.ptr, input_re.len, input_im.ptr, input_im.len, output.ptr, output.len, planner.get()));
}
inline void c2r_fft_f64(Slice<const double> input_re, Slice<const double> input_im, Slice<double> output) {
    check(phast_c2r_fft_f64(input_re.ptr, input_re.len, input_im.ptr, input_im.len, output.ptr, output.len));
}
inline void c2r_fft_f32(Slice<const float> input_re, Slice<const float> input_im, Slice<float> output) {
    check(phast_c2r_fft_f32(input_re.ptr, input_re.len, input_im.ptr, input_im.len, output.ptr, output.len));
}

// ---- complex transforms of any length N >= 1 (Bluestein; no reference counterpart: upstream takes powers of two only) ----
#define PHASTFT_PLANNER_ANY(NAME, CT, SFX)                                                                       \
    class NAME {                                                                                                 \
      public:                                                                                                    \
        explicit NAME(std::size_t n) { check(phast_planner_any##SFX##_new(n, &h_)); }                            \
        NAME(const NAME &) = delete;                                                                             \
        NAME &operator=(const NAME &) = delete;                                                                  \
        NAME(NAME &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }                                                   \
        ~NAME() {                                                                                                \
            if (h_) phast_planner_any##SFX##_free(h_);                                                           \
        }                                                                                                        \
        const CT *get() const { return h_; }                                                                     \
        std::string describe() const {                                                                           \
            std::string s(4096, '\0');                                                                           \
            check(phast_planner_any##SFX##_describe(h_, &s[0], s.size()));                                       \
            s.resize(s.find('\0'));                                                                              \
            return s;                                                                                            \
        }                                                                                                        \
        std::size_t device_bytes() const { return phast_planner_any##SFX##_device_bytes(h_); }                   \
        /* elements of T a _dev call of `batch` transforms works in (0 for a power of two) */                    \
        std::size_t workspace_len(std::size_t batch = 1) const { return phast_planner_any##SFX##_workspace_len(h_, batch); } \
                                                                                                                 \
      private:                                                                                                   \
        CT *h_ = nullptr;                                                                                        \
    };
PHASTFT_PLANNER_ANY(PlannerAny64, phast_planner_any64, 64)
PHASTFT_PLANNER_ANY(PlannerAny32, phast_planner_any32, 32)
#undef PHASTFT_PLANNER_ANY

inline void fft_64_any_with_planner(Slice<double> reals, Slice<double> imags, Direction direction, const PlannerAny64 &planner) {
    check(phast_fft_64_any_with_planner(reals.ptr, reals.len, imags.ptr, imags.len, static_cast<int>(direction), planner.get()));
}
inline void fft_32_any_with_planner(Slice<float> reals, Slice<float> imags, Direction direction, const PlannerAny32 &planner) {
    check(phast_fft_32_any_with_planner(reals.ptr, reals.len, imags.ptr, imags.len, static_cast<int>(direction), planner.get()));
}
inline void fft_64_any(Slice<double> reals, Slice<double> imags, Direction direction) {
    check(phast_fft_64_any(reals.ptr, reals.len, imags.ptr, imags.len, static_cast<int>(direction)));
}
inline void fft_32_any(Slice<float> reals, Slice<float> imags, Direction direction) {
    check(phast_fft_32_any(reals.ptr, reals.len, imags.ptr, imags.len, static_cast<int>(direction)));
}

// ---- real transforms of any length N >= 1 (no reference counterpart: r2c.rs takes powers of two >= 4) ----
#define PHASTFT_PLANNER_R2C_ANY(NAME, CT, SFX)                                                                   \
    class NAME {                                                                                                 \
      public:                                                                                                    \
        explicit NAME(std::size_t n) { check(phast_planner_r2c_any##SFX##_new(n, &h_)); }                        \
        NAME(const NAME &) = delete;                                                                             \
        NAME &operator=(const NAME &) = delete;                                                                  \
        NAME(NAME &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }                                                   \
        ~NAME() {                                                                                                \
            if (h_) phast_planner_r2c_any##SFX##_free(h_);                                                       \
        }                                                                                                        \
        const CT *get() const { return h_; }                                                                     \
        std::string describe() const {                                                                           \
            std::string s(4096, '\0');                                                                           \
            check(phast_planner_r2c_any##SFX##_describe(h_, &s[0], s.size()));                                   \
            s.resize(s.find('\0'));                                                                              \
            return s;                                                                                            \
        }                                                                                                        \
        std::size_t device_bytes() const { return phast_planner_r2c_any##SFX##_device_bytes(h_); }               \
        /* elements of T a _dev call of `batch` transforms works in (0 for a power of two, N = 1, 2) */          \
        std::size_t workspace_len(std::size_t batch = 1) const {                                                 \
            return phast_planner_r2c_any##SFX##_workspace_len(h_, batch);                                        \
        }                                                                                                        \
                                                                                                                 \
      private:                                                                                                   \
        CT *h_ = nullptr;                                                                                        \
    };
PHASTFT_PLANNER_R2C_ANY(PlannerR2cAny64, phast_planner_r2c_any64, 64)
PHASTFT_PLANNER_R2C_ANY(PlannerR2cAny32, phast_planner_r2c_any32, 32)
#undef PHASTFT_PLANNER_R2C_ANY

inline void r2c_fft_f64_any_with_planner(Slice<const double> input, Slice<double> output_re, Slice<double> output_im,
                                         const PlannerR2cAny64 &planner) {
    check(phast_r2c_fft_f64_any_with_planner(input.ptr, input.len, output_re.ptr, output_re.len, output_im.ptr, output_im.len,
                                             planner.get()));
}
inline void r2c_fft_f32_any_with_planner(Slice<const float> input, Slice<float> output_re, Slice<float> output_im,
                                         const PlannerR2cAny32 &planner) {
    check(phast_r2c_fft_f32_any_with_planner(input.ptr, input.len, output_re.ptr, output_re.len, output_im.ptr, output_im.len,
                                             planner.get()));
}
inline void r2c_fft_f64_any(Slice<const double> input, Slice<double> output_re, Slice<double> output_im) {
    check(phast_r2c_fft_f64_any(input.ptr, input.len, output_re.ptr, output_re.len, output_im.ptr, output_im.len));
}
inline void r2c_fft_f32_any(Slice<const float> input, Slice<float> output_re, Slice<float> output_im) {
    check(phast_r2c_fft_f32_any(input.ptr, input.len, output_re.ptr, output_re.len, output_im.ptr, output_im.len));
}
inline void c2r_fft_f64_any_with_planner(Slice<const double> input_re, Slice<const double> input_im, Slice<double> output,
                                         const PlannerR2cAny64 &planner) {
    check(phast_c2r_fft_f64_any_with_planner(input_re.ptr, input_re.len, input_im.ptr, input_im.len, output.ptr, output.len,
                                             planner.get()));
}
inline void c2r_fft_f32_any_with_planner(Slice<const float> input_re, Slice<const float> input_im, Slice<float> output,
                                         const PlannerR2cAny32 &planner) {
    check(phast_c2r_fft_f32_any_with_planner(input_re.ptr, input_re.len, input_im.ptr, input_im.len, output.ptr, output.len,
                                             planner.get()));
}
inline void c2r_fft_f64_any(Slice<const double> input_re, Slice<const double> input_im, Slice<double> output) {
    check(phast_c2r_fft_f64_any(input_re.ptr, input_re.len, input_im.ptr, input_im.len, output.ptr, output.len));
}
inline void c2r_fft_f32_any(Slice<const float> input_re, Slice<const float> input_im, Slice<float> output) {
    check(phast_c2r_fft_f32_any(input_re.ptr, input_re.len, input_im.ptr, input_im.len, output.ptr, output.len));
}

// ---- DCT / DST of types II and III, any length N >= 1 (no reference counterpart; scipy.fft.dct / dst) ----
enum class Norm : int { Backward = PHAST_NORM_BACKWARD, Ortho = PHAST_NORM_ORTHO, Forward = PHAST_NORM_FORWARD };
#define PHASTFT_PLANNER_DCT(NAME, CT, SFX)                                                                       \
    class NAME {                                                                                                 \
      public:                                                                                                    \
        explicit NAME(std::size_t n) { check(phast_planner_dct##SFX##_new(n, &h_)); }                            \
        NAME(const NAME &) = delete;                                                                             \
        NAME &operator=(const NAME &) = delete;                                                                  \
        NAME(NAME &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }                                                   \
        ~NAME() {                                                                                                \
            if (h_) phast_planner_dct##SFX##_free(h_);                                                           \
        }                                                                                                        \
        const CT *get() const { return h_; }                                                                     \
        std::string describe() const {                                                                           \
            std::string s(4096, '\0');                                                                           \
            check(phast_planner_dct##SFX##_describe(h_, &s[0], s.size()));                                       \
            s.resize(s.find('\0'));                                                                              \
            return s;                                                                                            \
        }                                                                                                        \
        std::size_t device_bytes() const { return phast_planner_dct##SFX##_device_bytes(h_); }                   \
        /* elements of T a _dev call of `batch` transforms works in (any length >= workspace_len(1) is legal) */ \
        std::size_t workspace_len(std::size_t batch = 1) const { return phast_planner_dct##SFX##_workspace_len(h_, batch); } \
                                                                                                                 \
      private:                                                                                                   \
        CT *h_ = nullptr;                                                                                        \
    };
PHASTFT_PLANNER_DCT(PlannerDct64, phast_planner_dct64, 64)
PHASTFT_PLANNER_DCT(PlannerDct32, phast_planner_dct32, 32)
#undef PHASTFT_PLANNER_DCT

#define PHASTFT_R2R(KIND, FS, T, P)                                                                              \
    inline void KIND##_##FS(Slice<const T> input, Slice<T> output, int type = 2, Norm norm = Norm::Backward) {   \
        check(phast_##KIND##_##FS(input.ptr, input.len, output.ptr, output.len, type, static_cast<int>(norm)));  \
    }                                                                                                            \
    inline void KIND##_##FS##_with_planner(Slice<const T> input, Slice<T> output, const P &planner, int type = 2, \
                                           Norm norm = Norm::Backward) {                                         \
        check(phast_##KIND##_##FS##_with_planner(input.ptr, input.len, output.ptr, output.len, type,             \
                                                 static_cast<int>(norm), planner.get()));                        \
    }
PHASTFT_R2R(dct, f64, double, PlannerDct64)
PHASTFT_R2R(dct, f32, float, PlannerDct32)
PHASTFT_R2R(dst, f64, double, PlannerDct64)
PHASTFT_R2R(dst, f32, float, PlannerDct32)
#undef PHASTFT_R2R

// ---- the short-time Fourier transform and its inverse (no reference counterpart; torch.stft / torch.istft(length = L)) ----
enum class PadMode : int { Reflect = PHAST_PAD_REFLECT, Zero = PHAST_PAD_ZERO };
#define PHASTFT_PLANNER_STFT(NAME, CT, SFX, T)                                                                   \
    class NAME {                                                                                                 \
      public:                                                                                                    \
        /* `window`: n_fft values, or empty for all ones */                                                      \
        NAME(std::size_t signal_len, std::size_t n_fft, std::size_t hop, Slice<const T> window = Slice<const T>(nullptr, 0), \
             bool center = true, PadMode pad_mode = PadMode::Reflect) {                                          \
            if (window.len && window.len != n_fft) check(PHAST_ERR_INVALID_ARG);                                 \
            check(phast_planner_stft##SFX##_new(signal_len, n_fft, hop, window.len ? window.ptr : nullptr, center ? 1 : 0, \
                                                static_cast<int>(pad_mode), &h_));                               \
        }                                                                                                        \
        NAME(const NAME &) = delete;                                                                             \
        NAME &operator=(const NAME &) = delete;                                                                  \
        NAME(NAME &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }                                                   \
        ~NAME() {                                                                                                \
            if (h_) phast_planner_stft##SFX##_free(h_);                                                          \
        }                                                                                                        \
        const CT *get() const { return h_; }                                                                     \
        std::string describe() const {                                                                           \
            std::string s(4096, '\0');                                                                           \
            check(phast_planner_stft##SFX##_describe(h_, &s[0], s.size()));                                      \
            s.resize(s.find('\0'));                                                                              \
            return s;                                                                                            \
        }                                                                                                        \
        std::size_t device_bytes() const { return phast_planner_stft##SFX##_device_bytes(h_); }                  \
        std::size_t frames() const { return phast_planner_stft##SFX##_frames(h_); }                              \
        std::size_t bins() const { return phast_planner_stft##SFX##_bins(h_); }                                  \
        /* the minimum of sum_f w^2 over the samples some frame holds: the inverse needs more than 1e-11 */      \
        double envelope_min() const { return phast_planner_stft##SFX##_envelope_min(h_); }                       \
        /* elements of T a _dev call of `batch` signals works in; workspace_min: the least a call runs in */     \
        std::size_t workspace_len(std::size_t batch = 1) const { return phast_planner_stft##SFX##_workspace_len(h_, batch); } \
        std::size_t workspace_min(bool inverse = false) const { return phast_planner_stft##SFX##_workspace_min(h_, inverse); } \
                                                                                                                 \
      private:                                                                                                   \
        CT *h_ = nullptr;                                                                                        \
    };
PHASTFT_PLANNER_STFT(PlannerStft64, phast_planner_stft64, 64, double)
PHASTFT_PLANNER_STFT(PlannerStft32, phast_planner_stft32, 32, float)
#undef PHASTFT_PLANNER_STFT

// one host signal of L samples <-> dense planes of frames * bins (frame-major); blocking
#define PHASTFT_STFT(FS, T, P)                                                                                   \
    inline void stft_##FS##_with_planner(Slice<const T> signal, Slice<T> output_re, Slice<T> output_im, const P &planner) { \
        check(phast_stft_##FS##_with_planner(signal.ptr, signal.len, output_re.ptr, output_re.len, output_im.ptr, \
                                             output_im.len, planner.get()));                                     \
    }                                                                                                            \
    inline void istft_##FS##_with_planner(Slice<const T> input_re, Slice<const T> input_im, Slice<T> signal, const P &planner) { \
        check(phast_istft_##FS##_with_planner(input_re.ptr, input_re.len, input_im.ptr, input_im.len, signal.ptr, \
                                              signal.len, planner.get()));                                       \
    }
PHASTFT_STFT(f64, double, PlannerStft64)
PHASTFT_STFT(f32, float, PlannerStft32)
#undef PHASTFT_STFT

// ---- the modified discrete cosine transform and its inverse (no reference counterpart, and none in torch or scipy) ----
#define PHASTFT_PLANNER_MDCT(NAME, CT, SFX, T)                                                                   \
    class NAME {                                                                                                 \
      public:                                                                                                    \
        /* `n` coefficients (even) per frame of 2 n samples; `window`: 2 n values, or empty for the sine window */ \
        NAME(std::size_t signal_len, std::size_t n, Slice<const T> window = Slice<const T>(nullptr, 0), bool padded = true) { \
            if (window.len && window.len != 2 * n) check(PHAST_ERR_INVALID_ARG);                                 \
            check(phast_planner_mdct##SFX##_new(signal_len, n, window.len ? window.ptr : nullptr, padded ? 1 : 0, &h_)); \
        }                                                                                                        \
        NAME(const NAME &) = delete;                                                                             \
        NAME &operator=(const NAME &) = delete;                                                                  \
        NAME(NAME &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }                                                   \
        ~NAME() {                                                                                                \
            if (h_) phast_planner_mdct##SFX##_free(h_);                                                          \
        }                                                                                                        \
        const CT *get() const { return h_; }                                                                     \
        std::string describe() const {                                                                           \
            std::string s(4096, '\0');                                                                           \
            check(phast_planner_mdct##SFX##_describe(h_, &s[0], s.size()));                                      \
            s.resize(s.find('\0'));                                                                              \
            return s;                                                                                            \
        }                                                                                                        \
        std::size_t device_bytes() const { return phast_planner_mdct##SFX##_device_bytes(h_); }                  \
        std::size_t frames() const { return phast_planner_mdct##SFX##_frames(h_); }                              \
        /* how far the window is from perfect reconstruction: 0 for sine, Vorbis and Kaiser-Bessel-derived windows */ \
        double tdac_defect() const { return phast_planner_mdct##SFX##_tdac_defect(h_); }                         \
        /* elements of T a _dev call of `batch` signals works in; workspace_min: the least a call runs in */     \
        std::size_t workspace_len(std::size_t batch = 1) const { return phast_planner_mdct##SFX##_workspace_len(h_, batch); } \
        std::size_t workspace_min(bool inverse = false) const { return phast_planner_mdct##SFX##_workspace_min(h_, inverse); } \
                                                                                                                 \
      private:                                                                                                   \
        CT *h_ = nullptr;                                                                                        \
    };
PHASTFT_PLANNER_MDCT(PlannerMdct64, phast_planner_mdct64, 64, double)
PHASTFT_PLANNER_MDCT(PlannerMdct32, phast_planner_mdct32, 32, float)
#undef PHASTFT_PLANNER_MDCT

// one host signal of L samples <-> frames * n coefficients (frame-major); blocking
#define PHASTFT_MDCT(FS, T, P)                                                                                   \
    inline void mdct_##FS##_with_planner(Slice<const T> signal, Slice<T> coefs, const P &planner) {              \
        check(phast_mdct_##FS##_with_planner(signal.ptr, signal.len, coefs.ptr, coefs.len, planner.get()));      \
    }                                                                                                            \
    inline void imdct_##FS##_with_planner(Slice<const T> coefs, Slice<T> signal, const P &planner) {             \
        check(phast_imdct_##FS##_with_planner(coefs.ptr, coefs.len, signal.ptr, signal.len, planner.get()));     \
    }
PHASTFT_MDCT(f64, double, PlannerMdct64)
PHASTFT_MDCT(f32, float, PlannerMdct32)
#undef PHASTFT_MDCT

// ---- Welch spectral estimation (no reference counterpart; scipy.signal.welch / csd / spectrogram) ----
enum class Detrend : int { None = PHAST_DETREND_NONE, Constant = PHAST_DETREND_CONSTANT };
enum class PsdScaling : int { Density = PHAST_PSD_DENSITY, Spectrum = PHAST_PSD_SPECTRUM };
#define PHASTFT_PLANNER_PSD(NAME, CT, SFX, T)                                                                    \
    class NAME {                                                                                                 \
      public:                                                                                                    \
        /* segments of `nperseg` samples `hop` apart, zero-padded to `nfft`; `window`: nperseg doubles, or empty for Hann */ \
        NAME(std::size_t signal_len, std::size_t nperseg, std::size_t hop, std::size_t nfft,                     \
             Slice<const double> window = Slice<const double>(nullptr, 0), Detrend detrend = Detrend::Constant,  \
             PsdScaling scaling = PsdScaling::Density, double fs = 1.0) {                                        \
            if (window.len && window.len != nperseg) check(PHAST_ERR_INVALID_ARG);                               \
            check(phast_planner_psd##SFX##_new(signal_len, nperseg, hop, nfft, window.len ? window.ptr : nullptr, \
                                               static_cast<int>(detrend), static_cast<int>(scaling), fs, &h_));  \
        }                                                                                                        \
        NAME(const NAME &) = delete;                                                                             \
        NAME &operator=(const NAME &) = delete;                                                                  \
        NAME(NAME &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }                                                   \
        ~NAME() {                                                                                                \
            if (h_) phast_planner_psd##SFX##_free(h_);                                                           \
        }                                                                                                        \
        const CT *get() const { return h_; }                                                                     \
        std::string describe() const {                                                                           \
            std::string s(4096, '\0');                                                                           \
            check(phast_planner_psd##SFX##_describe(h_, &s[0], s.size()));                                       \
            s.resize(s.find('\0'));                                                                              \
            return s;                                                                                            \
        }                                                                                                        \
        std::size_t device_bytes() const { return phast_planner_psd##SFX##_device_bytes(h_); }                   \
        std::size_t segments() const { return phast_planner_psd##SFX##_segments(h_); }                           \
        std::size_t bins() const { return phast_planner_psd##SFX##_bins(h_); }                                   \
        /* frames per slab of the sum over frames: a function of segments() and bins() alone */                  \
        std::size_t slab() const { return phast_planner_psd##SFX##_slab(h_); }                                   \
        /* elements of T a _dev call of `batch` signals (cross: pairs) works in; workspace_min: the least a call runs in */ \
        std::size_t workspace_len(std::size_t batch = 1, bool cross = false) const {                             \
            return phast_planner_psd##SFX##_workspace_len(h_, batch, cross);                                     \
        }                                                                                                        \
        std::size_t workspace_min(bool cross = false) const { return phast_planner_psd##SFX##_workspace_min(h_, cross); } \
                                                                                                                 \
      private:                                                                                                   \
        CT *h_ = nullptr;                                                                                        \
    };
PHASTFT_PLANNER_PSD(PlannerPsd64, phast_planner_psd64, 64, double)
PHASTFT_PLANNER_PSD(PlannerPsd32, phast_planner_psd32, 32, float)
#undef PHASTFT_PLANNER_PSD

// one host signal (csd: one pair) of L samples -> bins values, or segments * bins frame-major for average = false; blocking.
// csd: P_xy = <conj(X) Y> in two planes; pxx and pyy may be empty
#define PHASTFT_PSD(FS, T, P)                                                                                    \
    inline void psd_##FS##_with_planner(Slice<const T> signal, Slice<T> out, const P &planner, bool average = true) { \
        check(phast_psd_##FS##_with_planner(signal.ptr, signal.len, out.ptr, out.len, average ? 1 : 0, planner.get())); \
    }                                                                                                            \
    inline void csd_##FS##_with_planner(Slice<const T> x, Slice<const T> y, Slice<T> out_re, Slice<T> out_im, const P &planner, \
                                        Slice<T> pxx = Slice<T>(nullptr, 0), Slice<T> pyy = Slice<T>(nullptr, 0), \
                                        bool average = true) {                                                   \
        check(phast_csd_##FS##_with_planner(x.ptr, x.len, y.ptr, y.len, out_re.ptr, out_re.len, out_im.ptr, out_im.len, \
                                            pxx.len ? pxx.ptr : nullptr, pxx.len, pyy.len ? pyy.ptr : nullptr, pyy.len, \
                                            average ? 1 : 0, planner.get()));                                    \
    }
PHASTFT_PSD(f64, double, PlannerPsd64)
PHASTFT_PSD(f32, float, PlannerPsd32)
#undef PHASTFT_PSD

// ---- the Lomb-Scargle periodogram of unevenly spaced samples (no reference counterpart; scipy.signal.lombscargle) ----
enum class LombNorm : int { Power = PHAST_LOMB_POWER, Normalize = PHAST_LOMB_NORMALIZE, Amplitude = PHAST_LOMB_AMPLITUDE };
#define PHASTFT_PLANNER_LOMB(NAME, CT, SFX, T)                                                                   \
    class NAME {                                                                                                 \
      public:                                                                                                    \
        /* M times, K frequencies in cycles per unit of time; `weights`: M doubles >= 0, or empty for equal weights */ \
        NAME(Slice<const double> times, Slice<const double> freqs, Slice<const double> weights = Slice<const double>(nullptr, 0), \
             bool floating_mean = false, double eps = sizeof(T) == 4 ? 1e-6 : 1e-12)                             \
            : m_(times.len), k_(freqs.len) {                                                                     \
            if (weights.len && weights.len != times.len) check(PHAST_ERR_INVALID_ARG);                           \
            check(phast_planner_lomb##SFX##_new(times.ptr, times.len, freqs.ptr, freqs.len,                      \
                                                weights.len ? weights.ptr : nullptr, floating_mean ? 1 : 0, eps, &h_)); \
        }                                                                                                        \
        NAME(const NAME &) = delete;                                                                             \
        NAME &operator=(const NAME &) = delete;                                                                  \
        NAME(NAME &&o) noexcept : h_(o.h_), m_(o.m_), k_(o.k_) { o.h_ = nullptr; }                               \
        ~NAME() {                                                                                                \
            if (h_) phast_planner_lomb##SFX##_free(h_);                                                          \
        }                                                                                                        \
        const CT *get() const { return h_; }                                                                     \
        std::string describe() const {                                                                           \
            std::string s(4096, '\0');                                                                           \
            check(phast_planner_lomb##SFX##_describe(h_, &s[0], s.size()));                                      \
            s.resize(s.find('\0'));                                                                              \
            return s;                                                                                            \
        }                                                                                                        \
        std::size_t points() const { return m_; }                                                                \
        std::size_t freqs() const { return k_; }                                                                 \
        std::size_t device_bytes() const { return phast_planner_lomb##SFX##_device_bytes(h_); }                  \
        /* points per slab of the two reductions: a function of points() alone */                                \
        std::size_t slab() const { return phast_planner_lomb##SFX##_slab(h_); }                                  \
        std::size_t grid_len() const { return phast_planner_lomb##SFX##_grid_len(h_); }                          \
        /* elements of T a _dev call of `batch` signals works in; workspace_min: the least a call runs in */     \
        std::size_t workspace_len(std::size_t batch = 1) const { return phast_planner_lomb##SFX##_workspace_len(h_, batch); } \
        std::size_t workspace_min() const { return phast_planner_lomb##SFX##_workspace_min(h_); }                \
                                                                                                                 \
      private:                                                                                                   \
        CT *h_ = nullptr;                                                                                        \
        std::size_t m_ = 0, k_ = 0;                                                                              \
    };
PHASTFT_PLANNER_LOMB(PlannerLomb64, phast_planner_lomb64, 64, double)
PHASTFT_PLANNER_LOMB(PlannerLomb32, phast_planner_lomb32, 32, float)
#undef PHASTFT_PLANNER_LOMB

// one host signal of M values -> K values; blocking.  Amplitude: the real parts into `out`, the imaginary parts into `out_im`
// (required for it, unused otherwise)
#define PHASTFT_LOMB(FS, T, P)                                                                                   \
    inline void lombscargle_##FS##_with_planner(Slice<const T> y, Slice<T> out, const P &planner,                \
                                                LombNorm normalize = LombNorm::Power, Slice<T> out_im = Slice<T>(nullptr, 0)) { \
        check(phast_lombscargle_##FS##_with_planner(y.ptr, y.len, out.ptr, out.len, out_im.len ? out_im.ptr : nullptr, \
                                                    out_im.len, static_cast<int>(normalize), planner.get()));    \
    }
PHASTFT_LOMB(f64, double, PlannerLomb64)
PHASTFT_LOMB(f32, float, PlannerLomb32)
#undef PHASTFT_LOMB

// ---- sample-rate conversion (no reference counterpart; scipy.signal.upfirdn / resample_poly / decimate / resample) ----
#define PHASTFT_PLANNER_UPFIRDN(NAME, CT, SFX, T)                                                                \
    class NAME {                                                                                                 \
      public:                                                                                                    \
        /* upfirdn(taps, x, up, down) of signals of signal_len samples: the out_len samples from `first` on (out_len = 0: up to \
           full_len; first + out_len may pass it: zeros).  up and down are used as given */                      \
        NAME(std::size_t signal_len, Slice<const T> taps, std::size_t up = 1, std::size_t down = 1, std::size_t first = 0, \
             std::size_t out_len = 0) {                                                                          \
            check(phast_planner_upfirdn##SFX##_new(signal_len, taps.ptr, taps.len, up, down, first, out_len, &h_)); \
        }                                                                                                        \
        NAME(const NAME &) = delete;                                                                             \
        NAME &operator=(const NAME &) = delete;                                                                  \
        NAME(NAME &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }                                                   \
        ~NAME() {                                                                                                \
            if (h_) phast_planner_upfirdn##SFX##_free(h_);                                                       \
        }                                                                                                        \
        const CT *get() const { return h_; }                                                                     \
        std::string describe() const {                                                                           \
            std::string s(4096, '\0');                                                                           \
            check(phast_planner_upfirdn##SFX##_describe(h_, &s[0], s.size()));                                   \
            s.resize(s.find('\0'));                                                                              \
            return s;                                                                                            \
        }                                                                                                        \
        std::size_t device_bytes() const { return phast_planner_upfirdn##SFX##_device_bytes(h_); }               \
        std::size_t out_len() const { return phast_planner_upfirdn##SFX##_out_len(h_); }                         \
        std::size_t full_len() const { return phast_planner_upfirdn##SFX##_full_len(h_); }                       \
        /* outputs per workgroup and taps of a phase per LDS chunk: functions of (K, up, down) alone */          \
        std::size_t tile() const { return phast_planner_upfirdn##SFX##_tile(h_); }                               \
        std::size_t chunk() const { return phast_planner_upfirdn##SFX##_chunk(h_); }                             \
        /* 0: the kernel needs no workspace */                                                                   \
        std::size_t workspace_len(std::size_t batch = 1) const { return phast_planner_upfirdn##SFX##_workspace_len(h_, batch); } \
                                                                                                                 \
      private:                                                                                                   \
        CT *h_ = nullptr;                                                                                        \
    };
PHASTFT_PLANNER_UPFIRDN(PlannerUpfirdn64, phast_planner_upfirdn64, 64, double)
PHASTFT_PLANNER_UPFIRDN(PlannerUpfirdn32, phast_planner_upfirdn32, 32, float)
#undef PHASTFT_PLANNER_UPFIRDN
#define PHASTFT_PLANNER_RESAMPLE(NAME, CT, SFX)                                                                  \
    class NAME {                                                                                                 \
      public:                                                                                                    \
        /* scipy.signal.resample(x, num) of real signals of signal_len samples (Fourier method, no window) */    \
        NAME(std::size_t signal_len, std::size_t num) : num_(num) { check(phast_planner_resample##SFX##_new(signal_len, num, &h_)); } \
        NAME(const NAME &) = delete;                                                                             \
        NAME &operator=(const NAME &) = delete;                                                                  \
        NAME(NAME &&o) noexcept : h_(o.h_), num_(o.num_) { o.h_ = nullptr; }                                     \
        ~NAME() {                                                                                                \
            if (h_) phast_planner_resample##SFX##_free(h_);                                                      \
        }                                                                                                        \
        const CT *get() const { return h_; }                                                                     \
        std::string describe() const {                                                                           \
            std::string s(4096, '\0');                                                                           \
            check(phast_planner_resample##SFX##_describe(h_, &s[0], s.size()));                                  \
            s.resize(s.find('\0'));                                                                              \
            return s;                                                                                            \
        }                                                                                                        \
        std::size_t device_bytes() const { return phast_planner_resample##SFX##_device_bytes(h_); }              \
        std::size_t out_len() const { return num_; }                                                             \
        /* elements of T a _dev call of `batch` signals works in; workspace_min: the least a call runs in */     \
        std::size_t workspace_len(std::size_t batch = 1) const { return phast_planner_resample##SFX##_workspace_len(h_, batch); } \
        std::size_t workspace_min() const { return phast_planner_resample##SFX##_workspace_min(h_); }            \
                                                                                                                 \
      private:                                                                                                   \
        CT *h_ = nullptr;                                                                                        \
        std::size_t num_ = 0;                                                                                    \
    };
PHASTFT_PLANNER_RESAMPLE(PlannerResample64, phast_planner_resample64, 64)
PHASTFT_PLANNER_RESAMPLE(PlannerResample32, phast_planner_resample32, 32)
#undef PHASTFT_PLANNER_RESAMPLE

// one host signal of L samples -> its out_len() output samples; blocking
#define PHASTFT_RESAMPLE(NAME, FS, T, P)                                                                         \
    inline void NAME##_##FS##_with_planner(Slice<const T> signal, Slice<T> output, const P &planner) {           \
        check(phast_##NAME##_##FS##_with_planner(signal.ptr, signal.len, output.ptr, output.len, planner.get())); \
    }
PHASTFT_RESAMPLE(upfirdn, f64, double, PlannerUpfirdn64)
PHASTFT_RESAMPLE(upfirdn, f32, float, PlannerUpfirdn32)
PHASTFT_RESAMPLE(resample, f64, double, PlannerResample64)
PHASTFT_RESAMPLE(resample, f32, float, PlannerResample32)
#undef PHASTFT_RESAMPLE

// ---- discrete wavelet transform and its inverse (no reference counterpart; pywt.dwt / idwt / wavedec / waverec) ----
// the extension modes of include/phastft_hip.h (PHAST_DWT_*): PyWavelets' definitions
enum class DwtMode : int { Zero = 0, Constant = 1, Symmetric = 2, Reflect = 3, Periodic = 4, Periodization = 5 };
#define PHASTFT_PLANNER_DWT(NAME, CT, SFX, T)                                                                    \
    class NAME {                                                                                                 \
      public:                                                                                                    \
        /* pywt.wavedec / waverec of real signals of signal_len samples with `level` levels (1 .. 32): the four filters of one\
           even length 2 .. 256, used as given.  A signal's result is the packed row [cA_J | cD_J | .. | cD_1] */\
        NAME(std::size_t signal_len, Slice<const T> dec_lo, Slice<const T> dec_hi, Slice<const T> rec_lo,        \
             Slice<const T> rec_hi, std::size_t level = 1, DwtMode mode = DwtMode::Symmetric) {                  \
            if (dec_hi.len != dec_lo.len || rec_lo.len != dec_lo.len || rec_hi.len != dec_lo.len) check(PHAST_ERR_INVALID_ARG);\
            check(phast_planner_dwt##SFX##_new(signal_len, dec_lo.ptr, dec_hi.ptr, rec_lo.ptr, rec_hi.ptr, dec_lo.len, level,\
                                               static_cast<int>(mode), &h_));                                    \
        }                                                                                                        \
        NAME(const NAME &) = delete;                                                                             \
        NAME &operator=(const NAME &) = delete;                                                                  \
        NAME(NAME &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }                                                   \
        ~NAME() {                                                                                                \
            if (h_) phast_planner_dwt##SFX##_free(h_);                                                           \
        }                                                                                                        \
        const CT *get() const { return h_; }                                                                     \
        std::string describe() const {                                                                           \
            std::string s(4096, '\0');                                                                           \
            check(phast_planner_dwt##SFX##_describe(h_, &s[0], s.size()));                                       \
            s.resize(s.find('\0'));                                                                              \
            return s;                                                                                            \
        }                                                                                                        \
        std::size_t device_bytes() const { return phast_planner_dwt##SFX##_device_bytes(h_); }                   \
        /* elements of a packed row; n_l for 0 <= l <= J; where cD_l starts in the row for 1 <= l <= J (cA_J starts at 0) */\
        std::size_t coeff_len() const { return phast_planner_dwt##SFX##_coeff_len(h_); }                         \
        std::size_t level_len(std::size_t l) const { return phast_planner_dwt##SFX##_level_len(h_, l); }         \
        std::size_t level_offset(std::size_t l) const { return phast_planner_dwt##SFX##_level_offset(h_, l); }   \
        /* coefficient indices / output pairs per workgroup */                                                   \
        std::size_t tile() const { return phast_planner_dwt##SFX##_tile(h_); }                                   \
        /* elements of T a _dev call of `batch` signals works in (0 for one level); workspace_min: the least a call runs in */\
        std::size_t workspace_len(std::size_t batch = 1) const { return phast_planner_dwt##SFX##_workspace_len(h_, batch); }\
        std::size_t workspace_min() const { return phast_planner_dwt##SFX##_workspace_min(h_); }                 \
                                                                                                                 \
      private:                                                                                                   \
        CT *h_ = nullptr;                                                                                        \
    };
PHASTFT_PLANNER_DWT(PlannerDwt64, phast_planner_dwt64, 64, double)
PHASTFT_PLANNER_DWT(PlannerDwt32, phast_planner_dwt32, 32, float)
#undef PHASTFT_PLANNER_DWT

// one host signal of L samples -> its packed row of coeff_len() coefficients, and back; blocking
#define PHASTFT_DWT(FS, T, P)                                                                                    \
    inline void wavedec_##FS##_with_planner(Slice<const T> signal, Slice<T> coeffs, const P &planner) {          \
        check(phast_wavedec_##FS##_with_planner(signal.ptr, signal.len, coeffs.ptr, coeffs.len, planner.get())); \
    }                                                                                                            \
    inline void waverec_##FS##_with_planner(Slice<const T> coeffs, Slice<T> signal, const P &planner) {          \
        check(phast_waverec_##FS##_with_planner(coeffs.ptr, coeffs.len, signal.ptr, signal.len, planner.get())); \
    }
PHASTFT_DWT(f64, double, PlannerDwt64)
PHASTFT_DWT(f32, float, PlannerDwt32)
#undef PHASTFT_DWT

// ---- polyphase filter-bank channelizer (no reference counterpart; cuSignal's channelize_poly) ----
#define PHASTFT_PLANNER_CHANNELIZER(NAME, CT, SFX, T)                                                            \
    class NAME {                                                                                                 \
      public:                                                                                                    \
        /* `channels` equally spaced channels of signals of signal_len samples, each filtered with the real taps and \
           decimated by `hop` (0: channels, critically sampled), zero extension: the out_frames frames from first_frame on \
           (out_frames = 0: up to full_frames; the window may pass it: zeros).  complex_input: the signals are (re, im) \
           planes and a frame has `channels` bins; real signals give channels / 2 + 1 */                        \
        NAME(std::size_t signal_len, Slice<const T> taps, std::size_t channels, std::size_t hop = 0, std::size_t first_frame = 0, \
             std::size_t out_frames = 0, bool complex_input = false) {                                           \
            check(phast_planner_channelizer##SFX##_new(signal_len, taps.ptr, taps.len, channels, hop ? hop : channels, first_frame, \
                                                       out_frames, complex_input ? 1 : 0, &h_));                 \
        }                                                                                                        \
        NAME(const NAME &) = delete;                                                                             \
        NAME &operator=(const NAME &) = delete;                                                                  \
        NAME(NAME &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }                                                   \
        ~NAME() {                                                                                                \
            if (h_) phast_planner_channelizer##SFX##_free(h_);                                                   \
        }                                                                                                        \
        const CT *get() const { return h_; }                                                                     \
        std::string describe() const {                                                                           \
            std::string s(4096, '\0');                                                                           \
            check(phast_planner_channelizer##SFX##_describe(h_, &s[0], s.size()));                               \
            s.resize(s.find('\0'));                                                                              \
            return s;                                                                                            \
        }                                                                                                        \
        std::size_t device_bytes() const { return phast_planner_channelizer##SFX##_device_bytes(h_); }           \
        std::size_t out_frames() const { return phast_planner_channelizer##SFX##_out_frames(h_); }               \
        std::size_t full_frames() const { return phast_planner_channelizer##SFX##_full_frames(h_); }             \
        std::size_t bins() const { return phast_planner_channelizer##SFX##_bins(h_); }                           \
        /* the fold's tile (frames x columns per workgroup), tap rows per LDS chunk and periods of the signal in LDS: \
           functions of (K, channels, hop) alone */                                                              \
        std::size_t tile_frames() const { return phast_planner_channelizer##SFX##_tile_frames(h_); }             \
        std::size_t tile_cols() const { return phast_planner_channelizer##SFX##_tile_cols(h_); }                 \
        std::size_t chunk() const { return phast_planner_channelizer##SFX##_chunk(h_); }                         \
        std::size_t periods() const { return phast_planner_channelizer##SFX##_periods(h_); }                     \
        /* elements of T a _dev call of `batch` signals works in; workspace_min: the least a call runs in */     \
        std::size_t workspace_len(std::size_t batch = 1) const { return phast_planner_channelizer##SFX##_workspace_len(h_, batch); } \
        std::size_t workspace_min() const { return phast_planner_channelizer##SFX##_workspace_min(h_); }         \
                                                                                                                 \
      private:                                                                                                   \
        CT *h_ = nullptr;                                                                                        \
    };
PHASTFT_PLANNER_CHANNELIZER(PlannerChannelizer64, phast_planner_channelizer64, 64, double)
PHASTFT_PLANNER_CHANNELIZER(PlannerChannelizer32, phast_planner_channelizer32, 32, float)
#undef PHASTFT_PLANNER_CHANNELIZER

// one host signal of L samples (signal_im: its imaginary plane for a complex planner, an empty slice for a real one) -> the
// out_frames() x bins() points of both output planes, frame-major; blocking
#define PHASTFT_CHANNELIZE(FS, T, P)                                                                             \
    inline void channelize_##FS##_with_planner(Slice<const T> signal, Slice<const T> signal_im, Slice<T> out_re, Slice<T> out_im, \
                                               const P &planner) {                                               \
        if (out_re.len != out_im.len || (signal_im.ptr && signal_im.len != signal.len)) check(PHAST_ERR_LEN_MISMATCH); \
        check(phast_channelize_##FS##_with_planner(signal.ptr, signal_im.ptr, signal.len, out_re.ptr, out_im.ptr, out_re.len, \
                                                   planner.get()));                                              \
    }
PHASTFT_CHANNELIZE(f64, double, PlannerChannelizer64)
PHASTFT_CHANNELIZE(f32, float, PlannerChannelizer32)
#undef PHASTFT_CHANNELIZE

// ---- polyphase synthesis filter bank, the channelizer's inverse (no reference counterpart) ----
#define PHASTFT_PLANNER_SYNTHESIZER(NAME, CT, SFX, T)                                                            \
    class NAME {                                                                                                 \
      public:                                                                                                    \
        /* `frames` frames of `channels` channels back into a signal: every channel raised by `hop` (0: channels), filtered \
           with the real taps, brought back to its band, and the channels summed, zero extension: the out_len samples from \
           `first` on (out_len = 0: up to full_len; the window may pass it: zeros).  complex_output: a frame has `channels` \
           bins and the signal is (re, im) planes; otherwise channels / 2 + 1 bins and one plane.  The phases are in absolute \
           time: the delay of an analysis / synthesis pair must be a multiple of `channels` (taps (0, h reversed)) */ \
        NAME(std::size_t frames, Slice<const T> taps, std::size_t channels, std::size_t hop = 0, std::size_t first = 0, \
             std::size_t out_len = 0, bool complex_output = false) {                                             \
            check(phast_planner_synthesizer##SFX##_new(frames, taps.ptr, taps.len, channels, hop ? hop : channels, first, out_len, \
                                                       complex_output ? 1 : 0, &h_));                            \
        }                                                                                                        \
        NAME(const NAME &) = delete;                                                                             \
        NAME &operator=(const NAME &) = delete;                                                                  \
        NAME(NAME &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }                                                   \
        ~NAME() {                                                                                                \
            if (h_) phast_planner_synthesizer##SFX##_free(h_);                                                   \
        }                                                                                                        \
        const CT *get() const { return h_; }                                                                     \
        std::string describe() const {                                                                           \
            std::string s(4096, '\0');                                                                           \
            check(phast_planner_synthesizer##SFX##_describe(h_, &s[0], s.size()));                               \
            s.resize(s.find('\0'));                                                                              \
            return s;                                                                                            \
        }                                                                                                        \
        std::size_t device_bytes() const { return phast_planner_synthesizer##SFX##_device_bytes(h_); }           \
        std::size_t out_len() const { return phast_planner_synthesizer##SFX##_out_len(h_); }                     \
        std::size_t full_len() const { return phast_planner_synthesizer##SFX##_full_len(h_); }                   \
        std::size_t bins() const { return phast_planner_synthesizer##SFX##_bins(h_); }                           \
        /* the unfold's tile (output samples per workgroup and per thread) and the terms of an output at most */ \
        std::size_t tile_samples() const { return phast_planner_synthesizer##SFX##_tile_samples(h_); }           \
        std::size_t per_thread() const { return phast_planner_synthesizer##SFX##_per_thread(h_); }               \
        std::size_t max_terms() const { return phast_planner_synthesizer##SFX##_max_terms(h_); }                 \
        /* elements of T a _dev call of `batch` signals works in; workspace_min: the least a call runs in */     \
        std::size_t workspace_len(std::size_t batch = 1) const { return phast_planner_synthesizer##SFX##_workspace_len(h_, batch); } \
        std::size_t workspace_min() const { return phast_planner_synthesizer##SFX##_workspace_min(h_); }         \
                                                                                                                 \
      private:                                                                                                   \
        CT *h_ = nullptr;                                                                                        \
    };
PHASTFT_PLANNER_SYNTHESIZER(PlannerSynthesizer64, phast_planner_synthesizer64, 64, double)
PHASTFT_PLANNER_SYNTHESIZER(PlannerSynthesizer32, phast_planner_synthesizer32, 32, float)
#undef PHASTFT_PLANNER_SYNTHESIZER

// one signal's frames from host planes of frames x bins() points -> out_len() samples (out_im: the imaginary plane for a complex
// planner, an empty slice for a real one); blocking
#define PHASTFT_SYNTHESIZE(FS, T, P)                                                                             \
    inline void synthesize_##FS##_with_planner(Slice<const T> in_re, Slice<const T> in_im, Slice<T> out, Slice<T> out_im, \
                                               const P &planner) {                                               \
        if (in_re.len != in_im.len || (out_im.ptr && out_im.len != out.len)) check(PHAST_ERR_LEN_MISMATCH);      \
        check(phast_synthesize_##FS##_with_planner(in_re.ptr, in_im.ptr, in_re.len, out.ptr, out_im.ptr, out.len, planner.get())); \
    }
PHASTFT_SYNTHESIZE(f64, double, PlannerSynthesizer64)
PHASTFT_SYNTHESIZE(f32, float, PlannerSynthesizer32)
#undef PHASTFT_SYNTHESIZE

// ---- continuous wavelet transform and analytic signal (no reference counterpart; Torrence & Compo 1998) ----
enum class CwtFamily : int { Morlet = PHAST_CWT_MORLET, Paul = PHAST_CWT_PAUL, Dog = PHAST_CWT_DOG, Step = PHAST_CWT_STEP };
enum class CwtNorm : int { L2 = PHAST_CWT_L2, Peak = PHAST_CWT_PEAK };
#define PHASTFT_PLANNER_CWT(NAME, CT, SFX, T)                                                                    \
    class NAME {                                                                                                 \
      public:                                                                                                    \
        /* signals of `signal_len` points at the scales `scales` (in samples: finite, > 0), through a periodic convolution of \
           `pad_len` >= signal_len points (0: signal_len; the signal is zero-extended): W[j][n] = ifft(fft(x) conj(c_j \
           psi0^(s_j w)))[n], n < signal_len.  `param`: w0 of Morlet (customarily 6), the integer m of Paul (<= 85) and DOG \
           (<= 170); Step (the analytic-signal filter) ignores it, the scales' values and the norm.  real_input: one input \
           plane and the one-sided spectrum; otherwise (re, im) planes */ \
        NAME(std::size_t signal_len, Slice<const double> scales, CwtFamily family = CwtFamily::Morlet, double param = 6.0, \
             CwtNorm norm = CwtNorm::L2, std::size_t pad_len = 0, bool real_input = true)                        \
            : signal_len_(signal_len) {                                                                          \
            check(phast_planner_cwt##SFX##_new(signal_len, pad_len, scales.ptr, scales.len, static_cast<int>(family), param, \
                                               static_cast<int>(norm), real_input ? 1 : 0, &h_));                \
        }                                                                                                        \
        NAME(const NAME &) = delete;                                                                             \
        NAME &operator=(const NAME &) = delete;                                                                  \
        NAME(NAME &&o) noexcept : h_(o.h_), signal_len_(o.signal_len_) { o.h_ = nullptr; }                       \
        ~NAME() {                                                                                                \
            if (h_) phast_planner_cwt##SFX##_free(h_);                                                           \
        }                                                                                                        \
        const CT *get() const { return h_; }                                                                     \
        std::string describe() const {                                                                           \
            std::string s(4096, '\0');                                                                           \
            check(phast_planner_cwt##SFX##_describe(h_, &s[0], s.size()));                                       \
            s.resize(s.find('\0'));                                                                              \
            return s;                                                                                            \
        }                                                                                                        \
        std::size_t device_bytes() const { return phast_planner_cwt##SFX##_device_bytes(h_); }                   \
        std::size_t signal_len() const { return signal_len_; }                                                   \
        std::size_t pad_len() const { return phast_planner_cwt##SFX##_pad_len(h_); }                             \
        std::size_t num_scales() const { return phast_planner_cwt##SFX##_num_scales(h_); }                       \
        /* the bank's tile: bins and scales per workgroup */                                                     \
        std::size_t tile_bins() const { return phast_planner_cwt##SFX##_tile_bins(h_); }                         \
        std::size_t scale_group() const { return phast_planner_cwt##SFX##_scale_group(h_); }                     \
        /* elements of T a _dev call of `batch` signals works in; workspace_min: the least a call runs in */     \
        std::size_t workspace_len(std::size_t batch = 1) const { return phast_planner_cwt##SFX##_workspace_len(h_, batch); } \
        std::size_t workspace_min() const { return phast_planner_cwt##SFX##_workspace_min(h_); }                 \
                                                                                                                 \
      private:                                                                                                   \
        CT *h_ = nullptr;                                                                                        \
        std::size_t signal_len_ = 0;                                                                             \
    };
PHASTFT_PLANNER_CWT(PlannerCwt64, phast_planner_cwt64, 64, double)
PHASTFT_PLANNER_CWT(PlannerCwt32, phast_planner_cwt32, 32, float)
#undef PHASTFT_PLANNER_CWT

// one signal from a host slice of signal_len() points (x_im: the imaginary plane for a complex planner, an empty slice for a
// real one) -> host planes of num_scales() * signal_len() points, scale-major; blocking
#define PHASTFT_CWT(FS, T, P)                                                                                    \
    inline void cwt_##FS##_with_planner(Slice<const T> x, Slice<const T> x_im, Slice<T> out_re, Slice<T> out_im, \
                                        const P &planner) {                                                      \
        if ((x_im.ptr && x_im.len != x.len) || out_re.len != out_im.len) check(PHAST_ERR_LEN_MISMATCH);          \
        check(phast_cwt_##FS##_with_planner(x.ptr, x_im.ptr, x.len, out_re.ptr, out_im.ptr, out_re.len, planner.get())); \
    }
PHASTFT_CWT(64, double, PlannerCwt64)
PHASTFT_CWT(32, float, PlannerCwt32)
#undef PHASTFT_CWT

// ---- overlap-save convolution and correlation of real signals (no reference counterpart; scipy.signal.convolve / correlate) ----
enum class ConvMode : int { Full = PHAST_CONV_FULL, Same = PHAST_CONV_SAME, Valid = PHAST_CONV_VALID };
#define PHASTFT_PLANNER_CONV(NAME, CT, SFX, T)                                                                   \
    class NAME {                                                                                                 \
      public:                                                                                                    \
        /* `taps`: the K filter taps (correlate: the template); block = 0 picks the block from K */              \
        NAME(std::size_t signal_len, Slice<const T> taps, ConvMode mode = ConvMode::Full, bool correlate = false, \
             std::size_t block = 0) {                                                                            \
            check(phast_planner_conv##SFX##_new(signal_len, taps.ptr, taps.len, static_cast<int>(mode), correlate ? 1 : 0, \
                                                block, &h_));                                                    \
        }                                                                                                        \
        NAME(const NAME &) = delete;                                                                             \
        NAME &operator=(const NAME &) = delete;                                                                  \
        NAME(NAME &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }                                                   \
        ~NAME() {                                                                                                \
            if (h_) phast_planner_conv##SFX##_free(h_);                                                          \
        }                                                                                                        \
        const CT *get() const { return h_; }                                                                     \
        std::string describe() const {                                                                           \
            std::string s(4096, '\0');                                                                           \
            check(phast_planner_conv##SFX##_describe(h_, &s[0], s.size()));                                      \
            s.resize(s.find('\0'));                                                                              \
            return s;                                                                                            \
        }                                                                                                        \
        std::size_t device_bytes() const { return phast_planner_conv##SFX##_device_bytes(h_); }                  \
        std::size_t out_len() const { return phast_planner_conv##SFX##_out_len(h_); }                            \
        std::size_t block() const { return phast_planner_conv##SFX##_block(h_); }                                \
        std::size_t segments() const { return phast_planner_conv##SFX##_segments(h_); }                          \
        /* elements of T a _dev call of `batch` signals works in; workspace_min: the least a call runs in */     \
        std::size_t workspace_len(std::size_t batch = 1) const { return phast_planner_conv##SFX##_workspace_len(h_, batch); } \
        std::size_t workspace_min() const { return phast_planner_conv##SFX##_workspace_min(h_); }                \
                                                                                                                 \
      private:                                                                                                   \
        CT *h_ = nullptr;                                                                                        \
    };
PHASTFT_PLANNER_CONV(PlannerConv64, phast_planner_conv64, 64, double)
PHASTFT_PLANNER_CONV(PlannerConv32, phast_planner_conv32, 32, float)
#undef PHASTFT_PLANNER_CONV

// one host signal of L samples -> its out_len() output samples; blocking
#define PHASTFT_CONV(FS, T, P)                                                                                   \
    inline void conv_##FS##_with_planner(Slice<const T> signal, Slice<T> output, const P &planner) {             \
        check(phast_conv_##FS##_with_planner(signal.ptr, signal.len, output.ptr, output.len, planner.get()));    \
    }
PHASTFT_CONV(f64, double, PlannerConv64)
PHASTFT_CONV(f32, float, PlannerConv32)
#undef PHASTFT_CONV

// ---- overlap-save convolution and correlation of real arrays of rank 1 .. 3 (no reference counterpart; scipy.signal.convolve /
// correlate of N-d arrays) ----
#define PHASTFT_PLANNER_CONVND(NAME, CT, SFX, T)                                                                 \
    class NAME {                                                                                                 \
      public:                                                                                                    \
        /* row-major arrays of `signal_shape`, `taps` of `taps_shape` (the same rank); block: empty = automatic, or one \
           entry per axis (0: automatic) */                                                                      \
        NAME(const std::vector<std::size_t> &signal_shape, const std::vector<std::size_t> &taps_shape, Slice<const T> taps, \
             ConvMode mode = ConvMode::Full, bool correlate = false, const std::vector<std::size_t> &block = {})  \
            : rank_(signal_shape.size()) {                                                                       \
            std::size_t k = 1;                                                                                   \
            for (std::size_t v : taps_shape) k *= v;                                                             \
            if (taps_shape.size() != rank_ || (!block.empty() && block.size() != rank_) || (rank_ && taps.len != k)) \
                check(PHAST_ERR_INVALID_ARG);                                                                    \
            check(phast_planner_convnd##SFX##_new(signal_shape.data(), taps_shape.data(), rank_, taps.ptr,       \
                                                  static_cast<int>(mode), correlate ? 1 : 0,                     \
                                                  block.empty() ? nullptr : block.data(), &h_));                 \
        }                                                                                                        \
        NAME(const NAME &) = delete;                                                                             \
        NAME &operator=(const NAME &) = delete;                                                                  \
        NAME(NAME &&o) noexcept : h_(o.h_), rank_(o.rank_) { o.h_ = nullptr; }                                   \
        ~NAME() {                                                                                                \
            if (h_) phast_planner_convnd##SFX##_free(h_);                                                        \
        }                                                                                                        \
        const CT *get() const { return h_; }                                                                     \
        std::string describe() const {                                                                           \
            std::string s(4096, '\0');                                                                           \
            check(phast_planner_convnd##SFX##_describe(h_, &s[0], s.size()));                                    \
            s.resize(s.find('\0'));                                                                              \
            return s;                                                                                            \
        }                                                                                                        \
        std::size_t device_bytes() const { return phast_planner_convnd##SFX##_device_bytes(h_); }                \
        std::size_t out_len() const { return phast_planner_convnd##SFX##_out_len(h_); }                          \
        std::vector<std::size_t> out_shape() const {                                                             \
            std::vector<std::size_t> d(rank_);                                                                   \
            check(phast_planner_convnd##SFX##_out_dims(h_, d.data(), rank_));                                    \
            return d;                                                                                            \
        }                                                                                                        \
        std::vector<std::size_t> block() const {                                                                 \
            std::vector<std::size_t> d(rank_);                                                                   \
            check(phast_planner_convnd##SFX##_block(h_, d.data(), rank_));                                       \
            return d;                                                                                            \
        }                                                                                                        \
        std::size_t tiles() const { return phast_planner_convnd##SFX##_tiles(h_); }                              \
        /* elements of T a _dev call of `batch` arrays works in; workspace_min: the least a call runs in */      \
        std::size_t workspace_len(std::size_t batch = 1) const { return phast_planner_convnd##SFX##_workspace_len(h_, batch); } \
        std::size_t workspace_min() const { return phast_planner_convnd##SFX##_workspace_min(h_); }              \
                                                                                                                 \
      private:                                                                                                   \
        CT *h_ = nullptr;                                                                                        \
        std::size_t rank_ = 0;                                                                                   \
    };
PHASTFT_PLANNER_CONVND(PlannerConvNd64, phast_planner_convnd64, 64, double)
PHASTFT_PLANNER_CONVND(PlannerConvNd32, phast_planner_convnd32, 32, float)
#undef PHASTFT_PLANNER_CONVND

// one host array of the planner's shape -> its out_len() output samples (row-major, out_shape()); blocking
#define PHASTFT_CONVND(FS, T, P)                                                                                 \
    inline void convnd_##FS##_with_planner(Slice<const T> signal, Slice<T> output, const P &planner) {           \
        check(phast_convnd_##FS##_with_planner(signal.ptr, signal.len, output.ptr, output.len, planner.get()));  \
    }
PHASTFT_CONVND(f64, double, PlannerConvNd64)
PHASTFT_CONVND(f32, float, PlannerConvNd32)
#undef PHASTFT_CONVND

// ---- the chirp-Z transform on the unit circle and the zoom FFT (no reference counterpart; scipy.signal.czt / zoom_fft) ----
#define PHASTFT_PLANNER_CZT(NAME, CT, SFX)                                                                       \
    class NAME {                                                                                                 \
      public:                                                                                                    \
        /* m bins of n points at start + k step turns: X[k] = sum x[n] exp(-2 pi i n (start + k step)) */       \
        NAME(std::size_t n, std::size_t m, double step, double start = 0.0) : n_(n), m_(m) {                     \
            check(phast_planner_czt##SFX##_new(n, m, step, start, &h_));                                         \
        }                                                                                                        \
        NAME(const NAME &) = delete;                                                                             \
        NAME &operator=(const NAME &) = delete;                                                                  \
        NAME(NAME &&o) noexcept : h_(o.h_), n_(o.n_), m_(o.m_) { o.h_ = nullptr; }                               \
        ~NAME() {                                                                                                \
            if (h_) phast_planner_czt##SFX##_free(h_);                                                           \
        }                                                                                                        \
        const CT *get() const { return h_; }                                                                     \
        std::string describe() const {                                                                           \
            std::string s(4096, '\0');                                                                           \
            check(phast_planner_czt##SFX##_describe(h_, &s[0], s.size()));                                       \
            s.resize(s.find('\0'));                                                                              \
            return s;                                                                                            \
        }                                                                                                        \
        std::size_t input_len() const { return n_; }                                                             \
        std::size_t output_len() const { return m_; }                                                            \
        std::size_t device_bytes() const { return phast_planner_czt##SFX##_device_bytes(h_); }                   \
        std::size_t conv_len() const { return phast_planner_czt##SFX##_conv_len(h_); }                           \
        /* elements of T a _dev call of `batch` transforms works in: 2 L batch */                                \
        std::size_t workspace_len(std::size_t batch = 1) const { return phast_planner_czt##SFX##_workspace_len(h_, batch); } \
                                                                                                                 \
      private:                                                                                                   \
        CT *h_ = nullptr;                                                                                        \
        std::size_t n_, m_;                                                                                      \
    };
PHASTFT_PLANNER_CZT(PlannerCzt64, phast_planner_czt64, 64)
PHASTFT_PLANNER_CZT(PlannerCzt32, phast_planner_czt32, 32)
#undef PHASTFT_PLANNER_CZT

// one host signal (in_im.ptr may be null: a real signal) -> its output_len() bins; blocking.  Without a planner the call builds
// its own from the lengths of the slices.
#define PHASTFT_CZT(SFX, T, P)                                                                                   \
    inline void czt_##SFX(Slice<const T> in_re, Slice<const T> in_im, Slice<T> out_re, Slice<T> out_im, double step, \
                          double start = 0.0) {                                                                  \
        if ((in_im.ptr && in_im.len != in_re.len) || out_re.len != out_im.len) check(PHAST_ERR_LEN_MISMATCH);    \
        check(phast_czt_##SFX(in_re.ptr, in_im.ptr, in_re.len, out_re.ptr, out_im.ptr, out_re.len, step, start)); \
    }                                                                                                            \
    inline void czt_##SFX##_with_planner(Slice<const T> in_re, Slice<const T> in_im, Slice<T> out_re, Slice<T> out_im, \
                                         const P &planner) {                                                     \
        if ((in_im.ptr && in_im.len != in_re.len) || out_re.len != out_im.len) check(PHAST_ERR_LEN_MISMATCH);    \
        check(phast_czt_##SFX##_with_planner(in_re.ptr, in_im.ptr, in_re.len, out_re.ptr, out_im.ptr, out_re.len, \
                                             planner.get()));                                                    \
    }
PHASTFT_CZT(64, double, PlannerCzt64)
PHASTFT_CZT(32, float, PlannerCzt32)
#undef PHASTFT_CZT

// ---- non-uniform FFTs of types 1 and 2 in one dimension (no reference counterpart) ----
#define PHASTFT_PLANNER_NUFFT(NAME, CT, SFX)                                                                     \
    class NAME {                                                                                                 \
      public:                                                                                                    \
        /* n_modes modes in fftfreq order and the points x (host doubles in turns, reduced mod 1), to the accuracy eps */\
        NAME(std::size_t n_modes, Slice<const double> x, double eps) : n_(n_modes), m_(x.len) {                  \
            check(phast_planner_nufft##SFX##_new(n_modes, x.ptr, x.len, eps, &h_));                              \
        }                                                                                                        \
        NAME(const NAME &) = delete;                                                                             \
        NAME &operator=(const NAME &) = delete;                                                                  \
        NAME(NAME &&o) noexcept : h_(o.h_), n_(o.n_), m_(o.m_) { o.h_ = nullptr; }                               \
        ~NAME() {                                                                                                \
            if (h_) phast_planner_nufft##SFX##_free(h_);                                                         \
        }                                                                                                        \
        /* the same from m_points doubles in DEVICE memory, sorted on the device into the tables the constructor builds on the\
           host; ordered after the earlier work of `stream`, blocks until the planner is built */\
        static NAME from_device(std::size_t n_modes, const double *d_x, std::size_t m_points, double eps,        \
                                void *stream = nullptr) {                                                        \
            CT *h = nullptr;                                                                                     \
            check(phast_planner_nufft##SFX##_new_dev(n_modes, d_x, m_points, eps, stream, &h));                  \
            return NAME(h, n_modes, m_points);                                                                   \
        }                                                                                                        \
        /* new points, the same number of them, from device memory: the tables are rewritten in place (a captured graph\
           stays valid).  Ordered after the earlier work of `stream` ONLY: work on other streams that uses the planner must\
           have finished.  Blocks; a rejected point set leaves the planner as it was */                          \
        void set_points_dev(const double *d_x, std::size_t m_points, void *stream = nullptr) {                   \
            check(phast_planner_nufft##SFX##_set_points_dev(h_, d_x, m_points, stream));                         \
        }                                                                                                        \
        const CT *get() const { return h_; }                                                                     \
        std::string describe() const {                                                                           \
            std::string s(4096, '\0');                                                                           \
            check(phast_planner_nufft##SFX##_describe(h_, &s[0], s.size()));                                     \
            s.resize(s.find('\0'));                                                                              \
            return s;                                                                                            \
        }                                                                                                        \
        std::size_t num_modes() const { return n_; }                                                             \
        std::size_t num_points() const { return m_; }                                                            \
        std::size_t device_bytes() const { return phast_planner_nufft##SFX##_device_bytes(h_); }                 \
        std::size_t grid_len() const { return phast_planner_nufft##SFX##_grid_len(h_); }                         \
        int width() const { return phast_planner_nufft##SFX##_width(h_); }                                       \
        /* elements of T a _dev call of `batch` transforms works in: 2 n_g batch */                              \
        std::size_t workspace_len(std::size_t batch = 1) const { return phast_planner_nufft##SFX##_workspace_len(h_, batch); }\
                                                                                                                 \
      private:                                                                                                   \
        NAME(CT *h, std::size_t n, std::size_t m) : h_(h), n_(n), m_(m) {}                                       \
        CT *h_ = nullptr;                                                                                        \
        std::size_t n_, m_;                                                                                      \
    };
PHASTFT_PLANNER_NUFFT(PlannerNufft64, phast_planner_nufft64, 64)
PHASTFT_PLANNER_NUFFT(PlannerNufft32, phast_planner_nufft32, 32)
#undef PHASTFT_PLANNER_NUFFT

// one host vector (in_im.ptr may be null: real data): type 1 takes the values at the points and gives the modes, type 2 the
// reverse; blocking.  Without a planner the call builds its own from x, eps and the lengths of the slices.
#define PHASTFT_NUFFT(TYPE, SFX, T, P)                                                                           \
    inline void nufft##TYPE##_##SFX(Slice<const double> x, Slice<const T> in_re, Slice<const T> in_im, Slice<T> out_re,\
                                    Slice<T> out_im, double eps, Direction direction = Direction::Forward) {     \
        if ((in_im.ptr && in_im.len != in_re.len) || out_re.len != out_im.len) check(PHAST_ERR_LEN_MISMATCH);    \
        if (x.len != (TYPE == 1 ? in_re.len : out_re.len)) check(PHAST_ERR_LEN_MISMATCH);                        \
        check(phast_nufft##TYPE##_##SFX(x.ptr, x.len, in_re.ptr, in_im.ptr, out_re.ptr, out_im.ptr,              \
                                        TYPE == 1 ? out_re.len : in_re.len, eps, static_cast<int>(direction)));  \
    }                                                                                                            \
    inline void nufft##TYPE##_##SFX##_with_planner(Slice<const T> in_re, Slice<const T> in_im, Slice<T> out_re, Slice<T> out_im,\
                                                   const P &planner, Direction direction = Direction::Forward) { \
        if ((in_im.ptr && in_im.len != in_re.len) || out_re.len != out_im.len) check(PHAST_ERR_LEN_MISMATCH);    \
        check(phast_nufft##TYPE##_##SFX##_with_planner(in_re.ptr, in_im.ptr, in_re.len, out_re.ptr, out_im.ptr, out_re.len,\
                                                       static_cast<int>(direction), planner.get()));             \
    }
PHASTFT_NUFFT(1, 64, double, PlannerNufft64)
PHASTFT_NUFFT(1, 32, float, PlannerNufft32)
PHASTFT_NUFFT(2, 64, double, PlannerNufft64)
PHASTFT_NUFFT(2, 32, float, PlannerNufft32)
#undef PHASTFT_NUFFT

// ---- the non-uniform FFT of type 3 in one dimension (no reference counterpart) ----
#define PHASTFT_PLANNER_NUFFT_T3(NAME, CT, SFX)                                                                  \
    class NAME {                                                                                                 \
      public:                                                                                                    \
        /* the sources x and the target frequencies s (host doubles, any finite values, s x in turns), to the accuracy eps */\
        NAME(Slice<const double> x, Slice<const double> s, double eps) : m_(x.len), k_(s.len) {                  \
            check(phast_planner_nufft_t3_##SFX##_new(x.ptr, x.len, s.ptr, s.len, eps, &h_));                     \
        }                                                                                                        \
        NAME(const NAME &) = delete;                                                                             \
        NAME &operator=(const NAME &) = delete;                                                                  \
        NAME(NAME &&o) noexcept : h_(o.h_), m_(o.m_), k_(o.k_) { o.h_ = nullptr; }                               \
        ~NAME() {                                                                                                \
            if (h_) phast_planner_nufft_t3_##SFX##_free(h_);                                                     \
        }                                                                                                        \
        const CT *get() const { return h_; }                                                                     \
        std::string describe() const {                                                                           \
            std::string s(4096, '\0');                                                                           \
            check(phast_planner_nufft_t3_##SFX##_describe(h_, &s[0], s.size()));                                 \
            s.resize(s.find('\0'));                                                                              \
            return s;                                                                                            \
        }                                                                                                        \
        std::size_t num_points() const { return m_; }                                                            \
        std::size_t num_targets() const { return k_; }                                                           \
        std::size_t device_bytes() const { return phast_planner_nufft_t3_##SFX##_device_bytes(h_); }             \
        /* the fine grid n_f */                                                                                  \
        std::size_t grid_len() const { return phast_planner_nufft_t3_##SFX##_grid_len(h_); }                     \
        int width() const { return phast_planner_nufft_t3_##SFX##_width(h_); }                                   \
        /* elements of T a _dev call of `batch` transforms works in: 4 n_f batch */                              \
        std::size_t workspace_len(std::size_t batch = 1) const { return phast_planner_nufft_t3_##SFX##_workspace_len(h_, batch); }\
                                                                                                                 \
      private:                                                                                                   \
        CT *h_ = nullptr;                                                                                        \
        std::size_t m_, k_;                                                                                      \
    };
PHASTFT_PLANNER_NUFFT_T3(PlannerNufftT3_64, phast_planner_nufft_t3_64, 64)
PHASTFT_PLANNER_NUFFT_T3(PlannerNufftT3_32, phast_planner_nufft_t3_32, 32)
#undef PHASTFT_PLANNER_NUFFT_T3

// one host vector of values at the sources (c_im.ptr may be null: real data) to the values at the targets; blocking.  Without a
// planner the call builds its own from x, s and eps.
#define PHASTFT_NUFFT_T3(SFX, T, P)                                                                              \
    inline void nufft3_##SFX(Slice<const double> x, Slice<const double> s, Slice<const T> c_re, Slice<const T> c_im,\
                             Slice<T> out_re, Slice<T> out_im, double eps, Direction direction = Direction::Forward) {\
        if ((c_im.ptr && c_im.len != c_re.len) || out_re.len != out_im.len) check(PHAST_ERR_LEN_MISMATCH);       \
        if (x.len != c_re.len || s.len != out_re.len) check(PHAST_ERR_LEN_MISMATCH);                             \
        check(phast_nufft3_##SFX(x.ptr, x.len, s.ptr, s.len, c_re.ptr, c_im.ptr, out_re.ptr, out_im.ptr, eps,    \
                                 static_cast<int>(direction)));                                                  \
    }                                                                                                            \
    inline void nufft3_##SFX##_with_planner(Slice<const T> c_re, Slice<const T> c_im, Slice<T> out_re, Slice<T> out_im,\
                                            const P &planner, Direction direction = Direction::Forward) {        \
        if ((c_im.ptr && c_im.len != c_re.len) || out_re.len != out_im.len) check(PHAST_ERR_LEN_MISMATCH);       \
        check(phast_nufft3_##SFX##_with_planner(c_re.ptr, c_im.ptr, c_re.len, out_re.ptr, out_im.ptr, out_re.len,\
                                                static_cast<int>(direction), planner.get()));                    \
    }
PHASTFT_NUFFT_T3(64, double, PlannerNufftT3_64)
PHASTFT_NUFFT_T3(32, float, PlannerNufftT3_32)
#undef PHASTFT_NUFFT_T3

// ---- non-uniform FFTs of types 1 and 2 in two dimensions (no reference counterpart) ----
#define PHASTFT_PLANNER_NUFFT2D(NAME, CT, SFX)                                                                   \
    class NAME {                                                                                                 \
      public:                                                                                                    \
        /* n1 x n2 modes, row-major, each axis in fftfreq order, and the points (x, y) (host doubles in turns, reduced  \
           mod 1 per coordinate; k1 pairs with x, k2 with y), to the accuracy eps */                             \
        NAME(std::size_t n1, std::size_t n2, Slice<const double> x, Slice<const double> y, double eps)           \
            : n1_(n1), n2_(n2), m_(x.len) {                                                                      \
            if (x.len != y.len) check(PHAST_ERR_LEN_MISMATCH);                                                   \
            check(phast_planner_nufft2d##SFX##_new(n1, n2, x.ptr, y.ptr, x.len, eps, &h_));                      \
        }                                                                                                        \
        NAME(const NAME &) = delete;                                                                             \
        NAME &operator=(const NAME &) = delete;                                                                  \
        NAME(NAME &&o) noexcept : h_(o.h_), n1_(o.n1_), n2_(o.n2_), m_(o.m_) { o.h_ = nullptr; }                 \
        ~NAME() {                                                                                                \
            if (h_) phast_planner_nufft2d##SFX##_free(h_);                                                       \
        }                                                                                                        \
        /* the same from m_points doubles per coordinate in DEVICE memory: as PlannerNufft64::from_device */     \
        static NAME from_device(std::size_t n1, std::size_t n2, const double *d_x, const double *d_y, std::size_t m_points,\
                                double eps, void *stream = nullptr) {                                            \
            CT *h = nullptr;                                                                                     \
            check(phast_planner_nufft2d##SFX##_new_dev(n1, n2, d_x, d_y, m_points, eps, stream, &h));            \
            return NAME(h, n1, n2, m_points);                                                                    \
        }                                                                                                        \
        /* new points, the same number of them, from device memory: as PlannerNufft64::set_points_dev */         \
        void set_points_dev(const double *d_x, const double *d_y, std::size_t m_points, void *stream = nullptr) {\
            check(phast_planner_nufft2d##SFX##_set_points_dev(h_, d_x, d_y, m_points, stream));                  \
        }                                                                                                        \
        const CT *get() const { return h_; }                                                                     \
        std::string describe() const {                                                                           \
            std::string s(4096, '\0');                                                                           \
            check(phast_planner_nufft2d##SFX##_describe(h_, &s[0], s.size()));                                   \
            s.resize(s.find('\0'));                                                                              \
            return s;                                                                                            \
        }                                                                                                        \
        std::size_t num_modes_1() const { return n1_; }                                                          \
        std::size_t num_modes_2() const { return n2_; }                                                          \
        std::size_t num_points() const { return m_; }                                                            \
        std::size_t device_bytes() const { return phast_planner_nufft2d##SFX##_device_bytes(h_); }               \
        std::size_t grid_len() const { return phast_planner_nufft2d##SFX##_grid_len(h_); }                       \
        std::size_t grid_rows() const { return phast_planner_nufft2d##SFX##_grid_rows(h_); }                     \
        std::size_t grid_cols() const { return phast_planner_nufft2d##SFX##_grid_cols(h_); }                     \
        int width() const { return phast_planner_nufft2d##SFX##_width(h_); }                                     \
        /* elements of T a _dev call of `batch` transforms works in: 4 G batch, G = grid_len() */                \
        std::size_t workspace_len(std::size_t batch = 1) const { return phast_planner_nufft2d##SFX##_workspace_len(h_, batch); }\
                                                                                                                 \
      private:                                                                                                   \
        NAME(CT *h, std::size_t n1, std::size_t n2, std::size_t m) : h_(h), n1_(n1), n2_(n2), m_(m) {}           \
        CT *h_ = nullptr;                                                                                        \
        std::size_t n1_, n2_, m_;                                                                                \
    };
PHASTFT_PLANNER_NUFFT2D(PlannerNufft2d64, phast_planner_nufft2d64, 64)
PHASTFT_PLANNER_NUFFT2D(PlannerNufft2d32, phast_planner_nufft2d32, 32)
#undef PHASTFT_PLANNER_NUFFT2D

// one host vector (in_im.ptr may be null: real data): type 1 takes the values at the points and gives the n1 x n2 modes
// (row-major), type 2 the reverse; blocking.  Without a planner the call builds its own from x, y, (n1, n2) and eps.
#define PHASTFT_NUFFT2D(TYPE, SFX, T, P)                                                                         \
    inline void nufft2d##TYPE##_##SFX(Slice<const double> x, Slice<const double> y, Slice<const T> in_re, Slice<const T> in_im,\
                                      Slice<T> out_re, Slice<T> out_im, std::size_t n1, std::size_t n2, double eps,\
                                      Direction direction = Direction::Forward) {                                \
        if ((in_im.ptr && in_im.len != in_re.len) || out_re.len != out_im.len || x.len != y.len) check(PHAST_ERR_LEN_MISMATCH);\
        if (x.len != (TYPE == 1 ? in_re.len : out_re.len)) check(PHAST_ERR_LEN_MISMATCH);                        \
        if (n2 == 0 || (TYPE == 1 ? out_re.len : in_re.len) / n2 != n1 || (TYPE == 1 ? out_re.len : in_re.len) % n2)\
            check(PHAST_ERR_LEN_MISMATCH);                                                                       \
        check(phast_nufft2d##TYPE##_##SFX(x.ptr, y.ptr, x.len, in_re.ptr, in_im.ptr, out_re.ptr, out_im.ptr, n1, n2, eps,\
                                          static_cast<int>(direction)));                                         \
    }                                                                                                            \
    inline void nufft2d##TYPE##_##SFX##_with_planner(Slice<const T> in_re, Slice<const T> in_im, Slice<T> out_re, Slice<T> out_im,\
                                                     const P &planner, Direction direction = Direction::Forward) {\
        if ((in_im.ptr && in_im.len != in_re.len) || out_re.len != out_im.len) check(PHAST_ERR_LEN_MISMATCH);    \
        check(phast_nufft2d##TYPE##_##SFX##_with_planner(in_re.ptr, in_im.ptr, in_re.len, out_re.ptr, out_im.ptr, out_re.len,\
                                                         static_cast<int>(direction), planner.get()));           \
    }
PHASTFT_NUFFT2D(1, 64, double, PlannerNufft2d64)
PHASTFT_NUFFT2D(1, 32, float, PlannerNufft2d32)
PHASTFT_NUFFT2D(2, 64, double, PlannerNufft2d64)
PHASTFT_NUFFT2D(2, 32, float, PlannerNufft2d32)
#undef PHASTFT_NUFFT2D

// ---- non-uniform FFTs of types 1 and 2 in three dimensions (no reference counterpart) ----
#define PHASTFT_PLANNER_NUFFT3D(NAME, CT, SFX)                                                                   \
    class NAME {                                                                                                 \
      public:                                                                                                    \
        /* n1 x n2 x n3 modes, row-major, each axis in fftfreq order, and the points (x, y, z) (host doubles in turns,  \
           reduced mod 1 per coordinate; k1 pairs with x, k2 with y, k3 with z), to the accuracy eps */          \
        NAME(std::size_t n1, std::size_t n2, std::size_t n3, Slice<const double> x, Slice<const double> y,       \
             Slice<const double> z, double eps)                                                                  \
            : n1_(n1), n2_(n2), n3_(n3), m_(x.len) {                                                             \
            if (x.len != y.len || x.len != z.len) check(PHAST_ERR_LEN_MISMATCH);                                 \
            check(phast_planner_nufft3d##SFX##_new(n1, n2, n3, x.ptr, y.ptr, z.ptr, x.len, eps, &h_));           \
        }                                                                                                        \
        NAME(const NAME &) = delete;                                                                             \
        NAME &operator=(const NAME &) = delete;                                                                  \
        NAME(NAME &&o) noexcept : h_(o.h_), n1_(o.n1_), n2_(o.n2_), n3_(o.n3_), m_(o.m_) { o.h_ = nullptr; }     \
        ~NAME() {                                                                                                \
            if (h_) phast_planner_nufft3d##SFX##_free(h_);                                                       \
        }                                                                                                        \
        /* the same from m_points doubles per coordinate in DEVICE memory: as PlannerNufft64::from_device */     \
        static NAME from_device(std::size_t n1, std::size_t n2, std::size_t n3, const double *d_x, const double *d_y,\
                                const double *d_z, std::size_t m_points, double eps, void *stream = nullptr) {   \
            CT *h = nullptr;                                                                                     \
            check(phast_planner_nufft3d##SFX##_new_dev(n1, n2, n3, d_x, d_y, d_z, m_points, eps, stream, &h));   \
            return NAME(h, n1, n2, n3, m_points);                                                                \
        }                                                                                                        \
        /* new points, the same number of them, from device memory: as PlannerNufft64::set_points_dev */         \
        void set_points_dev(const double *d_x, const double *d_y, const double *d_z, std::size_t m_points,       \
                            void *stream = nullptr) {                                                            \
            check(phast_planner_nufft3d##SFX##_set_points_dev(h_, d_x, d_y, d_z, m_points, stream));             \
        }                                                                                                        \
        const CT *get() const { return h_; }                                                                     \
        std::string describe() const {                                                                           \
            std::string s(4096, '\0');                                                                           \
            check(phast_planner_nufft3d##SFX##_describe(h_, &s[0], s.size()));                                   \
            s.resize(s.find('\0'));                                                                              \
            return s;                                                                                            \
        }                                                                                                        \
        std::size_t num_modes_1() const { return n1_; }                                                          \
        std::size_t num_modes_2() const { return n2_; }                                                          \
        std::size_t num_modes_3() const { return n3_; }                                                          \
        std::size_t num_points() const { return m_; }                                                            \
        std::size_t device_bytes() const { return phast_planner_nufft3d##SFX##_device_bytes(h_); }               \
        std::size_t grid_len() const { return phast_planner_nufft3d##SFX##_grid_len(h_); }                       \
        /* g1, g2, g3 for axis 0, 1, 2 */                                                                        \
        std::size_t grid_dim(int axis) const { return phast_planner_nufft3d##SFX##_grid_dim(h_, axis); }         \
        int width() const { return phast_planner_nufft3d##SFX##_width(h_); }                                     \
        /* elements of T a _dev call of `batch` transforms works in: 4 G batch, G = grid_len() */                \
        std::size_t workspace_len(std::size_t batch = 1) const { return phast_planner_nufft3d##SFX##_workspace_len(h_, batch); }\
                                                                                                                 \
      private:                                                                                                   \
        NAME(CT *h, std::size_t n1, std::size_t n2, std::size_t n3, std::size_t m) : h_(h), n1_(n1), n2_(n2), n3_(n3), m_(m) {}\
        CT *h_ = nullptr;                                                                                        \
        std::size_t n1_, n2_, n3_, m_;                                                                           \
    };
PHASTFT_PLANNER_NUFFT3D(PlannerNufft3d64, phast_planner_nufft3d64, 64)
PHASTFT_PLANNER_NUFFT3D(PlannerNufft3d32, phast_planner_nufft3d32, 32)
#undef PHASTFT_PLANNER_NUFFT3D

// one host vector (in_im.ptr may be null: real data): type 1 takes the values at the points and gives the n1 x n2 x n3 modes
// (row-major), type 2 the reverse; blocking.  Without a planner the call builds its own from x, y, z, (n1, n2, n3) and eps.
#define PHASTFT_NUFFT3D(TYPE, SFX, T, P)                                                                         \
    inline void nufft3d##TYPE##_##SFX(Slice<const double> x, Slice<const double> y, Slice<const double> z, Slice<const T> in_re,\
                                      Slice<const T> in_im, Slice<T> out_re, Slice<T> out_im, std::size_t n1, std::size_t n2,\
                                      std::size_t n3, double eps, Direction direction = Direction::Forward) {    \
        if ((in_im.ptr && in_im.len != in_re.len) || out_re.len != out_im.len || x.len != y.len || x.len != z.len)\
            check(PHAST_ERR_LEN_MISMATCH);                                                                       \
        if (x.len != (TYPE == 1 ? in_re.len : out_re.len)) check(PHAST_ERR_LEN_MISMATCH);                        \
        const std::size_t modes = TYPE == 1 ? out_re.len : in_re.len;                                            \
        if (n2 == 0 || n3 == 0 || modes % n3 || modes / n3 % n2 || modes / n3 / n2 != n1) check(PHAST_ERR_LEN_MISMATCH);\
        check(phast_nufft3d##TYPE##_##SFX(x.ptr, y.ptr, z.ptr, x.len, in_re.ptr, in_im.ptr, out_re.ptr, out_im.ptr, n1, n2, n3,\
                                          eps, static_cast<int>(direction)));                                    \
    }                                                                                                            \
    inline void nufft3d##TYPE##_##SFX##_with_planner(Slice<const T> in_re, Slice<const T> in_im, Slice<T> out_re, Slice<T> out_im,\
                                                     const P &planner, Direction direction = Direction::Forward) {\
        if ((in_im.ptr && in_im.len != in_re.len) || out_re.len != out_im.len) check(PHAST_ERR_LEN_MISMATCH);    \
        check(phast_nufft3d##TYPE##_##SFX##_with_planner(in_re.ptr, in_im.ptr, in_re.len, out_re.ptr, out_im.ptr, out_re.len,\
                                                         static_cast<int>(direction), planner.get()));           \
    }
PHASTFT_NUFFT3D(1, 64, double, PlannerNufft3d64)
PHASTFT_NUFFT3D(1, 32, float, PlannerNufft3d32)
PHASTFT_NUFFT3D(2, 64, double, PlannerNufft3d64)
PHASTFT_NUFFT3D(2, 32, float, PlannerNufft3d32)
#undef PHASTFT_NUFFT3D

// ---- transforms over every axis of a row-major array (numpy fftn / rfftn / irfftn; no reference counterpart) ----
#define PHASTFT_PLANNER_ND(NAME, CT, PFX)                                                                        \
    class NAME {                                                                                                 \
      public:                                                                                                    \
        explicit NAME(const std::vector<std::size_t> &shape) : shape_(shape) {                                   \
            check(phast_planner_##PFX##_new(shape.data(), shape.size(), &h_));                                   \
        }                                                                                                        \
        NAME(const NAME &) = delete;                                                                             \
        NAME &operator=(const NAME &) = delete;                                                                  \
        NAME(NAME &&o) noexcept : h_(o.h_), shape_(std::move(o.shape_)) { o.h_ = nullptr; }                      \
        ~NAME() {                                                                                                \
            if (h_) phast_planner_##PFX##_free(h_);                                                              \
        }                                                                                                        \
        const CT *get() const { return h_; }                                                                     \
        const std::vector<std::size_t> &shape() const { return shape_; }                                         \
        std::string describe() const {                                                                           \
            std::string s(16384, '\0');                                                                          \
            check(phast_planner_##PFX##_describe(h_, &s[0], s.size()));                                          \
            s.resize(s.find('\0'));                                                                              \
            return s;                                                                                            \
        }                                                                                                        \
        std::size_t device_bytes() const { return phast_planner_##PFX##_device_bytes(h_); }                      \
        /* elements of T a _dev call of `batch` arrays works in at full speed; workspace_len(1) serves any batch */   \
        std::size_t workspace_len(std::size_t batch = 1) const { return phast_planner_##PFX##_workspace_len(h_, batch); } \
                                                                                                                 \
      private:                                                                                                   \
        CT *h_ = nullptr;                                                                                        \
        std::vector<std::size_t> shape_;                                                                         \
    };
PHASTFT_PLANNER_ND(PlannerNd64, phast_planner_nd64, nd64)
PHASTFT_PLANNER_ND(PlannerNd32, phast_planner_nd32, nd32)
PHASTFT_PLANNER_ND(PlannerR2cNd64, phast_planner_r2c_nd64, r2c_nd64)
PHASTFT_PLANNER_ND(PlannerR2cNd32, phast_planner_r2c_nd32, r2c_nd32)
#undef PHASTFT_PLANNER_ND

inline void fft_64_nd_with_planner(Slice<double> reals, Slice<double> imags, Direction direction, const PlannerNd64 &planner) {
    check(phast_fft_64_nd_with_planner(reals.ptr, reals.len, imags.ptr, imags.len, static_cast<int>(direction), planner.get()));
}
inline void fft_32_nd_with_planner(Slice<float> reals, Slice<float> imags, Direction direction, const PlannerNd32 &planner) {
    check(phast_fft_32_nd_with_planner(reals.ptr, reals.len, imags.ptr, imags.len, static_cast<int>(direction), planner.get()));
}
inline void fft_64_nd(Slice<double> reals, Slice<double> imags, const std::vector<std::size_t> &shape, Direction direction) {
    check(phast_fft_64_nd(reals.ptr, reals.len, imags.ptr, imags.len, shape.data(), shape.size(), static_cast<int>(direction)));
}
inline void fft_32_nd(Slice<float> reals, Slice<float> imags, const std::vector<std::size_t> &shape, Direction direction) {
    check(phast_fft_32_nd(reals.ptr, reals.len, imags.ptr, imags.len, shape.data(), shape.size(), static_cast<int>(direction)));
}
inline void r2c_fft_f64_nd_with_planner(Slice<const double> input, Slice<double> output_re, Slice<double> output_im,
                                        const PlannerR2cNd64 &planner) {
    check(phast_r2c_fft_f64_nd_with_planner(input.ptr, input.len, output_re.ptr, output_re.len, output_im.ptr, output_im.len,
                                            planner.get()));
}
inline void r2c_fft_f32_nd_with_planner(Slice<const float> input, Slice<float> output_re, Slice<float> output_im,
                                        const PlannerR2cNd32 &planner) {
    check(phast_r2c_fft_f32_nd_with_planner(input.ptr, input.len, output_re.ptr, output_re.len, output_im.ptr, output_im.len,
                                            planner.get()));
}
inline void r2c_fft_f64_nd(Slice<const double> input, Slice<double> output_re, Slice<double> output_im,
                           const std::vector<std::size_t> &shape) {
    check(phast_r2c_fft_f64_nd(input.ptr, input.len, output_re.ptr, output_re.len, output_im.ptr, output_im.len, shape.data(),
                               shape.size()));
}
inline void r2c_fft_f32_nd(Slice<const float> input, Slice<float> output_re, Slice<float> output_im,
                           const std::vector<std::size_t> &shape) {
    check(phast_r2c_fft_f32_nd(input.ptr, input.len, output_re.ptr, output_re.len, output_im.ptr, output_im.len, shape.data(),
                               shape.size()));
}
inline void c2r_fft_f64_nd_with_planner(Slice<const double> input_re, Slice<const double> input_im, Slice<double> output,
                                        const PlannerR2cNd64 &planner) {
    check(phast_c2r_fft_f64_nd_with_planner(input_re.ptr, input_re.len, input_im.ptr, input_im.len, output.ptr, output.len,
                                            planner.get()));
}
inline void c2r_fft_f32_nd_with_planner(Slice<const float> input_re, Slice<const float> input_im, Slice<float> output,
                                        const PlannerR2cNd32 &planner) {
    check(phast_c2r_fft_f32_nd_with_planner(input_re.ptr, input_re.len, input_im.ptr, input_im.len, output.ptr, output.len,
                                            planner.get()));
}
inline void c2r_fft_f64_nd(Slice<const double> input_re, Slice<const double> input_im, Slice<double> output,
                           const std::vector<std::size_t> &shape) {
    check(phast_c2r_fft_f64_nd(input_re.ptr, input_re.len, input_im.ptr, input_im.len, output.ptr, output.len, shape.data(),
                               shape.size()));
}
inline void c2r_fft_f32_nd(Slice<const float> input_re, Slice<const float> input_im, Slice<float> output,
                           const std::vector<std::size_t> &shape) {
    check(phast_c2r_fft_f32_nd(input_re.ptr, input_re.len, input_im.ptr, input_im.len, output.ptr, output.len, shape.data(),
                               shape.size()));
}

}  // namespace phastft
#endif
