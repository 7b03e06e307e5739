// stft.hpp -- the short-time Fourier transform and its inverse around one real transform of the frame length.
//
// Signal length L, frame length F, hop H <= F, window w[0..F), p = floor(F / 2) (center) or 0, frames = 1 + (L + 2p - F) / H:
//     forward  frame    a[f][j] = w[j] x~[f H - p + j]; x~ is x, reflected or zero outside [0, L)   caller x -> workspace   kStftFrame
//              R2C      S[f] = rfft_F(a[f])                                 AnyRealPlanner (unchanged), workspace -> caller's planes
//     inverse  C2R      y[f] = irfft_F(S[f])                                AnyRealPlanner (unchanged), caller's planes -> workspace
//              overlap  out[t] = sum_f w[u - f H] y[f][u - f H] / sum_f w^2[u - f H], u = t + p, over the frames that   kStftOla
//                       hold u, in ascending f; 0 where no frame does                                workspace -> caller out
// These are torch.stft / torch.istft(length = L) with win_length = n_fft and normalized = False; the spectrogram is stored
// frame-major (torch's transposed).
//
// The top of this header (frame count, reflected index, tap range, envelope minimum) has no HIP dependency:
// tests/test_stft_cpu.py compiles it with g++.
#pragma once

#include <cstddef>
#include <vector>

#if defined(__HIPCC__)
#include "common.hpp"  // PHAST_HD
#else
#ifndef PHAST_HD
#define PHAST_HD inline  // the host-only top, for g++
#endif
#endif

namespace phast {

enum StftPad { kStftReflect = 0, kStftZero = 1 };  // PHAST_PAD_*

constexpr unsigned long long kStftMaxLen = 1ull << 29;        // L and F
constexpr unsigned long long kStftMaxFramePoints = 1ull << 30;  // frames * F

// the frames of a signal of L samples padded by p on both sides (L + 2p >= F)
PHAST_HD unsigned long long stft_frames(unsigned long long len, unsigned long long f, unsigned long long h, unsigned long long p) {
    return 1 + (len + 2 * p - f) / h;
}
// the sample of x that position i of the padded signal mirrors, -L < i < 2L - 1 (one reflection: p < L)
PHAST_HD long long stft_reflect(long long i, long long len) { return i < 0 ? -i : i >= len ? 2 * (len - 1) - i : i; }
// the frames that hold position u = t + p of the padded signal: f H <= u < f H + F, f < frames; *lo > *hi: none.  Every
// operand is below 2^31 (u < L + F), so the divisions are 32-bit ones
PHAST_HD void stft_taps(unsigned long long u, unsigned long long f, unsigned long long h, unsigned long long frames, long long *lo,
                        long long *hi) {
    const unsigned u32 = (unsigned)u, f32 = (unsigned)f, h32 = (unsigned)h;
    *lo = u32 >= f32 ? (long long)((u32 - f32) / h32 + 1) : 0;
    const unsigned long long top = u32 / h32;
    *hi = (long long)(top < frames - 1 ? top : frames - 1);
}

// The argument rules of a planner, before the device is touched: 0 when (L, F, H, center, pad_mode) is legal.
inline int stft_bad_args(unsigned long long len, unsigned long long f, unsigned long long h, int center, int pad) {
    if (h < 1 || h > f || f > kStftMaxLen || len < 1 || len > kStftMaxLen) return 1;
    if (center != 0 && center != 1) return 1;
    if (pad != kStftReflect && pad != kStftZero) return 1;
    if (center && pad == kStftReflect && f / 2 >= len) return 1;
    if (!center && len < f) return 1;
    const unsigned long long p = center ? f / 2 : 0;
    if (stft_frames(len, f, h, p) * f > kStftMaxFramePoints) return 1;
    return 0;
}

// min over the output samples t < L that some frame holds of sum_f w^2[t + p - f H], in O(L + F): the taps of position u are
// the window points j = u mod H, + H, ... between j_lo = u - hi H and j_hi = u - lo H, so the sum is a difference of the
// prefix sums S[j] = w^2[j] + S[j - H] of u's residue class (a position whose taps start at the class's first point reads S
// alone, without a subtraction).  `w` NULL: all ones.
inline double stft_envelope_min(const double *w, unsigned long long len, unsigned long long f, unsigned long long h,
                                unsigned long long p, unsigned long long frames) {
    std::vector<double> s((size_t)f);
    for (unsigned long long j = 0; j < f; ++j) {
        const double v = w ? w[j] : 1.0;
        s[(size_t)j] = v * v + (j >= h ? s[(size_t)(j - h)] : 0.0);
    }
    double best = -1.0;
    for (unsigned long long t = 0; t < len; ++t) {
        const unsigned long long u = t + p;
        long long lo, hi;
        stft_taps(u, f, h, frames, &lo, &hi);
        if (lo > hi) continue;
        const unsigned long long j_lo = u - (unsigned long long)hi * h, j_hi = u - (unsigned long long)lo * h;
        const double d = s[(size_t)j_hi] - (j_lo >= h ? s[(size_t)(j_lo - h)] : 0.0);
        if (best < 0 || d < best) best = d;
    }
    return best < 0 ? 0.0 : best;
}

}  // namespace phast

#if defined(__HIPCC__)
#include "any_len.hpp"

namespace phast {

enum StftKind { kStftFrame = 0, kStftOla = 1 };

// one sweep over `groups` thread groups; a thread owns one group of V = 16 / sizeof(T) consecutive elements: of a workspace
// row (frame sweep) or of a signal's output (overlap-add sweep)
struct StftArgs {
    const void *in;   // frame: the caller's signals; overlap-add: the workspace rows y
    void *out;        // frame: the workspace rows; overlap-add: the caller's signals
    const void *win;  // the window, fd elements (zeros beyond F)
    unsigned long long sig_dist;  // elements between the caller's signals
    unsigned long long len, f, h, p, frames;
    unsigned long long fd;      // elements between workspace rows
    unsigned long long q0;      // frame: the flattened (signal, frame) index of workspace row 0
    unsigned long long groups;  // groups in this launch
    unsigned long long g0;      // first group of this launch (launches split at 2^31 - 1 workgroups)
    unsigned gpt;               // groups per workspace row (frame) or per signal (overlap-add)
    int pad;                    // kStftReflect / kStftZero
};
template <typename T> hipError_t launch_stft(int kind, const StftArgs &a, hipStream_t stream);

}  // namespace phast
#endif
