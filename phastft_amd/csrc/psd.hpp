// psd.hpp -- Welch spectral estimation around one real transform of the segment length.  The definitions are
// scipy.signal's (welch, csd, spectrogram with mode = "psd", return_onesided = True, boundary = None, padded = False):
//
//     sizes     L samples per signal, P = nperseg, H = hop = nperseg - noverlap, F = nfft; 1 <= H <= P <= F <= 2^29,
//               P <= L <= 2^29.  Segments S = 1 + floor((L - P) / H): the tail beyond the last segment is not read.
//               bins = floor(F / 2) + 1.  fd = F rounded up to 16 bytes, S fd <= 2^30.
//     window    P host values (double); NULL: Hann, scipy.signal.get_window("hann", P), the periodic form
//               w[j] = 1/2 - 1/2 cos(2 pi j / P), built on the host in long double.
//     segment   r_f[j] = w[j] (x[f H + j] - m_f), j < P; 0 for P <= j < F.  m_f = the mean of the P samples of the segment
//               (detrend = constant, scipy's default) or 0 (detrend = none).  X_f = rfft_F(r_f).
//     scale     density: sigma = 1 / (fs sum w^2); spectrum: sigma = 1 / (sum w)^2; in double from the values given.
//     one side  c_k = 2 for every bin but c_0 = 1 and, F even, c_{F/2} = 1.
//     auto      P_xx[k] = sigma c_k (1/S) sum_f |X_f[k]|^2
//     cross     P_xy[k] = sigma c_k (1/S) sum_f conj(X_f[k]) Y_f[k]   (scipy's csd convention); two planes, re and im
//     average = 0 (spectrogram): no sum over f and no 1/S; frame-major [batch][S][bins] (scipy returns the transpose).
//
// The schedule, per chunk of whole frames of the flattened (signal, frame) index:
//     mean     d_f = m_f - x[f H] = (1/P) sum_j (x[f H + j] - x[f H]) in double, one LDS tree of fixed order per segment: the
//              mean is kept as the pair (x[f H], d_f), so that its error is eps of the signal's variation, not of its offset
//                                                                             caller x -> workspace means     psd_mean
//     frame    row = T(w[j] ((x - x[f H]) - d_f)), in double                  caller x -> workspace rows      psd_frame
//     R2C      X_f = rfft_F(row)                                              AnyRealPlanner (unchanged)
//     accum    a slab of Q frames adds, in ascending f and in double, into its partial row    planes -> partial rows   psd_accum
//     final    the partial rows of a signal in ascending slab order, times sigma c_k / S, rounded to T once    psd_final
//     point    average = 0: sigma c_k |X_f[k]|^2 of each frame's row                          planes -> caller  psd_point
// The partition of the frames into slabs is a function of (S, bins) alone, every sum runs in ascending frame order and there
// are no atomics: the bits do not depend on the batch, on the chunking of the workspace or on the stream.
//
// Out of scope: linear detrend, average = "median", two-sided output, complex input, scipy's boundary / padded extension,
// modes other than psd, one window per signal of a batch.
//
// The top of this header (segment count, slab partition, argument rules, sigma, c_k, the Hann window) has no HIP dependency:
// tests/test_psd_cpu.py compiles it with g++.
#pragma once

#include <cmath>
#include <cstddef>

#if defined(__HIPCC__)
#include "common.hpp"  // PHAST_HD
#else
#ifndef PHAST_HD
#define PHAST_HD inline  // the host-only top, for g++
#endif
#endif

namespace phast {

enum PsdDetrend { kPsdDetrendNone = 0, kPsdDetrendConstant = 1 };  // PHAST_DETREND_*
enum PsdScaling { kPsdDensity = 0, kPsdSpectrum = 1 };             // PHAST_PSD_*

constexpr unsigned long long kPsdMaxLen = 1ull << 29;          // L and F
constexpr unsigned long long kPsdMaxFramePoints = 1ull << 30;  // S * fd
// The slab rule: a signal's frames are cut into slabs of Q = max(kPsdMinSlab, floor(S bins / kPsdFillPoints)) frames.
// slabs * bins is then at least kPsdFillPoints = 2^19 wherever S allows it: 2^17 threads of four f32 bins (two waves on each
// SIMD of 256 CUs), and a slab never has fewer than 16 frames, so a partial row (one read and one write of 8 bytes per bin)
// moves at most an eighth of the bytes of the 16 spectrum rows (2 x 4 bytes per bin each) it sums.
constexpr unsigned long long kPsdMinSlab = 16;
constexpr unsigned long long kPsdFillPoints = 1ull << 19;

PHAST_HD unsigned long long psd_segments(unsigned long long len, unsigned long long p, unsigned long long h) {
    return 1 + (len - p) / h;
}
PHAST_HD unsigned long long psd_bins(unsigned long long f) { return f / 2 + 1; }
// c_k of the one-sided spectrum
PHAST_HD int psd_onesided(unsigned long long k, unsigned long long f) { return k == 0 || 2 * k == f ? 1 : 2; }
// frames per slab, from S and bins alone
PHAST_HD unsigned long long psd_slab_len(unsigned long long segments, unsigned long long bins) {
    const unsigned long long q = segments * bins / kPsdFillPoints;
    return q < kPsdMinSlab ? kPsdMinSlab : q;
}
PHAST_HD unsigned long long psd_slabs(unsigned long long segments, unsigned long long q) { return (segments + q - 1) / q; }
// the frames [*lo, *hi) of slab s that lie in [c_lo, c_hi) (the frames of the signal the current chunk holds); empty: *lo >= *hi
PHAST_HD void psd_slab_range(unsigned long long s, unsigned long long q, unsigned long long c_lo, unsigned long long c_hi,
                             unsigned long long *lo, unsigned long long *hi) {
    const unsigned long long a = s * q, b = a + q;
    *lo = a > c_lo ? a : c_lo;
    *hi = b < c_hi ? b : c_hi;
}
// threads that share one segment's mean (a power of two <= 256, from P alone): each adds at least four samples where P allows
PHAST_HD unsigned psd_mean_threads(unsigned long long p) {
    unsigned t = 1;
    while (t < 256 && 4ull * t < p) t <<= 1;
    return t;
}

// The argument rules of a planner, before the device is touched: 0 when legal.  `v`: elements of T in 16 bytes.
inline int psd_bad_args(unsigned long long len, unsigned long long p, unsigned long long h, unsigned long long f, int detrend,
                        int scaling, double fs, unsigned v) {
    if (h < 1 || h > p || p > f || f > kPsdMaxLen || len < p || len > kPsdMaxLen) return 1;
    if (detrend != kPsdDetrendNone && detrend != kPsdDetrendConstant) return 1;
    if (scaling != kPsdDensity && scaling != kPsdSpectrum) return 1;
    if (!(fs > 0) || !std::isfinite(fs)) return 1;
    const unsigned long long fd = (f + v - 1) / v * v;
    if (psd_segments(len, p, h) * fd > kPsdMaxFramePoints) return 1;
    return 0;
}

// w[j] of the periodic Hann window of P points
inline long double psd_hann(unsigned long long j, unsigned long long p) {
    if (p == 1) return 1.0L;  // (get_window returns [1.] for one point)
    const long double pi = 3.14159265358979323846264338327950288L;
    return 0.5L - 0.5L * cosl(2.0L * pi * (long double)j / (long double)p);
}

// sigma of the window's P values; 1 when the sum it divides by is 0 or not finite
inline int psd_sigma(const double *w, unsigned long long p, int scaling, double fs, double *sigma) {
    double s1 = 0, s2 = 0;
    for (unsigned long long j = 0; j < p; ++j) {
        s1 += w[j];
        s2 += w[j] * w[j];
    }
    const double d = scaling == kPsdDensity ? fs * s2 : s1 * s1;
    if (!(d > 0) || !std::isfinite(d)) return 1;
    *sigma = 1.0 / d;
    return 0;
}

}  // namespace phast

#if defined(__HIPCC__)
#include "any_len.hpp"

namespace phast {

enum PsdKind { kPsdMean = 0, kPsdFrame = 1, kPsdAccum = 2, kPsdFinal = 3, kPsdPoint = 4 };

// one sweep over `groups` thread groups.  mean: a group is one thread, psd_mean_threads(P) of them share a row.  frame: a
// group is V = 16 / sizeof(T) consecutive elements of a workspace row.  accum: V consecutive bins of a partial row.  final and
// point: V consecutive elements of the caller's packed output.  With `y` set (a cross call) the chunk's rows are the c frames
// of x followed by the same c frames of y, in the rows, the means and both planes.
struct PsdArgs {
    const void *x, *y;       // mean, frame: the caller's signals
    const double *win;       // frame: the window, fd doubles (zeros beyond P)
    double *mean;            // mean: out; frame: in (NULL: no detrend); one double per row
    void *rows;              // frame: the workspace rows, fd apart
    const void *re, *im;     // accum, point: the spectrum planes, rows bd apart
    double *acc;             // accum, final: partial rows [slot][plane][slab][bd]; a signal's slot is b mod slots
    void *out[4];            // final, point: the caller's outputs (auto: P_xx; cross: re, im, P_xx, P_yy; NULL: not asked for)
    unsigned long long sig_dist;      // elements between the caller's signals
    unsigned long long p, h, frames;  // P, H, S
    unsigned long long fd, bd, bins, nfft;
    unsigned long long q0, c;         // the flattened (signal, frame) index of row 0 and the frames of this chunk
    unsigned long long q, slabs;      // frames per slab, slabs per signal
    unsigned long long b0;            // accum, final: the first signal of this launch
    unsigned long long s0, ns;        // accum: the first slab and the number of slabs of this launch
    unsigned long long slots;         // signals the partial rows hold
    unsigned long long count;         // final, point: elements of the packed output this launch covers
    unsigned long long groups;        // groups in this launch
    unsigned long long g0;            // first group of this launch (launches split at 2^31 - 1 workgroups)
    unsigned gpt;                     // groups per row (frame, accum)
    unsigned tpr;                     // mean: threads per row
    int planes;                       // partial planes per slot: 1 (auto) or 4 (cross)
    double scale;                     // final: sigma / S; point: sigma
};
template <typename T> hipError_t launch_psd(int kind, const PsdArgs &a, hipStream_t stream);

}  // namespace phast
#endif
