// mdct.hpp -- the modified discrete cosine transform and its inverse around one DCT-IV (dct4.hpp) of N points.
//
// N coefficients per frame (N even, h = N / 2), frame length 2N, hop N, window w[0..2N), frame t starts at s_t = (t - padded) N:
//     forward  X_t[k] = sum_{n < 2N} w[n] x[s_t + n] cos(pi/N (n + 1/2 + N/2)(k + 1/2)),  x = 0 outside [0, L); no scale
//         fold    xw[n] = w[n] x[s_t + n];  u[n] = -xw[3h-1-n] - xw[3h+n] (n < h),  xw[n-h] - xw[3h-1-n] (h <= n < N)
//         pre     fold and the DCT-IV's pre-twiddle in one pass               caller x -> workspace z        kMdctPre
//         FFT     Z = FFT_h(z)                                                AnyPlanner (unchanged)
//         post    X_t = the DCT-IV's post-twiddle and de-interleave           workspace Z -> caller X        kDct4Post
//     inverse  y_t[n] = (2/N) w[n] sum_k X_t[k] cos(...);  out[s] = sum_t y_t[s - s_t], 0 <= s < L; 0 where no frame holds s
//         pre     the DCT-IV's pre-twiddle of X_t                             caller X -> workspace z        kDct4Pre
//         FFT     as above
//         post    v_t = (2/N) DCT-IV(X_t)                                     workspace Z -> workspace v     kDct4Post
//         unfold  sum_k X_t[k] cos(...) = v[n+h] (n < h), -v[3h-1-n] (h <= n < 3h), -v[n-3h] (3h <= n < 2N);
//                 window and overlap-add as a gather of at most two frames    workspace v -> caller out      kMdctOla
// padded = 1: frames = ceil(L / N) + 1, every sample lies in exactly two frames.  padded = 0: frames = floor(L / N) - 1
// (L >= 2N), the tail beyond (frames + 1) N is not read.  There is no division by an envelope: with w[n]^2 + w[n+N]^2 = 1 and
// w[2N-1-n] = w[n] the time-domain aliasing of neighbouring frames cancels (TDAC) and the inverse returns x.
//
// The top of this header (frame count, fold and unfold indices, argument rules, the window's TDAC defect) has no HIP
// dependency: tests/test_mdct_cpu.py compiles it with g++.
#pragma once

#include <cstddef>

#include "dct4.hpp"

namespace phast {

constexpr unsigned long long kMdctMaxLen = 1ull << 29;          // L and N
constexpr unsigned long long kMdctMaxFramePoints = 1ull << 30;  // frames * N

PHAST_HD unsigned long long mdct_frames(unsigned long long len, unsigned long long n, int padded) {
    return padded ? (len + n - 1) / n + 1 : len / n - 1;
}
// the fold: u[n] = -xw[mdct_fold_a(n, h)] + sign xw[mdct_fold_b(n, h, &sign)]
PHAST_HD unsigned long long mdct_fold_a(unsigned long long n, unsigned long long h) { return 3 * h - 1 - n; }
PHAST_HD unsigned long long mdct_fold_b(unsigned long long n, unsigned long long h, int *sign) {
    *sign = n < h ? -1 : 1;
    return n < h ? 3 * h + n : n - h;
}
// the unfold: point n < 2N of the frame's 2N-point sum is sign v[mdct_unfold(n, h, &sign)]
PHAST_HD unsigned long long mdct_unfold(unsigned long long n, unsigned long long h, int *sign) {
    *sign = n < h ? 1 : -1;
    return n < h ? n + h : n < 3 * h ? 3 * h - 1 - n : n - 3 * h;
}

// The argument rules of a planner, before the device is touched: 0 when (L, N, padded) is legal.
inline int mdct_bad_args(unsigned long long len, unsigned long long n, int padded) {
    if (n < 2 || (n & 1) || n > kMdctMaxLen || len < 1 || len > kMdctMaxLen) return 1;
    if (padded != 0 && padded != 1) return 1;
    if (!padded && len < 2 * n) return 1;
    if (mdct_frames(len, n, padded) * n > kMdctMaxFramePoints) return 1;
    return 0;
}

// max(max_n |w[n]^2 + w[n+N]^2 - 1|, max_n |w[n] - w[2N-1-n]|) over the 2N window values, in double: 0 for a window that
// reconstructs perfectly
inline double mdct_tdac_defect(const double *w, unsigned long long n) {
    double worst = 0;
    for (unsigned long long j = 0; j < n; ++j) {
        const double p = fabs(w[j] * w[j] + w[j + n] * w[j + n] - 1.0), q = fabs(w[j] - w[2 * n - 1 - j]);
        worst = p > worst ? p : worst;
        worst = q > worst ? q : worst;
    }
    return worst;
}

}  // namespace phast

#if defined(__HIPCC__)
#include "any_len.hpp"

namespace phast {

enum MdctKind { kMdctPre = 0, kDct4Pre = 1, kDct4Post = 2, kMdctOla = 3 };

// one sweep over `groups` thread groups; a thread owns one group of V = 16 / sizeof(T) consecutive elements: of a row of each
// z plane (the pre and post sweeps) or of a signal's output (the overlap-add sweep)
struct MdctArgs {
    const void *in;     // kMdctPre: the caller's signals; kDct4Pre: the caller's coefficients; kDct4Post: Z's re plane; kMdctOla: v
    const void *in_im;  // kDct4Post: Z's im plane
    void *out;          // pre: z's re plane; kDct4Post: rows of N reals; kMdctOla: the caller's signals
    void *out_im;       // pre: z's im plane
    const void *win;    // the window, 2N elements
    const void *tw_c, *tw_s;  // cos and sin of the sweep's twiddle angles, h entries (pre: (4m+1) / (4N), post: k / N)
    unsigned long long in_dist, out_dist;  // elements between rows (kMdctPre in_dist, kMdctOla out_dist: between signals)
    unsigned long long len, n, frames;     // L, N, frames per signal
    unsigned long long q0;      // kMdctPre: the flattened (signal, frame) index of row 0
    unsigned long long groups;  // groups in this launch
    unsigned long long g0;      // first group of this launch (launches split at 2^31 - 1 workgroups)
    unsigned gpt;               // groups per row (pre, post) or per signal (overlap-add)
    int padded;
    double scale;  // kDct4Post: 1 (forward) or 2 / N (inverse)
};
// `to_caller` (kDct4Post): the rows are the caller's coefficients (non-temporal stores), not the workspace's v
template <typename T> hipError_t launch_mdct(int kind, bool to_caller, const MdctArgs &a, hipStream_t stream);

}  // namespace phast
#endif
