// dct.hpp -- DCT / DST of types II and III of any length N around one real transform of the same N.
//
// Makhoul's algorithm, h = floor(N / 2), e = ceil(N / 2):
//     DCT-II   pre    v[i] = x[2i] (i < e), v[N-1-i] = x[2i+1] (i < h)          caller x -> workspace v      kDct2Pre
//              R2C    V = rfft(v)                                                 AnyRealPlanner (unchanged)
//              post   z = e^{-i pi k/(2N)} V[k]: y[k] = 2 f Re z (k <= h),        workspace V -> caller y      kDct2Post
//                     y[N-k] = -2 f Im z (1 <= k < e)
//     DCT-III  pre    V[k] = N f e^{+i pi k/(2N)} (X[k] - i X[N-k]), X[N] = 0     caller X -> workspace V      kDct3Pre
//              C2R    v = irfft(V, N)                                             AnyRealPlanner (unchanged)
//              post   x[2i] = v[i] (i < e), x[2i+1] = v[N-1-i] (i < h)           workspace v -> caller x      kDct3Post
// DST-II is DCT-II of x[n] (-1)^n stored reversed; DST-III is DCT-III of X reversed with (-1)^k on the output.  The DST
// therefore differs from the DCT in signs and index order only: every rounding is the same.  All scaling (the norm, the
// ortho sqrt 2 on bin 0 and the N of the C2R) sits in the twiddle sweep; the permutation sweeps move data only.
//
// The top of this header (indices, signs, scales) has no HIP dependency: tests/test_dct_cpu.py compiles it with g++.
#pragma once

#include <cmath>

#if defined(__HIPCC__)
#include "common.hpp"  // PHAST_HD
#else
#ifndef PHAST_HD
#define PHAST_HD inline  // the host-only top, for g++
#endif
#endif

namespace phast {

enum DctNorm { kDctBackward = 0, kDctOrtho = 1, kDctForward = 2 };  // PHAST_NORM_*

// the permutation: v[i] holds x[dct_perm_src(i, N)] (II-pre reads it, III-post writes it back)
PHAST_HD unsigned long long dct_perm_src(unsigned long long i, unsigned long long n) {
    return i < (n + 1) / 2 ? 2 * i : 2 * (n - 1 - i) + 1;
}
// the DST's sign on v[i]: an odd sample of x is negated (II on load, III on store)
PHAST_HD double dct_perm_sign(bool dst, unsigned long long i, unsigned long long n) {
    return dst && i >= (n + 1) / 2 ? -1.0 : 1.0;
}
// the factor of the twiddle sweep: type II 2 f, type III N f, with f = 1 (backward), 1 / sqrt(2N) (ortho), 1 / (2N) (forward)
PHAST_HD double dct_scale(int type, int norm, unsigned long long n) {
    const double f = norm == kDctForward ? 1.0 / (2.0 * (double)n) : norm == kDctOrtho ? 1.0 / sqrt(2.0 * (double)n) : 1.0;
    return (type == 2 ? 2.0 : (double)n) * f;
}
// ... and its factor at bin 0 (ortho: y[0] / sqrt 2 for II, x[0] * sqrt 2 for III; the DST's y[N-1] / x[N-1] are the same bin)
PHAST_HD double dct_scale0(int type, int norm, unsigned long long n) {
    const double s = dct_scale(type, norm, n);
    if (norm != kDctOrtho) return s;
    return type == 2 ? s * 0.70710678118654752440 : s * 1.41421356237309504880;
}
// the twiddle's angle in units of pi: e^{-i pi k / (2N)} (II), e^{+i pi k / (2N)} (III); one rounding from exact
PHAST_HD double dct_turns(int type, unsigned long long k, unsigned long long n) {
    const double t = (double)k / (double)(2 * n);
    return type == 2 ? -t : t;
}
// II-post: where bin k's real part (k <= h) and imaginary part (1 <= k < e) land
PHAST_HD unsigned long long dct2_re_index(bool dst, unsigned long long k, unsigned long long n) { return dst ? n - 1 - k : k; }
PHAST_HD unsigned long long dct2_im_index(bool dst, unsigned long long k, unsigned long long n) { return dst ? k - 1 : n - k; }
// III-pre: the sources of A = X'[k] (k <= h) and B = X'[N-k] (1 <= k <= h) of the pair behind V[k]
PHAST_HD unsigned long long dct3_a_index(bool dst, unsigned long long k, unsigned long long n) { return dst ? n - 1 - k : k; }
PHAST_HD unsigned long long dct3_b_index(bool dst, unsigned long long k, unsigned long long n) { return dst ? k - 1 : n - k; }

}  // namespace phast

#if defined(__HIPCC__)
#include "any_len.hpp"

namespace phast {

enum DctKind { kDct2Pre = 0, kDct2Post = 1, kDct3Pre = 2, kDct3Post = 3 };

// one sweep over `groups` thread groups; a thread owns one group of V = 16 / sizeof(T) consecutive workspace elements
struct DctArgs {
    const void *in;     // II-pre / III-pre: the caller's input; II-post: V's re plane; III-post: v
    const void *in_im;  // II-post: V's im plane
    void *out;          // II-pre: v; III-pre: V's re plane; II-post / III-post: the caller's output
    void *out_im;       // III-pre: V's im plane
    unsigned long long in_dist, out_dist;  // elements between transforms on either side
    unsigned long long n;                  // N
    unsigned long long groups;             // groups in this launch
    unsigned long long g0;                 // first group of this launch (launches split at 2^31 - 1 workgroups)
    unsigned gpt;                          // groups per transform
    double scale, scale0;                  // twiddle sweeps: dct_scale, dct_scale0
};
// `vec`: the caller's side allows 16-byte accesses (16-byte aligned base, dist a multiple of V); the workspace side always does
template <typename T> hipError_t launch_dct(int kind, bool dst, bool vec, const DctArgs &a, hipStream_t stream);

}  // namespace phast
#endif
