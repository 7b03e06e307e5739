// dct4.hpp -- the DCT of type IV of an even length N by one complex transform of h = N / 2 points.
//
//     X[k] = sum_n u[n] cos(pi/N (n + 1/2)(k + 1/2)),  k < N  (no scale):
//     pre     z[m] = (u[2m] + i u[N-1-2m]) e^{-i pi (4m+1) / (4N)},  m < h
//     FFT     Z = FFT_h(z)  (forward)                                  AnyPlanner (unchanged)
//     post    c[k] = Z[k] e^{-i pi k / N};  X[2k] = Re c[k],  X[N-1-2k] = -Im c[k],  k < h
// The transform is its own inverse up to 2 / N.  Both twiddle sets are tables of h entries that the host builds once from
// exactly reduced angles (dct4_twiddle) and rounds to T: the sweeps evaluate no sine.  mdct.hip holds the two sweeps; the
// MDCT (mdct.hpp) is the only caller today, and nothing here knows of frames or windows.
//
// This header has no HIP dependency: tests/test_mdct_cpu.py compiles it with g++.
#pragma once

#include <cmath>

#if defined(__HIPCC__)
#include "common.hpp"  // PHAST_HD
#else
#ifndef PHAST_HD
#define PHAST_HD inline  // host-only, for g++
#endif
#endif

namespace phast {

// pre: the sources of the real and the imaginary part of z[m]
PHAST_HD unsigned long long dct4_re_src(unsigned long long m) { return 2 * m; }
PHAST_HD unsigned long long dct4_im_src(unsigned long long m, unsigned long long n) { return n - 1 - 2 * m; }
// post: where Re c[k] and -Im c[k] land
PHAST_HD unsigned long long dct4_re_dst(unsigned long long k) { return 2 * k; }
PHAST_HD unsigned long long dct4_im_dst(unsigned long long k, unsigned long long n) { return n - 1 - 2 * k; }
// the twiddles' angles as exact fractions of pi: pre (4m+1) / (4N), post k / N = 4k / (4N); both below 1/2 for m, k < h
PHAST_HD unsigned long long dct4_pre_num(unsigned long long m) { return 4 * m + 1; }
PHAST_HD unsigned long long dct4_post_num(unsigned long long k) { return 4 * k; }

// cos and sin of pi num / den for 0 <= num / den <= 1/2, in long double: the angle is reduced in integers to [0, pi/4], where
// both functions are well conditioned, so the result rounds to T with an error of half an ulp plus ~1e-19
inline void dct4_twiddle(unsigned long long num, unsigned long long den, long double *c, long double *s) {
    const long double pi = 3.14159265358979323846264338327950288L;
    if (4 * num <= den) {
        const long double a = pi * (long double)num / (long double)den;
        *c = cosl(a);
        *s = sinl(a);
    } else {  // cos(pi x) = sin(pi (1/2 - x)): 1/2 - x = (den - 2 num) / (2 den), exact
        const long double a = pi * (long double)(den - 2 * num) / (long double)(2 * den);
        *c = sinl(a);
        *s = cosl(a);
    }
}

}  // namespace phast
