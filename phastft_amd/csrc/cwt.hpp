// cwt.hpp -- the continuous wavelet transform and the analytic signal: one forward transform, a bank of filters given in
// closed form in the frequency domain, one inverse transform per filter (Torrence & Compo 1998).
//
// Samples at unit spacing, scales in samples.  A real or complex signal x of L points, zero-extended to P points
// (L <= P <= 2^29), S scales s_j (finite doubles > 0, any order, repeats allowed):
//     X       = fft_P(x)                                     (numpy's convention)
//     w_k     = 2 pi k / P for k <= P div 2, 2 pi (k - P) / P above     (for even P the bin P / 2 counts as positive)
//     W[j, n] = ifft_P( X[k] conj( c_j psi0^(s_j w_k) ) )[n],  n < L
// in two planes of shape (batch, S, L).  Families (Torrence & Compo's table 1, the frequency-domain column; H(x) = 1 for
// x > 0, else 0):
//     MORLET(w0 > 0)            pi^(-1/4) H(x) exp(-(x - w0)^2 / 2)
//     PAUL(integer m, 1..85)    2^m / sqrt(m (2m - 1)!) H(x) x^m exp(-x)
//     DOG(integer m, 1..170)    -(i^m) / sqrt(Gamma(m + 1/2)) x^m exp(-x^2 / 2)       (m = 2: the Mexican hat)
//     STEP                      1 at k = 0 and at k = P / 2 (even P), 2 for 0 < k < P / 2, 0 above; no scale, no norm:
//                               with one scale the analytic signal, scipy.signal.hilbert(x, N=P)[:L]
// The caps on m are where (2m - 1)! and Gamma(m + 1/2) stay finite in double.  The transform is DEFINED by these
// frequency-domain formulas (for odd m of DOG the paper's time-domain column differs by a sign).  Norms:
//     L2      c_j = sqrt(2 pi s_j)             (Torrence & Compo eq. 6 at dt = 1: unit energy)
//     PEAK    c_j = 2 / max_x |psi0^(x)|       (a unit sinusoid at the centre frequency has |W| = 1 for the analytic families)
// with max |psi0^| = pi^(-1/4) (Morlet), 2^m m^m e^-m / sqrt(m (2m - 1)!) (Paul), m^(m/2) e^(-m/2) / sqrt(Gamma(m + 1/2)) (DOG).
//
// The bank kernel writes Y[row, k] = X[signal, k] conj(c_j psi0^(s_j w_k)) for the rows (signal, scale) of a chunk and all
// k < P into two planes of rows.  A 256-thread workgroup owns a tile of 256 x 16 bytes of consecutive bins of a group of
// kCwtGroup scales of one signal: a thread loads its 16 bytes of X per plane once and walks the scales of the group; per scale
// one evaluation per bin, one product of a complex number with a real or unit-imaginary one, one 16-byte store per plane where
// the row is 16-byte aligned (element stores otherwise).  The device tables hold, per scale, s_j and g_j = c_j times the
// family's constant, both in double; they are wave-uniform reads.  No LDS, no atomics, no cross-lane operations.
// Real input keeps the one-sided spectrum (P div 2 + 1 bins): the bins above P div 2 are zeros for the analytic families
// (nothing is read) and the mirrored bin conjugated for DOG.
//
// The expression order (tests/cpp/cwt_emu_test.cpp pins it), in double in both types, kk = k or k - P:
//     x      = s_j * ((6.283185307179586 * (double)kk) / (double)P)
//     MORLET d = x - w0;  h = x > 0 ? g_j * E(-0.5 * d * d) : 0
//     PAUL   y = x * E(-x / m);          h = x > 0 ? g_j * ipow(y, m) : 0
//     DOG    y = x * E(-(x * x) / (2 m));  h = g_j * ipow(y, m)
//     ipow(y, m): r = 1; for (e = m; e; e >>= 1) { if (e & 1) r *= y; y *= y; }       (no intermediate passes the result)
//     E(a) = exp(a) in double in both types (f32 with expf missed the error budget: DESIGN.md §30)
//     (Paul: also 0 unless E > 0; DOG: 0 unless E > 0 -- an overflowed x must not meet an underflowed E)
//     hT = (T)h; Y = (X.re * hT, X.im * hT) times the unit factor of DOG: conj(-(i^m)) = -1, i, 1, -i for m mod 4 = 0, 1, 2, 3
//     (a swap of planes and a sign); STEP: hT = the gain above.
// Every element is a function of X[k], s_j, g_j, k and P alone: the bits do not depend on the tile, the scale group, the chunk,
// the batch, alignment, the stream or a graph replay.
//
// Out of scope: the inverse transform, real output by C2R for DOG of real signals, a fused |W|^2, pruning rows of narrow
// support, other families, padding other than zeros.
//
// The top of this header (argument rules, geometry) has no HIP dependency: tests/test_cwt_cpu.py compiles it with g++.
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

constexpr unsigned long long kCwtMaxLen = 1ull << 29;     // L, P
constexpr unsigned long long kCwtMaxScales = 1ull << 20;  // S
constexpr unsigned kCwtGroup = 8;                         // scales a workgroup walks
constexpr int kCwtMorlet = 0, kCwtPaul = 1, kCwtDog = 2, kCwtStep = 3;
constexpr int kCwtL2 = 0, kCwtPeak = 1;
constexpr int kCwtPaulMaxM = 85, kCwtDogMaxM = 170;

PHAST_HD unsigned long long cwt_round_up(unsigned long long n, unsigned long long v) { return (n + v - 1) / v * v; }
// bins of the spectrum kept per signal
PHAST_HD unsigned long long cwt_bins(unsigned long long p, int real_input) { return real_input ? p / 2 + 1 : p; }
// the signed frequency index of bin k
PHAST_HD long long cwt_signed_bin(unsigned long long k, unsigned long long p) {
    return k <= p / 2 ? (long long)k : (long long)k - (long long)p;
}
// the STEP family's gain at bin k
PHAST_HD double cwt_step_gain(unsigned long long k, unsigned long long p) {
    if (k == 0 || 2 * k == p) return 1.0;
    return 2 * k < p ? 2.0 : 0.0;
}
// is the filter 0 above P div 2 whatever the scale?
PHAST_HD bool cwt_analytic(int family) { return family != kCwtDog; }

struct CwtGeom {
    unsigned v;                // elements of 16 bytes
    unsigned tile;             // bins of a workgroup: 256 v
    unsigned group;            // scales of a workgroup at most
    unsigned long long tiles;  // tiles of a row: ceil(P / tile)
    unsigned long long ngrp;   // scale groups of a signal: ceil(S / group)
    unsigned long long bins;   // bins of X per signal
    unsigned long long xd;     // distance of the signals' X planes: bins rounded up to 16 bytes
    unsigned long long rd;     // distance of workspace rows: P rounded up to 16 bytes
};
PHAST_HD CwtGeom cwt_geom(unsigned long long p, unsigned long long s, int real_input, unsigned elem_size) {
    CwtGeom g;
    g.v = 16 / elem_size;
    g.tile = 256 * g.v;
    g.group = kCwtGroup;
    g.tiles = (p + g.tile - 1) / g.tile;
    g.ngrp = (s + g.group - 1) / g.group;
    g.bins = cwt_bins(p, real_input);
    g.xd = cwt_round_up(g.bins, g.v);
    g.rd = cwt_round_up(p, g.v);
    return g;
}

// The rows of a call are (signal, scale) pairs in signal-major order: row = b S + j.  A chunk is `r` consecutive rows from
// row0 on; it touches the signals row0 div S .. (row0 + r - 1) div S.
PHAST_HD unsigned long long cwt_first_signal(unsigned long long row0, unsigned long long s) { return row0 / s; }
PHAST_HD unsigned long long cwt_signals(unsigned long long row0, unsigned long long r, unsigned long long s) {
    return (row0 + r - 1) / s - row0 / s + 1;
}
// ... and at most this many wherever a chunk of r rows starts, in a call of `batch` signals
PHAST_HD unsigned long long cwt_max_signals(unsigned long long r, unsigned long long s, unsigned long long batch) {
    const unsigned long long worst = (r + 2 * s - 2) / s;  // a chunk that starts at the last scale of a signal
    return worst < batch ? worst : batch;
}
// the scale groups a chunk launches, counted over the whole call (group = b ngrp + j div group): the first and how many
PHAST_HD unsigned long long cwt_first_group(unsigned long long row0, unsigned long long s, unsigned long long ngrp) {
    return row0 / s * ngrp + row0 % s / kCwtGroup;
}
PHAST_HD unsigned long long cwt_groups(unsigned long long row0, unsigned long long r, unsigned long long s, unsigned long long ngrp) {
    return cwt_first_group(row0 + r - 1, s, ngrp) - cwt_first_group(row0, s, ngrp) + 1;
}
// Elements of workspace a chunk of r rows needs: per signal it touches sig_per (the X planes, the padded input, the forward
// transform's own workspace), per row row_per (the row's two planes when P > L, the inverse transform's own workspace), and
// v - 1 to reach a 16-byte boundary.
PHAST_HD unsigned long long cwt_need(unsigned long long r, unsigned long long s, unsigned long long batch, unsigned long long sig_per,
                                     unsigned long long row_per, unsigned v) {
    return cwt_max_signals(r, s, batch) * sig_per + r * row_per + (v - 1);
}
// the largest chunk (rows) that fits `len` elements, at most `total` = batch S rows; 0: not even one row fits
PHAST_HD unsigned long long cwt_rows_per_chunk(unsigned long long len, unsigned long long total, unsigned long long s,
                                               unsigned long long batch, unsigned long long sig_per, unsigned long long row_per,
                                               unsigned v) {
    if (cwt_need(1, s, batch, sig_per, row_per, v) > len) return 0;
    unsigned long long lo = 1, hi = total;  // need(lo) fits; need() does not decrease
    while (lo < hi) {
        const unsigned long long mid = lo + (hi - lo + 1) / 2;
        if (cwt_need(mid, s, batch, sig_per, row_per, v) <= len) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// The argument rules of a planner, before the device is touched: 0 when legal.  `param`: w0 (Morlet), m (Paul, DOG; an
// integer), ignored by STEP.
PHAST_HD int cwt_bad_args(unsigned long long l, unsigned long long p, unsigned long long s, int family, double param, int norm) {
    if (l < 1 || p < l || p > kCwtMaxLen || s < 1 || s > kCwtMaxScales) return 1;
    if (norm != kCwtL2 && norm != kCwtPeak) return 1;
    if (family == kCwtMorlet) return !(param > 0 && param <= 1e6);
    if (family == kCwtPaul || family == kCwtDog) {
        const int cap = family == kCwtPaul ? kCwtPaulMaxM : kCwtDogMaxM;
        return !(param >= 1 && param <= cap && param == (double)(int)param);
    }
    return family != kCwtStep;
}
PHAST_HD int cwt_bad_scale(double s) { return !(s > 0 && s <= 1.79769313486231570815e308); }  // NaN, inf, <= 0

// max_x |psi0^(x)| of a family, and the family's constant (both host side, in double)
// (products in long double: (2m - 1)! <= 170! and Gamma(m + 1/2) <= Gamma(170.5) are finite in double, so they are here)
inline long double cwt_family_const_l(int family, double param) {
    const long double pi = 3.141592653589793238462643383279502884L;
    const int m = (int)param;
    if (family == kCwtMorlet) return 1 / std::sqrt(std::sqrt(pi));
    if (family == kCwtPaul) {
        long double fact = 1;  // (2m - 1)!
        for (int i = 2; i <= 2 * m - 1; ++i) fact *= i;
        return std::ldexp(1.0L, m) / std::sqrt(m * fact);
    }
    if (family == kCwtDog) {
        long double gam = std::sqrt(pi);  // Gamma(m + 1/2) = sqrt(pi) prod_{i < m} (i + 1/2)
        for (int i = 0; i < m; ++i) gam *= i + 0.5L;
        return 1 / std::sqrt(gam);
    }
    return 1;
}
inline long double cwt_bare_peak_l(int family, double param) {  // max of x^m exp(-x) at x = m, of x^m exp(-x^2 / 2) at x = sqrt(m)
    if (family == kCwtPaul) return std::exp(param * (std::log((long double)param) - 1));
    if (family == kCwtDog) return std::exp(0.5L * param * (std::log((long double)param) - 1));
    return 1;
}
inline double cwt_family_const(int family, double param) { return (double)cwt_family_const_l(family, param); }
inline double cwt_family_peak(int family, double param) {
    return (double)(cwt_family_const_l(family, param) * cwt_bare_peak_l(family, param));
}
// g_j = c_j times the family's constant: what the kernel multiplies the bare x^m exp(..) with
inline double cwt_gain(int family, double param, int norm, double scale) {
    if (family == kCwtStep) return 1.0;
    if (norm == kCwtL2)
        return (double)(std::sqrt(6.283185307179586476925286766559L * (long double)scale) * cwt_family_const_l(family, param));
    return (double)(2 / cwt_bare_peak_l(family, param));
}

}  // namespace phast

#if defined(__HIPCC__)
#include "any_len.hpp"

namespace phast {

// The bank of the rows [row0, row0 + rows) of a call.  Row (b, j) lies at out[plane] + b out_sig + j out_row - out_off; the
// spectrum of signal b at x[plane] + (b - sig0) xd.
struct CwtArgs {
    const void *x[2];
    void *out[2];
    const double *scales, *gains;  // device tables, S entries each
    unsigned long long xd, out_sig, out_row, out_off;
    unsigned long long p, s, row0, rows, sig0;
    unsigned long long tiles, ngrp, grp0;  // CwtGeom; the first scale group of this call
    unsigned long long groups;             // 256 x the workgroups of this call: tiles x cwt_groups()
    unsigned long long g0;                 // first thread of this launch (launches split at 2^31 - 1 workgroups)
    double param;
    int family, real_input;
};
template <typename T> hipError_t launch_cwt_bank(const CwtArgs &a, hipStream_t stream);

// Rows of n_out elements, the first n_in copied and the rest written as 0, of one or two planes: row r of the launch is row
// row0 + r = b s + j of the call and goes from in[plane] + b in_sig + j in_row - in_off to out[plane] + b out_sig + j out_row -
// out_off.  The pad (x into P-point rows, s = 1) and the crop (the first L of each P-point row into the caller's planes).
struct CwtCopyArgs {
    const void *in[2];
    void *out[2];
    unsigned long long n_in, n_out, s, row0, rows;
    unsigned long long in_sig, in_row, in_off, out_sig, out_row, out_off;
    unsigned long long groups;  // planes x rows x n_out threads
    unsigned long long g0;
};
template <typename T> hipError_t launch_cwt_copy(const CwtCopyArgs &a, hipStream_t stream);

}  // namespace phast
#endif
