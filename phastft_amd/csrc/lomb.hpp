// lomb.hpp -- the generalised Lomb-Scargle periodogram of unevenly sampled signals around one type-3 non-uniform transform
// (DESIGN.md §26).  The definitions are scipy.signal.lombscargle's (1.15):
//
//     inputs    M times t_j, values y_j, K frequencies f_k in cycles per unit of t, weights w_j >= 0 normalised to sum w = 1
//               (none: 1 / M), floating_mean, normalize in {power, normalize, amplitude}.  phi = 2 pi f_k t_j.
//     tables    A0 = sum w e^{i phi} = C + i S,  A2 = sum w e^{2 i phi} = C2 + i S2
//               CC = (1 + C2) / 2, SS = (1 - C2) / 2, CS = S2 / 2; floating mean: CC -= C^2, SS -= S^2, CS -= C S
//               tau = atan2(2 CS, CC - SS) / 2
//               CCt = (1 + C2 cos 2 tau + S2 sin 2 tau) / 2, SSt = 1 - CCt; floating mean: Ct = C cos tau + S sin tau,
//               St = S cos tau - C sin tau, CCt -= Ct^2, SSt -= St^2; both clamped from below at finfo(T).epsneg
//     signal    Y = sum w y (floating mean; else 0), c_j = w_j (y_j - Y), A1 = sum c_j e^{i phi}
//               YC = Re A1 cos tau + Im A1 sin tau, YS = Im A1 cos tau - Re A1 sin tau, a = YC / CCt, b = YS / SSt
//               P = 2 (a YC + b YS)
//     power     P M / 4;   normalize: P / (2 YY), YY = sum w (y - Y)^2;   amplitude: (a + i b) e^{i tau}, complex
//
// The tables depend on (t, f, w) alone: the planner builds them once, in double for both types.  Per call and signal:
//     partial   (floating mean) a workgroup adds w_j (y_j - y_0) over one slab of points, in double, through an LDS tree
//               of fixed order, into one partial                                     caller y -> partials    lomb_partial
//     final     the partials of a signal in ascending slab order: Y - y_0, then YY    partials -> two doubles lomb_final
//     strength  c_j = T(w_j ((y_j - y_0) - (Y - y_0))), in double, and the partials of YY from the same residuals
//                                                                                    caller y -> workspace   lomb_strength
//     type 3    A1 = the Reverse transform of the real strengths                     NufftT3Planner (unchanged)
//     post      the rotation by tau, a, b and the normalisation                       planes -> caller        lomb_post
// The mean is carried as y_0 plus the mean difference from it (as §25 carries a segment's), and it is taken off before the
// transform: the transform's error is then eps of the signal's variation, not of its offset.  The slab length is a function
// of M alone, every sum has a fixed order and there are no atomics: the bits do not depend on the batch, on the chunking of
// the workspace, on alignment or on the stream.
//
// The top of this header (argument rules, slab rule, table and post formulas) has no HIP dependency: tests/test_lomb_cpu.py
// compiles it with g++.
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

enum LombNorm { kLombPower = 0, kLombNormalize = 1, kLombAmplitude = 2 };  // PHAST_LOMB_*

constexpr unsigned long long kLombMaxPoints = 1ull << 30;  // M and K
// The slab rule: a signal's M points are cut into slabs of Q = max(kLombMinSlab, ceil(M / kLombMaxSlabs) rounded up to
// kLombMinSlab / 2) points.  One 256-thread workgroup owns a slab (at least eight points per thread of a full slab), Q is a
// multiple of 256 groups of 16 bytes of either type, and a signal has at most kLombMaxSlabs partials for the final sweep.
constexpr unsigned long long kLombMinSlab = 2048;
constexpr unsigned long long kLombMaxSlabs = 1024;

PHAST_HD unsigned long long lomb_slab_len(unsigned long long m) {
    const unsigned long long half = kLombMinSlab / 2;
    const unsigned long long q = ((m + kLombMaxSlabs - 1) / kLombMaxSlabs + half - 1) / half * half;
    return q < kLombMinSlab ? kLombMinSlab : q;
}
PHAST_HD unsigned long long lomb_slabs(unsigned long long m, unsigned long long q) { return (m + q - 1) / q; }

// finfo(T).epsneg: the clamp of CCt and SSt
PHAST_HD double lomb_epsneg(bool f32) { return f32 ? 5.9604644775390625e-08 : 1.1102230246251565e-16; }

// The argument rules of a planner that need no grid: 0 when legal.  (The planner then asks nufft_t3_bad_args for both
// point sets, the one of 2 f included.)  `w` may be null.
inline int lomb_bad_args(const double *t, unsigned long long m, const double *f, unsigned long long k, const double *w) {
    if (!t || !f || m == 0 || m > kLombMaxPoints || k == 0 || k > kLombMaxPoints) return 1;
    for (unsigned long long j = 0; j < m; ++j)
        if (!std::isfinite(t[j])) return 1;
    for (unsigned long long i = 0; i < k; ++i)
        if (!std::isfinite(f[i]) || !std::isfinite(2 * f[i])) return 1;
    if (w) {
        long double sum = 0;
        for (unsigned long long j = 0; j < m; ++j) {
            if (!std::isfinite(w[j]) || w[j] < 0) return 1;
            sum += w[j];
        }
        if (!(sum > 0) || !std::isfinite((double)sum)) return 1;
    }
    return 0;
}

// the weights normalised to sum 1 (null: 1 / M), in double
inline void lomb_weights(const double *w, unsigned long long m, double *out) {
    if (!w) {
        for (unsigned long long j = 0; j < m; ++j) out[j] = 1.0 / (double)m;
        return;
    }
    long double sum = 0;
    for (unsigned long long j = 0; j < m; ++j) sum += w[j];
    for (unsigned long long j = 0; j < m; ++j) out[j] = (double)((long double)w[j] / sum);
}

// the four table values of one frequency from A0 = (c, s) (ignored without the floating mean) and A2 = (c2, s2):
// cos tau, sin tau, CCt and SSt, clamped at epsneg
PHAST_HD void lomb_table(double c, double s, double c2, double s2, int floating_mean, double epsneg, double *cos_tau,
                         double *sin_tau, double *cct, double *sst) {
    double cc = 0.5 * (1 + c2), ss = 0.5 * (1 - c2), cs = 0.5 * s2;
    if (floating_mean) {
        cc -= c * c;
        ss -= s * s;
        cs -= c * s;
    }
    const double tau = 0.5 * atan2(2 * cs, cc - ss);
    const double ct = cos(tau), st = sin(tau);
    double a = 0.5 * (1 + c2 * (ct * ct - st * st) + s2 * (2 * ct * st));
    double b = 1 - a;
    if (floating_mean) {
        const double c_t = c * ct + s * st, s_t = s * ct - c * st;
        a -= c_t * c_t;
        b -= s_t * s_t;
    }
    *cos_tau = ct;
    *sin_tau = st;
    *cct = a < epsneg ? epsneg : a;
    *sst = b < epsneg ? epsneg : b;
}

// one frequency of one signal from A1 = (ar, ai) and the tables (icc = 1 / CCt, iss = 1 / SSt): the coefficients a, b and
// the power P = 2 (a YC + b YS)
PHAST_HD double lomb_post(double ar, double ai, double ct, double st, double icc, double iss, double *a, double *b) {
    const double yc = ar * ct + ai * st;
    const double ys = ai * ct - ar * st;
    *a = yc * icc;
    *b = ys * iss;
    return 2 * (*a * yc + *b * ys);
}

}  // namespace phast

#if defined(__HIPCC__)
#include "any_len.hpp"

namespace phast {

enum LombKind { kLombPartial = 0, kLombFinal = 1, kLombStrength = 2, kLombPost = 3 };

// one sweep over `groups` thread groups.  partial and strength: a group is one thread, 256 of them (one workgroup) own slab
// s of signal b, workgroup b * slabs + s.  final: a group is one thread, workgroup b owns signal b.  post: V = 16 / sizeof(T)
// consecutive frequencies of one signal.
struct LombArgs {
    const void *y;           // partial, strength: the caller's signals, signal b at b * sig_dist
    const void *w;           // partial, strength: the M weights as T (md elements, zeros beyond M)
    double *part;            // partial, strength: out; final: in.  [c][slabs] partials of this pass
    double *stat;            // final: out; strength, post: in.  [c][2]: Y - y_0 and YY of signal b of the chunk
    void *strength;          // strength: the workspace plane, md apart
    const void *re, *im;     // post: A1's planes, kd apart
    const void *tab[4];      // post: cos tau, sin tau, 1 / CCt, 1 / SSt; kd elements of T each
    void *out_re, *out_im;   // post: the caller's outputs, signal b at b * out_dist (out_im: amplitude only)
    unsigned long long sig_dist, out_dist;
    unsigned long long m, k, md, kd;
    unsigned long long q, slabs;  // points per slab, slabs per signal
    unsigned long long groups;    // groups in this launch
    unsigned long long g0;        // first group of this launch (launches split at 2^31 - 1 workgroups)
    unsigned gpt;                 // post: groups per signal, kd / V
    int which;                    // final: 0 = Y - y_0 from the first pass, 1 = YY from the second
    int floating_mean;            // strength: take Y off (stat holds it)
    int norm;                     // post: LombNorm
    double scale;                 // final: 1 / sum of the rounded weights; post: M / 4 (power)
};
// vec (post): the caller's output planes and out_dist allow 16-byte stores
template <typename T> hipError_t launch_lomb(int kind, bool vec, const LombArgs &a, hipStream_t stream);

}  // namespace phast
#endif
