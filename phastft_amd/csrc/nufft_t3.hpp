// nufft_t3.hpp -- the non-uniform FFT of type 3 in one dimension: M sources x_j in a unit U, K target
// frequencies s_k in 1 / U, the product s_k x_j in turns,
//
//     f_k = sum_j c_j exp(-+2 pi i s_k x_j)        (- Forward, + Reverse; no scaling)
//
// With x' = x - C_x, s' = s - C_s (centres C, half-widths X and S) the phase splits exactly,
// s x = s' x' + C_s x' + s C_x, and s' x' is band-limited on both sides.  On an outer fine grid of n_f points of spacing
// h = 1 / (4 S) around x' = 0 (point l at (l - n_f / 2) h):
//
//     a   spread     g_l = sum_j phi(2 (l - p_j) / w) c_j exp(-+2 pi i C_s x'_j),  p_j = x'_j / h + n_f / 2, and, fused, the
//                    "pre" of the inner type 2: g_l / phi^_inner(k) into the slot of mode k = l - n_f / 2 of a grid of
//                    n_g = 2 n_f points, exact zeros elsewhere                                       nufft_t3_spread_kernel
//     b   FFT_{n_g}  in place on the engine                                                          NufftPlanner::transform
//     c   interpolate at the K points t_k = s'_k h turns (|t_k| <= 1 / 4)                            NufftPlanner::interpolate
//     d   post       f_k = (c)_k D_k,  D_k = exp(-+2 pi i s_k C_x) / phi^_outer(t_k)                  nufft_t3_post_kernel
//
// The two phases are formed exactly mod 1 turn (the product of two doubles is p + fma(a, b, -p)), so neither |C_x| nor |C_s|
// costs accuracy beyond the conditioning of the problem, Q = 2 pi (|C_s| + S) X.
//
// The top of this header has no HIP dependency: tests/test_nufft_t3_cpu.py compiles it with g++.
#pragma once

#include "nufft.hpp"

namespace phast {

// the schedule of a plan: fixed by the two point sets and eps
struct NufftT3Grid {
    double cx = 0, cs = 0;      // the centres C_x, C_s
    double X = 0, S = 0;        // the half-widths after the degenerate replacements
    double h = 0;               // the spacing of the outer grid, 1 / (4 S)
    unsigned long long nf = 0;  // the outer grid n_f, a power of two; 0: no grid within kNufftMaxModes
    unsigned log_f = 0;
    int w = 0;
};

// C = (min + max) / 2 and the half-width max |v_j - C|; false where either is not finite
inline bool nufft_t3_centre(const double *v, unsigned long long n, double *c, double *half) {
    double lo = v[0], hi = v[0];
    for (unsigned long long j = 1; j < n; ++j) {
        lo = v[j] < lo ? v[j] : lo;
        hi = v[j] > hi ? v[j] : hi;
    }
    *c = 0.5 * lo + 0.5 * hi;
    double r = 0;
    for (unsigned long long j = 0; j < n; ++j) {
        const double d = std::fabs(v[j] - *c);
        r = d > r ? d : r;
    }
    *half = r;
    return std::isfinite(*c) && std::isfinite(r);
}

// Centres, half-widths (X = S = 0 -> 1, 1; X = 0 -> 1 / S; S = 0 -> 1 / X), w and the outer grid: the smallest power of two
// n_f >= max(8 S X + w, 2 w, 8), held as n_f - w >= 2 fl(4 S X) -- both sides exact -- so that every p_j lies within
// [w / 2, n_f - w / 2] as computed.  nf = 0 where that exceeds kNufftMaxModes or a width is not finite.
inline NufftT3Grid nufft_t3_grid(const double *x, unsigned long long m, const double *s, unsigned long long k, double eps) {
    NufftT3Grid g;
    g.w = nufft_width(eps);
    if (!nufft_t3_centre(x, m, &g.cx, &g.X) || !nufft_t3_centre(s, k, &g.cs, &g.S)) return g;
    if (g.X == 0 && g.S == 0)
        g.X = g.S = 1;
    else if (g.X == 0)
        g.X = 1 / g.S;
    else if (g.S == 0)
        g.S = 1 / g.X;
    g.h = 1 / (4 * g.S);
    const double reach = 2 * (4 * g.S * g.X);  // 8 S X
    if (!std::isfinite(g.X) || !std::isfinite(g.S) || !std::isfinite(g.h) || !(reach <= (double)kNufftMaxModes)) return g;
    unsigned long long nf = 8;
    unsigned lg = 3;
    while ((double)nf - g.w < reach || nf < 2ull * g.w) nf <<= 1, ++lg;
    if (nf > kNufftMaxModes) return g;
    g.nf = nf;
    g.log_f = lg;
    return g;
}

// 1 <= M, K <= 2^30, eps as nufft_bad_args, every x_j and s_k finite, n_f <= 2^28, and the phases representable: the products
// C_s x'_j and s_k C_x stay finite
inline bool nufft_t3_bad_args(const double *x, unsigned long long m, const double *s, unsigned long long k, double eps, bool f32) {
    if (!x || !s || m == 0 || m > kNufftMaxPoints || k == 0 || k > kNufftMaxPoints) return true;
    if (!(eps >= (f32 ? 1e-6 : 1e-14) && eps <= 1e-1)) return true;
    for (unsigned long long j = 0; j < m; ++j)
        if (!std::isfinite(x[j])) return true;
    for (unsigned long long j = 0; j < k; ++j)
        if (!std::isfinite(s[j])) return true;
    const NufftT3Grid g = nufft_t3_grid(x, m, s, k, eps);
    if (g.nf == 0) return true;
    return !std::isfinite((std::fabs(g.cs) + g.S) * (std::fabs(g.cx) + g.X));
}

// a b mod 1 turn in [-1, 1], exact to the last rounding: a b = p + e with p = fl(a b), e = fma(a, b, -p); p - rint(p) and
// e - rint(e) are exact (e is a whole number of turns and more once |p| >= 2^53), and only then are the two added
inline long double nufft_t3_turns(double a, double b) {
    const double p = a * b, e = std::fma(a, b, -p);
    return (long double)(p - std::rint(p)) + (long double)(e - std::rint(e));
}

// (cos, sin) of 2 pi a b, rounded to T once
template <typename T> inline void nufft_t3_phase(double a, double b, T *c, T *s) {
    const long double t = 6.283185307179586476925286766559005768L * nufft_t3_turns(a, b);
    *c = (T)std::cos(t);
    *s = (T)std::sin(t);
}

// the source positions as fractions of the outer grid, u_j = p_j / n_f = 4 S x'_j / n_f + 1 / 2 in [w / 2 n_f, 1 - w / 2 n_f]:
// what nufft_bin sorts
inline void nufft_t3_positions(const NufftT3Grid &g, const double *x, unsigned long long m, double *u) {
    const double four_s = 4 * g.S, inv = 1.0 / (double)g.nf;
    for (unsigned long long j = 0; j < m; ++j) u[j] = four_s * (x[j] - g.cx) * inv + 0.5;
}

// the K points of the inner type 2, t_k = s'_k h turns per cell, |t_k| <= 1 / 4
inline void nufft_t3_targets(const NufftT3Grid &g, const double *s, unsigned long long k, double *t) {
    for (unsigned long long i = 0; i < k; ++i) t[i] = (s[i] - g.cs) * g.h;
}

// phi^_outer at xi turns per cell, |xi| <= 1 / 4: NufftQuad's rule at a real argument
struct NufftT3Hat {
    NufftQuad q;
    explicit NufftT3Hat(int w) : q(w, 1) {}
    double operator()(double xi) const { return q.at(xi); }
};

// pre[2 i], pre[2 i + 1] = (cos, sin) of 2 pi C_s x'_{perm[i]}: the prephase in sorted order
template <typename T>
inline void nufft_t3_pre_table(const NufftT3Grid &g, const double *x, const uint32_t *perm, unsigned long long m, T *pre) {
    for (unsigned long long i = 0; i < m; ++i) nufft_t3_phase<T>(g.cs, x[perm[i]] - g.cx, &pre[2 * i], &pre[2 * i + 1]);
}

// the Forward post factors D_k = exp(-2 pi i s_k C_x) / phi^_outer(t_k) as planes, in the caller's order
template <typename T>
inline void nufft_t3_post_table(const NufftT3Grid &g, const double *s, const double *t, unsigned long long k, T *d_re, T *d_im) {
    const NufftT3Hat hat(g.w);
    for (unsigned long long i = 0; i < k; ++i) {
        const long double a = 6.283185307179586476925286766559005768L * nufft_t3_turns(s[i], g.cx);
        const long double r = 1.0L / (long double)hat(t[i]);
        d_re[i] = (T)(std::cos(a) * r);
        d_im[i] = (T)(-std::sin(a) * r);
    }
}

}  // namespace phast

#if defined(__HIPCC__)
namespace phast {

// one launch of one of the two kernels over `c` transforms (nufft_t3.hip)
struct NufftT3Args {
    const void *in_re;  // spread: the caller's planes (transform b at b * in_dist); in_im null: real data.  post: unused
    const void *in_im;
    void *out_re;  // spread: the workspace (b * n_g, n_g = 2 n_f); post: the caller's planes (b * out_dist), in place
    void *out_im;
    const double *xs;            // [M] sorted positions, fractions of the outer grid in [0, 1)
    const uint32_t *perm;        // [M] original index of sorted source i
    const uint32_t *cell_start;  // [n_f + 1]
    const void *pre;             // [M][2] (cos, sin) of the prephase, sorted order
    const void *inv_hat;         // [n_f] the inner planner's 1 / phi^(k(m))
    const void *d_re, *d_im;     // [K] the Forward post factors
    unsigned long long in_dist, out_dist;
    unsigned long long k;       // K targets
    unsigned long long groups;  // spread: c n_g threads; post: c gpt groups
    unsigned long long g0;      // first group of this launch
    unsigned log_f;             // n_f = 2^log_f
    unsigned gpt;               // post: groups per transform, ceil(K / V)
    int w;                      // kernel width in cells
    int reverse;                // the + sign: both phases conjugated
};
// kind: 0 spread (one thread per slot of the inner grid, element accesses), 1 post (a streaming sweep; `vec`: the caller's
// output planes and out_dist allow 16-byte accesses)
template <typename T> hipError_t launch_nufft_t3(int kind, bool vec, const NufftT3Args &a, hipStream_t stream);

}  // namespace phast
#endif
