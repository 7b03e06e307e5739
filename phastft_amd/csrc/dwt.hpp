// dwt.hpp -- the discrete wavelet transform of real signals and its inverse: the two-channel filter bank of
// pywt.dwt / idwt, and its cascade, pywt.wavedec / waverec, as direct LDS-tiled kernels.  PyWavelets' definitions; the formulas
// here are the authority.
//
// Filter bank.  Four real filters of one even length F, 2 <= F <= 256: dec_lo, dec_hi, rec_lo, rec_hi, host values of T, used as
// given (an odd-length biorthogonal filter is padded with a zero by the caller).
//
// Extension.  ext(x, t) for any integer t and a signal of n samples:
//     zero           0 outside [0, n)
//     constant       x[clamp(t, 0, n - 1)]
//     periodic       x[t mod n]
//     symmetric      u = t mod 2n;        x[u] if u < n, else x[2n - 1 - u]
//     reflect        u = t mod (2n - 2);  x[u] if u < n, else x[2n - 2 - u];  n = 1: x[0]
// The modulus is what makes F > n legal: the extension wraps more than once.
//
// One analysis level on n samples, H = F / 2:
//     the five modes above:  m = (n + F - 1) div 2,  cA[i] = sum_{j=0}^{F-1} dec_lo[j] ext(x, 2i + 1 - j),  0 <= i < m
//     periodization:         n' = n + (n mod 2), x[n] := x[n - 1] for odd n, m = n' / 2,
//                            cA[i] = sum_j dec_lo[j] x[(2i + H - j) mod n']
// cD is the same sum with dec_hi.  One synthesis level from m coefficients of each band:
//     the five modes:        N = 2m - F + 2,  y[r] = sum_k rec_lo[r + F - 2 - 2k] cA[k] + rec_hi[r + F - 2 - 2k] cD[k]
//                            over the k whose tap index lies in [0, F)
//     periodization:         N = 2m,          y[r] = sum_k' rec_lo[t] cA[k' mod m] + rec_hi[t] cD[k' mod m],  t = r + H - 1 - 2k',
//                            over ALL integers k' with t in [0, F): more than one tap per coefficient when F > N
// Multi-level, 1 <= J <= 32 (J above dwt_max_level is legal): n_0 = L, n_l = m of n_{l-1}.  The packed result of one signal is
// [cA_J | cD_J | cD_{J-1} | ... | cD_1], coeff_len = n_J + sum_l n_l elements: pywt.wavedec's list, concatenated.  waverec undoes
// the levels from J down and keeps, at each, the first n_{l-1} of the N reconstructed samples (N is n_{l-1} or n_{l-1} + 1).
//
// The kernels.  A 256-thread workgroup owns a tile of one signal and one level; thread t owns the items t, t + 256, ... of it.
//     analysis   a tile of kDwtTile coefficient indices.  The 2 tile + F - 2 samples the tile meets are staged THROUGH THE EXTENSION
//                MAP (the input is never padded in memory, a batch neighbour never read), split by parity into two LDS arrays:
//                lane i reads sample 2i + 1 - j, a stride of two elements as stored, consecutive elements once split.  Every
//                staged sample feeds the low-pass and the high-pass chain.
//                    acc = fma(dec[j], ext(x, 2i + 1 - j), acc), j = 0 .. F - 1 ascending from acc = 0, one chain per band
//     synthesis  a tile of kDwtTile output PAIRS (rho, rho + 1), rho = r + s even, s = F - 2 (periodization: H - 1): both outputs
//                of a pair meet the same H coefficients k' = rho / 2 - H + 1 .. rho / 2 with the taps 2d and 2d + 1,
//                d = rho / 2 - k', so one LDS read of cA[k'] and one of cD[k'] serve four FMAs.  A gather: no atomics.
//                    k' ascending (tap descending) from acc = 0; per tap acc = fma(rec_lo[t], cA, acc), acc = fma(rec_hi[t], cD, acc)
// The taps are uniform across a wave: a small device table, interleaved in the order the loops meet it, read at uniform
// addresses (scalar loads; no LDS traffic).  Tiles never reorder a sum: the bits depend on the filters, the mode and the
// values alone -- not on the batch, the distances, alignment, the chunks of the workspace, the stream or a graph replay.
// Element loads and stores throughout: pointers and distances need element alignment only.
//
// The top of this header (argument rules, geometry, the extension map) has no HIP dependency: tests/test_dwt_cpu.py compiles it
// with g++.
#pragma once

#include <cstddef>

#if defined(__HIPCC__)
#include "common.hpp"  // PHAST_HD
#else
#ifndef PHAST_HD
#define PHAST_HD inline  // the host-only top, for g++
#endif
#endif

namespace phast {

constexpr unsigned long long kDwtMaxLen = 1ull << 29;  // L
constexpr unsigned kDwtMaxFilter = 256;                // F, even
constexpr unsigned kDwtMaxLevel = 32;                  // J
// items per workgroup: coefficient indices (analysis), output pairs (synthesis); 256 threads of kDwtPerThread items
constexpr unsigned kDwtTile = 1024;
constexpr unsigned kDwtPerThread = 4;
// LDS of a workgroup, in elements of T: two arrays (analysis: the staged samples of even and of odd position in the run;
// synthesis: the staged cA and cD) of tile + F / 2 - 1 <= 1151 elements, kDwtHalfLds apart.  1168 = 16 mod 32: lane pairs
// that write one sample to each array while staging land 16 elements apart in the banks.  DESIGN.md §31 says why these sizes:
// f64 18.25 KiB, f32 9.125 KiB, eight workgroups per CU either way (the wave slots bind, not LDS).
constexpr unsigned kDwtHalfLds = 1168;

// the modes of include/phastft_hip.h (PHAST_DWT_*)
enum DwtMode : int {
    kDwtZero = 0,
    kDwtConstant = 1,
    kDwtSymmetric = 2,
    kDwtReflect = 3,
    kDwtPeriodic = 4,
    kDwtPeriodization = 5,
    kDwtModes = 6
};

// coefficients of each band of one analysis level on n samples
PHAST_HD unsigned long long dwt_level_len(unsigned long long n, unsigned f, int mode) {
    return mode == kDwtPeriodization ? (n + (n & 1)) / 2 : (n + f - 1) / 2;
}
// samples one synthesis level reconstructs from m coefficients of each band (>= 1: m >= F / 2 for the lengths an analysis gives)
PHAST_HD unsigned long long dwt_synth_len(unsigned long long m, unsigned f, int mode) {
    return mode == kDwtPeriodization ? 2 * m : 2 * m - f + 2;
}
// pywt.dwt_max_level: floor(log2(L / (F - 1))), 0 when L < F - 1
PHAST_HD unsigned dwt_max_level(unsigned long long len, unsigned f) {
    unsigned j = 0;
    if (f < 2) return 0;
    while ((len >> (j + 1)) >= (unsigned long long)(f - 1)) ++j;
    return j;
}

// The index of the sample ext(x, t) of a signal of n samples, or -1 for a zero.  Periodization: the signal of an odd n counts
// n + 1 samples, the last one repeated.
PHAST_HD long long dwt_ext_index(int mode, long long n, long long t) {
    if (t >= 0 && t < n) return t;
    switch (mode) {
    case kDwtConstant: return t < 0 ? 0 : n - 1;
    case kDwtPeriodic: {
        const long long u = t % n;
        return u < 0 ? u + n : u;
    }
    case kDwtSymmetric: {
        long long u = t % (2 * n);
        if (u < 0) u += 2 * n;
        return u < n ? u : 2 * n - 1 - u;
    }
    case kDwtReflect: {
        if (n == 1) return 0;
        long long u = t % (2 * n - 2);
        if (u < 0) u += 2 * n - 2;
        return u < n ? u : 2 * n - 2 - u;
    }
    case kDwtPeriodization: {
        const long long np = n + (n & 1);
        long long u = t % np;
        if (u < 0) u += np;
        return u < n ? u : n - 1;
    }
    default: return -1;  // zero
    }
}

// The index of coefficient k' of a synthesis level with m coefficients per band, or -1 for a zero: periodization wraps, the
// other modes never leave [0, m) (dwt_synth_span)
PHAST_HD long long dwt_synth_index(int mode, long long m, long long k) {
    if (k >= 0 && k < m) return k;
    if (mode != kDwtPeriodization) return -1;
    const long long u = k % m;
    return u < 0 ? u + m : u;
}

// the sample of the run that tap j of coefficient i meets is 2i + dwt_analysis_shift - j
PHAST_HD long long dwt_analysis_shift(unsigned f, int mode) { return mode == kDwtPeriodization ? (long long)(f / 2) : 1; }
// output r of a synthesis level has rho = r + dwt_synth_shift; the pair of rho = 2Q, 2Q + 1 meets k' = Q - H + 1 .. Q
PHAST_HD long long dwt_synth_shift(unsigned f, int mode) { return mode == kDwtPeriodization ? (long long)(f / 2) - 1 : (long long)f - 2; }

// the run of the input that the analysis tile of the coefficients [i0, i0 + n) meets: samples lo .. lo + count, through ext
PHAST_HD void dwt_analysis_span(unsigned long long i0, unsigned long long n, unsigned f, int mode, long long *lo,
                                unsigned long long *count) {
    *lo = 2 * (long long)i0 + dwt_analysis_shift(f, mode) - (long long)(f - 1);
    *count = 2 * n + f - 2;
}
// the pairs of a synthesis level that keeps out_len samples: Q = q_first .. q_first + pairs - 1
PHAST_HD void dwt_synth_pairs(unsigned long long out_len, unsigned f, int mode, long long *q_first, unsigned long long *pairs) {
    const long long s = dwt_synth_shift(f, mode);
    *q_first = s / 2;
    *pairs = (unsigned long long)((s + (long long)out_len - 1) / 2 - s / 2 + 1);
}
// the coefficients of each band that the synthesis tile of the pairs [q0, q0 + n) meets: k' = lo .. lo + count (periodization:
// taken mod m)
PHAST_HD void dwt_synth_span(long long q0, unsigned long long n, unsigned f, long long *lo, unsigned long long *count) {
    *lo = q0 - (long long)(f / 2) + 1;
    *count = n + f / 2 - 1;
}

struct DwtGeom {
    unsigned levels;                          // J
    unsigned long long n[kDwtMaxLevel + 1];   // n_0 = L .. n_J
    unsigned long long off[kDwtMaxLevel + 1]; // off[l], 1 <= l <= J: where cD_l starts in the packed row; off[0] = 0: cA_J
    unsigned long long coeff_len;             // n_J + sum n_l
    unsigned long long row_a, row_b;          // workspace rows of one signal: the approximations of odd and of even level < J
    unsigned tile;                            // kDwtTile
};
PHAST_HD DwtGeom dwt_geom(unsigned long long len, unsigned f, unsigned levels, int mode) {
    DwtGeom g{};
    g.levels = levels;
    g.tile = kDwtTile;
    g.n[0] = len;
    for (unsigned l = 1; l <= levels; ++l) g.n[l] = dwt_level_len(g.n[l - 1], f, mode);
    g.off[0] = 0;
    unsigned long long at = g.n[levels];
    for (unsigned l = levels; l >= 1; --l) {
        g.off[l] = at;
        at += g.n[l];
    }
    g.coeff_len = at;
    for (unsigned l = 1; l < levels; ++l) {  // n_1 and n_2, but for a signal shorter than the filter, whose levels grow
        unsigned long long &row = l % 2 ? g.row_a : g.row_b;
        if (g.n[l] > row) row = g.n[l];
    }
    return g;
}

// The argument rules of a planner, before the device is touched: 0 when legal
PHAST_HD int dwt_bad_args(unsigned long long len, unsigned long long f, unsigned long long levels, int mode) {
    if (len < 1 || len > kDwtMaxLen) return 1;
    if (f < 2 || f > kDwtMaxFilter || f % 2) return 1;
    if (levels < 1 || levels > kDwtMaxLevel) return 1;
    if (mode < 0 || mode >= kDwtModes) return 1;
    return 0;
}

}  // namespace phast

#if defined(__HIPCC__)
#include "any_len.hpp"  // launch_in_slices

namespace phast {

// one level of either kernel: workgroup w of the launch owns tile (w mod tiles) of signal (w div tiles)
struct DwtArgs {
    const void *in_lo, *in_hi;   // analysis: in_lo = the samples (in_hi unused); synthesis: cA and cD
    void *out_lo, *out_hi;       // analysis: cA and cD; synthesis: out_lo = the samples (out_hi unused)
    const void *taps;            // 2F values in the order the loop meets them (DwtPlanner::init)
    unsigned long long in_lo_dist, in_hi_dist, out_lo_dist, out_hi_dist;  // between the signals of the batch
    unsigned long long n_in;     // analysis: samples; synthesis: coefficients per band (m)
    unsigned long long n_out;    // analysis: coefficients per band (m); synthesis: samples kept
    long long q_first;           // synthesis: Q of the first pair
    unsigned long long items;    // analysis: n_out; synthesis: pairs
    unsigned long long tiles;    // tiles per signal
    unsigned long long groups;   // 256 x the workgroups of this call
    unsigned long long g0;       // first group of this launch (launches split at 2^31 - 1 workgroups)
    unsigned f;
    int mode;
};
template <typename T> hipError_t launch_dwt_analysis(const DwtArgs &a, hipStream_t stream);
template <typename T> hipError_t launch_dwt_synthesis(const DwtArgs &a, hipStream_t stream);

}  // namespace phast
#endif
