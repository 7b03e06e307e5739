// synthesizer.hpp -- the polyphase synthesis filter bank, the inverse side of the channelizer (channelizer.hpp).
//
// Channel data Y[m, k] of F frames by M channels, K real taps g, hop D; zero extension as upfirdn:
//     full_len = (F - 1) D + K
//     s[n]   = sum_m g[n - m D] sum_k Y[m, k] exp(+2 pi i k n / M),   0 <= n < full_len;   s[n] = 0 for n >= full_len
//     out[i] = s[first + i],                                          0 <= i < out_len
// so s = sum_k exp(2 pi i k n / M) upfirdn(g, Y[:, k], D, 1): the phase is referred to absolute sample time, as on the analysis
// side, and the sum over k is unnormalised.  Polyphase form:
//     v[m][p] = sum_k Y[m, k] exp(2 pi i k p / M)                     (an unnormalised inverse DFT of M points, periodic in p)
//     s[n]    = sum_{m = m_lo(n)}^{m_hi(n)} g[n - m D] v[m][n mod M]
//     m_lo(n) = max(0, ceil((n - K + 1) / D)),   m_hi(n) = min(F - 1, floor(n / D))
// An output sample is a gather of at most ceil(K / D) terms.  The rotation by m D mod M sits in the column n mod M, which does
// not depend on the frame: there is no circular shift pass.  This file has the gather, the unfold; the transform is the
// any-length engine's inverse (planner_synthesizer.hpp), which carries 1/M, so the planner keeps the taps on the device as
// tab[j] = M g[j] (the product in double, rounded once to T), in the order of g.  Real output (one plane, v by irfft
// semantics: the imaginary parts of bin 0 and, for even M, of bin M / 2 are ignored) and complex output (two planes) are the
// same unfold: the prototype is real.
//
// A 256-thread workgroup owns a tile of kSynthTile consecutive output samples of one plane of one signal; thread t owns the
// samples t + 256 i, i < kSynthPer, so neighbouring lanes read neighbouring columns of a row of v (with one wrap at M),
// neighbouring taps and write neighbouring samples.  Nothing is staged in LDS: the rows and the taps come through the caches
// (DESIGN.md §29 has the measurement).  Every output is acc = fma(tab[n - m D], v[m][n mod M], acc) for m = m_lo .. m_hi
// ascending from acc = 0, in T; a thread walks its kSynthPer chains side by side and skips the terms a chain does not have, so
// the bits depend on (F, K, M, D) and the values alone -- not on the batch, the distances, the workspace, alignment, the
// stream or a graph replay.  An output with no term (m_lo > m_hi: every n >= full_len, and gaps where D > K) is 0.  No
// atomics; a workgroup talks to no other.
//
// Out of scope: complex taps, subsets of the channels, fusing the unfold behind the transform's last pass.
//
// The top of this header (argument rules, geometry) has no HIP dependency: tests/test_synthesizer_cpu.py compiles it with g++.
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

constexpr unsigned long long kSynthMaxLen = 1ull << 29;  // F, K, M, D
constexpr unsigned long long kSynthMaxOut = 1ull << 30;  // F x M; out_len
constexpr unsigned kSynthPer = 4;                        // output samples per thread
constexpr unsigned kSynthTile = 256 * kSynthPer;         // output samples per workgroup

PHAST_HD unsigned long long synth_full_len(unsigned long long f, unsigned long long k, unsigned long long d) {
    return (f - 1) * d + k;
}
// the first and the last frame that reach sample n; m_lo > m_hi: none does
PHAST_HD unsigned long long synth_m_lo(unsigned long long n, unsigned long long k, unsigned long long d) {
    return n + 1 <= k ? 0 : (n - k + d) / d;  // ceil((n - K + 1) / D)
}
PHAST_HD long long synth_m_hi(unsigned long long n, unsigned long long f, unsigned long long d) {
    const unsigned long long q = n / d;
    return (long long)(q < f - 1 ? q : f - 1);
}
// the column of v that sample n reads, in every frame
PHAST_HD unsigned long long synth_col(unsigned long long n, unsigned long long m) { return n % m; }

struct SynthGeom {
    unsigned tile;   // output samples of a workgroup: 256 x per
    unsigned per;    // output samples of a thread, 256 apart
    unsigned terms;  // terms of an output at most: ceil(K / D)
    unsigned sq, sr; // 256 div D and 256 mod D: from one of a thread's samples to its next
    unsigned sm;     // 256 mod M
    unsigned kq, kr; // K div D and K mod D: m_lo from floor(n / D)
};
// The schedule: a function of (K, M, D) alone.
PHAST_HD SynthGeom synth_geom(unsigned long long k, unsigned long long m, unsigned long long d) {
    SynthGeom g;
    g.per = kSynthPer;
    g.tile = kSynthTile;
    g.terms = (unsigned)((k + d - 1) / d);
    g.sq = (unsigned)(256 / d);
    g.sr = (unsigned)(256 % d);
    g.sm = (unsigned)(256 % m);
    g.kq = (unsigned)(k / d);
    g.kr = (unsigned)(k % d);
    return g;
}

// The argument rules of a synthesizer planner, before the device is touched: 0 when legal.  out_len = 0 stands for
// full_len - first (which must then be at least 1).
PHAST_HD int synth_bad_args(unsigned long long f, unsigned long long k, unsigned long long m, unsigned long long d,
                            unsigned long long first, unsigned long long out_len) {
    if (f < 1 || f > kSynthMaxLen || k < 1 || k > kSynthMaxLen) return 1;
    if (m < 1 || m > kSynthMaxLen || d < 1 || d > kSynthMaxLen) return 1;
    if (f * m > kSynthMaxOut) return 1;
    const unsigned long long full = synth_full_len(f, k, d);
    if (first > full) return 1;
    if (out_len == 0) out_len = full - first;
    if (out_len < 1 || out_len > kSynthMaxOut) return 1;
    return 0;
}

}  // namespace phast

#if defined(__HIPCC__)
#include "any_len.hpp"

namespace phast {

// The unfold of `count` signals: signal b reads the rows v[plane] + (b F + m) ld, m < F, and writes out[plane] + b out_dist.
// Workgroup w of the launch owns tile w mod tiles of signal (w div tiles) mod count of plane w div (tiles count).
struct SynthArgs {
    const void *v[2];   // the rows of v, per plane: M points at distance ld
    void *out[2];       // the caller's signals, per plane
    const void *taps;   // K taps, M g[j]
    unsigned long long ld, out_dist;
    unsigned long long f, k, m, d, first, out_len;
    unsigned long long count;   // signals of this call
    unsigned long long tiles;   // tiles per signal: ceil(out_len / tile)
    unsigned long long groups;  // 256 x the workgroups of this call: planes x count x tiles
    unsigned long long g0;      // first group of this launch (launches split at 2^31 - 1 workgroups)
    SynthGeom geom;
};
template <typename T> hipError_t launch_synth_unfold(const SynthArgs &a, hipStream_t stream);

// rows of `n` elements from in + r in_ld to out + r out_ld, r < rows, of one or two planes: complex output's way into the
// workspace, and real output's copy of the imaginary plane with the columns zero_a and zero_b written as 0 (bin 0 and bin
// M / 2 for even M >= 4, where the engine's C2R does not ignore them; a column >= n names none)
struct SynthCopyArgs {
    const void *in[2];
    void *out[2];
    unsigned long long n, in_ld, out_ld, rows;
    unsigned long long zero_a, zero_b;
    unsigned long long groups;  // planes x rows x n threads
    unsigned long long g0;
};
template <typename T> hipError_t launch_synth_copy(const SynthCopyArgs &a, hipStream_t stream);

}  // namespace phast
#endif
