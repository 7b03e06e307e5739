// channelizer.hpp -- the polyphase filter-bank channelizer, the analysis side of a uniform DFT filter bank.
//
// Signal x of L samples (real: one plane; complex: planes re and im), K real taps h, M channels, hop D; zero extension:
//     full_frames = (L + K - 2) div D + 1
//     y[m, k] = sum_n h[m D - n] x[n] exp(-2 pi i k n / M),   0 <= m < full_frames, 0 <= k < M;   y[m, .] = 0 for m >= full_frames
//     out[i]  = y[first_frame + i],                            0 <= i < out_frames
// so channel k is upfirdn(h, x exp(-2 pi i k n / M), 1, D): the phase is referred to absolute sample time.  Polyphase form:
//     r0 = (m D - p) mod M,   T = ceil(K / M)
//     u[m][p] = sum_{j < T} h[r0 + j M] x[m D - r0 - j M]      (taps at or beyond K are 0, samples outside [0, L) are 0)
//     y[m, .] = DFT_M(u[m][.])
// The rotation by m D mod M sits in r0: there is no circular shift pass.  This file has the fold u; the transform is the
// any-length engine's (planner_channelizer.hpp).  The prototype is real, so a complex signal is the same fold on two planes.
//
// The planner keeps the taps on the device as T rows of M, zeros behind K (tab[j M + r] = h[j M + r]).  A 256-thread
// workgroup owns a tile of `frames` consecutive frames by `cols` <= 256 consecutive columns of one plane of one signal:
//     cols    min(M, 256); for M < 256 the workgroup takes `fpp` = 256 div M frames abreast
//     frames  fpp x per: thread t owns column t mod cols of the frames t div cols + i fpp, i < per, one accumulator each
//     chunk   the taps are walked in chunks of jc rows; per chunk the periods of the signal the tile meets in those rows
//             (rows of `cols` samples, M apart; at most span + jc - 1 <= kChanLds / cols of them) are brought into LDS with
//             zeros outside [0, L), so a sample comes from memory once per tile and chunk, not once per tap
// The taps come straight from the table: neighbouring columns read neighbouring taps (descending, one wrap), and where
// D mod M = 0 a column's taps do not depend on the frame, so in f64 tap j is loaded once for the `per` frames of a thread (a
// launch-uniform branch; the order of summation is the same; f32 measured faster without it).
// Every element is acc = fma(tab[j M + r0], x[m D - r0 - j M], acc) for j = 0 .. T - 1 ascending from acc = 0, in T, zero taps
// and zero samples included: its bits depend on (K, M, D) and the values alone -- not on the batch, the distances, the
// workspace, alignment, the stream or a graph replay.  No atomics; a workgroup talks to no other.
//
// The synthesis bank (the inverse) is synthesizer.hpp.  Out of scope: complex taps, subsets of the channels,
// any choice of method by size.
//
// The top of this header (argument rules, geometry) has no HIP dependency: tests/test_channelizer_cpu.py compiles it with g++.
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

constexpr unsigned long long kChanMaxLen = 1ull << 29;     // L, K, M, D
constexpr unsigned long long kChanMaxOut = 1ull << 30;     // out_frames x M
constexpr unsigned kChanLds = 4096;       // samples of the signal in LDS: f64 32 KiB, f32 16 KiB
constexpr unsigned kChanMaxCols = 256;    // columns of a tile: one per thread
constexpr unsigned kChanPerThread = 4;    // frames per thread at most

PHAST_HD unsigned long long chan_full_frames(unsigned long long len, unsigned long long k, unsigned long long d) {
    return (len + k - 2) / d + 1;
}
// taps per column
PHAST_HD unsigned long long chan_t(unsigned long long k, unsigned long long m) { return (k + m - 1) / m; }
// the first tap of column p in frame fr: (fr D - p) mod M
PHAST_HD unsigned long long chan_r0(unsigned long long fr, unsigned long long p, unsigned long long m, unsigned long long d) {
    const unsigned long long a = fr * d % m;
    return a >= p ? a - p : a + m - p;
}

struct ChanGeom {
    unsigned cols;    // columns of a tile
    unsigned fpp;     // frames abreast: 256 div cols, fewer where the hop is long
    unsigned per;     // frames per thread
    unsigned frames;  // frames of a tile: fpp x per
    unsigned span;    // periods between the newest samples of a tile's columns, at most: ceil((frames - 1) D / M) + 2
    unsigned jc;      // tap rows per chunk
    unsigned rows;    // periods in LDS: span + jc - 1; rows x cols <= kChanLds
};
// The schedule: a function of (K, M, D) alone.  The tile is as many frames as 256 threads of kChanPerThread accumulators
// hold, fewer while the periods its newest samples span take more than half the LDS rows; jc is what is left, at most T.
PHAST_HD ChanGeom chan_geom(unsigned long long k, unsigned long long m, unsigned long long d) {
    ChanGeom g;
    g.cols = m < kChanMaxCols ? (unsigned)m : kChanMaxCols;
    g.fpp = 256 / g.cols;
    g.per = kChanPerThread;
    const unsigned max_rows = kChanLds / g.cols;  // >= 16
    for (;;) {
        g.frames = g.fpp * g.per;
        const unsigned long long span = ((g.frames - 1) * d + m - 1) / m + 2;
        if (span <= max_rows / 2 || g.frames == 1) {
            g.span = (unsigned)span;  // frames == 1: 2
            break;
        }
        if (g.per > 1) g.per /= 2;
        else g.fpp /= 2;
    }
    const unsigned long long t = chan_t(k, m);
    const unsigned room = max_rows - g.span + 1;
    g.jc = t < room ? (unsigned)t : room;
    g.rows = g.span + g.jc - 1;
    return g;
}
// the periods q (samples q M + p) that the frames [m0, m0 + n) meet in the columns [p0, p0 + c) and the tap rows
// [j0, j0 + jc): q_lo .. q_lo + count - 1; q_lo may be negative
PHAST_HD void chan_span(unsigned long long m0, unsigned long long n, unsigned long long p0, unsigned long long c,
                        unsigned long long m, unsigned long long d, unsigned long long j0, unsigned long long jc,
                        long long *q_lo, unsigned long long *count) {
    const long long lo = (long long)(m0 * d) - (long long)(p0 + c - 1), hi = (long long)((m0 + n - 1) * d) - (long long)p0;
    const long long mm = (long long)m;
    const long long fl = lo >= 0 ? lo / mm : -((-lo + mm - 1) / mm), fh = hi >= 0 ? hi / mm : -((-hi + mm - 1) / mm);
    *q_lo = fl - (long long)(j0 + jc - 1);
    *count = (unsigned long long)(fh - fl) + jc;
}

// The argument rules of a channelizer planner, before the device is touched: 0 when legal.  out_frames = 0 stands for
// full_frames - first_frame (which must then be at least 1).
PHAST_HD int chan_bad_args(unsigned long long len, unsigned long long k, unsigned long long m, unsigned long long d,
                           unsigned long long first, unsigned long long out_frames) {
    if (len < 1 || len > kChanMaxLen || k < 1 || k > kChanMaxLen) return 1;
    if (m < 1 || m > kChanMaxLen || d < 1 || d > kChanMaxLen) return 1;
    const unsigned long long full = chan_full_frames(len, k, d);
    if (first > full) return 1;
    if (out_frames == 0) out_frames = full - first;
    if (out_frames < 1 || out_frames > kChanMaxOut || out_frames * m > kChanMaxOut) return 1;
    return 0;
}

}  // namespace phast

#if defined(__HIPCC__)
#include "any_len.hpp"

namespace phast {

// The fold.  Rows are the frames of the flattened (signal, frame) index q = b out_frames + i; a launch writes the rows
// [q0, q0 + count) at out + (q - q0) ld.  Tiles are counted from frame 0 of signal 0, whatever q0 is: workgroup w of the
// launch owns column tile (w mod ctiles) of frame tile ft0 + (w div ctiles) mod ..., of plane w div (tiles of a plane).
struct ChanArgs {
    const void *x[2];    // the planes of the caller's signals, signal b at b * sig_dist
    void *out[2];        // the rows of the fold, per plane
    const void *taps;    // T rows of M
    unsigned long long sig_dist, ld;
    unsigned long long len, t, m, d, first, out_frames;
    unsigned long long q0, count;  // the rows of this call
    unsigned long long ft0;        // the first frame tile of this call: (q0 div out_frames) ftiles + (q0 mod out_frames) div frames
    unsigned long long ftn;        // its frame tiles
    unsigned long long ftiles;     // frame tiles per signal
    unsigned long long ctiles;     // column tiles per frame
    unsigned long long groups;     // 256 x the workgroups of this call: planes x ftn x ctiles
    unsigned long long g0;         // first group of this launch (launches split at 2^31 - 1 workgroups)
    unsigned dqv, dm;              // D div M (saturated: used only where the tile has more than one frame) and D mod M
    unsigned sq, sm;               // (fpp D) div M and mod M: from one of a thread's frames to its next
    ChanGeom geom;
};
template <typename T> hipError_t launch_chan_fold(const ChanArgs &a, hipStream_t stream);

}  // namespace phast
#endif
