// resample.hpp -- sample-rate conversion of real signals: the polyphase FIR of scipy.signal.upfirdn (and with it
// resample_poly and decimate) as a direct LDS-tiled kernel, and the sweep between the two real transforms of the Fourier
// method, scipy.signal.resample.
//
// Polyphase FIR.  Signal x of L samples, K taps h, up, down >= 1 (used as given: not reduced by their gcd):
//     full[m] = sum_n h[m down - n up] x[n],   0 <= m < full_len = ((L - 1) up + K - 1) / down + 1
//     out[i]  = full[first + i],               0 <= i < out_len;  full[m] = 0 for m >= full_len
// With p = (m down) mod up and q = (m down) div up: full[m] = sum_{j >= 0, p + j up < K} h[p + j up] x[q - j], x = 0 outside
// [0, L).  The planner keeps the taps phase-major: up rows of Kp = ceil(K / up) at a stride of Kp | 1, row p = h[p], h[p + up],
// ..., zeros behind the last tap.  An output is then Kp multiply-adds of one row with a run of the signal, and a phase
// without taps (up > K) is a row of zeros: no branch.
//     tile      a 256-thread workgroup owns `tile` <= 1024 consecutive outputs of one signal; thread t owns outputs t, t + 256,
//               ... of the tile, one accumulator each
//     chunk     the rows are walked in chunks of jc taps: the chunk of every row the tile uses (kResampleTapLds elements at
//               most) and the run of the signal those taps meet (kResampleSigLds samples at most, zeros outside [0, L)) are
//               brought into LDS, then every thread adds its jc products                        caller x -> caller out   upfirdn_kernel
// tile and jc are functions of (K, up, down) alone, and an output's sum is acc = fma(row[j], x[q - j], acc) for j = 0 .. Kp - 1
// ascending from acc = 0, whatever the chunks: the bits depend on nothing else -- not on the batch, the distances, alignment,
// the stream or a graph replay.  No atomics, no workspace.
//
// Fourier method.  X = rfft_L(x); N = min(L, num); Y[k] = X[k] for k <= N / 2, 0 above; N even: Y[N / 2] *= 2 (num < L) or
// 1/2 (num > L); y = irfft_num(Y) num / L.  The spectrum sweep writes Y from X with the factor num / L (the C2R divides by num
// itself) and the Nyquist factor folded in, and with the imaginary parts of Y[0] and, for even num, of Y[num / 2] set to 0,
// as an inverse real transform defines them.
//     R2C       X = rfft_L(rows)                 AnyRealPlanner(L), caller x -> workspace planes
//     spectrum  Y from X                          workspace -> workspace                         resample_spectrum_kernel
//     C2R       y = irfft_num(Y)                  AnyRealPlanner(num), workspace -> caller out
//
// The top of this header (argument rules, geometry) has no HIP dependency: tests/test_resample_cpu.py compiles it with g++.
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

constexpr unsigned long long kResampleMaxLen = 1ull << 29;    // L, K, out_len; L and num of the Fourier method
constexpr unsigned long long kResampleMaxRate = 1ull << 20;   // up, down
// LDS of a workgroup, in elements of T: the tap chunk (rows of an odd stride) and the run of the signal.  DESIGN.md §27 says
// why these sizes: f64 68 KiB, two workgroups per CU; f32 34 KiB, four.
constexpr unsigned kResampleTapLds = 4096;   // tap elements of a chunk, before the padding of the rows
constexpr unsigned kResampleTapPad = 512;    // room for one element of padding per row, and to spare
constexpr unsigned kResampleSigLds = 4096;   // samples of the signal
constexpr unsigned kResampleMaxTile = 1024;  // outputs per workgroup: 256 threads of kResamplePerThread outputs
constexpr unsigned kResamplePerThread = 4;
constexpr unsigned kResampleMaxRows = 256;   // tap rows in LDS: the phases (up <= 256) or the tile's outputs (up > 256)

// the samples of the full result
PHAST_HD unsigned long long upfirdn_full_len(unsigned long long len, unsigned long long k, unsigned long long up,
                                             unsigned long long down) {
    return ((len - 1) * up + k - 1) / down + 1;
}
// taps per phase
PHAST_HD unsigned long long upfirdn_kp(unsigned long long k, unsigned long long up) { return (k + up - 1) / up; }
// elements between the rows of the device table: odd, the stride of the rows in LDS when one chunk holds a whole row
PHAST_HD unsigned long long upfirdn_table_stride(unsigned long long kp) { return kp | 1ull; }

struct UpfirdnGeom {
    unsigned rows;    // tap rows of a chunk in LDS: up (by_phase) or the tile's outputs
    unsigned jc;      // taps of a row per chunk
    unsigned stride;  // elements between rows in LDS: jc | 1, odd, so that neighbouring rows start in different banks
    unsigned tile;    // outputs per workgroup
    int by_phase;     // LDS row r holds phase r (up <= kResampleMaxRows); else row i holds the phase of the tile's output i
};
// The schedule: a function of (K, up, down) alone.  Rows: the `up` phases where they fit, else one row per output of the
// tile.  jc: the most taps per row that fit the table, at most half the signal's LDS.  tile: the most outputs, up to
// kResampleMaxTile (kResampleMaxRows with a row per output), whose run of the signal, the chunk included, fits LDS:
// (q of the last output - q of the first) + 1 + (jc - 1) <= ceil((tile - 1) down / up) + jc <= kResampleSigLds.
PHAST_HD UpfirdnGeom upfirdn_geom(unsigned long long k, unsigned long long up, unsigned long long down) {
    UpfirdnGeom g;
    const unsigned long long kp = upfirdn_kp(k, up);
    g.by_phase = up <= kResampleMaxRows;
    g.rows = g.by_phase ? (unsigned)up : kResampleMaxRows;
    unsigned long long jc = kResampleTapLds / g.rows;
    if (jc > kResampleSigLds / 2) jc = kResampleSigLds / 2;
    if (jc > kp) jc = kp;
    g.jc = (unsigned)jc;
    g.stride = g.jc | 1u;
    unsigned long long tile = 1 + (kResampleSigLds - jc) * up / down;
    const unsigned long long cap = g.by_phase ? kResampleMaxTile : kResampleMaxRows;
    g.tile = (unsigned)(tile > cap ? cap : tile);
    return g;
}
// the run of the signal that outputs [m0, m0 + n) meet in the taps [j0, j0 + jc) of their rows: x[lo .. lo + count), lo may
// be negative and lo + count may pass L (zeros there)
PHAST_HD void upfirdn_span(unsigned long long m0, unsigned long long n, unsigned long long up, unsigned long long down,
                           unsigned long long j0, unsigned long long jc, long long *lo, unsigned long long *count) {
    const unsigned long long q_lo = m0 * down / up, q_hi = (m0 + n - 1) * down / up;
    *lo = (long long)q_lo - (long long)(j0 + jc - 1);
    *count = q_hi - q_lo + jc;
}

// The argument rules of an upfirdn planner, before the device is touched: 0 when legal.  out_len = 0 stands for
// full_len - first (which must then be in 1 .. 2^29).
PHAST_HD int upfirdn_bad_args(unsigned long long len, unsigned long long k, unsigned long long up, unsigned long long down,
                              unsigned long long first, unsigned long long out_len) {
    if (len < 1 || len > kResampleMaxLen || k < 1 || k > kResampleMaxLen) return 1;
    if (up < 1 || up > kResampleMaxRate || down < 1 || down > kResampleMaxRate) return 1;
    const unsigned long long full = upfirdn_full_len(len, k, up, down);
    if (first > full) return 1;
    if (out_len == 0) out_len = full - first;
    if (out_len < 1 || out_len > kResampleMaxLen) return 1;
    return 0;
}

// The Fourier method: 0 when (L, num) is legal
PHAST_HD int resample_bad_args(unsigned long long len, unsigned long long num) {
    return len < 1 || len > kResampleMaxLen || num < 1 || num > kResampleMaxLen;
}
// the bins copied from X (the others of Y are 0), and the factor of the last of them over num / L
PHAST_HD unsigned long long resample_bins(unsigned long long len, unsigned long long num) { return (len < num ? len : num) / 2 + 1; }
PHAST_HD double resample_nyquist(unsigned long long len, unsigned long long num) {
    const unsigned long long n = len < num ? len : num;
    if (n % 2 || len == num) return 1.0;
    return num < len ? 2.0 : 0.5;
}

}  // namespace phast

#if defined(__HIPCC__)
#include "any_len.hpp"

namespace phast {

// the polyphase kernel: workgroup w of the launch owns tile (w mod tiles) of signal (w div tiles)
struct UpfirdnArgs {
    const void *x;       // the caller's signals, signal b at b * sig_dist
    void *out;           // the caller's outputs, signal b at b * out_dist
    const void *taps;    // up rows of kp taps, ts apart
    unsigned long long sig_dist, out_dist;
    unsigned long long len, kp, ts, up, down, first, out_len;
    unsigned long long tiles;   // tiles per signal
    unsigned long long groups;  // 256 x the workgroups of this call
    unsigned long long g0;      // first group of this launch (launches split at 2^31 - 1 workgroups)
    unsigned long long dq, dp;  // (256 down) div up and mod up: from one of a thread's outputs to its next
    UpfirdnGeom geom;
};
template <typename T> hipError_t launch_upfirdn(const UpfirdnArgs &a, hipStream_t stream);

// the spectrum sweep of the Fourier method: a thread owns V = 16 / sizeof(T) consecutive bins of both planes of one signal
struct ResampleArgs {
    const void *x_re, *x_im;  // X: rows xd apart
    void *y_re, *y_im;        // Y: rows yd apart
    unsigned long long xd, yd;
    unsigned long long bins;      // the bins of X that are copied
    unsigned long long zero_im;   // the bin of Y whose imaginary part is 0 besides bin 0 (num / 2 for even num; else none: ~0)
    double scale, last;           // num / L; the factor of bin bins - 1 (scale times the Nyquist factor)
    unsigned long long groups, g0;
    unsigned gpt;                 // groups per signal: yd / V
};
template <typename T> hipError_t launch_resample_spectrum(const ResampleArgs &a, hipStream_t stream);

}  // namespace phast
#endif
