// conv.hpp -- overlap-save FIR convolution and correlation of real signals around one real transform of the block length
// (DESIGN.md §16).
//
// Signal x of L samples, K taps h, block B >= K, hop S = B - K + 1.  full[t] = sum_j g[j] x[t - j], t in [0, L + K - 1), with
// g = h (convolution) or g[j] = h[K - 1 - j] (correlation); out[i] = full[t0 + i], i < out_len:
//     mode   t0             out_len
//     full   0              L + K - 1
//     same   (K - 1) / 2    L
//     valid  K - 1          L - K + 1   (L >= K)
// These are scipy.signal.convolve / correlate(x, h, mode, method="direct").  segs = ceil(out_len / S) segments per signal:
//     segment   row s = x~[t0 + s S - (K - 1) + j], j < B; x~ is x inside [0, L), 0 outside   caller x -> workspace   kConvSegment
//     R2C       X[s] = rfft_B(row s)                                       AnyRealPlanner (unchanged), workspace -> workspace
//     spectrum  X[s] *= H^, H^ = rfft_B(g zero-padded to B), unscaled (the C2R scales by 1/B)  workspace, in place    kConvSpectrum
//     C2R       y[s] = irfft_B(X[s])                                       AnyRealPlanner (unchanged), workspace -> workspace
//     save      out[s S + i] = y[s][K - 1 + i], i < S, s S + i < out_len                      workspace -> caller out kConvSave
//
// The top of this header (geometry, automatic block, argument rules) has no HIP dependency: tests/test_conv_cpu.py compiles
// it with g++.
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

enum ConvMode { kConvFull = 0, kConvSame = 1, kConvValid = 2 };  // PHAST_CONV_*

constexpr unsigned long long kConvMaxLen = 1ull << 29;        // L, K, B and out_len
constexpr unsigned long long kConvMaxRowPoints = 1ull << 30;  // segs * fd

// the sample of the full convolution that out[0] is
PHAST_HD unsigned long long conv_t0(unsigned long long k, int mode) {
    return mode == kConvFull ? 0 : mode == kConvSame ? (k - 1) / 2 : k - 1;
}
// the samples of the output; 0 where the mode has none (valid with L < K, an unknown mode)
PHAST_HD unsigned long long conv_out_len(unsigned long long len, unsigned long long k, int mode) {
    if (mode == kConvFull) return len + k - 1;
    if (mode == kConvSame) return len;
    return mode == kConvValid && len >= k ? len - k + 1 : 0;
}
// the segments of one signal: every segment but the last yields S = B - K + 1 output samples (B >= K)
PHAST_HD unsigned long long conv_segments(unsigned long long out_len, unsigned long long k, unsigned long long b) {
    const unsigned long long s = b - k + 1;
    return (out_len + s - 1) / s;
}
// a row of b elements rounded up to `vec` = 16 / sizeof(T) elements
PHAST_HD unsigned long long conv_row(unsigned long long b, unsigned long long vec) { return (b + vec - 1) / vec * vec; }

PHAST_HD unsigned long long conv_pow2_ceil(unsigned long long v) {
    unsigned long long p = 1;
    while (p < v) p <<= 1;
    return p;
}
// The block of `block = 0` (1 <= L, K <= 2^29): the smallest power of two >= 4 (K - 1), so that at least 3/4 of a row is
// output, at least 1024 and at most 2^29; or the smallest power of two >= L + K - 1 (one segment holds the whole full
// convolution) where that is smaller.  DESIGN.md §16 has the measurements behind it.
PHAST_HD unsigned long long conv_auto_block(unsigned long long len, unsigned long long k) {
    unsigned long long b = conv_pow2_ceil(4 * (k - 1));
    if (b < 1024) b = 1024;
    if (b > kConvMaxLen) b = kConvMaxLen;
    const unsigned long long whole = conv_pow2_ceil(len + k - 1);
    return whole < b ? whole : b;
}

// The argument rules of a planner, before the device is touched: 0 when (L, K, mode, flip, block) is legal for elements of
// which `vec` fill 16 bytes.  block = 0 is the automatic block.
PHAST_HD int conv_bad_args(unsigned long long len, unsigned long long k, int mode, int flip, unsigned long long block,
                           unsigned long long vec) {
    if (len < 1 || len > kConvMaxLen || k < 1 || k > kConvMaxLen) return 1;
    if (mode != kConvFull && mode != kConvSame && mode != kConvValid) return 1;
    if (flip != 0 && flip != 1) return 1;
    if (vec != 2 && vec != 4) return 1;
    if (mode == kConvValid && len < k) return 1;
    const unsigned long long b = block ? block : conv_auto_block(len, k);
    if (b < k || b > kConvMaxLen) return 1;
    const unsigned long long n = conv_out_len(len, k, mode);
    if (n < 1 || n > kConvMaxLen) return 1;
    if (conv_segments(n, k, b) * conv_row(b, vec) > kConvMaxRowPoints) return 1;
    return 0;
}

}  // namespace phast

#if defined(__HIPCC__)
#include "any_len.hpp"

namespace phast {

enum ConvKind { kConvSegment = 0, kConvSpectrum = 1, kConvSave = 2 };

// one sweep over `groups` thread groups; a thread owns one group of V = 16 / sizeof(T) consecutive elements: of a workspace
// row (segment sweep), of both spectrum planes (spectrum sweep) or of a signal's output (save sweep)
struct ConvArgs {
    const void *in;          // segment: the caller's signals; save: the workspace rows y
    void *out;               // segment: the workspace rows; save: the caller's outputs
    void *re, *im;           // spectrum: the workspace planes, bd elements per segment
    const void *h_re, *h_im;  // spectrum: H^, bd elements (zeros beyond the bins)
    unsigned long long sig_dist, out_dist;  // elements between the caller's signals / outputs
    unsigned long long len, k, b, s, t0, out_len, segs;
    unsigned long long fd, bd;   // elements between workspace rows / between the rows of a spectrum plane
    unsigned long long q0, q1;   // the flattened (signal, segment) indices [q0, q1) of this chunk; workspace row 0 is q0
    unsigned long long first;    // save: the flattened (signal, group) index of the launch's group 0
    unsigned long long groups;   // groups in this launch
    unsigned long long g0;       // first group of this launch (launches split at 2^31 - 1 workgroups)
    unsigned gpt;                // groups per workspace row (segment), per plane row (spectrum) or per signal (save)
};
template <typename T> hipError_t launch_conv(int kind, const ConvArgs &a, hipStream_t stream);

}  // namespace phast
#endif
