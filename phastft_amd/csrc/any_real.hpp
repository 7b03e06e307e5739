// any_real.hpp -- arbitrary-length real transforms (R2C / C2R) around the Bluestein core of any_len.hpp.
//
// Even N = 2H, not a power of two: z[n] = x[2n] + i x[2n+1] is transformed by an H-point Bluestein and untangled,
//     X[k] = (Z[k] + conj Z[H-k]) / 2 - i W^k (Z[k] - conj Z[H-k]) / 2,   W = exp(-2 pi i / N),  k = 0 .. H
// and C2R runs the power-of-two path's preprocess (oracle pho_c2r_preprocess), an inverse H-point Bluestein and the interleave.
// Odd N: a length-N Bluestein that reads one real plane (R2C) or builds the Hermitian extension X[N-k] = conj X[k] on load
// (C2R); the post sweeps write the half spectrum / the real part.  N = 1, 2: one direct kernel.
//
//     R2C even   pack + chirp-pad     x -> a = z w_H (n < H), 0 up to M               caller -> workspace    kind kR2cPack
//                engine, spectrum, engine (AnyPlanner::convolve, planner_any.hpp)
//                chirp-post+untangle  Z = w_H c; X[k], X[H-k] from (Z[k], Z[H-k])     workspace -> caller    kind kR2cUntangle
//     C2R even   preprocess + pad     z~[k], z~[H-k] from (X[k], X[H-k]); planes swapped    caller -> workspace   kC2rPre
//                chirp-post+interleave  x[2n] = Im(w_H c) / H, x[2n+1] = Re(w_H c) / H     workspace -> caller   kC2rInterleave
//     R2C odd    real pad / half post (k <= (N-1)/2, Im X[0] = 0)                                  kR2cOddPad / kR2cOddPost
//     C2R odd    Hermitian pad (Im X[0] ignored) / real-part post (* 1/N)                          kC2rOddPad / kC2rOddPost
#pragma once

#include "any_len.hpp"

#if defined(__HIPCC__)
namespace phast {

enum AnyRealKind {
    kR2cPack = 0,
    kR2cUntangle = 1,
    kC2rPre = 2,
    kC2rInterleave = 3,
    kR2cOddPad = 4,
    kR2cOddPost = 5,
    kC2rOddPad = 6,
    kC2rOddPost = 7,
    kR2cTiny = 8,  // N = 1, 2: one thread per transform, no workspace
    kC2rTiny = 9,
};

// one launch over `groups` thread groups (16 bytes per plane each, V = 16 / sizeof(T) points); the workspace holds transform
// b at b * M (re plane) and c M + b * M (im plane) -- `in_*` / `out_*` point at it for the sweeps that read / write it
struct AnyRealArgs {
    const void *in_re;  // pad sweeps: the caller's input (R2C: the real signal in in_re); post sweeps: the workspace
    const void *in_im;
    void *out_re;  // pad sweeps: the workspace; post sweeps: the caller's output (C2R: the real signal in out_re)
    void *out_im;
    unsigned long long in_dist, out_dist;  // the caller's side (elements between transforms)
    unsigned long long n;                  // N, the real length
    unsigned long long l;                  // the Bluestein length: H = N / 2 (even N) or N (odd N)
    unsigned long long groups;             // groups in this launch
    unsigned long long g0;                 // first group of this launch (launches split at 2^31 - 1 workgroups)
    unsigned log_m;                        // M = 2^log_m
    unsigned gpt;                          // post sweeps: groups per transform
    double scale;                          // C2R post: 1 / H (even) or 1 / N (odd)
};
// `vec`: the caller's side allows 16-byte accesses (16-byte aligned bases, dist a multiple of V); the workspace always does
template <typename T> hipError_t launch_any_real(int kind, bool vec, const AnyRealArgs &a, hipStream_t stream);

}  // namespace phast
#endif
