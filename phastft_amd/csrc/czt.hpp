// czt.hpp -- the chirp-Z transform on the unit circle (zoom FFT): M bins of N points at the frequencies start + k step, both
// in turns (cycles per sample),
//
//     X[k] = sum_{n < N} x[n] exp(-2 pi i n (start + k step)),   k < M.
//
// With h = step / 2 (mod 1) and c[j] = exp(-2 pi i j^2 h), n k step = (n^2 + k^2 - (k - n)^2) h (mod 1), so X is the
// convolution of a[n] = x[n] exp(-2 pi i n start) c[n] with b[j] = conj(c[j]), -N < j < M, times c[k]: Bluestein's schedule
// (any_len.hpp) with the step freed from 1/N and the output length freed from N, in L = 2^ceil(log2(N + M - 1)) points:
//
//     pre         a = x exp(-2 pi i n start) c (n < N), 0 up to L     caller's planes -> workspace    czt_pre_kernel
//     engine      A = FFT_L(a)                                        workspace, in place             Planner<T>::exec_in
//     spectrum    A *= Bh,  Bh = FFT_L(b) / L                         workspace, in place             any_spectrum_kernel
//     engine      L IFFT_L(A) (swap trick)                            workspace, in place             Planner<T>::exec_in
//     post        X = c (k < M)                                       workspace -> caller's planes    czt_post_kernel
//
// The top of this header (the exact phase) has no HIP dependency: tests/test_czt_cpu.py compiles it for the host.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#include "common.hpp"  // PHAST_HD
#else
#define PHAST_HD inline  // the host-only top, for g++
#endif

namespace phast {

constexpr unsigned long long kCztMaxConv = 1ull << 30;  // N + M - 1 <= 2^30: the f64 engine's limit
constexpr unsigned long long kCztMinConv = 8;           // the shortest workspace row: every sweep moves whole 16-byte groups

// A fraction of a turn in [0, 1) on a 2^-128 grid: hi 2^-64 + lo 2^-128.  n^2 step / 2 in double is no good (n^2 ~ 2^40 at
// n ~ 10^6 leaves 13 bits below the point of the angle), and the step is no rational p / N as in any_len.hpp's chirp_r; on
// this grid a double of magnitude >= 2^-75 is exact, a smaller one is cut below 2^-128, which costs n^2 2^-128 < 2^-68 turns.
struct CztFrac {
    unsigned long long hi, lo;
};

// (v / 2^down) mod 1 on the grid (v finite; down = 1 halves the step).  v = +-mant 2^(e - 53) with mant < 2^53, so the
// value is mant shifted left by 75 + e - down places of the 128-bit word, wrapped; a negative v is the two's complement.
// Plain arithmetic on the bits of the double, so that host and device code share it (nufft_sort.hip): a normal v has
// mant = 2^52 | fraction field and e = exponent field - 1022; a zero or a subnormal lies far below 2^-128 and is cut to 0.
PHAST_HD CztFrac czt_frac(double v, int down) {
    unsigned long long bits = 0;
    __builtin_memcpy(&bits, &v, sizeof bits);
    const int field = (int)((bits >> 52) & 0x7ffull);
    const unsigned long long mant = field ? (bits & 0xfffffffffffffull) | (1ull << 52) : 0;
    const long long sh = 75ll + (field - 1022) - down;
    CztFrac r{0, 0};
    if (mant != 0 && sh < 128 && sh > -53) {
        if (sh >= 64) {
            r.hi = mant << (sh - 64);
        } else if (sh > 0) {
            r.hi = mant >> (64 - sh);
            r.lo = mant << sh;
        } else {
            r.lo = mant >> -sh;
        }
    }
    if (v < 0) {
        r.lo = ~r.lo + 1;
        r.hi = ~r.hi + (r.lo == 0 ? 1 : 0);
    }
    return r;
}

PHAST_HD unsigned long long czt_mulhi(unsigned long long a, unsigned long long b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (unsigned long long)(((unsigned __int128)a * b) >> 64);
#endif
}

// (n^2 h + n s) mod 1 for n < 2^32 in wrapping 128-bit integers, as a signed turn in [-1/2, 1/2): the top 64 bits of the sum
// converted to double.  Off the true angle by < 2^-64 (the bits dropped) + 2^-55 (the conversion) turns, and by what
// czt_frac cut from a tiny h or s.
PHAST_HD double czt_phase(unsigned long long n, CztFrac h, CztFrac s) {
    const unsigned long long sq = n * n;
    const unsigned long long a_lo = sq * h.lo, a_hi = sq * h.hi + czt_mulhi(sq, h.lo);
    const unsigned long long b_lo = n * s.lo, b_hi = n * s.hi + czt_mulhi(n, s.lo);
    const unsigned long long lo = a_lo + b_lo;
    const unsigned long long hi = a_hi + b_hi + (lo < a_lo ? 1 : 0);
    return (double)(long long)hi * 0x1p-64;
}

// the convolution length: the smallest power of two >= N + M - 1, at least kCztMinConv
inline unsigned long long czt_conv_len(unsigned long long n, unsigned long long m) {
    unsigned long long l = kCztMinConv;
    while (l < n + m - 1) l <<= 1;
    return l;
}

// 1 <= N, 1 <= M, N + M - 1 <= 2^30, finite step and start
inline bool czt_bad_args(unsigned long long n, unsigned long long m, double step, double start) {
    if (n == 0 || m == 0 || n > kCztMaxConv || m > kCztMaxConv || n + m - 1 > kCztMaxConv) return true;
    return !std::isfinite(step) || !std::isfinite(start);
}

}  // namespace phast

#if defined(__HIPCC__)
#include "any_len.hpp"

namespace phast {

// one launch of a sweep over `xforms` transforms; every thread handles one group of 16 bytes per plane, as in any_len.hpp
struct CztSweepArgs {
    const void *in_re;  // pre: the caller's input planes (transform b at b * in_dist); post: the workspace (b * L)
    const void *in_im;  // pre: null for a real signal
    void *out_re;       // pre: the workspace; post: the caller's output planes (b * out_dist)
    void *out_im;
    unsigned long long in_dist, out_dist;
    unsigned long long n;       // pre: N; post: M
    unsigned long long groups;  // groups in this launch
    unsigned long long g0;      // first group of this launch (launches split at 2^31 - 1 workgroups)
    unsigned log_l;             // L = 2^log_l
    unsigned gpt;               // post: groups per transform, ceil(M / V)
    CztFrac half_step, start;   // step / 2 and start, mod 1
};
// kind: 0 pre, 2 post (the spectrum sweep is launch_any_sweep's kind 1).  `vec`: the caller's planes allow 16-byte accesses.
template <typename T> hipError_t launch_czt_sweep(int kind, bool vec, const CztSweepArgs &a, hipStream_t stream);
// b[j] = conj(c[j]) for j < M, b[L - j] = conj(c[j]) for 0 < j < N, 0 elsewhere, as f64 planes [L]
hipError_t launch_czt_chirp_b(double *re, double *im, unsigned long long n, unsigned long long m, unsigned log_l, CztFrac half_step,
                              hipStream_t stream);

}  // namespace phast
#endif
