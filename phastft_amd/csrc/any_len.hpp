// any_len.hpp -- arbitrary-length complex transforms (Bluestein): the exact chirp phase and the three streaming sweeps
// around the power-of-two engine.  A length-N DFT is the cyclic convolution of a[n] = x[n] w[n] with b[n] = conj(w[n]),
// w[n] = exp(-i pi n^2 / N), in M = 2^ceil(log2(2N - 1)) points, multiplied by w[k] ("Arbitrary lengths"):
//
//     chirp-pad   a = x w (n < N), 0 (N <= n < M)         caller's planes -> workspace         any_pre_kernel
//     engine      A = FFT_M(a)                            workspace, in place                  Planner<T>::exec_in
//     spectrum    A *= Bh,  Bh = FFT_M(b) / M             workspace, in place                  any_spectrum_kernel
//     engine      c = M IFFT_M(A) (swap trick)            workspace, in place                  Planner<T>::exec_in
//     chirp-post  X = w c * scale  (k < N)                workspace -> caller's planes         any_post_kernel
//
// The top of this header (the exact phase) has no HIP dependency: tests/test_any_len_cpu.py compiles it for the host.  The HIP
// section below it holds the launch interface of the three sweeps and the device helpers they share with the real sweeps
// (any_real.hip): the 16-byte group type, the chirp, the split of a group index and the launch split at 2^31 - 1 workgroups.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#include "common.hpp"  // PHAST_HD
#else
#define PHAST_HD inline  // the host-only top, for g++
#endif

namespace phast {

constexpr unsigned long long kAnyMaxN = 1ull << 29;  // M <= 2^30: the f64 engine's limit (the f32 planner's Bh is built in f64)

// r = n^2 mod 2N, exact, for n < 2^30 and 1 <= N <= 2^29.  w[n] = exp(-i pi n^2 / N) = exp(-i pi r / N): n^2 / N itself
// is no good in floating point (n^2 ~ 2^40 at N ~ 10^6 leaves ~13 bits below the point of the angle: a phase error of
// ~3e-10).  The quotient is estimated in double and corrected in integers: n mod 2N < 2^30, so its square is < 2^60 and the
// estimate is off by at most one.
PHAST_HD unsigned long long chirp_r(unsigned long long n, unsigned long long N) {
    const unsigned long long two_n = 2 * N;
    if (n >= two_n) n = (unsigned)n % (unsigned)two_n;  // (n + 2N k)^2 = n^2 (mod 2N); both operands < 2^31
    const unsigned long long sq = n * n;
    const unsigned long long q = (unsigned long long)((double)sq / (double)two_n);
    long long r = (long long)(sq - q * two_n);
    if (r < 0) r += (long long)two_n;
    if (r >= (long long)two_n) r -= (long long)two_n;
    return (unsigned long long)r;
}

// the chirp's angle in units of pi: w[n] = exp(i pi t), t = -r / N in (-2, 0] (one rounding: r and N are exact in double)
PHAST_HD double chirp_turns(unsigned long long n, unsigned long long N) { return -(double)chirp_r(n, N) / (double)N; }

// the convolution length: the smallest power of two >= 2N - 1 (N itself for a power of two, which never convolves)
inline unsigned long long any_conv_len(unsigned long long N) {
    if ((N & (N - 1)) == 0) return N;
    unsigned long long m = 1;
    while (m < 2 * N - 1) m <<= 1;
    return m;
}

}  // namespace phast

#if defined(__HIPCC__)
#include "kernels.hpp"

namespace phast {

// one launch of a sweep over `xforms` transforms; every thread handles one group of 16 bytes per plane (2 f64 / 4 f32 points)
struct AnySweepArgs {
    const void *in_re;  // pre: the caller's planes (transform b at b * in_dist); spectrum / post: the workspace (b * M)
    const void *in_im;
    void *out_re;  // pre / spectrum: the workspace; post: the caller's planes (b * out_dist)
    void *out_im;
    const void *bh_re;  // spectrum: Bh planes [M] (1/M folded in)
    const void *bh_im;
    unsigned long long in_dist, out_dist;
    unsigned long long n;       // N
    unsigned long long groups;  // groups in this launch
    unsigned long long g0;      // first group of this launch (launches split at 2^31 - 1 workgroups)
    unsigned log_m;             // M = 2^log_m
    unsigned gpt;               // post: groups per transform, ceil(N / V)
    double scale;               // post: 1 or 1/N
};
// kind: 0 chirp-pad, 1 spectrum, 2 chirp-post.  `vec`: the caller's planes allow 16-byte accesses (16-byte aligned, dist a
// multiple of the group); the workspace side always does.
template <typename T> hipError_t launch_any_sweep(int kind, bool vec, const AnySweepArgs &a, hipStream_t stream);
// b[n] = conj(w[n]) for n < N, b[M - n] = b[n] for 0 < n < N, 0 elsewhere, as f64 planes [M]
hipError_t launch_any_chirp_b(double *re, double *im, unsigned long long n, unsigned log_m, hipStream_t stream);
// out[i] = (float)in[i], i < count (the f32 planner's Bh, built in f64)
hipError_t launch_any_round(const double *in, float *out, unsigned long long count, hipStream_t stream);

// ---- shared by the sweeps of any_len.hip and any_real.hip ----
template <typename T> struct AnyVec;  // 16 bytes of T: the group of one thread
template <> struct AnyVec<double> { typedef double type __attribute__((ext_vector_type(2))); static constexpr int N = 2; };
template <> struct AnyVec<float> { typedef float type __attribute__((ext_vector_type(4))); static constexpr int N = 4; };
// 16 bytes of T at element alignment: the gathered side of a sweep (stft.hip, conv.hip)
template <typename T> struct Unaligned;
template <> struct Unaligned<double> { typedef double type __attribute__((ext_vector_type(2), aligned(8))); };
template <> struct Unaligned<float> { typedef float type __attribute__((ext_vector_type(4), aligned(4))); };
__device__ inline bool aligned16(const void *p) { return (reinterpret_cast<unsigned long long>(p) & 15ull) == 0; }

// w[k] = exp(-i pi k^2 / n) (cos, sin) in double
__device__ inline void chirp(unsigned long long k, unsigned long long n, double *c, double *s) {
    sincospi(chirp_turns(k, n), s, c);
}

// the group of this thread in a launch of AnySweepArgs / AnyRealArgs (a.g0: the launch's first group)
template <typename A> __device__ inline unsigned long long global_group(const A &a) {
    return a.g0 + (unsigned long long)blockIdx.x * 256 + threadIdx.x;
}
// (transform, group within it) of group g of a sweep with gpt groups per transform
__device__ inline unsigned long long split_group(unsigned long long g, unsigned gpt, unsigned long long *b) {
    *b = g < 0xffffffffull ? (unsigned)g / gpt : g / gpt;
    return g - *b * gpt;
}

// `groups` groups in 256-thread workgroups: launch(grid, g0) once per slice of at most 2^31 - 1 workgroups from group g0 on
template <typename F> hipError_t launch_in_slices(unsigned long long groups, F &&launch) {
    constexpr unsigned long long kMaxBlocks = 0x7fffffffull;
    for (unsigned long long g0 = 0; g0 < groups; g0 += kMaxBlocks * 256) {
        const unsigned long long blocks = (groups - g0 + 255) / 256;
        launch(dim3((unsigned)(blocks < kMaxBlocks ? blocks : kMaxBlocks)), g0);
    }
    return hipGetLastError();
}

}  // namespace phast
#endif
