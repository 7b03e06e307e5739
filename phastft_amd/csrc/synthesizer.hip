// synthesizer.hip -- the unfold of the polyphase synthesis bank (synthesizer.hpp has the definition and the schedule).
//
//     unfold    workgroup w owns one tile: kSynthTile consecutive output samples of one plane of one signal.  Thread t owns the
//               samples i0 + t + 256 i, i < kSynthPer (neighbouring lanes: neighbouring columns of a row of v with one wrap at
//               M, neighbouring taps, neighbouring output samples).  One division gives floor(n / D) and n mod D of its first
//               sample and one n mod M; the others follow by steps.  Then acc = fma(tap, v, acc) over the frames m_lo .. m_hi
//               ascending, the thread's chains side by side, a chain skipping the steps it does not have.  One store per
//               sample, by elements: pointers and distances need element alignment only.
//     copy      rows of M elements of two planes into workspace rows (complex output: the transform runs in place there), or the
//               imaginary plane of real output with bin 0 and bin M / 2 set to 0 (even M >= 4).
// Launches are split at 2^31 - 1 workgroups, as in the other sweeps.  No LDS, no atomics, no scratch memory.
#include "synthesizer.hpp"

namespace phast {

// one rounding per product and sum, in T
__device__ inline double synth_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }
__device__ inline float synth_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

// v div m (and v mod m) of v < 2^62, by a 32-bit division where both allow it
__device__ inline unsigned long long synth_divmod(unsigned long long v, unsigned long long m, unsigned long long *rem) {
    const unsigned long long q = v < 0xffffffffull && m < 0xffffffffull ? (unsigned)v / (unsigned)m : v / m;
    *rem = v - q * m;
    return q;
}

template <typename T>
__global__ void __launch_bounds__(256) synth_unfold_kernel(SynthArgs a) {
    constexpr unsigned R = kSynthPer;
    const unsigned t = threadIdx.x;
    const unsigned long long wg = (a.g0 >> 8) + blockIdx.x;
    if (wg * 256 >= a.groups) return;
    // (plane, signal, tile) of this workgroup
    unsigned long long tile;
    const unsigned long long pb = synth_divmod(wg, a.tiles, &tile);
    const unsigned plane = pb >= a.count;
    const unsigned long long b = pb - plane * a.count;
    const unsigned long long i0 = tile * kSynthTile + t;  // this thread's first sample of the window
    const SynthGeom g = a.geom;
    const unsigned m = (unsigned)a.m, d = (unsigned)a.d;
    const T *v = (const T *)a.v[plane] + b * a.f * a.ld, *tab = (const T *)a.taps;

    // floor(n / D), n mod D and n mod M of the first sample n = first + i0 (< 2^61); the next ones 256 further by steps
    unsigned long long r64, c64;
    unsigned long long q = synth_divmod(a.first + i0, a.d, &r64);
    synth_divmod(a.first + i0, a.m, &c64);
    unsigned r = (unsigned)r64, col = (unsigned)c64;
    unsigned cnt[R], jt[R];   // terms of the chain still to come; the tap of its next term
    unsigned long long vo[R]; // the element of v of its next term
    T acc[R];
    unsigned most = 0;
#pragma unroll
    for (unsigned i = 0; i < R; ++i) {
        // m_lo = max(0, ceil((n - K + 1) / D)) = max(0, floor(n / D) - K div D - (n mod D < K mod D) + 1), m_hi = min(F - 1, floor(n / D))
        long long m_lo = (long long)q - (long long)g.kq - (r < g.kr ? 1 : 0) + 1;
        if (m_lo < 0) m_lo = 0;
        long long m_hi = (long long)q;
        if (m_hi > (long long)a.f - 1) m_hi = (long long)a.f - 1;
        const bool live = i0 + i * 256ull < a.out_len && m_hi >= m_lo;
        cnt[i] = live ? (unsigned)(m_hi - m_lo + 1) : 0;                          // <= ceil(K / D)
        jt[i] = live ? (unsigned)((q - (unsigned long long)m_lo) * d + r) : 0;    // n - m_lo D, in [0, K)
        vo[i] = live ? (unsigned long long)m_lo * a.ld + col : 0;
        acc[i] = T(0);
        most = cnt[i] > most ? cnt[i] : most;
        q += g.sq;
        r += g.sr;
        if (r >= d) {
            r -= d;
            ++q;
        }
        col += g.sm;
        if (col >= m) col -= m;
    }
    // `per` independent chains, each over its frames in ascending order
    for (unsigned s = 0; s < most; ++s) {
#pragma unroll
        for (unsigned i = 0; i < R; ++i) {
            if (s < cnt[i]) {
                acc[i] = synth_fma(tab[jt[i]], v[vo[i]], acc[i]);
                jt[i] -= s + 1 < cnt[i] ? d : 0;
                vo[i] += a.ld;
            }
        }
    }
    T *out = (T *)a.out[plane] + b * a.out_dist;
#pragma unroll
    for (unsigned i = 0; i < R; ++i) {
        const unsigned long long o = i0 + i * 256ull;
        if (o < a.out_len) out[o] = acc[i];
    }
}

template <typename T>
__global__ void __launch_bounds__(256) synth_copy_kernel(SynthCopyArgs a) {
    const unsigned long long e = a.g0 + (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= a.groups) return;
    const unsigned long long per_plane = a.rows * a.n;
    const unsigned plane = e >= per_plane;
    unsigned long long c;
    const unsigned long long row = synth_divmod(e - plane * per_plane, a.n, &c);
    const T x = ((const T *)a.in[plane])[row * a.in_ld + c];
    ((T *)a.out[plane])[row * a.out_ld + c] = c == a.zero_a || c == a.zero_b ? T(0) : x;
}

template <typename T> hipError_t launch_synth_unfold(const SynthArgs &a0, hipStream_t stream) {
    SynthArgs a = a0;
    return launch_in_slices(a.groups, [&](dim3 grid, unsigned long long g0) {
        a.g0 = g0;
        hipLaunchKernelGGL(synth_unfold_kernel<T>, grid, dim3(256), 0, stream, a);
    });
}
template hipError_t launch_synth_unfold<double>(const SynthArgs &, hipStream_t);
template hipError_t launch_synth_unfold<float>(const SynthArgs &, hipStream_t);

template <typename T> hipError_t launch_synth_copy(const SynthCopyArgs &a0, hipStream_t stream) {
    SynthCopyArgs a = a0;
    return launch_in_slices(a.groups, [&](dim3 grid, unsigned long long g0) {
        a.g0 = g0;
        hipLaunchKernelGGL(synth_copy_kernel<T>, grid, dim3(256), 0, stream, a);
    });
}
template hipError_t launch_synth_copy<double>(const SynthCopyArgs &, hipStream_t);
template hipError_t launch_synth_copy<float>(const SynthCopyArgs &, hipStream_t);

}  // namespace phast
