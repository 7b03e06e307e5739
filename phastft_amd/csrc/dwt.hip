// dwt.hip -- the two kernels of the discrete wavelet transform (dwt.hpp has the definitions, the geometry and the orders of
// the sums).
//
//     analysis   workgroup w owns tile (w mod tiles) of signal (w div tiles): up to kDwtTile consecutive coefficient indices of
//                one level.  All threads stage the run of the input the tile meets through the extension map, the samples of
//                even position in the run into one LDS array and those of odd position into the other; a barrier; thread t
//                owns the coefficients t, t + 256, ... of the tile: neighbouring lanes read neighbouring elements of an array,
//                and every element read feeds both bands.  One store per coefficient and band, by elements.
//     synthesis  the same with tiles of up to kDwtTile output pairs: cA and cD of the coefficients the tile meets are staged
//                (periodization wraps here), and every pair of LDS reads feeds two FMAs of each of the pair's two outputs.
// The taps come from a device table at addresses that are uniform across the wave.  A thread whose item the tile does not have
// computes on whatever LDS holds (inside the arrays: 255 + 768 + F / 2 - 1 < kDwtHalfLds) and stores nothing.  Launches are
// split at 2^31 - 1 workgroups, as in the other sweeps.  No atomics, no scratch memory.
#include "dwt.hpp"

namespace phast {

// one rounding per product and sum, in T
__device__ inline double dwt_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }
__device__ inline float dwt_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

// (signal, tile) of workgroup wg
__device__ inline unsigned long long dwt_split(unsigned long long wg, unsigned long long tiles, unsigned long long *b) {
    *b = wg < 0xffffffffull && tiles < 0xffffffffull ? (unsigned)wg / (unsigned)tiles : wg / tiles;
    return wg - *b * tiles;
}

template <typename T>
__global__ void __launch_bounds__(256) dwt_analysis_kernel(DwtArgs a) {
    __shared__ T lds[2 * kDwtHalfLds];
    T *const ev = lds, *const od = lds + kDwtHalfLds;
    constexpr unsigned R = kDwtPerThread;
    const unsigned t = threadIdx.x;
    const unsigned long long wg = (a.g0 >> 8) + blockIdx.x;
    if (wg * 256 >= a.groups) return;  // whole workgroups: all threads agree
    unsigned long long b;
    const unsigned long long tl = dwt_split(wg, a.tiles, &b);
    const unsigned f = a.f, h = f / 2;
    const unsigned long long i0 = tl * kDwtTile;                                        // the tile's first coefficient
    const unsigned n = a.n_out - i0 < kDwtTile ? (unsigned)(a.n_out - i0) : kDwtTile;  // its coefficients
    const T *__restrict__ x = (const T *)a.in_lo + b * a.in_lo_dist;

    // the run: position u holds ext(x, lo + u); tap j of coefficient i0 + c meets position 2c + F - 1 - j
    const long long lo = 2 * (long long)i0 + dwt_analysis_shift(f, a.mode) - (long long)(f - 1);
    const unsigned count = 2 * n + f - 2;
    for (unsigned u = t; u < count; u += 256) {
        const long long s = dwt_ext_index(a.mode, (long long)a.n_in, lo + (long long)u);
        (u & 1 ? od : ev)[u >> 1] = s >= 0 ? x[s] : T(0);
    }
    __syncthreads();

    // taps 2p and 2p + 1 of coefficient c: od[c + h - 1 - p] and ev[c + h - 1 - p].  2R independent chains, each in ascending j
    T lo_acc[R], hi_acc[R];
#pragma unroll
    for (unsigned r = 0; r < R; ++r) lo_acc[r] = hi_acc[r] = T(0);
    const T *__restrict__ taps = (const T *)a.taps;  // dec_lo[2p], dec_hi[2p], dec_lo[2p + 1], dec_hi[2p + 1]
    const T *const po = od + t + (h - 1), *const pe = ev + t + (h - 1);
#pragma unroll 2
    for (unsigned p = 0; p < h; ++p) {
        const T l0 = taps[4 * p], h0 = taps[4 * p + 1], l1 = taps[4 * p + 2], h1 = taps[4 * p + 3];
#pragma unroll
        for (unsigned r = 0; r < R; ++r) {
            const T o = po[(int)(256 * r) - (int)p], e = pe[(int)(256 * r) - (int)p];
            lo_acc[r] = dwt_fma(l0, o, lo_acc[r]);
            hi_acc[r] = dwt_fma(h0, o, hi_acc[r]);
            lo_acc[r] = dwt_fma(l1, e, lo_acc[r]);
            hi_acc[r] = dwt_fma(h1, e, hi_acc[r]);
        }
    }
    T *out_lo = (T *)a.out_lo + b * a.out_lo_dist + i0, *out_hi = (T *)a.out_hi + b * a.out_hi_dist + i0;
#pragma unroll
    for (unsigned r = 0; r < R; ++r) {
        const unsigned i = t + 256 * r;
        if (i < n) {
            out_lo[i] = lo_acc[r];
            out_hi[i] = hi_acc[r];
        }
    }
}

template <typename T> hipError_t launch_dwt_analysis(const DwtArgs &a0, hipStream_t stream) {
    DwtArgs a = a0;
    return launch_in_slices(a.groups, [&](dim3 grid, unsigned long long g0) {
        a.g0 = g0;
        hipLaunchKernelGGL(dwt_analysis_kernel<T>, grid, dim3(256), 0, stream, a);
    });
}
template hipError_t launch_dwt_analysis<double>(const DwtArgs &, hipStream_t);
template hipError_t launch_dwt_analysis<float>(const DwtArgs &, hipStream_t);

template <typename T>
__global__ void __launch_bounds__(256) dwt_synthesis_kernel(DwtArgs a) {
    __shared__ T lds[2 * kDwtHalfLds];
    T *const ca = lds, *const cd = lds + kDwtHalfLds;
    constexpr unsigned R = kDwtPerThread;
    const unsigned t = threadIdx.x;
    const unsigned long long wg = (a.g0 >> 8) + blockIdx.x;
    if (wg * 256 >= a.groups) return;  // whole workgroups: all threads agree
    unsigned long long b;
    const unsigned long long tl = dwt_split(wg, a.tiles, &b);
    const unsigned f = a.f, h = f / 2;
    const unsigned long long c0 = tl * kDwtTile;                                      // the tile's first pair of the level
    const unsigned n = a.items - c0 < kDwtTile ? (unsigned)(a.items - c0) : kDwtTile;  // its pairs
    const long long q0 = a.q_first + (long long)c0;
    const T *__restrict__ in_a = (const T *)a.in_lo + b * a.in_lo_dist, *__restrict__ in_d = (const T *)a.in_hi + b * a.in_hi_dist;

    // position u holds coefficient k' = q0 - h + 1 + u of both bands; pair c meets the positions c .. c + h - 1
    const long long lo = q0 - (long long)h + 1, m = (long long)a.n_in;
    const unsigned count = n + h - 1;
    for (unsigned u = t; u < count; u += 256) {
        const long long k = dwt_synth_index(a.mode, m, lo + (long long)u);
        ca[u] = k >= 0 ? in_a[k] : T(0);
        cd[u] = k >= 0 ? in_d[k] : T(0);
    }
    __syncthreads();

    // k' ascending: tap pair d = h - 1 - i descending.  2R independent chains
    T y0[R], y1[R];
#pragma unroll
    for (unsigned r = 0; r < R; ++r) y0[r] = y1[r] = T(0);
    const T *__restrict__ taps = (const T *)a.taps + 2 * f;  // rec_lo[2d], rec_hi[2d], rec_lo[2d + 1], rec_hi[2d + 1], d = h - 1 - i
    const T *const pa = ca + t, *const pd = cd + t;
#pragma unroll 2
    for (unsigned i = 0; i < h; ++i) {
        const T l0 = taps[4 * i], h0 = taps[4 * i + 1], l1 = taps[4 * i + 2], h1 = taps[4 * i + 3];
#pragma unroll
        for (unsigned r = 0; r < R; ++r) {
            const T va = pa[256 * r + i], vd = pd[256 * r + i];
            y0[r] = dwt_fma(l0, va, y0[r]);
            y0[r] = dwt_fma(h0, vd, y0[r]);
            y1[r] = dwt_fma(l1, va, y1[r]);
            y1[r] = dwt_fma(h1, vd, y1[r]);
        }
    }
    T *out = (T *)a.out_lo + b * a.out_lo_dist;
    const long long s = dwt_synth_shift(f, a.mode), len = (long long)a.n_out;
#pragma unroll
    for (unsigned r = 0; r < R; ++r) {
        const unsigned c = t + 256 * r;
        const long long r0 = 2 * (q0 + (long long)c) - s;  // the pair's outputs: r0 (>= -1) and r0 + 1
        if (c < n) {
            if (r0 >= 0 && r0 < len) out[r0] = y0[r];
            if (r0 + 1 < len) out[r0 + 1] = y1[r];
        }
    }
}

template <typename T> hipError_t launch_dwt_synthesis(const DwtArgs &a0, hipStream_t stream) {
    DwtArgs a = a0;
    return launch_in_slices(a.groups, [&](dim3 grid, unsigned long long g0) {
        a.g0 = g0;
        hipLaunchKernelGGL(dwt_synthesis_kernel<T>, grid, dim3(256), 0, stream, a);
    });
}
template hipError_t launch_dwt_synthesis<double>(const DwtArgs &, hipStream_t);
template hipError_t launch_dwt_synthesis<float>(const DwtArgs &, hipStream_t);

}  // namespace phast
