// cwt.hip -- the filter bank of the continuous wavelet transform (cwt.hpp has the definitions and the expression order).
//
//     bank      workgroup w owns one tile of 256 x 16 bytes of consecutive bins of one scale group (kCwtGroup scales of one
//               signal); thread t owns the V = 16 / sizeof(T) bins k0 = (tile 256 + t) V on.  It loads its X once (16 bytes per
//               plane where the vector lies inside the kept spectrum and is aligned, by elements otherwise: above P div 2 a real
//               signal's bin is the mirrored bin P - k conjugated for DOG and is not read at all for the analytic families),
//               forms 2 pi kk / P once per bin and walks the scales of the group that belong to the chunk: per scale and bin
//               one evaluation in double, one product with a real or unit-imaginary number, one 16-byte store per plane where
//               the row is aligned and the vector whole, element stores otherwise.  Pointers and distances need element
//               alignment only.  For the analytic families (Morlet, Paul, STEP) every bin above P div 2 is written as +0.
//     copy      rows of n_out elements, the first n_in from the source and zeros behind them: the pad and the crop.
// Launches are split at 2^31 - 1 workgroups, as in the other sweeps.  No LDS, no atomics, no cross-lane operations, no scratch.
#include "cwt.hpp"

#include <cstdint>

namespace phast {

template <typename T> struct alignas(16) CwtVec {
    T v[16 / sizeof(T)];
};

// E(a) of cwt.hpp: the exponential in double in both types.  f32 with expf (of the exponent rounded to float, the rounding
// brought back as the factor 1 + (a - ah)) was measured on the MI355X at 0.53 of the f32 rel-L2 gate -- Paul raises E to the
// m-th power and with it expf's error --, over the 0.5 the error budget allows; in double the filter is exact next to its one
// rounding to float
template <typename T> __device__ inline double cwt_exp(double a) { return exp(a); }

// y^m by squaring: |y| <= 1 or the result is the largest intermediate
__device__ inline double cwt_ipow(double y, unsigned m) {
    double r = 1.0;
    for (unsigned e = m; e; e >>= 1) {
        if (e & 1) r *= y;
        y *= y;
    }
    return r;
}

// g_j psi0^(s_j w_k) without the family's unit factor, rounded once to T
template <typename T> __device__ inline T cwt_filter(int family, double param, unsigned m, double s, double g, double om) {
    const double x = s * om;
    double h;
    if (family == kCwtMorlet) {
        const double d = x - param;
        h = x > 0 ? g * cwt_exp<T>(-0.5 * d * d) : 0.0;
    } else if (family == kCwtPaul) {
        const double e = cwt_exp<T>(-x / (double)m);
        h = x > 0 && e > 0 ? g * cwt_ipow(x * e, m) : 0.0;
    } else {
        const double e = cwt_exp<T>(-(x * x) / (double)(2 * m));
        h = e > 0 ? g * cwt_ipow(x * e, m) : 0.0;
    }
    return (T)h;
}

// the bins k0 .. k0 + V of the rows (b, j_lo .. j_hi) as +0: an analytic family above P div 2
template <typename T>
__device__ inline void cwt_zero_rows(const CwtArgs &a, unsigned long long b, unsigned long long j_lo, unsigned long long j_hi,
                                     unsigned long long k0, bool whole) {
    constexpr unsigned V = 16 / sizeof(T);
    for (unsigned long long j = j_lo; j < j_hi; ++j) {
        const unsigned long long at = b * a.out_sig + j * a.out_row - a.out_off + k0;
        T *yr = (T *)a.out[0] + at, *yi = (T *)a.out[1] + at;
        if (whole && (((uintptr_t)yr | (uintptr_t)yi) & 15) == 0) {
            CwtVec<T> z;
#pragma unroll
            for (unsigned e = 0; e < V; ++e) z.v[e] = T(0);
            *(CwtVec<T> *)yr = z;
            *(CwtVec<T> *)yi = z;
        } else {
#pragma unroll
            for (unsigned e = 0; e < V; ++e)
                if (k0 + e < a.p) yr[e] = yi[e] = T(0);
        }
    }
}

template <typename T>
__global__ void __launch_bounds__(256) cwt_bank_kernel(CwtArgs a) {
    constexpr unsigned V = 16 / sizeof(T);
    const unsigned long long wg = (a.g0 >> 8) + blockIdx.x;
    if (wg * 256 >= a.groups) return;
    // (tile, scale group) of this workgroup; the group as counted over the whole call: b ngrp + j div kCwtGroup
    const unsigned long long gi = wg / a.tiles, tile = wg - gi * a.tiles;
    const unsigned long long gg = a.grp0 + gi, b = gg / a.ngrp, g = gg - b * a.ngrp;
    const unsigned long long k0 = (tile * 256 + threadIdx.x) * V;
    if (k0 >= a.p) return;
    const unsigned long long half = a.p / 2;
    const bool analytic = a.family != kCwtDog;
    const unsigned m = a.family == kCwtPaul || a.family == kCwtDog ? (unsigned)a.param : 0;
    const unsigned unit = a.family == kCwtDog ? m & 3 : 2;  // conj(-(i^m)): -1, i, 1, -i
    const unsigned long long direct = a.real_input ? half + 1 : a.p;  // the bins X holds
    const T *xr = (const T *)a.x[0] + (b - a.sig0) * a.xd, *xi = (const T *)a.x[1] + (b - a.sig0) * a.xd;

    // the scales of this group that are rows of the chunk
    unsigned long long j_lo = g * kCwtGroup, j_hi = j_lo + kCwtGroup < a.s ? j_lo + kCwtGroup : a.s;
    if (b * a.s + j_lo < a.row0) j_lo = a.row0 - b * a.s;
    if (b * a.s + j_hi > a.row0 + a.rows) j_hi = a.row0 + a.rows - b * a.s;
    const bool whole = k0 + V <= a.p;

    if (analytic && k0 > half) {  // nothing to read, nothing to evaluate
        cwt_zero_rows<T>(a, b, j_lo, j_hi, k0, whole);
        return;
    }

    T re[V], im[V], gain[V];  // gain: STEP's
    double om[V];
    bool dead[V];  // an analytic family's bin above P div 2: +0
    if (k0 + V <= direct && (((uintptr_t)(xr + k0) | (uintptr_t)(xi + k0)) & 15) == 0) {
        const CwtVec<T> vr = *(const CwtVec<T> *)(xr + k0), vi = *(const CwtVec<T> *)(xi + k0);
#pragma unroll
        for (unsigned e = 0; e < V; ++e) {
            re[e] = vr.v[e];
            im[e] = vi.v[e];
        }
    } else {
#pragma unroll
        for (unsigned e = 0; e < V; ++e) {
            const unsigned long long k = k0 + e;
            re[e] = im[e] = T(0);
            if (k < direct) {
                re[e] = xr[k];
                im[e] = xi[k];
            } else if (k < a.p && !analytic) {  // a real signal: X[k] = conj(X[P - k])
                const unsigned long long mk = a.p - k;  // in 1 .. P - P div 2 - 1 <= P div 2
                re[e] = xr[mk];
                im[e] = -xi[mk];
            }
        }
    }
#pragma unroll
    for (unsigned e = 0; e < V; ++e) {
        const unsigned long long k = k0 + e;
        dead[e] = analytic && k > half;
        om[e] = (6.283185307179586 * (double)cwt_signed_bin(k, a.p)) / (double)a.p;
        gain[e] = (T)cwt_step_gain(k, a.p);
    }

    for (unsigned long long j = j_lo; j < j_hi; ++j) {
        const double s = a.scales[j], gj = a.gains[j];
        CwtVec<T> wr, wi;
#pragma unroll
        for (unsigned e = 0; e < V; ++e) {
            const T h = a.family == kCwtStep ? gain[e] : cwt_filter<T>(a.family, a.param, m, s, gj, om[e]);
            const T pr = re[e] * h, pi = im[e] * h;
            T yr = pr, yi = pi;
            if (unit == 0) {
                yr = -pr;
                yi = -pi;
            } else if (unit == 1) {
                yr = -pi;
                yi = pr;
            } else if (unit == 3) {
                yr = pi;
                yi = -pr;
            }
            wr.v[e] = dead[e] ? T(0) : yr;
            wi.v[e] = dead[e] ? T(0) : yi;
        }
        const unsigned long long at = b * a.out_sig + j * a.out_row - a.out_off + k0;
        T *yr = (T *)a.out[0] + at, *yi = (T *)a.out[1] + at;
        if (whole && (((uintptr_t)yr | (uintptr_t)yi) & 15) == 0) {
            *(CwtVec<T> *)yr = wr;
            *(CwtVec<T> *)yi = wi;
        } else {
#pragma unroll
            for (unsigned e = 0; e < V; ++e)
                if (k0 + e < a.p) {
                    yr[e] = wr.v[e];
                    yi[e] = wi.v[e];
                }
        }
    }
}

template <typename T>
__global__ void __launch_bounds__(256) cwt_copy_kernel(CwtCopyArgs a) {
    const unsigned long long t = a.g0 + (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= a.groups) return;
    const unsigned long long per_plane = a.rows * a.n_out;
    const unsigned plane = t >= per_plane;
    const unsigned long long e = t - plane * per_plane, r = e / a.n_out, c = e - r * a.n_out;
    const unsigned long long row = a.row0 + r, b = row / a.s, j = row - b * a.s;
    const T x = c < a.n_in ? ((const T *)a.in[plane])[b * a.in_sig + j * a.in_row - a.in_off + c] : T(0);
    ((T *)a.out[plane])[b * a.out_sig + j * a.out_row - a.out_off + c] = x;
}

template <typename T> hipError_t launch_cwt_bank(const CwtArgs &a0, hipStream_t stream) {
    CwtArgs a = a0;
    return launch_in_slices(a.groups, [&](dim3 grid, unsigned long long g0) {
        a.g0 = g0;
        hipLaunchKernelGGL(cwt_bank_kernel<T>, grid, dim3(256), 0, stream, a);
    });
}
template hipError_t launch_cwt_bank<double>(const CwtArgs &, hipStream_t);
template hipError_t launch_cwt_bank<float>(const CwtArgs &, hipStream_t);

template <typename T> hipError_t launch_cwt_copy(const CwtCopyArgs &a0, hipStream_t stream) {
    CwtCopyArgs a = a0;
    return launch_in_slices(a.groups, [&](dim3 grid, unsigned long long g0) {
        a.g0 = g0;
        hipLaunchKernelGGL(cwt_copy_kernel<T>, grid, dim3(256), 0, stream, a);
    });
}
template hipError_t launch_cwt_copy<double>(const CwtCopyArgs &, hipStream_t);
template hipError_t launch_cwt_copy<float>(const CwtCopyArgs &, hipStream_t);

}  // namespace phast
