// psd.hip -- the sweeps of Welch spectral estimation (psd.hpp has the definitions and the schedule).
//
// Built as stft.hip and mdct.hip are: 256-thread workgroups in address order, launches split at 2^31 - 1 workgroups, a thread
// owns one group of V = 16 / sizeof(T) consecutive elements of the side it writes (the mean sweep: one thread is one group).
//     mean    psd_mean_threads(P) threads share a segment: each adds every tpr-th sample (less the segment's first) in double, and one LDS tree of fixed
//             order adds the threads.  No cross-lane moves: the order of the additions is a function of P alone.
//     frame   the interior fast path of stft.hip's frame sweep (one 16-byte load of element alignment, one 16-byte store)
//             with the mean taken off and the window applied in double; nothing lies outside [0, L), so there is no padding path.
//     accum   a thread owns V bins of one slab of one signal: it adds the slab's frames that the chunk holds in ascending
//             order to the slab's partial row (doubles; a slab whose first frame the chunk holds starts from 0) and stores it.
//     final   a thread owns V elements of the packed output: per element the partial rows of the signal in ascending slab
//             order, times sigma c_k / S, rounded to T once and stored non-temporally (16 bytes where the address allows).
//     point   average = 0: sigma c_k |X|^2 (cross: sigma c_k conj(X) Y) of every frame, same ownership as final.
// The spectrum planes and the partial rows are workspace: ordinary cached accesses.  No atomics, no scratch memory.
#include "psd.hpp"

namespace phast {

// (signal, frame) of row r of the chunk and the signal's base: rows [c, 2c) of a cross call are y's
template <typename T>
__device__ inline const T *psd_segment(const PsdArgs &a, unsigned long long r) {
    const bool second = r >= a.c;
    unsigned long long b;
    const unsigned long long f = split_group(a.q0 + (second ? r - a.c : r), (unsigned)a.frames, &b);  // frames <= 2^30
    return (const T *)(second ? a.y : a.x) + b * a.sig_dist + f * a.h;
}

// ---- mean: mean[r] = (1/P) sum_j (x[f H + j] - x[f H]) in double: m_f less the segment's first sample.  (The differences
// are of the size of the signal's variation, not of its offset: a plain double sum of samples near 1000 is wrong by 1e-13 of
// them, which an f64 estimate shows.) ----
template <typename T>
__global__ void __launch_bounds__(256) psd_mean_kernel(PsdArgs a) {
    __shared__ double part[256];
    const unsigned t = threadIdx.x, tpr = a.tpr, lane = t & (tpr - 1);
    const unsigned long long g = global_group(a), r = g >> __builtin_ctz(tpr);  // (every slice starts at a multiple of 256)
    const bool live = g < a.groups;
    double s = 0;
    if (live) {
        const T *x = psd_segment<T>(a, r);
        const double x0 = (double)x[0];
        for (unsigned long long j = lane; j < a.p; j += tpr) s += (double)x[j] - x0;
    }
    part[t] = s;
    for (unsigned step = tpr >> 1; step; step >>= 1) {
        __syncthreads();
        if (lane < step) part[t] += part[t + step];
    }
    if (live && lane == 0) a.mean[r] = part[t] / (double)a.p;
}

// ---- frame: row r = T(w[j] (x[f H + j] - m_f)), j < P, with x - m_f = (x - x[f H]) - mean[r]; zeros up to fd ----
template <typename T>
__global__ void __launch_bounds__(256) psd_frame_kernel(PsdArgs a) {
    using V = typename AnyVec<T>::type;
    using VU = typename Unaligned<T>::type;
    using D2 = typename AnyVec<double>::type;
    constexpr int L = AnyVec<T>::N;
    const unsigned long long g = global_group(a);
    if (g >= a.groups) return;
    unsigned long long r;
    const unsigned long long j0 = split_group(g, a.gpt, &r) * L;
    const T *x = psd_segment<T>(a, r);
    const double m = a.mean ? a.mean[r] : 0.0, x0 = a.mean ? (double)x[0] : 0.0;
    double w[L];
#pragma unroll
    for (int j = 0; j < L; j += 2) {
        const D2 d = *(const D2 *)(a.win + j0 + j);  // zeros beyond P
        w[j] = d[0];
        w[j + 1] = d[1];
    }
    V v;
    if (j0 + L <= a.p) {  // an interior group
        const VU u = *(const VU *)(x + j0);
#pragma unroll
        for (int j = 0; j < L; ++j) v[j] = (T)((((double)u[j] - x0) - m) * w[j]);
    } else {
#pragma unroll
        for (int j = 0; j < L; ++j) v[j] = j0 + j < a.p ? (T)((((double)x[j0 + j] - x0) - m) * w[j]) : T(0);
    }
    *(V *)((T *)a.rows + r * a.fd + j0) = v;
}

// the partial row of (signal b, plane, slab)
__device__ inline double *psd_partial(const PsdArgs &a, unsigned long long b, int plane, unsigned long long slab) {
    return a.acc + (((b % a.slots) * (unsigned)a.planes + (unsigned)plane) * a.slabs + slab) * a.bd;
}

// ---- accum: partial[slab][k] += sum over the slab's frames in the chunk, ascending, of |X|^2 (CROSS: conj(X) Y, |X|^2, |Y|^2) ----
template <typename T, bool CROSS>
__global__ void __launch_bounds__(256) psd_accum_kernel(PsdArgs a) {
    using V = typename AnyVec<T>::type;
    constexpr int L = AnyVec<T>::N, NP = CROSS ? 4 : 1;
    const unsigned long long g = global_group(a);
    if (g >= a.groups) return;
    unsigned long long u, bb;
    const unsigned long long k0 = split_group(g, a.gpt, &u) * L;
    const unsigned long long slab = a.s0 + split_group(u, (unsigned)a.ns, &bb), b = a.b0 + bb;  // slabs < 2^27
    const unsigned long long first = b * a.frames, end = first + a.frames, q1 = a.q0 + a.c;
    const unsigned long long c_lo = (a.q0 > first ? a.q0 : first) - first, c_hi = (q1 < end ? q1 : end) - first;
    unsigned long long lo, hi;
    psd_slab_range(slab, a.q, c_lo, c_hi, &lo, &hi);
    if (lo >= hi) return;
    double s[NP][L];
    const bool fresh = lo == slab * a.q;  // the chunk holds the slab's first frame
#pragma unroll
    for (int pl = 0; pl < NP; ++pl) {
        const double *row = psd_partial(a, b, pl, slab) + k0;
#pragma unroll
        for (int j = 0; j < L; ++j) s[pl][j] = fresh ? 0.0 : row[j];
    }
    const T *re = (const T *)a.re + k0, *im = (const T *)a.im + k0;
    for (unsigned long long f = lo; f < hi; ++f) {
        const unsigned long long r = first + f - a.q0;
        const V xr = *(const V *)(re + r * a.bd), xi = *(const V *)(im + r * a.bd);
        if constexpr (CROSS) {
            const V yr = *(const V *)(re + (r + a.c) * a.bd), yi = *(const V *)(im + (r + a.c) * a.bd);
#pragma unroll
            for (int j = 0; j < L; ++j) {
                const double ar = xr[j], ai = xi[j], br = yr[j], bi = yi[j];
                s[0][j] += ar * br + ai * bi;
                s[1][j] += ar * bi - ai * br;
                s[2][j] += ar * ar + ai * ai;
                s[3][j] += br * br + bi * bi;
            }
        } else {
#pragma unroll
            for (int j = 0; j < L; ++j) {
                const double ar = xr[j], ai = xi[j];
                s[0][j] += ar * ar + ai * ai;
            }
        }
    }
#pragma unroll
    for (int pl = 0; pl < NP; ++pl) {
        double *row = psd_partial(a, b, pl, slab) + k0;
#pragma unroll
        for (int j = 0; j < L; ++j) row[j] = s[pl][j];
    }
}

// V consecutive elements of a packed output from element e0 on: 16 bytes where the address allows, elements otherwise
template <typename T>
__device__ inline void psd_store(T *out, unsigned long long e0, unsigned long long count, typename AnyVec<T>::type o) {
    using V = typename AnyVec<T>::type;
    constexpr int L = AnyVec<T>::N;
    if (e0 + L <= count && aligned16(out + e0)) {
        __builtin_nontemporal_store(o, (V *)(out + e0));
    } else {
#pragma unroll
        for (int j = 0; j < L; ++j)
            if (e0 + j < count) __builtin_nontemporal_store((T)o[j], out + e0 + j);
    }
}

// ---- final: out[b][k] = T(scale c_k sum_slab partial[slab][k]), ascending slabs, for the signals b0 .. of this launch ----
template <typename T, bool CROSS>
__global__ void __launch_bounds__(256) psd_final_kernel(PsdArgs a) {
    using V = typename AnyVec<T>::type;
    constexpr int L = AnyVec<T>::N, NP = CROSS ? 4 : 1;
    const unsigned long long g = global_group(a);
    if (g >= a.groups) return;
    const unsigned long long e0 = g * L;
    V o[NP];
#pragma unroll
    for (int j = 0; j < L; ++j) {
        unsigned long long bb = 0;
        const unsigned long long e = e0 + j < a.count ? e0 + j : a.count - 1;  // (a lane past the end repeats the last element)
        const unsigned long long k = split_group(e, (unsigned)a.bins, &bb);
        const double sc = a.scale * psd_onesided(k, a.nfft);
#pragma unroll
        for (int pl = 0; pl < NP; ++pl) {
            if (!a.out[pl]) continue;
            const double *row = psd_partial(a, a.b0 + bb, pl, 0) + k;
            double s = 0;
            for (unsigned long long sl = 0; sl < a.slabs; ++sl) s += row[sl * a.bd];
            o[pl][j] = (T)(s * sc);
        }
    }
#pragma unroll
    for (int pl = 0; pl < NP; ++pl)
        if (a.out[pl]) psd_store<T>((T *)a.out[pl] + a.b0 * a.bins, e0, a.count, o[pl]);
}

// ---- point: out[q0 + r][k] = T(scale c_k |X_r[k]|^2) (CROSS: conj(X) Y, |X|^2, |Y|^2) for the c rows of the chunk ----
template <typename T, bool CROSS>
__global__ void __launch_bounds__(256) psd_point_kernel(PsdArgs a) {
    using V = typename AnyVec<T>::type;
    constexpr int L = AnyVec<T>::N, NP = CROSS ? 4 : 1;
    const unsigned long long g = global_group(a);
    if (g >= a.groups) return;
    const unsigned long long e0 = g * L;
    const T *re = (const T *)a.re, *im = (const T *)a.im;
    V o[NP];
#pragma unroll
    for (int j = 0; j < L; ++j) {
        unsigned long long r = 0;
        const unsigned long long e = e0 + j < a.count ? e0 + j : a.count - 1;
        const unsigned long long k = split_group(e, (unsigned)a.bins, &r);
        const double sc = a.scale * psd_onesided(k, a.nfft);
        const double ar = re[r * a.bd + k], ai = im[r * a.bd + k];
        if constexpr (CROSS) {
            const double br = re[(r + a.c) * a.bd + k], bi = im[(r + a.c) * a.bd + k];
            o[0][j] = (T)((ar * br + ai * bi) * sc);
            o[1][j] = (T)((ar * bi - ai * br) * sc);
            o[2][j] = (T)((ar * ar + ai * ai) * sc);
            o[3][j] = (T)((br * br + bi * bi) * sc);
        } else {
            o[0][j] = (T)((ar * ar + ai * ai) * sc);
        }
    }
#pragma unroll
    for (int pl = 0; pl < NP; ++pl)
        if (a.out[pl]) psd_store<T>((T *)a.out[pl] + a.q0 * a.bins, e0, a.count, o[pl]);
}

template <typename T> hipError_t launch_psd(int kind, const PsdArgs &a0, hipStream_t stream) {
    if (kind < kPsdMean || kind > kPsdPoint) return hipErrorInvalidValue;
    PsdArgs a = a0;
    const bool cross = a.planes == 4;
    return launch_in_slices(a.groups, [&](dim3 grid, unsigned long long g0) {
        a.g0 = g0;
        const dim3 block(256);
        switch (kind) {
        case kPsdMean: hipLaunchKernelGGL((psd_mean_kernel<T>), grid, block, 0, stream, a); break;
        case kPsdFrame: hipLaunchKernelGGL((psd_frame_kernel<T>), grid, block, 0, stream, a); break;
        case kPsdAccum:
            if (cross) hipLaunchKernelGGL((psd_accum_kernel<T, true>), grid, block, 0, stream, a);
            else hipLaunchKernelGGL((psd_accum_kernel<T, false>), grid, block, 0, stream, a);
            break;
        case kPsdFinal:
            if (cross) hipLaunchKernelGGL((psd_final_kernel<T, true>), grid, block, 0, stream, a);
            else hipLaunchKernelGGL((psd_final_kernel<T, false>), grid, block, 0, stream, a);
            break;
        default:
            if (cross) hipLaunchKernelGGL((psd_point_kernel<T, true>), grid, block, 0, stream, a);
            else hipLaunchKernelGGL((psd_point_kernel<T, false>), grid, block, 0, stream, a);
        }
    });
}

template hipError_t launch_psd<double>(int, const PsdArgs &, hipStream_t);
template hipError_t launch_psd<float>(int, const PsdArgs &, hipStream_t);

}  // namespace phast
