// lomb.hip -- the sweeps of the Lomb-Scargle periodogram (lomb.hpp has the definitions and the schedule).
//
// Built as psd.hip and nufft_t3.hip are: 256-thread workgroups in address order, launches split at 2^31 - 1 workgroups.
//     partial   workgroup b * slabs + s owns slab s of signal b: thread t adds w_j (y_j - y_0) over the 16-byte groups
//               t, t + 256, ... of the slab in ascending order, in double; one LDS tree of fixed order adds the threads.
//               No cross-lane moves: the order of the additions is a function of M alone.
//     final     workgroup b owns signal b: its threads load the partials into LDS, thread 0 adds them in ascending slab order.
//     strength  the same ownership as partial: c_j = T(w_j r_j), r_j = (y_j - y_0) - (Y - y_0), one 16-byte store per group
//               (zeros from M to the plane's end), and w_j r_j^2 through the same tree into the partials of YY.
//     post      a thread owns V consecutive frequencies of one signal: 16-byte loads of A1's planes and of the four tables,
//               the rotation, a, b, the normalisation, one non-temporal store (VEC: 16 bytes; else elements).
// The caller's signals are read with 16-byte loads of element alignment (any pointer, any distance) and by elements at a
// signal's end.  The strengths, A1's planes, the partials and the tables are workspace or planner memory: ordinary cached
// accesses.  No atomics, no scratch memory.
#include "lomb.hpp"

namespace phast {

// the workgroup's sum of `s` over its 256 threads, in thread 0
__device__ inline double lomb_tree(double *part, double s) {
    const unsigned t = threadIdx.x;
    part[t] = s;
    for (unsigned step = 128; step; step >>= 1) {
        __syncthreads();
        if (t < step) part[t] += part[t + step];
    }
    return part[0];
}

// ---- partial and strength: STRENGTH = false: part[wg] = sum over the slab of w_j (y_j - y_0); true: the strengths of the
// slab and part[wg] = sum w_j r_j^2 ----
template <typename T, bool STRENGTH>
__global__ void __launch_bounds__(256) lomb_slab_kernel(LombArgs a) {
    using V = typename AnyVec<T>::type;
    using VU = typename Unaligned<T>::type;
    constexpr int L = AnyVec<T>::N;
    __shared__ double part[256];
    const unsigned long long wg = (a.g0 >> 8) + blockIdx.x;  // (every slice starts at a multiple of 256 groups)
    const bool live = wg * 256 < a.groups;                   // whole workgroups: all threads agree
    double s = 0;
    if (live) {
        unsigned long long b;
        const unsigned long long slab = split_group(wg, (unsigned)a.slabs, &b);
        const T *y = (const T *)a.y + b * a.sig_dist, *w = (const T *)a.w;
        const unsigned long long lo = slab * a.q, hi = lo + a.q < a.md ? lo + a.q : a.md;
        const bool shift = !STRENGTH || a.floating_mean;
        const double y0 = shift ? (double)y[0] : 0.0, d = STRENGTH && a.floating_mean ? a.stat[2 * b] : 0.0;
        for (unsigned long long j0 = lo + (unsigned long long)threadIdx.x * L; j0 < hi; j0 += 256ull * L) {
            const V wv = *(const V *)(w + j0);  // zeros beyond M
            double r[L];
            if (j0 + L <= a.m) {
                const VU u = *(const VU *)(y + j0);
#pragma unroll
                for (int j = 0; j < L; ++j) r[j] = ((double)u[j] - y0) - d;
            } else {
#pragma unroll
                for (int j = 0; j < L; ++j) r[j] = j0 + j < a.m ? ((double)y[j0 + j] - y0) - d : 0.0;
            }
            if constexpr (STRENGTH) {
                V c;
#pragma unroll
                for (int j = 0; j < L; ++j) {
                    const double p = (double)wv[j] * r[j];
                    c[j] = (T)p;
                    s += p * r[j];
                }
                *(V *)((T *)a.strength + b * a.md + j0) = c;
            } else {
#pragma unroll
                for (int j = 0; j < L; ++j) s += (double)wv[j] * r[j];
            }
        }
    }
    const double sum = lomb_tree(part, s);
    if (live && threadIdx.x == 0) a.part[wg] = sum;
}

// ---- final: stat[b][which] = scale * the partials of signal b in ascending slab order.  Workgroup b: its threads bring the
// partials (at most kLombMaxSlabs) into LDS side by side, thread 0 adds them one after the other -- the order of a serial
// loop at the latency of LDS instead of a dependent chain of global loads ----
__global__ void __launch_bounds__(256) lomb_final_kernel(LombArgs a) {
    __shared__ double part[kLombMaxSlabs];
    const unsigned long long b = (a.g0 >> 8) + blockIdx.x;
    const bool live = b * 256 < a.groups;  // whole workgroups: all threads agree
    if (live) {
        const double *p = a.part + b * a.slabs;
        for (unsigned long long i = threadIdx.x; i < a.slabs; i += 256) part[i] = p[i];
    }
    __syncthreads();
    if (!live || threadIdx.x) return;
    double s = 0;
    for (unsigned long long i = 0; i < a.slabs; ++i) s += part[i];
    a.stat[2 * b + a.which] = s * a.scale;
}

// ---- post: out[b][k] from A1[b][k] and the tables of k ----
template <typename T, bool VEC>
__global__ void __launch_bounds__(256) lomb_post_kernel(LombArgs a) {
    using V = typename AnyVec<T>::type;
    constexpr int L = AnyVec<T>::N;
    const unsigned long long g = global_group(a);
    if (g >= a.groups) return;
    unsigned long long b;
    const unsigned long long k0 = split_group(g, a.gpt, &b) * L;
    const V ar = *(const V *)((const T *)a.re + b * a.kd + k0), ai = *(const V *)((const T *)a.im + b * a.kd + k0);
    const V ct = *(const V *)((const T *)a.tab[0] + k0), st = *(const V *)((const T *)a.tab[1] + k0);
    const V icc = *(const V *)((const T *)a.tab[2] + k0), iss = *(const V *)((const T *)a.tab[3] + k0);
    const double sc = a.norm == kLombNormalize ? 0.5 / a.stat[2 * b + 1] : a.scale;
    V o_re, o_im;
#pragma unroll
    for (int j = 0; j < L; ++j) {
        double ca, cb;
        const double p = lomb_post((double)ar[j], (double)ai[j], (double)ct[j], (double)st[j], (double)icc[j], (double)iss[j], &ca, &cb);
        if (a.norm == kLombAmplitude) {
            o_re[j] = (T)(ca * (double)ct[j] - cb * (double)st[j]);
            o_im[j] = (T)(ca * (double)st[j] + cb * (double)ct[j]);
        } else {
            o_re[j] = (T)(p * sc);
            o_im[j] = T(0);
        }
    }
    const bool amp = a.norm == kLombAmplitude;
    T *out_re = (T *)a.out_re + b * a.out_dist + k0, *out_im = amp ? (T *)a.out_im + b * a.out_dist + k0 : nullptr;
    if (VEC && k0 + L <= a.k) {
        __builtin_nontemporal_store(o_re, (V *)out_re);
        if (amp) __builtin_nontemporal_store(o_im, (V *)out_im);
    } else {
#pragma unroll
        for (int j = 0; j < L; ++j)
            if (k0 + j < a.k) {
                __builtin_nontemporal_store((T)o_re[j], out_re + j);
                if (amp) __builtin_nontemporal_store((T)o_im[j], out_im + j);
            }
    }
}

template <typename T> hipError_t launch_lomb(int kind, bool vec, const LombArgs &a0, hipStream_t stream) {
    if (kind < kLombPartial || kind > kLombPost) return hipErrorInvalidValue;
    LombArgs a = a0;
    return launch_in_slices(a.groups, [&](dim3 grid, unsigned long long g0) {
        a.g0 = g0;
        const dim3 block(256);
        switch (kind) {
        case kLombPartial: hipLaunchKernelGGL((lomb_slab_kernel<T, false>), grid, block, 0, stream, a); break;
        case kLombFinal: hipLaunchKernelGGL(lomb_final_kernel, grid, block, 0, stream, a); break;
        case kLombStrength: hipLaunchKernelGGL((lomb_slab_kernel<T, true>), grid, block, 0, stream, a); break;
        default:
            if (vec) hipLaunchKernelGGL((lomb_post_kernel<T, true>), grid, block, 0, stream, a);
            else hipLaunchKernelGGL((lomb_post_kernel<T, false>), grid, block, 0, stream, a);
        }
    });
}

template hipError_t launch_lomb<double>(int, bool, const LombArgs &, hipStream_t);
template hipError_t launch_lomb<float>(int, bool, const LombArgs &, hipStream_t);

}  // namespace phast
