// nufft_t3.hip -- the two kernels of the type-3 non-uniform FFT (nufft_t3.hpp has the algorithm).
//
// spread is the gather of nufft.hip's spread kernel on the outer grid of n_f points, with the prephase multiply inside the
// walk, fused with the inner type 2's "pre": one thread per slot of the inner grid of n_g = 2 n_f points and transform.  A
// slot that holds a mode walks the sorted sources of the cells within ceil(w / 2) of its grid point, sums in registers in
// sorted order, multiplies by the inner 1 / phi^ and stores once; every other slot stores an exact zero.  No atomics, no LDS:
// the bits depend on nothing but the points and the data.  phi and the sums are in double for f64 and in float for f32.
//
// post is a streaming sweep built like nufft.hip's deconvolve: one group of 16 bytes per plane per thread, 256-thread
// workgroups in address order, launch_in_slices, and an element-access variant for planes that do not allow 16-byte accesses.
// It runs in place on the caller's output planes, where the interpolation kernel left its values.
#include "nufft_t3.hpp"

namespace phast {

template <typename T> struct NufftT3Real { typedef double type; };
template <> struct NufftT3Real<float> { typedef float type; };

// Slot s of transform b: mode k = s (s < n_f / 2) or s - n_g (s >= n_g - n_f / 2) sits at outer grid point l = k + n_f / 2;
// w[b n_g + s] = inv_hat[k mod n_f] sum_j phi(2 (l - p_j) / w) c[b in_dist + j] e^{-+2 pi i C_s x'_j}.  REAL: no imaginary plane
template <typename T, bool REAL>
__global__ void __launch_bounds__(256) nufft_t3_spread_kernel(NufftT3Args a) {
    using R = typename NufftT3Real<T>::type;
    const unsigned long long g = global_group(a);
    if (g >= a.groups) return;
    const unsigned log_g = a.log_f + 1;
    const unsigned long long nf = 1ull << a.log_f, mask = nf - 1, half = nf >> 1;
    const unsigned long long b = g >> log_g, slot = g & ((1ull << log_g) - 1);
    const bool low = slot < half, high = slot >= 2 * nf - half;
    R sr = 0, si = 0;
    if (low || high) {
        const unsigned long long l = low ? slot + half : slot - (2 * nf - half);  // the outer grid point, < n_f
        const unsigned long long mode = low ? slot : slot - nf;                   // its index in fftfreq order, < n_f
        const T *cr = (const T *)a.in_re + b * a.in_dist;
        const T *ci = REAL ? nullptr : (const T *)a.in_im + b * a.in_dist;
        const T *pre = (const T *)a.pre;
        const long long h = (a.w + 1) / 2;
        const double dgrid = (double)nf, two_over_w = 2.0 / a.w;
        const R beta = (R)nufft_beta(a.w), sg = a.reverse ? R(1) : R(-1);
        const unsigned long long lo = (l - (unsigned long long)h) & mask;  // the first cell; 2h <= n_f cells from there
        // the sorted range of those cells: one run, or two where the cells wrap past the end of the grid (no source lies
        // within w / 2 of the ends, so the far run is empty; it is walked all the same, as nufft_spread_kernel walks it)
        const unsigned long long end = lo + 2 * (unsigned long long)h;
        const bool wraps = end > nf;
        uint32_t i0 = a.cell_start[lo], i1 = a.cell_start[wraps ? nf : end];
        for (int run = 0; run < (wraps ? 2 : 1); ++run) {
            for (uint32_t i = i0; i < i1; ++i) {
                double t;
                const long long q = nufft_cell(a.xs[i], dgrid, &t);
                const long long dq = (long long)(((unsigned long long)((long long)l - q + (long long)half)) & mask) - (long long)half;
                const R k = nufft_weight<R>(dq, t, two_over_w, beta);
                const R pc = (R)pre[2 * (size_t)i], ps = sg * (R)pre[2 * (size_t)i + 1];
                const uint32_t j = a.perm[i];
                const R vr = (R)cr[j];
                if (REAL) {
                    sr += k * (vr * pc);
                    si += k * (vr * ps);
                } else {
                    const R vi = (R)ci[j];
                    sr += k * (vr * pc - vi * ps);
                    si += k * (vi * pc + vr * ps);
                }
            }
            if (wraps) {
                i0 = 0;
                i1 = a.cell_start[end - nf];
            }
        }
        const R p = (R)((const T *)a.inv_hat)[mode];
        sr *= p;
        si *= p;
    }
    ((T *)a.out_re)[g] = (T)sr;
    ((T *)a.out_im)[g] = (T)si;
}

// (vr + i vi) (pr + i pi) with the roundings spelled out, so that the 16-byte and the element variants give the same bits
template <typename T> __device__ inline void nufft_t3_mul(T vr, T vi, T pr, T pi, T *o_re, T *o_im) {
    *o_re = fma(vr, pr, -(vi * pi));
    *o_im = fma(vr, pi, vi * pr);
}

// f[b out_dist + k] *= D_k (Forward) or its phase conjugated (Reverse: phi^ is real, so conj D_k), k < K, in place
template <typename T, bool VEC>
__global__ void __launch_bounds__(256) nufft_t3_post_kernel(NufftT3Args a) {
    using V = typename AnyVec<T>::type;
    constexpr int W = AnyVec<T>::N;
    const unsigned long long g = global_group(a);
    if (g >= a.groups) return;
    unsigned long long b;
    const unsigned long long k0 = split_group(g, a.gpt, &b) * W;
    const T *dr = (const T *)a.d_re, *di = (const T *)a.d_im;
    T *fr = (T *)a.out_re + b * a.out_dist, *fi = (T *)a.out_im + b * a.out_dist;
    const T sg = a.reverse ? T(-1) : T(1);
    if (VEC && k0 + W <= a.k) {
        const V vr = *(const V *)(fr + k0), vi = *(const V *)(fi + k0);
        const V pr = *(const V *)(dr + k0), pi = *(const V *)(di + k0);
        V orr, oi;
#pragma unroll
        for (int j = 0; j < W; ++j) {
            T x, y;
            nufft_t3_mul<T>(vr[j], vi[j], pr[j], pi[j] * sg, &x, &y);
            orr[j] = x;
            oi[j] = y;
        }
        __builtin_nontemporal_store(orr, (V *)(fr + k0));
        __builtin_nontemporal_store(oi, (V *)(fi + k0));
    } else {
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const unsigned long long k = k0 + j;
            if (k < a.k) {
                T x, y;
                nufft_t3_mul<T>(fr[k], fi[k], dr[k], di[k] * sg, &x, &y);
                __builtin_nontemporal_store(x, fr + k);
                __builtin_nontemporal_store(y, fi + k);
            }
        }
    }
}

template <typename T> hipError_t launch_nufft_t3(int kind, bool vec, const NufftT3Args &a0, hipStream_t stream) {
    NufftT3Args a = a0;
    const bool real = a.in_im == nullptr;
    return launch_in_slices(a.groups, [&](dim3 grid, unsigned long long g0) {
        a.g0 = g0;
        if (kind == 0 && real)
            hipLaunchKernelGGL((nufft_t3_spread_kernel<T, true>), grid, dim3(256), 0, stream, a);
        else if (kind == 0)
            hipLaunchKernelGGL((nufft_t3_spread_kernel<T, false>), grid, dim3(256), 0, stream, a);
        else if (vec)
            hipLaunchKernelGGL((nufft_t3_post_kernel<T, true>), grid, dim3(256), 0, stream, a);
        else
            hipLaunchKernelGGL((nufft_t3_post_kernel<T, false>), grid, dim3(256), 0, stream, a);
    });
}

template hipError_t launch_nufft_t3<double>(int, bool, const NufftT3Args &, hipStream_t);
template hipError_t launch_nufft_t3<float>(int, bool, const NufftT3Args &, hipStream_t);

}  // namespace phast
