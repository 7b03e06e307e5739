// czt.hip -- the pre and post sweeps and the b table of the chirp-Z transform (czt.hpp has the algorithm).
//
// Built like any_len.hip: ONE step per thread (a group of 16 bytes per plane), one workgroup per 256 groups, workgroups in
// address order.  The workspace side is always 16-byte aligned (L is a power of two >= 8); the caller's planes take 16-byte
// accesses where base pointers and distance allow it and element accesses otherwise, non-temporal either way.  The chirp is
// computed on the fly from the exact fixed-point phase (czt.hpp: czt_phase) in double, for f32 too, as any_len.hip does.
#include "czt.hpp"

namespace phast {

// exp(-2 pi i t) of a signed turn t as (cos, sin)
__device__ inline void czt_unit(double turns, double *c, double *s) { sincospi(-2.0 * turns, s, c); }

// a[b * L + n] = x[b * in_dist + n] exp(-2 pi i (n start + n^2 step / 2)) for n < N, 0 up to L.  REAL: no imaginary plane
template <typename T, bool VEC, bool REAL>
__global__ void __launch_bounds__(256) czt_pre_kernel(CztSweepArgs a) {
    using V = typename AnyVec<T>::type;
    constexpr int W = AnyVec<T>::N;
    const unsigned long long g = global_group(a);
    if (g >= a.groups) return;
    const unsigned log_gpt = a.log_l - (W == 2 ? 1 : 2);
    const unsigned long long b = g >> log_gpt, k0 = (g & ((1ull << log_gpt) - 1)) * W;
    const T *xr = (const T *)a.in_re + b * a.in_dist;
    const T *xi = REAL ? nullptr : (const T *)a.in_im + b * a.in_dist;
    V vr, vi;
    T lr[W], li[W];
    if (VEC && k0 + W <= a.n) {
        vr = __builtin_nontemporal_load((const V *)(xr + k0));
        if (!REAL) vi = __builtin_nontemporal_load((const V *)(xi + k0));
#pragma unroll
        for (int j = 0; j < W; ++j) {
            lr[j] = vr[j];
            li[j] = REAL ? T(0) : vi[j];
        }
    } else {
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const bool in = k0 + j < a.n;
            lr[j] = in ? __builtin_nontemporal_load(xr + k0 + j) : T(0);
            li[j] = in && !REAL ? __builtin_nontemporal_load(xi + k0 + j) : T(0);
        }
    }
#pragma unroll
    for (int j = 0; j < W; ++j) {
        T orr = 0, oi = 0;
        if (k0 + j < a.n) {
            double c, s;
            czt_unit(czt_phase(k0 + j, a.half_step, a.start), &c, &s);
            const double x = lr[j], y = li[j];
            orr = (T)(x * c - y * s);
            oi = (T)(x * s + y * c);
        }
        vr[j] = orr;
        vi[j] = oi;
    }
    const unsigned long long o = (b << a.log_l) + k0;
    *(V *)((T *)a.out_re + o) = vr;
    *(V *)((T *)a.out_im + o) = vi;
}

// X[b * out_dist + k] = c[k] w[b * L + k] for k < M
template <typename T, bool VEC>
__global__ void __launch_bounds__(256) czt_post_kernel(CztSweepArgs a) {
    using V = typename AnyVec<T>::type;
    constexpr int W = AnyVec<T>::N;
    const unsigned long long g = global_group(a);
    if (g >= a.groups) return;
    unsigned long long b;
    const unsigned long long k0 = split_group(g, a.gpt, &b) * W;
    const unsigned long long o = (b << a.log_l) + k0;  // k0 + W <= L: M <= L and both are multiples of W after rounding up
    const V cr = *(const V *)((const T *)a.in_re + o), ci = *(const V *)((const T *)a.in_im + o);
    T *xr = (T *)a.out_re + b * a.out_dist, *xi = (T *)a.out_im + b * a.out_dist;
    const CztFrac none{0, 0};
    V vr, vi;
#pragma unroll
    for (int j = 0; j < W; ++j) {
        double c = 0, s = 0;
        if (k0 + j < a.n) czt_unit(czt_phase(k0 + j, a.half_step, none), &c, &s);
        const double x = cr[j], y = ci[j];
        vr[j] = (T)(x * c - y * s);
        vi[j] = (T)(x * s + y * c);
    }
    if (VEC && k0 + W <= a.n) {
        __builtin_nontemporal_store(vr, (V *)(xr + k0));
        __builtin_nontemporal_store(vi, (V *)(xi + k0));
    } else {
#pragma unroll
        for (int j = 0; j < W; ++j)
            if (k0 + j < a.n) {
                __builtin_nontemporal_store(vr[j], xr + k0 + j);
                __builtin_nontemporal_store(vi[j], xi + k0 + j);
            }
    }
}

__global__ void __launch_bounds__(256) czt_chirp_b_kernel(double *re, double *im, unsigned long long n, unsigned long long m,
                                                          unsigned log_l, CztFrac half_step) {
    const unsigned long long l = 1ull << log_l, i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= l) return;
    const unsigned long long j = i < m ? i : (i > l - n ? l - i : l);  // |lag| of entry i, l = none
    double c = 0, s = 0;
    if (j < l) czt_unit(czt_phase(j, half_step, CztFrac{0, 0}), &c, &s);
    re[i] = c;
    im[i] = -s;  // conj(c)
}

template <typename T> hipError_t launch_czt_sweep(int kind, bool vec, const CztSweepArgs &a0, hipStream_t stream) {
    CztSweepArgs a = a0;
    const bool real = a.in_im == nullptr;
    return launch_in_slices(a.groups, [&](dim3 grid, unsigned long long g0) {
        a.g0 = g0;
        if (kind == 0 && vec && real)
            hipLaunchKernelGGL((czt_pre_kernel<T, true, true>), grid, dim3(256), 0, stream, a);
        else if (kind == 0 && vec)
            hipLaunchKernelGGL((czt_pre_kernel<T, true, false>), grid, dim3(256), 0, stream, a);
        else if (kind == 0 && real)
            hipLaunchKernelGGL((czt_pre_kernel<T, false, true>), grid, dim3(256), 0, stream, a);
        else if (kind == 0)
            hipLaunchKernelGGL((czt_pre_kernel<T, false, false>), grid, dim3(256), 0, stream, a);
        else if (vec)
            hipLaunchKernelGGL((czt_post_kernel<T, true>), grid, dim3(256), 0, stream, a);
        else
            hipLaunchKernelGGL((czt_post_kernel<T, false>), grid, dim3(256), 0, stream, a);
    });
}

hipError_t launch_czt_chirp_b(double *re, double *im, unsigned long long n, unsigned long long m, unsigned log_l, CztFrac half_step,
                              hipStream_t stream) {
    const unsigned long long blocks = ((1ull << log_l) + 255) / 256;  // L <= 2^30: 2^22 workgroups at most
    hipLaunchKernelGGL(czt_chirp_b_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, re, im, n, m, log_l, half_step);
    return hipGetLastError();
}

template hipError_t launch_czt_sweep<double>(int, bool, const CztSweepArgs &, hipStream_t);
template hipError_t launch_czt_sweep<float>(int, bool, const CztSweepArgs &, hipStream_t);

}  // namespace phast
