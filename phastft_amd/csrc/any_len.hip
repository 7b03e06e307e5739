// any_len.hip -- the streaming sweeps of the arbitrary-length (Bluestein) transform (any_len.hpp has the algorithm).
//
// Built like complex_nums.hip, the repository's copy-rate kernel: ONE step per thread (a group of 16 bytes per plane),
// one workgroup per 256 groups, workgroups in address order.  The workspace side is always 16-byte aligned (M is a power of
// two >= 8); the caller's planes take 16-byte accesses where base pointers and distance allow it and element accesses
// otherwise (`buf[1:]`), non-temporal either way (nothing of the caller's data is read twice).  The chirp is computed on the
// fly from the exact phase (any_len.hpp: chirp_r) in double, for f32 too -- a table of N points would add 16 bytes per point
// to the pre and post sweeps; profiles/any_len_rate.log has the rates that settled it.
#include "any_len.hpp"

namespace phast {

// a[b * M + k] = x[b * in_dist + k] w[k] for k < N, 0 up to M
template <typename T, bool VEC>
__global__ void __launch_bounds__(256) any_pre_kernel(AnySweepArgs a) {
    using V = typename AnyVec<T>::type;
    constexpr int L = AnyVec<T>::N;
    const unsigned long long g = global_group(a);
    if (g >= a.groups) return;
    const unsigned log_gpt = a.log_m - (L == 2 ? 1 : 2);
    const unsigned long long b = g >> log_gpt, k0 = (g & ((1ull << log_gpt) - 1)) * L;
    const T *xr = (const T *)a.in_re + b * a.in_dist, *xi = (const T *)a.in_im + b * a.in_dist;
    V vr, vi;
    T lr[L], li[L];
    if (VEC && k0 + L <= a.n) {
        vr = __builtin_nontemporal_load((const V *)(xr + k0));
        vi = __builtin_nontemporal_load((const V *)(xi + k0));
#pragma unroll
        for (int j = 0; j < L; ++j) {
            lr[j] = vr[j];
            li[j] = vi[j];
        }
    } else {
#pragma unroll
        for (int j = 0; j < L; ++j) {
            const bool in = k0 + j < a.n;
            lr[j] = in ? __builtin_nontemporal_load(xr + k0 + j) : T(0);
            li[j] = in ? __builtin_nontemporal_load(xi + k0 + j) : T(0);
        }
    }
#pragma unroll
    for (int j = 0; j < L; ++j) {
        T orr = 0, oi = 0;
        if (k0 + j < a.n) {
            double c, s;
            chirp(k0 + j, a.n, &c, &s);
            const double x = lr[j], y = li[j];
            orr = (T)(x * c - y * s);
            oi = (T)(x * s + y * c);
        }
        vr[j] = orr;
        vi[j] = oi;
    }
    const unsigned long long o = (b << a.log_m) + k0;
    *(V *)((T *)a.out_re + o) = vr;
    *(V *)((T *)a.out_im + o) = vi;
}

// A[b * M + k] *= Bh[k]
template <typename T>
__global__ void __launch_bounds__(256) any_spectrum_kernel(AnySweepArgs a) {
    using V = typename AnyVec<T>::type;
    constexpr int L = AnyVec<T>::N;
    const unsigned long long g = global_group(a);
    if (g >= a.groups) return;
    const unsigned long long o = g * L, k0 = o & ((1ull << a.log_m) - 1);
    V *pr = (V *)((T *)a.out_re + o), *pi = (V *)((T *)a.out_im + o);
    const V xr = *pr, xi = *pi;
    const V br = *(const V *)((const T *)a.bh_re + k0), bi = *(const V *)((const T *)a.bh_im + k0);
    *pr = xr * br - xi * bi;
    *pi = xr * bi + xi * br;
}

// X[b * out_dist + k] = w[k] c[b * M + k] * scale for k < N
template <typename T, bool VEC>
__global__ void __launch_bounds__(256) any_post_kernel(AnySweepArgs a) {
    using V = typename AnyVec<T>::type;
    constexpr int L = AnyVec<T>::N;
    const unsigned long long g = global_group(a);
    if (g >= a.groups) return;
    unsigned long long b;
    const unsigned long long k0 = split_group(g, a.gpt, &b) * L;
    const unsigned long long o = (b << a.log_m) + k0;
    const V cr = *(const V *)((const T *)a.in_re + o), ci = *(const V *)((const T *)a.in_im + o);
    T *xr = (T *)a.out_re + b * a.out_dist, *xi = (T *)a.out_im + b * a.out_dist;
    V vr, vi;
#pragma unroll
    for (int j = 0; j < L; ++j) {
        double c = 0, s = 0;
        if (k0 + j < a.n) chirp(k0 + j, a.n, &c, &s);
        const double x = (double)cr[j] * a.scale, y = (double)ci[j] * a.scale;
        vr[j] = (T)(x * c - y * s);
        vi[j] = (T)(x * s + y * c);
    }
    if (VEC && k0 + L <= a.n) {
        __builtin_nontemporal_store(vr, (V *)(xr + k0));
        __builtin_nontemporal_store(vi, (V *)(xi + k0));
    } else {
#pragma unroll
        for (int j = 0; j < L; ++j)
            if (k0 + j < a.n) {
                __builtin_nontemporal_store(vr[j], xr + k0 + j);
                __builtin_nontemporal_store(vi[j], xi + k0 + j);
            }
    }
}

__global__ void __launch_bounds__(256) any_chirp_b_kernel(double *re, double *im, unsigned long long n, unsigned log_m) {
    const unsigned long long m = 1ull << log_m, i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const unsigned long long j = i < n ? i : (i > m - n ? m - i : m);  // |lag| of entry i, m = none
    double c = 0, s = 0;
    if (j < m) chirp(j, n, &c, &s);
    re[i] = c;
    im[i] = -s;  // conj(w)
}

__global__ void __launch_bounds__(256) any_round_kernel(const double *in, float *out, unsigned long long count) {
    const unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (i < count) out[i] = (float)in[i];
}

template <typename T> hipError_t launch_any_sweep(int kind, bool vec, const AnySweepArgs &a0, hipStream_t stream) {
    AnySweepArgs a = a0;
    return launch_in_slices(a.groups, [&](dim3 grid, unsigned long long g0) {
        a.g0 = g0;
        if (kind == 0 && vec)
            hipLaunchKernelGGL((any_pre_kernel<T, true>), grid, dim3(256), 0, stream, a);
        else if (kind == 0)
            hipLaunchKernelGGL((any_pre_kernel<T, false>), grid, dim3(256), 0, stream, a);
        else if (kind == 1)
            hipLaunchKernelGGL(any_spectrum_kernel<T>, grid, dim3(256), 0, stream, a);
        else if (vec)
            hipLaunchKernelGGL((any_post_kernel<T, true>), grid, dim3(256), 0, stream, a);
        else
            hipLaunchKernelGGL((any_post_kernel<T, false>), grid, dim3(256), 0, stream, a);
    });
}

hipError_t launch_any_chirp_b(double *re, double *im, unsigned long long n, unsigned log_m, hipStream_t stream) {
    const unsigned long long blocks = ((1ull << log_m) + 255) / 256;  // M <= 2^30: 2^22 workgroups at most
    hipLaunchKernelGGL(any_chirp_b_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, re, im, n, log_m);
    return hipGetLastError();
}

hipError_t launch_any_round(const double *in, float *out, unsigned long long count, hipStream_t stream) {
    const unsigned long long blocks = (count + 255) / 256;  // count <= 2^31
    hipLaunchKernelGGL(any_round_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, in, out, count);
    return hipGetLastError();
}

template hipError_t launch_any_sweep<double>(int, bool, const AnySweepArgs &, hipStream_t);
template hipError_t launch_any_sweep<float>(int, bool, const AnySweepArgs &, hipStream_t);

}  // namespace phast
