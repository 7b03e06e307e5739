// dct.hip -- the four streaming sweeps of the DCT / DST of types II and III (dct.hpp has the algorithm).
//
// Built as any_real.hip is: 256-thread workgroups in address order, launches split at 2^31 - 1 workgroups, non-temporal
// accesses on the caller's data, 16-byte accesses on the caller's side where base and dist allow it and element accesses
// otherwise.  A thread owns one group of L = 16 / sizeof(T) consecutive workspace elements (16-byte aligned: the planner pads
// every workspace row to a multiple of L), so the workspace side's ascending half always moves in 16-byte accesses.  The
// other half of every sweep runs descending (N - 1 - i, N - k): lane l of a wave owns index base + l, so those element
// accesses of one wave form one contiguous run.  Twiddles e^{-+i pi k / (2N)} are evaluated on the fly as sincospi in double,
// for f32 too (no table: DESIGN.md §14 has the measurement).
#include "dct.hpp"

namespace phast {

// ---- II-pre: v[i] = x[2i] (i < e), v[N-1-i] = +-x[2i+1] (i < h; DST: negated) ----
template <typename T, bool DST, bool VEC>
__global__ void __launch_bounds__(256) dct2_pre_kernel(DctArgs a) {
    using V = typename AnyVec<T>::type;
    constexpr int L = AnyVec<T>::N;
    const unsigned long long g = global_group(a);
    if (g >= a.groups) return;
    unsigned long long b;
    const unsigned long long i0 = split_group(g, a.gpt, &b) * L, n = a.n, e = (n + 1) / 2, h = n / 2;
    const T *x = (const T *)a.in + b * a.in_dist;
    T *v = (T *)a.out + b * a.out_dist;
    T ev[L], od[L];
    if (VEC && 2 * i0 + 2 * L <= n) {
        const V v0 = __builtin_nontemporal_load((const V *)(x + 2 * i0)), v1 = __builtin_nontemporal_load((const V *)(x + 2 * i0 + L));
#pragma unroll
        for (int j = 0; j < L / 2; ++j) {
            ev[j] = v0[2 * j];
            od[j] = v0[2 * j + 1];
            ev[L / 2 + j] = v1[2 * j];
            od[L / 2 + j] = v1[2 * j + 1];
        }
    } else {
#pragma unroll
        for (int j = 0; j < L; ++j) {
            const unsigned long long i = i0 + j;
            ev[j] = i < e ? __builtin_nontemporal_load(x + 2 * i) : T(0);
            od[j] = i < h ? __builtin_nontemporal_load(x + 2 * i + 1) : T(0);
        }
    }
    if (i0 + L <= e) {
        V w;
#pragma unroll
        for (int j = 0; j < L; ++j) w[j] = ev[j];
        *(V *)(v + i0) = w;
    } else {
#pragma unroll
        for (int j = 0; j < L; ++j)
            if (i0 + j < e) v[i0 + j] = ev[j];
    }
#pragma unroll
    for (int j = 0; j < L; ++j)
        if (i0 + j < h) v[n - 1 - i0 - j] = DST ? -od[j] : od[j];
}

// ---- II-post: z = e^{-i pi k/(2N)} V[k]; DCT y[k] = s Re z (k <= h), y[N-k] = -s Im z (1 <= k < e); DST y[N-1-k], y[k-1].
// For even N bin h = N/2 is written once, from the real part ----
template <typename T, bool DST, bool VEC>
__global__ void __launch_bounds__(256) dct2_post_kernel(DctArgs a) {
    using V = typename AnyVec<T>::type;
    constexpr int L = AnyVec<T>::N;
    const unsigned long long g = global_group(a);
    if (g >= a.groups) return;
    unsigned long long b;
    const unsigned long long k0 = split_group(g, a.gpt, &b) * L, n = a.n, e = (n + 1) / 2, h = n / 2;
    const V fr = *(const V *)((const T *)a.in + b * a.in_dist + k0), fi = *(const V *)((const T *)a.in_im + b * a.in_dist + k0);
    T *y = (T *)a.out + b * a.out_dist;
    T re[L], im[L];
#pragma unroll
    for (int j = 0; j < L; ++j) {
        const unsigned long long k = k0 + j;
        double c, s;
        sincospi(dct_turns(2, k, n), &s, &c);
        const double sc = k == 0 ? a.scale0 : a.scale;
        const double r = fr[j], i = fi[j];
        re[j] = (T)(sc * (r * c - i * s));
        im[j] = (T)(-sc * (r * s + i * c));
    }
    if (!DST && VEC && k0 + L - 1 <= h) {
        V w;
#pragma unroll
        for (int j = 0; j < L; ++j) w[j] = re[j];
        __builtin_nontemporal_store(w, (V *)(y + k0));
    } else {
#pragma unroll
        for (int j = 0; j < L; ++j)
            if (k0 + j <= h) __builtin_nontemporal_store(re[j], y + dct2_re_index(DST, k0 + j, n));
    }
#pragma unroll
    for (int j = 0; j < L; ++j) {
        const unsigned long long k = k0 + j;
        if (k >= 1 && k < e) __builtin_nontemporal_store(im[j], y + dct2_im_index(DST, k, n));
    }
}

// ---- III-pre: V[k] = s e^{i pi k/(2N)} (A - i B), A = X'[k], B = X'[N-k] (0 for k = 0); DCT X' = X, DST X' = X reversed.
// Im V[0] and, for even N, Im V[N/2] are written as exact zeros; the row's padding beyond h as zeros ----
template <typename T, bool DST, bool VEC>
__global__ void __launch_bounds__(256) dct3_pre_kernel(DctArgs a) {
    using V = typename AnyVec<T>::type;
    constexpr int L = AnyVec<T>::N;
    const unsigned long long g = global_group(a);
    if (g >= a.groups) return;
    unsigned long long b;
    const unsigned long long k0 = split_group(g, a.gpt, &b) * L, n = a.n, h = n / 2;
    const T *X = (const T *)a.in + b * a.in_dist;
    T av[L], bv[L];
    if (!DST && VEC && k0 + L - 1 <= h && k0 + L <= n) {
        const V v = __builtin_nontemporal_load((const V *)(X + k0));
#pragma unroll
        for (int j = 0; j < L; ++j) av[j] = v[j];
    } else {
#pragma unroll
        for (int j = 0; j < L; ++j) av[j] = k0 + j <= h ? __builtin_nontemporal_load(X + dct3_a_index(DST, k0 + j, n)) : T(0);
    }
#pragma unroll
    for (int j = 0; j < L; ++j) {
        const unsigned long long k = k0 + j;
        bv[j] = k >= 1 && k <= h ? __builtin_nontemporal_load(X + dct3_b_index(DST, k, n)) : T(0);
    }
    V wr, wi;
#pragma unroll
    for (int j = 0; j < L; ++j) {
        const unsigned long long k = k0 + j;
        wr[j] = wi[j] = 0;
        if (k > h) continue;
        double c, s;
        sincospi(dct_turns(3, k, n), &s, &c);
        const double sc = k == 0 ? a.scale0 : a.scale;
        const double A = av[j], B = bv[j];
        wr[j] = (T)(sc * (c * A + s * B));
        if (k != 0 && 2 * k != n) wi[j] = (T)(sc * (s * A - c * B));
    }
    *(V *)((T *)a.out + b * a.out_dist + k0) = wr;
    *(V *)((T *)a.out_im + b * a.out_dist + k0) = wi;
}

// ---- III-post: x[2i] = v[i] (i < e), x[2i+1] = +-v[N-1-i] (i < h; DST: negated) ----
template <typename T, bool DST, bool VEC>
__global__ void __launch_bounds__(256) dct3_post_kernel(DctArgs a) {
    using V = typename AnyVec<T>::type;
    constexpr int L = AnyVec<T>::N;
    const unsigned long long g = global_group(a);
    if (g >= a.groups) return;
    unsigned long long b;
    const unsigned long long i0 = split_group(g, a.gpt, &b) * L, n = a.n, e = (n + 1) / 2, h = n / 2;
    const T *v = (const T *)a.in + b * a.in_dist;
    T *x = (T *)a.out + b * a.out_dist;
    const V ev = *(const V *)(v + i0);
    T od[L];
#pragma unroll
    for (int j = 0; j < L; ++j) {
        const T o = i0 + j < h ? v[n - 1 - i0 - j] : T(0);
        od[j] = DST ? -o : o;
    }
    if (VEC && 2 * i0 + 2 * L <= n) {
        V v0, v1;
#pragma unroll
        for (int j = 0; j < L / 2; ++j) {
            v0[2 * j] = ev[j];
            v0[2 * j + 1] = od[j];
            v1[2 * j] = ev[L / 2 + j];
            v1[2 * j + 1] = od[L / 2 + j];
        }
        __builtin_nontemporal_store(v0, (V *)(x + 2 * i0));
        __builtin_nontemporal_store(v1, (V *)(x + 2 * i0 + L));
    } else {
#pragma unroll
        for (int j = 0; j < L; ++j) {
            const unsigned long long i = i0 + j;
            if (i < e) __builtin_nontemporal_store((T)ev[j], x + 2 * i);
            if (i < h) __builtin_nontemporal_store(od[j], x + 2 * i + 1);
        }
    }
}

template <typename T> hipError_t launch_dct(int kind, bool dst, bool vec, const DctArgs &a0, hipStream_t stream) {
    if (kind < kDct2Pre || kind > kDct3Post) return hipErrorInvalidValue;
    DctArgs a = a0;
    return launch_in_slices(a.groups, [&](dim3 grid, unsigned long long g0) {
        a.g0 = g0;
        const dim3 block(256);
#define PHAST_DCT_LAUNCH(KERNEL)                                                                                        \
    if (dst) {                                                                                                          \
        if (vec) hipLaunchKernelGGL((KERNEL<T, true, true>), grid, block, 0, stream, a);                                \
        else hipLaunchKernelGGL((KERNEL<T, true, false>), grid, block, 0, stream, a);                                   \
    } else {                                                                                                            \
        if (vec) hipLaunchKernelGGL((KERNEL<T, false, true>), grid, block, 0, stream, a);                               \
        else hipLaunchKernelGGL((KERNEL<T, false, false>), grid, block, 0, stream, a);                                  \
    }                                                                                                                   \
    break;
        switch (kind) {
        case kDct2Pre: PHAST_DCT_LAUNCH(dct2_pre_kernel)
        case kDct2Post: PHAST_DCT_LAUNCH(dct2_post_kernel)
        case kDct3Pre: PHAST_DCT_LAUNCH(dct3_pre_kernel)
        default: PHAST_DCT_LAUNCH(dct3_post_kernel)
        }
#undef PHAST_DCT_LAUNCH
    });
}

template hipError_t launch_dct<double>(int, bool, bool, const DctArgs &, hipStream_t);
template hipError_t launch_dct<float>(int, bool, bool, const DctArgs &, hipStream_t);

}  // namespace phast
