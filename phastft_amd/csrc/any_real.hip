// any_real.hip -- the streaming sweeps of the arbitrary-length real transforms (any_real.hpp has the algorithm).
//
// Built as any_len.hip is, on the device helpers of any_len.hpp: one group of 16 bytes per plane per thread, 256-thread
// workgroups in address order, launches split at 2^31 - 1 workgroups, non-temporal accesses on the caller's data, 16-byte
// accesses on the caller's side where bases and dist allow it and element accesses otherwise.  The workspace side is always
// 16-byte aligned (M is a power of two >= 8).
// The pairwise sweeps (untangle, preprocess) own a mirror pair (k, H - k) per point: the k side moves in groups, the H - k
// side (descending, usually unaligned) in elements.  Chirps (exact phase, any_len.hpp: chirp_r) and the twiddles
// W^k = exp(-2 pi i k / N) = sincospi(-2k / N) are evaluated on the fly in double, for f32 too: no N-point table.
#include "any_real.hpp"

namespace phast {

// W^k = exp(-2 pi i k / n), k < n (the quotient is one rounding from exact)
__device__ inline void real_twiddle(unsigned long long k, unsigned long long n, double *c, double *s) {
    sincospi(-(double)(2 * k) / (double)n, s, c);
}

// (re, im) * (c, s) in double, rounded to T into the two lanes
template <typename T> __device__ inline void cmul(double re, double im, double c, double s, T *o_re, T *o_im) {
    *o_re = (T)(re * c - im * s);
    *o_im = (T)(re * s + im * c);
}

// C2R preprocess of point k (the power-of-two path's formula, oracle pho_c2r_preprocess):
//     z~[k] = (A + conj B) / 2 + i conj(W^k) (A - conj B) / 2,   A = X[k], B = X[H - k]
__device__ inline void c2r_pre_point(double ar, double ai, double br, double bi, double c, double s, double *zr, double *zi) {
    const double xr = 0.5 * (ar + br), xi = 0.5 * (ai - bi);
    const double dr = ar - br, di = ai + bi;
    const double yr = 0.5 * (c * dr + s * di), yi = 0.5 * (c * di - s * dr);
    *zr = xr - yi;
    *zi = xi + yr;
}

// ---- R2C, even N: a[b M + k] = (x[2k] + i x[2k+1]) w_H[k] for k < H, 0 up to M ----
template <typename T, bool VEC>
__global__ void __launch_bounds__(256) any_r2c_pack_kernel(AnyRealArgs a) {
    using V = typename AnyVec<T>::type;
    constexpr int L = AnyVec<T>::N;
    const unsigned long long g = global_group(a);
    if (g >= a.groups) return;
    const unsigned log_gpt = a.log_m - (L == 2 ? 1 : 2);
    const unsigned long long b = g >> log_gpt, k0 = (g & ((1ull << log_gpt) - 1)) * L;
    const T *x = (const T *)a.in_re + b * a.in_dist + 2 * k0;
    T e[L], o[L];
    if (VEC && k0 + L <= a.l) {
        const V v0 = __builtin_nontemporal_load((const V *)x), v1 = __builtin_nontemporal_load((const V *)(x + L));
#pragma unroll
        for (int j = 0; j < L / 2; ++j) {
            e[j] = v0[2 * j];
            o[j] = v0[2 * j + 1];
            e[L / 2 + j] = v1[2 * j];
            o[L / 2 + j] = v1[2 * j + 1];
        }
    } else {
#pragma unroll
        for (int j = 0; j < L; ++j) {
            const bool in = k0 + j < a.l;
            e[j] = in ? __builtin_nontemporal_load(x + 2 * j) : T(0);
            o[j] = in ? __builtin_nontemporal_load(x + 2 * j + 1) : T(0);
        }
    }
    V vr, vi;
#pragma unroll
    for (int j = 0; j < L; ++j) {
        T orr = 0, oi = 0;
        if (k0 + j < a.l) {
            double c, s;
            chirp(k0 + j, a.l, &c, &s);
            cmul<T>((double)e[j], (double)o[j], c, s, &orr, &oi);
        }
        vr[j] = orr;
        vi[j] = oi;
    }
    const unsigned long long w = (b << a.log_m) + k0;
    *(V *)((T *)a.out_re + w) = vr;
    *(V *)((T *)a.out_im + w) = vi;
}

// ---- R2C, even N: Z = w_H c; one thread per pair (k, H - k), k <= H / 2:
//     X[k] = S + Q, X[H - k] = conj(S - Q),  S = (Z[k] + conj Z[H-k]) / 2,  Q = -i W^k (Z[k] - conj Z[H-k]) / 2
// X[0] = (Re Z[0] + Im Z[0], 0), X[H] = (Re Z[0] - Im Z[0], 0) exactly ----
template <typename T, bool VEC>
__global__ void __launch_bounds__(256) any_r2c_untangle_kernel(AnyRealArgs a) {
    using V = typename AnyVec<T>::type;
    constexpr int L = AnyVec<T>::N;
    const unsigned long long g = global_group(a);
    if (g >= a.groups) return;
    unsigned long long b;
    const unsigned long long k0 = split_group(g, a.gpt, &b) * L, h = a.l, q = h / 2;
    const T *cr = (const T *)a.in_re + (b << a.log_m), *ci = (const T *)a.in_im + (b << a.log_m);
    const V fr = *(const V *)(cr + k0), fi = *(const V *)(ci + k0);
    T *xr = (T *)a.out_re + b * a.out_dist, *xi = (T *)a.out_im + b * a.out_dist;
    V vr, vi;
#pragma unroll
    for (int j = 0; j < L; ++j) {
        const unsigned long long k = k0 + j;
        vr[j] = vi[j] = 0;
        if (k > q) continue;
        double c, s;
        chirp(k, h, &c, &s);
        const double zr = fr[j] * c - fi[j] * s, zi = fr[j] * s + fi[j] * c;
        if (k == 0) {
            vr[j] = (T)(zr + zi);
            __builtin_nontemporal_store((T)(zr - zi), xr + h);
            __builtin_nontemporal_store(T(0), xi + h);
            continue;
        }
        const unsigned long long mk = h - k;
        const double mr = cr[mk], mi = ci[mk];
        chirp(mk, h, &c, &s);
        const double yr = mr * c - mi * s, yi = mr * s + mi * c;
        const double sr = 0.5 * (zr + yr), si = 0.5 * (zi - yi);
        const double dr = zr - yr, di = zi + yi;
        real_twiddle(k, a.n, &c, &s);
        const double qr = 0.5 * (c * di + s * dr), qi = -0.5 * (c * dr - s * di);
        vr[j] = (T)(sr + qr);
        vi[j] = (T)(si + qi);
        if (mk != k) {
            __builtin_nontemporal_store((T)(sr - qr), xr + mk);
            __builtin_nontemporal_store((T)(qi - si), xi + mk);
        }
    }
    if (VEC && k0 + L - 1 <= q) {
        __builtin_nontemporal_store(vr, (V *)(xr + k0));
        __builtin_nontemporal_store(vi, (V *)(xi + k0));
    } else {
#pragma unroll
        for (int j = 0; j < L; ++j)
            if (k0 + j <= q) {
                __builtin_nontemporal_store(vr[j], xr + k0 + j);
                __builtin_nontemporal_store(vi[j], xi + k0 + j);
            }
    }
}

// ---- C2R, even N: z~ from the pair (X[k], X[H - k]) (c2r_pre_point), then the chirp-pad of the inverse by the swap trick:
// a[b M + k] = (Im z~[k] + i Re z~[k]) w_H[k] for k < H, 0 up to M.  One thread per pair, k <= H / 2; the points of
// H / 2 < k < H are written by their mirror's thread ----
template <typename T, bool VEC>
__global__ void __launch_bounds__(256) any_c2r_pre_kernel(AnyRealArgs a) {
    using V = typename AnyVec<T>::type;
    constexpr int L = AnyVec<T>::N;
    const unsigned long long g = global_group(a);
    if (g >= a.groups) return;
    const unsigned log_gpt = a.log_m - (L == 2 ? 1 : 2);
    const unsigned long long b = g >> log_gpt, k0 = (g & ((1ull << log_gpt) - 1)) * L, h = a.l, q = h / 2;
    const T *xr = (const T *)a.in_re + b * a.in_dist, *xi = (const T *)a.in_im + b * a.in_dist;
    T *wr = (T *)a.out_re + (b << a.log_m), *wi = (T *)a.out_im + (b << a.log_m);
    T fr[L], fi[L];
    if (VEC && k0 + L - 1 <= q) {
        const V r = __builtin_nontemporal_load((const V *)(xr + k0)), i = __builtin_nontemporal_load((const V *)(xi + k0));
#pragma unroll
        for (int j = 0; j < L; ++j) {
            fr[j] = r[j];
            fi[j] = i[j];
        }
    } else {
#pragma unroll
        for (int j = 0; j < L; ++j) {
            const bool in = k0 + j <= q;
            fr[j] = in ? __builtin_nontemporal_load(xr + k0 + j) : T(0);
            fi[j] = in ? __builtin_nontemporal_load(xi + k0 + j) : T(0);
        }
    }
    V vr, vi;
#pragma unroll
    for (int j = 0; j < L; ++j) {
        const unsigned long long k = k0 + j;
        vr[j] = vi[j] = 0;
        if (k > q) continue;  // k >= H: the zero pad; q < k < H: the mirror's thread
        const unsigned long long mk = h - k;
        const double ar = fr[j], ai = fi[j];
        const double br = __builtin_nontemporal_load(xr + mk), bi = __builtin_nontemporal_load(xi + mk);
        double c, s, zr, zi, wc, ws;
        real_twiddle(k, a.n, &c, &s);
        c2r_pre_point(ar, ai, br, bi, c, s, &zr, &zi);
        chirp(k, h, &wc, &ws);
        T orr, oi;
        cmul<T>(zi, zr, wc, ws, &orr, &oi);
        vr[j] = orr;
        vi[j] = oi;
        if (k != 0 && mk != k) {  // W^(H-k) = -conj(W^k)
            c2r_pre_point(br, bi, ar, ai, -c, s, &zr, &zi);
            chirp(mk, h, &wc, &ws);
            cmul<T>(zi, zr, wc, ws, &orr, &oi);
            wr[mk] = orr;
            wi[mk] = oi;
        }
    }
    if (k0 + L - 1 <= q || k0 >= h) {
        *(V *)(wr + k0) = vr;
        *(V *)(wi + k0) = vi;
    } else {
#pragma unroll
        for (int j = 0; j < L; ++j)
            if (k0 + j <= q || k0 + j >= h) {
                wr[k0 + j] = vr[j];
                wi[k0 + j] = vi[j];
            }
    }
}

// ---- C2R, even N: Y = w_H c * scale (the swap trick: z = Im Y + i Re Y), x[2k] = Im Y[k], x[2k+1] = Re Y[k], k < H ----
template <typename T, bool VEC>
__global__ void __launch_bounds__(256) any_c2r_interleave_kernel(AnyRealArgs a) {
    using V = typename AnyVec<T>::type;
    constexpr int L = AnyVec<T>::N;
    const unsigned long long g = global_group(a);
    if (g >= a.groups) return;
    unsigned long long b;
    const unsigned long long k0 = split_group(g, a.gpt, &b) * L;
    const unsigned long long w = (b << a.log_m) + k0;
    const V cr = *(const V *)((const T *)a.in_re + w), ci = *(const V *)((const T *)a.in_im + w);
    T e[L], o[L];
#pragma unroll
    for (int j = 0; j < L; ++j) {
        double c = 0, s = 0;
        if (k0 + j < a.l) chirp(k0 + j, a.l, &c, &s);
        cmul<T>((double)cr[j] * a.scale, (double)ci[j] * a.scale, c, s, &o[j], &e[j]);
    }
    T *x = (T *)a.out_re + b * a.out_dist + 2 * k0;
    if (VEC && k0 + L <= a.l) {
        V v0, v1;
#pragma unroll
        for (int j = 0; j < L / 2; ++j) {
            v0[2 * j] = e[j];
            v0[2 * j + 1] = o[j];
            v1[2 * j] = e[L / 2 + j];
            v1[2 * j + 1] = o[L / 2 + j];
        }
        __builtin_nontemporal_store(v0, (V *)x);
        __builtin_nontemporal_store(v1, (V *)(x + L));
    } else {
#pragma unroll
        for (int j = 0; j < L; ++j)
            if (k0 + j < a.l) {
                __builtin_nontemporal_store(e[j], x + 2 * j);
                __builtin_nontemporal_store(o[j], x + 2 * j + 1);
            }
    }
}

// ---- R2C, odd N: a[b M + k] = x[k] w_N[k] (k < N), 0 up to M ----
template <typename T, bool VEC>
__global__ void __launch_bounds__(256) any_r2c_odd_pad_kernel(AnyRealArgs a) {
    using V = typename AnyVec<T>::type;
    constexpr int L = AnyVec<T>::N;
    const unsigned long long g = global_group(a);
    if (g >= a.groups) return;
    const unsigned log_gpt = a.log_m - (L == 2 ? 1 : 2);
    const unsigned long long b = g >> log_gpt, k0 = (g & ((1ull << log_gpt) - 1)) * L;
    const T *x = (const T *)a.in_re + b * a.in_dist;
    T lx[L];
    if (VEC && k0 + L <= a.l) {
        const V v = __builtin_nontemporal_load((const V *)(x + k0));
#pragma unroll
        for (int j = 0; j < L; ++j) lx[j] = v[j];
    } else {
#pragma unroll
        for (int j = 0; j < L; ++j) lx[j] = k0 + j < a.l ? __builtin_nontemporal_load(x + k0 + j) : T(0);
    }
    V vr, vi;
#pragma unroll
    for (int j = 0; j < L; ++j) {
        double c = 0, s = 0;
        if (k0 + j < a.l) chirp(k0 + j, a.l, &c, &s);
        vr[j] = (T)(lx[j] * c);
        vi[j] = (T)(lx[j] * s);
    }
    const unsigned long long w = (b << a.log_m) + k0;
    *(V *)((T *)a.out_re + w) = vr;
    *(V *)((T *)a.out_im + w) = vi;
}

// ---- R2C, odd N: X[k] = w_N[k] c[k] for k <= (N - 1) / 2; Im X[0] = 0 exactly ----
template <typename T, bool VEC>
__global__ void __launch_bounds__(256) any_r2c_odd_post_kernel(AnyRealArgs a) {
    using V = typename AnyVec<T>::type;
    constexpr int L = AnyVec<T>::N;
    const unsigned long long g = global_group(a);
    if (g >= a.groups) return;
    unsigned long long b;
    const unsigned long long k0 = split_group(g, a.gpt, &b) * L, q = (a.l - 1) / 2;
    const unsigned long long w = (b << a.log_m) + k0;
    const V cr = *(const V *)((const T *)a.in_re + w), ci = *(const V *)((const T *)a.in_im + w);
    T *xr = (T *)a.out_re + b * a.out_dist, *xi = (T *)a.out_im + b * a.out_dist;
    V vr, vi;
#pragma unroll
    for (int j = 0; j < L; ++j) {
        double c = 0, s = 0;
        if (k0 + j <= q) chirp(k0 + j, a.l, &c, &s);
        T orr, oi;
        cmul<T>((double)cr[j], (double)ci[j], c, s, &orr, &oi);
        vr[j] = orr;
        vi[j] = k0 + j == 0 ? T(0) : oi;
    }
    if (VEC && k0 + L - 1 <= q) {
        __builtin_nontemporal_store(vr, (V *)(xr + k0));
        __builtin_nontemporal_store(vi, (V *)(xi + k0));
    } else {
#pragma unroll
        for (int j = 0; j < L; ++j)
            if (k0 + j <= q) {
                __builtin_nontemporal_store(vr[j], xr + k0 + j);
                __builtin_nontemporal_store(vi[j], xi + k0 + j);
            }
    }
}

// ---- C2R, odd N: the Hermitian extension Xh[k] = X[k] (k <= (N-1)/2, Im X[0] taken as 0), conj X[N - k] above, padded by
// the swap trick: a[b M + k] = (Im Xh[k] + i Re Xh[k]) w_N[k] (k < N), 0 up to M ----
template <typename T, bool VEC>
__global__ void __launch_bounds__(256) any_c2r_odd_pad_kernel(AnyRealArgs a) {
    using V = typename AnyVec<T>::type;
    constexpr int L = AnyVec<T>::N;
    const unsigned long long g = global_group(a);
    if (g >= a.groups) return;
    const unsigned log_gpt = a.log_m - (L == 2 ? 1 : 2);
    const unsigned long long b = g >> log_gpt, k0 = (g & ((1ull << log_gpt) - 1)) * L, n = a.l, q = (n - 1) / 2;
    const T *xr = (const T *)a.in_re + b * a.in_dist, *xi = (const T *)a.in_im + b * a.in_dist;
    T hr[L], hi[L];
    if (VEC && k0 + L - 1 <= q) {
        const V r = __builtin_nontemporal_load((const V *)(xr + k0)), i = __builtin_nontemporal_load((const V *)(xi + k0));
#pragma unroll
        for (int j = 0; j < L; ++j) {
            hr[j] = r[j];
            hi[j] = i[j];
        }
    } else {
#pragma unroll
        for (int j = 0; j < L; ++j) {
            const unsigned long long k = k0 + j;
            hr[j] = hi[j] = 0;
            if (k <= q) {
                hr[j] = __builtin_nontemporal_load(xr + k);
                hi[j] = __builtin_nontemporal_load(xi + k);
            } else if (k < n) {
                hr[j] = __builtin_nontemporal_load(xr + n - k);
                hi[j] = -__builtin_nontemporal_load(xi + n - k);
            }
        }
    }
    if (k0 == 0) hi[0] = 0;
    V vr, vi;
#pragma unroll
    for (int j = 0; j < L; ++j) {
        double c = 0, s = 0;
        if (k0 + j < n) chirp(k0 + j, n, &c, &s);
        T orr, oi;
        cmul<T>((double)hi[j], (double)hr[j], c, s, &orr, &oi);
        vr[j] = orr;
        vi[j] = oi;
    }
    const unsigned long long w = (b << a.log_m) + k0;
    *(V *)((T *)a.out_re + w) = vr;
    *(V *)((T *)a.out_im + w) = vi;
}

// ---- C2R, odd N: x[k] = Im(w_N[k] c[k]) * scale for k < N (the swap trick's real part) ----
template <typename T, bool VEC>
__global__ void __launch_bounds__(256) any_c2r_odd_post_kernel(AnyRealArgs a) {
    using V = typename AnyVec<T>::type;
    constexpr int L = AnyVec<T>::N;
    const unsigned long long g = global_group(a);
    if (g >= a.groups) return;
    unsigned long long b;
    const unsigned long long k0 = split_group(g, a.gpt, &b) * L;
    const unsigned long long w = (b << a.log_m) + k0;
    const V cr = *(const V *)((const T *)a.in_re + w), ci = *(const V *)((const T *)a.in_im + w);
    T *x = (T *)a.out_re + b * a.out_dist;
    V v;
#pragma unroll
    for (int j = 0; j < L; ++j) {
        double c = 0, s = 0;
        if (k0 + j < a.l) chirp(k0 + j, a.l, &c, &s);
        v[j] = (T)(((double)cr[j] * s + (double)ci[j] * c) * a.scale);
    }
    if (VEC && k0 + L <= a.l) {
        __builtin_nontemporal_store(v, (V *)(x + k0));
    } else {
#pragma unroll
        for (int j = 0; j < L; ++j)
            if (k0 + j < a.l) __builtin_nontemporal_store(v[j], x + k0 + j);
    }
}

// ---- N = 1, 2: X[0] = x0 (+ x1), X[1] = x0 - x1 (imaginary parts 0); C2R: irfft's x0 = Re X0 (N = 1), (Re X0 +- Re X1) / 2 ----
template <typename T>
__global__ void __launch_bounds__(256) any_real_tiny_kernel(AnyRealArgs a, int c2r) {
    const unsigned long long b = global_group(a);
    if (b >= a.groups) return;
    if (!c2r) {
        const T *x = (const T *)a.in_re + b * a.in_dist;
        T *xr = (T *)a.out_re + b * a.out_dist, *xi = (T *)a.out_im + b * a.out_dist;
        const T x0 = x[0];
        if (a.n == 1) {
            xr[0] = x0;
            xi[0] = 0;
        } else {
            const T x1 = x[1];
            xr[0] = x0 + x1;
            xr[1] = x0 - x1;
            xi[0] = xi[1] = 0;
        }
    } else {
        const T *xr = (const T *)a.in_re + b * a.in_dist;
        T *x = (T *)a.out_re + b * a.out_dist;
        if (a.n == 1) {
            x[0] = xr[0];
        } else {
            const double r0 = xr[0], r1 = xr[1];
            x[0] = (T)(0.5 * (r0 + r1));
            x[1] = (T)(0.5 * (r0 - r1));
        }
    }
}

template <typename T> hipError_t launch_any_real(int kind, bool vec, const AnyRealArgs &a0, hipStream_t stream) {
    if (kind < kR2cPack || kind > kC2rTiny) return hipErrorInvalidValue;
    AnyRealArgs a = a0;
    return launch_in_slices(a.groups, [&](dim3 grid, unsigned long long g0) {
        a.g0 = g0;
        const dim3 block(256);
#define PHAST_REAL_LAUNCH(KERNEL)                                                                                       \
    if (vec)                                                                                                            \
        hipLaunchKernelGGL((KERNEL<T, true>), grid, block, 0, stream, a);                                               \
    else                                                                                                                \
        hipLaunchKernelGGL((KERNEL<T, false>), grid, block, 0, stream, a);                                              \
    break;
        switch (kind) {
        case kR2cPack: PHAST_REAL_LAUNCH(any_r2c_pack_kernel)
        case kR2cUntangle: PHAST_REAL_LAUNCH(any_r2c_untangle_kernel)
        case kC2rPre: PHAST_REAL_LAUNCH(any_c2r_pre_kernel)
        case kC2rInterleave: PHAST_REAL_LAUNCH(any_c2r_interleave_kernel)
        case kR2cOddPad: PHAST_REAL_LAUNCH(any_r2c_odd_pad_kernel)
        case kR2cOddPost: PHAST_REAL_LAUNCH(any_r2c_odd_post_kernel)
        case kC2rOddPad: PHAST_REAL_LAUNCH(any_c2r_odd_pad_kernel)
        case kC2rOddPost: PHAST_REAL_LAUNCH(any_c2r_odd_post_kernel)
        default:  // kR2cTiny, kC2rTiny
            hipLaunchKernelGGL(any_real_tiny_kernel<T>, grid, block, 0, stream, a, kind == kC2rTiny ? 1 : 0);
            break;
        }
#undef PHAST_REAL_LAUNCH
    });
}

template hipError_t launch_any_real<double>(int, bool, const AnyRealArgs &, hipStream_t);
template hipError_t launch_any_real<float>(int, bool, const AnyRealArgs &, hipStream_t);

}  // namespace phast
