// mdct.hip -- the four streaming sweeps of the MDCT and its inverse (mdct.hpp has the schedule, dct4.hpp the DCT-IV).
//
// Built as dct.hip and stft.hip are: 256-thread workgroups in address order, launches split at 2^31 - 1 workgroups, a thread
// owns one group of V = 16 / sizeof(T) consecutive elements of each workspace plane (16-byte aligned: the planner pads every
// workspace row to a multiple of V) or of the caller's output (overlap-add: 16-byte stores where its address allows, elements
// otherwise).
//     pre    reads its sources strided by two in both directions (2m and N - 1 - 2m; the fold doubles that into four runs): lane
//            l of a wave owns m = base + V l .. + V - 1, so the element accesses of one wave cover one contiguous run per
//            direction, half of it used by this sweep's ascending threads and half by its descending ones.
//     post   pairs bin k with bin h - 1 - k, whose imaginary part lands beside k's real part: its own group of Z moves in
//            16-byte loads, the mirrored one in element loads of the workspace (one contiguous descending run per wave), and
//            the 2 V consecutive reals it owns leave in two 16-byte stores where the row's address allows.
// The signal is read twice (every sample lies in two frames) and the window once per frame: ordinary cached loads.  The
// caller's coefficients move non-temporally.  Both twiddle sets come from the planner's tables (no sine is evaluated here);
// the overlap-add is a gather of at most two frames: no atomics.
#include "mdct.hpp"

namespace phast {

// u[nn] of the fold of the frame that starts at sample s0 (mdct.hpp); x is zero outside [0, len).  INSIDE: the whole frame
// lies in [0, len)
template <typename T, bool INSIDE>
__device__ inline T mdct_fold_at(const T *x, const T *w, long long s0, long long len, unsigned long long nn, unsigned long long h) {
    int sg;
    const unsigned long long ia = mdct_fold_a(nn, h), ib = mdct_fold_b(nn, h, &sg);
    const long long sa = s0 + (long long)ia, sb = s0 + (long long)ib;
    const T xa = INSIDE || (sa >= 0 && sa < len) ? w[ia] * x[sa] : T(0);
    const T xb = INSIDE || (sb >= 0 && sb < len) ? w[ib] * x[sb] : T(0);
    return sg < 0 ? -xa - xb : xb - xa;
}

// ---- pre: z[m] = (u[2m] + i u[N-1-2m]) e^{-i pi (4m+1)/(4N)}, m < h; zeros in the row's padding.  SIGNAL: u is the fold of
// frame q0 + r of the caller's signals; else row r of the caller's coefficients ----
template <typename T, bool SIGNAL>
__global__ void __launch_bounds__(256) mdct_pre_kernel(MdctArgs a) {
    using V = typename AnyVec<T>::type;
    constexpr int L = AnyVec<T>::N;
    const unsigned long long g = global_group(a);
    if (g >= a.groups) return;
    unsigned long long r;
    const unsigned long long m0 = split_group(g, a.gpt, &r) * L, n = a.n, h = n / 2;
    const V tc = *(const V *)((const T *)a.tw_c + m0), ts = *(const V *)((const T *)a.tw_s + m0);  // (zeros beyond h)
    T re[L], im[L];
    if (SIGNAL) {
        unsigned long long b;
        const unsigned long long t = split_group(a.q0 + r, (unsigned)a.frames, &b);  // frames < 2^30
        const T *x = (const T *)a.in + b * a.in_dist, *w = (const T *)a.win;
        const long long s0 = ((long long)t - a.padded) * (long long)n, len = (long long)a.len;
        if (s0 >= 0 && s0 + 2 * (long long)n <= len) {  // an interior frame (all but the first and the last two): no bounds
#pragma unroll
            for (int j = 0; j < L; ++j) {
                const unsigned long long m = m0 + j;
                re[j] = m < h ? mdct_fold_at<T, true>(x, w, s0, len, dct4_re_src(m), h) : T(0);
                im[j] = m < h ? mdct_fold_at<T, true>(x, w, s0, len, dct4_im_src(m, n), h) : T(0);
            }
        } else {
#pragma unroll
            for (int j = 0; j < L; ++j) {
                const unsigned long long m = m0 + j;
                re[j] = m < h ? mdct_fold_at<T, false>(x, w, s0, len, dct4_re_src(m), h) : T(0);
                im[j] = m < h ? mdct_fold_at<T, false>(x, w, s0, len, dct4_im_src(m, n), h) : T(0);
            }
        }
    } else {
        const T *u = (const T *)a.in + r * a.in_dist;
#pragma unroll
        for (int j = 0; j < L; ++j) {
            const unsigned long long m = m0 + j;
            re[j] = m < h ? __builtin_nontemporal_load(u + dct4_re_src(m)) : T(0);
            im[j] = m < h ? __builtin_nontemporal_load(u + dct4_im_src(m, n)) : T(0);
        }
    }
    V zr, zi;
#pragma unroll
    for (int j = 0; j < L; ++j) {
        zr[j] = re[j] * tc[j] + im[j] * ts[j];
        zi[j] = im[j] * tc[j] - re[j] * ts[j];
    }
    *(V *)((T *)a.out + r * a.out_dist + m0) = zr;
    *(V *)((T *)a.out_im + r * a.out_dist + m0) = zi;
}

// ---- post: c = Z[k] e^{-i pi k/N}; y[2k] = s Re c[k], y[2k+1] = y[N-1-2(h-1-k)] = -s Im c[h-1-k], k < h: a thread reads its
// own group of Z ascending and the mirrored one descending, and stores 2 V consecutive reals.  NT: y is the caller's
// (forward), else v.  VEC: y's rows allow 16-byte stores ----
template <typename T, bool NT, bool VEC>
__global__ void __launch_bounds__(256) dct4_post_kernel(MdctArgs a) {
    using V = typename AnyVec<T>::type;
    constexpr int L = AnyVec<T>::N;
    const unsigned long long g = global_group(a);
    if (g >= a.groups) return;
    unsigned long long r;
    const unsigned long long k0 = split_group(g, a.gpt, &r) * L, n = a.n, h = n / 2;
    const T *zr = (const T *)a.in + r * a.in_dist, *zi = (const T *)a.in_im + r * a.in_dist;
    const T *c = (const T *)a.tw_c, *s = (const T *)a.tw_s;
    const V fr = *(const V *)(zr + k0), fi = *(const V *)(zi + k0), tc = *(const V *)(c + k0), ts = *(const V *)(s + k0);
    T *y = (T *)a.out + r * a.out_dist + 2 * k0;
    const T sc = (T)a.scale;
    T ev[L], od[L];
#pragma unroll
    for (int j = 0; j < L; ++j) {
        const unsigned long long k = k0 + j;
        ev[j] = od[j] = T(0);
        if (k >= h) continue;
        const unsigned long long m = h - 1 - k;  // the bin whose imaginary part lands beside bin k's real part
        const T mr = zr[m], mi = zi[m], mc = c[m], ms = s[m];
        ev[j] = sc * (fr[j] * tc[j] + fi[j] * ts[j]);
        od[j] = sc * (mr * ms - mi * mc);  // -s Im c[m]
    }
    if (VEC && k0 + L <= h) {
        V v0, v1;
#pragma unroll
        for (int j = 0; j < L / 2; ++j) {
            v0[2 * j] = ev[j];
            v0[2 * j + 1] = od[j];
            v1[2 * j] = ev[L / 2 + j];
            v1[2 * j + 1] = od[L / 2 + j];
        }
        if (NT) {
            __builtin_nontemporal_store(v0, (V *)y);
            __builtin_nontemporal_store(v1, (V *)(y + L));
        } else {
            *(V *)y = v0;
            *(V *)(y + L) = v1;
        }
    } else {
#pragma unroll
        for (int j = 0; j < L; ++j) {
            if (k0 + j >= h) continue;
            if (NT) {
                __builtin_nontemporal_store(ev[j], y + 2 * j);
                __builtin_nontemporal_store(od[j], y + 2 * j + 1);
            } else {
                y[2 * j] = ev[j];
                y[2 * j + 1] = od[j];
            }
        }
    }
}

// ---- overlap-add: sample s = q N + r lies in the second half of frame q - 1 + padded and in the first half of frame
// q + padded; out[s] = sum over those of them that exist, in ascending order, of w[n] (+-)v[unfold(n)]; 0 without a frame ----
template <typename T>
__global__ void __launch_bounds__(256) imdct_ola_kernel(MdctArgs a) {
    using V = typename AnyVec<T>::type;
    constexpr int L = AnyVec<T>::N;
    const unsigned long long g = global_group(a);
    if (g >= a.groups) return;
    unsigned long long b;
    const unsigned long long s0 = split_group(g, a.gpt, &b) * L, n = a.n, h = n / 2;
    const T *v = (const T *)a.in + b * a.frames * a.in_dist, *w = (const T *)a.win;
    T *out = (T *)a.out + b * a.out_dist;
    V o;
#pragma unroll
    for (int k = 0; k < L; ++k) {
        const unsigned long long s = s0 + k;
        T acc = T(0);
        if (s < a.len) {
            const unsigned q = (unsigned)s / (unsigned)n;  // s < L <= 2^29
            const unsigned long long r = s - (unsigned long long)q * n;
            const long long t1 = (long long)q + a.padded, t2 = t1 - 1;
            int sg;
            if (t2 >= 0 && t2 < (long long)a.frames) {
                const unsigned long long i = mdct_unfold(r + n, h, &sg);
                const T y = w[r + n] * v[(unsigned long long)t2 * a.in_dist + i];
                acc = sg < 0 ? -y : y;
            }
            if (t1 < (long long)a.frames) {
                const unsigned long long i = mdct_unfold(r, h, &sg);
                const T y = w[r] * v[(unsigned long long)t1 * a.in_dist + i];
                acc += sg < 0 ? -y : y;
            }
        }
        o[k] = acc;
    }
    if (s0 + L <= a.len && aligned16(out + s0)) {
        __builtin_nontemporal_store(o, (V *)(out + s0));
    } else {
#pragma unroll
        for (int k = 0; k < L; ++k)
            if (s0 + k < a.len) __builtin_nontemporal_store((T)o[k], out + s0 + k);
    }
}

template <typename T> hipError_t launch_mdct(int kind, bool to_caller, const MdctArgs &a0, hipStream_t stream) {
    if (kind < kMdctPre || kind > kMdctOla) return hipErrorInvalidValue;
    MdctArgs a = a0;
    return launch_in_slices(a.groups, [&](dim3 grid, unsigned long long g0) {
        a.g0 = g0;
        const dim3 block(256);
        switch (kind) {
        case kMdctPre: hipLaunchKernelGGL((mdct_pre_kernel<T, true>), grid, block, 0, stream, a); break;
        case kDct4Pre: hipLaunchKernelGGL((mdct_pre_kernel<T, false>), grid, block, 0, stream, a); break;
        case kDct4Post: {
            // the workspace's rows v always allow 16-byte stores; the caller's where the base and the row length do
            const bool vec = !to_caller || ((reinterpret_cast<unsigned long long>(a.out) & 15ull) == 0 && a.out_dist % (16 / sizeof(T)) == 0);
            if (to_caller && vec) hipLaunchKernelGGL((dct4_post_kernel<T, true, true>), grid, block, 0, stream, a);
            else if (to_caller) hipLaunchKernelGGL((dct4_post_kernel<T, true, false>), grid, block, 0, stream, a);
            else hipLaunchKernelGGL((dct4_post_kernel<T, false, true>), grid, block, 0, stream, a);
            break;
        }
        default: hipLaunchKernelGGL((imdct_ola_kernel<T>), grid, block, 0, stream, a);
        }
    });
}

template hipError_t launch_mdct<double>(int, bool, const MdctArgs &, hipStream_t);
template hipError_t launch_mdct<float>(int, bool, const MdctArgs &, hipStream_t);

}  // namespace phast
