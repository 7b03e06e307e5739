// stft.hip -- the two streaming sweeps of the short-time Fourier transform (stft.hpp has the definitions).
//
// Built as dct.hip is: 256-thread workgroups in address order, launches split at 2^31 - 1 workgroups, a thread owns one group
// of V = 16 / sizeof(T) consecutive elements on the side it writes.  That side moves in aligned 16-byte accesses (the caller's
// output: where its address allows, elements otherwise).  The gathered side starts wherever f H - p puts it, so it is read as
// one 16-byte load of element alignment (Unaligned<T>: gfx950 takes a dword-aligned global_load_dwordx4), with element loads
// only at the ends of the signal and of a frame.
// The frame sweep reads a sample of the signal F / H times: those are ordinary cached loads.  (Dealing its workgroups to the
// XCDs in contiguous runs of rows, so that the re-reads of a sample meet in one L2, and non-temporal stores of the rows were
// measured: neither moved it)  The overlap-add sweep is a gather: a thread walks the frames that hold its samples in ascending order, so no atomics
// and no dependence on the batch or the chunk; the caller's output is stored non-temporally.
#include "stft.hpp"

namespace phast {

// ---- frame: row q0 + r of the workspace = w[j] x~[f H - p + j], j < F; zeros in the row's padding up to fd ----
template <typename T>
__global__ void __launch_bounds__(256) stft_frame_kernel(StftArgs a) {
    using V = typename AnyVec<T>::type;
    using VU = typename Unaligned<T>::type;
    constexpr int L = AnyVec<T>::N;
    const unsigned long long g = global_group(a);
    if (g >= a.groups) return;
    unsigned long long r;
    const unsigned long long j0 = split_group(g, a.gpt, &r) * L;
    unsigned long long b;
    const unsigned long long f = split_group(a.q0 + r, (unsigned)a.frames, &b);  // frames <= 2^30
    const T *x = (const T *)a.in + b * a.sig_dist;
    const V w = *(const V *)((const T *)a.win + j0);  // zeros beyond F
    const long long len = (long long)a.len, i0 = (long long)(f * a.h + j0) - (long long)a.p;
    V v;
    if (i0 >= 0 && i0 + L <= len) {  // an interior group: no padding, no bounds
        const VU u = *(const VU *)(x + i0);
#pragma unroll
        for (int j = 0; j < L; ++j) v[j] = u[j];
    } else {
#pragma unroll
        for (int j = 0; j < L; ++j) {
            const long long i = i0 + j;
            T s = T(0);
            if (j0 + j < a.f) {  // (the padding of the row reads nothing)
                if (i >= 0 && i < len) s = x[i];
                else if (a.pad == kStftReflect) s = x[stft_reflect(i, len)];
            }
            v[j] = s;
        }
    }
#pragma unroll
    for (int j = 0; j < L; ++j) v[j] *= w[j];
    *(V *)((T *)a.out + r * a.fd + j0) = v;
}

// ---- overlap-add: out[t] = sum_f w[u - f H] y[f][u - f H] / sum_f w^2[u - f H], u = t + p, ascending f; 0 without a frame ----
template <typename T>
__global__ void __launch_bounds__(256) stft_ola_kernel(StftArgs a) {
    using V = typename AnyVec<T>::type;
    using VU = typename Unaligned<T>::type;
    constexpr int L = AnyVec<T>::N;
    const unsigned long long g = global_group(a);
    if (g >= a.groups) return;
    unsigned long long b;
    const unsigned long long t0 = split_group(g, a.gpt, &b) * L, u0 = t0 + a.p;
    const T *y = (const T *)a.in + b * a.frames * a.fd, *win = (const T *)a.win;
    T *out = (T *)a.out + b * a.sig_dist;
    long long lo, hi, unused;
    stft_taps(u0, a.f, a.h, a.frames, &lo, &unused);      // the first frame of the group's first sample ...
    stft_taps(u0 + L - 1, a.f, a.h, a.frames, &unused, &hi);  // ... to the last frame of its last
    V num, den;
#pragma unroll
    for (int k = 0; k < L; ++k) num[k] = den[k] = T(0);
    const long long flen = (long long)a.f;
    for (long long f = lo; f <= hi; ++f) {
        const long long j0 = (long long)u0 - f * (long long)a.h;  // > -L and < F by the range of f
        const T *row = y + (unsigned long long)f * a.fd;
        V yv, wv;
        if (j0 >= 0 && j0 + L <= flen) {
            const VU yu = *(const VU *)(row + j0), wu = *(const VU *)(win + j0);
#pragma unroll
            for (int k = 0; k < L; ++k) {
                yv[k] = yu[k];
                wv[k] = wu[k];
            }
        } else {
#pragma unroll
            for (int k = 0; k < L; ++k) {
                const long long j = j0 + k;
                const bool in = j >= 0 && j < flen;
                yv[k] = in ? row[j] : T(0);
                wv[k] = in ? win[j] : T(0);  // a sample this frame does not hold adds exact zeros
            }
        }
#pragma unroll
        for (int k = 0; k < L; ++k) {
            num[k] += wv[k] * yv[k];
            den[k] += wv[k] * wv[k];
        }
    }
    V o;
#pragma unroll
    for (int k = 0; k < L; ++k) {
        long long l1, h1;
        stft_taps(u0 + k, a.f, a.h, a.frames, &l1, &h1);
        o[k] = l1 <= h1 ? num[k] / den[k] : T(0);
    }
    if (t0 + L <= a.len && aligned16(out + t0)) {
        __builtin_nontemporal_store(o, (V *)(out + t0));
    } else {
#pragma unroll
        for (int k = 0; k < L; ++k)
            if (t0 + k < a.len) __builtin_nontemporal_store((T)o[k], out + t0 + k);
    }
}

template <typename T> hipError_t launch_stft(int kind, const StftArgs &a0, hipStream_t stream) {
    if (kind != kStftFrame && kind != kStftOla) return hipErrorInvalidValue;
    StftArgs a = a0;
    return launch_in_slices(a.groups, [&](dim3 grid, unsigned long long g0) {
        a.g0 = g0;
        const dim3 block(256);
        if (kind == kStftFrame) hipLaunchKernelGGL((stft_frame_kernel<T>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((stft_ola_kernel<T>), grid, block, 0, stream, a);
    });
}

template hipError_t launch_stft<double>(int, const StftArgs &, hipStream_t);
template hipError_t launch_stft<float>(int, const StftArgs &, hipStream_t);

}  // namespace phast
