// conv.hip -- the three streaming sweeps of overlap-save convolution (conv.hpp has the definitions).
//
// Built as stft.hip is: 256-thread workgroups in address order, launches split at 2^31 - 1 workgroups, a thread owns one group
// of V = 16 / sizeof(T) consecutive elements on the side it writes.  That side moves in aligned 16-byte accesses (the caller's
// output: where its address allows, elements otherwise).  The gathered side starts wherever the segment puts it, so it is
// read as one 16-byte load of element alignment (Unaligned<T>), with element loads only at the ends of a signal, of a row and
// of a segment's share of the output.  The caller's signal and output are accessed non-temporally: each is streamed once
// (the signal 1 + (K - 1) / S times), while the rows and the spectrum planes between the sweeps and the transforms are
// ordinary accesses that may stay in the caches.  No LDS, no atomics: an output sample has exactly one source.
#include "conv.hpp"

namespace phast {

// ---- segment: row r of the workspace = x~[t0 + s S - (K - 1) + j], j < B, of segment q0 + r; zeros in the padding up to fd ----
template <typename T>
__global__ void __launch_bounds__(256) conv_segment_kernel(ConvArgs a) {
    using V = typename AnyVec<T>::type;
    using VU = typename Unaligned<T>::type;
    constexpr int L = AnyVec<T>::N;
    const unsigned long long g = global_group(a);
    if (g >= a.groups) return;
    unsigned long long r;
    const unsigned long long j0 = split_group(g, a.gpt, &r) * L;
    unsigned long long b;
    const unsigned long long s = split_group(a.q0 + r, (unsigned)a.segs, &b);  // segs <= 2^30
    const T *x = (const T *)a.in + b * a.sig_dist;
    const long long len = (long long)a.len, i0 = (long long)(a.t0 + s * a.s + j0) - (long long)(a.k - 1);
    V v;
    if (i0 >= 0 && i0 + L <= len && j0 + L <= a.b) {  // an interior group: no zero fill, no bounds
        const VU u = __builtin_nontemporal_load((const VU *)(x + i0));
#pragma unroll
        for (int j = 0; j < L; ++j) v[j] = u[j];
    } else {
#pragma unroll
        for (int j = 0; j < L; ++j) {
            const long long i = i0 + j;
            v[j] = (j0 + j < a.b && i >= 0 && i < len) ? __builtin_nontemporal_load(x + i) : T(0);
        }
    }
    *(V *)((T *)a.out + r * a.fd + j0) = v;
}

// ---- spectrum: (re, im)[r][j] *= H^[j] in place, j < bd (H^ is zero beyond the bins) ----
template <typename T>
__global__ void __launch_bounds__(256) conv_spectrum_kernel(ConvArgs a) {
    using V = typename AnyVec<T>::type;
    constexpr int L = AnyVec<T>::N;
    const unsigned long long g = global_group(a);
    if (g >= a.groups) return;
    unsigned long long r;
    const unsigned long long j0 = split_group(g, a.gpt, &r) * L;
    V *pr = (V *)((T *)a.re + r * a.bd + j0), *pi = (V *)((T *)a.im + r * a.bd + j0);
    const V hr = *(const V *)((const T *)a.h_re + j0), hi = *(const V *)((const T *)a.h_im + j0);
    const V xr = *pr, xi = *pi;
    V yr, yi;
#pragma unroll
    for (int j = 0; j < L; ++j) {
        yr[j] = xr[j] * hr[j] - xi[j] * hi[j];
        yi[j] = xr[j] * hi[j] + xi[j] * hr[j];
    }
    *pr = yr;
    *pi = yi;
}

// ---- save: out[i] = y[s][K - 1 + i - s S], s = i / S, for the samples whose segment is in this chunk ----
template <typename T>
__global__ void __launch_bounds__(256) conv_save_kernel(ConvArgs a) {
    using V = typename AnyVec<T>::type;
    using VU = typename Unaligned<T>::type;
    constexpr int L = AnyVec<T>::N;
    const unsigned long long g = global_group(a);
    if (g >= a.groups) return;
    unsigned long long b;
    const unsigned i0 = (unsigned)split_group(a.first + g, a.gpt, &b) * L;  // out_len <= 2^29: 32-bit divisions below
    const unsigned hop = (unsigned)a.s, n_out = (unsigned)a.out_len;
    const unsigned n_in = n_out - i0 < (unsigned)L ? n_out - i0 : (unsigned)L;
    const unsigned s_a = i0 / hop, s_b = (i0 + n_in - 1) / hop;
    const unsigned long long qb = b * a.segs, q_a = qb + s_a;
    const T *y = (const T *)a.in + (a.k - 1);
    T *out = (T *)a.out + b * a.out_dist + i0;
    if (n_in == (unsigned)L && s_a == s_b && q_a >= a.q0 && q_a < a.q1 && aligned16(out)) {
        // the whole group in one segment of the chunk: its samples end at or before the row's element B - 1
        const VU u = *(const VU *)(y + (q_a - a.q0) * a.fd + (i0 - s_a * hop));
        V v;
#pragma unroll
        for (int k = 0; k < L; ++k) v[k] = u[k];
        __builtin_nontemporal_store(v, (V *)out);
        return;
    }
    unsigned s = s_a, off = i0 - s_a * hop;
#pragma unroll
    for (int k = 0; k < L; ++k) {
        if ((unsigned)k < n_in) {
            const unsigned long long q = qb + s;
            if (q >= a.q0 && q < a.q1) __builtin_nontemporal_store(y[(q - a.q0) * a.fd + off], out + k);
        }
        if (++off == hop) {
            off = 0;
            ++s;
        }
    }
}

template <typename T> hipError_t launch_conv(int kind, const ConvArgs &a0, hipStream_t stream) {
    if (kind != kConvSegment && kind != kConvSpectrum && kind != kConvSave) return hipErrorInvalidValue;
    ConvArgs a = a0;
    return launch_in_slices(a.groups, [&](dim3 grid, unsigned long long g0) {
        a.g0 = g0;
        const dim3 block(256);
        if (kind == kConvSegment) hipLaunchKernelGGL((conv_segment_kernel<T>), grid, block, 0, stream, a);
        else if (kind == kConvSpectrum) hipLaunchKernelGGL((conv_spectrum_kernel<T>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((conv_save_kernel<T>), grid, block, 0, stream, a);
    });
}

template hipError_t launch_conv<double>(int, const ConvArgs &, hipStream_t);
template hipError_t launch_conv<float>(int, const ConvArgs &, hipStream_t);

}  // namespace phast
