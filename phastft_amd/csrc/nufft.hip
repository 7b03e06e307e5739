// nufft.hip -- the four kernels of the non-uniform FFT (nufft.hpp has the algorithm).
//
// spread and interpolate are data-dependent gathers over the point set sorted by grid cell: one thread per grid point
// (spread) or per sorted point (interpolate) and transform, element accesses, every sum in registers in a fixed order and
// ONE store per output -- no atomics, so the bits depend on nothing but the points and the data.  Neighbouring threads walk
// overlapping runs of the sorted tables (spread) or read neighbouring grid cells (interpolate, in sorted order), which is what
// the caches are for; the caller's planes are reached through `perm`.  phi is evaluated in double for f64 and in float for
// f32, from an argument formed in double.
//
// pre and deconvolve are streaming sweeps built like any_len.hip: one group of 16 bytes per plane per thread, 256-thread
// workgroups in address order, launch_in_slices, and an element-access variant for planes (or a workspace) that do not allow
// 16-byte accesses.
#include "nufft.hpp"

namespace phast {

// g[b n_g + l] = sum_j phi(2 (l - n_g x_j) / w) c[b in_dist + j] over the points of the cells l - h .. l + h - 1 (mod n_g),
// h = ceil(w / 2), in cell order and sorted order.  REAL: no imaginary plane
template <typename T, bool REAL>
__global__ void __launch_bounds__(256) nufft_spread_kernel(NufftArgs a) {
    using R = typename NufftReal<T>::type;
    const unsigned long long g = global_group(a);
    if (g >= a.groups) return;
    const unsigned long long grid = 1ull << a.log_g, mask = grid - 1;
    const unsigned long long b = g >> a.log_g, l = g & mask;
    const T *cr = (const T *)a.in_re + b * a.in_dist;
    const T *ci = REAL ? nullptr : (const T *)a.in_im + b * a.in_dist;
    const long long h = (a.w + 1) / 2;
    const double dgrid = (double)grid, two_over_w = 2.0 / a.w;
    const R beta = (R)nufft_beta(a.w);
    const unsigned long long lo = (l - (unsigned long long)h) & mask;  // the first cell; 2h <= n_g cells from there
    // the sorted range of those cells: one run, or two where the cells wrap past the end of the grid
    const unsigned long long end = lo + 2 * (unsigned long long)h;
    const bool wraps = end > grid;
    uint32_t i0 = a.cell_start[lo], i1 = a.cell_start[wraps ? grid : end];
    R sr = 0, si = 0;
    for (int run = 0; run < (wraps ? 2 : 1); ++run) {
        for (uint32_t i = i0; i < i1; ++i) {
            double t;
            const long long q = nufft_cell(a.xs[i], dgrid, &t);
            const R k = nufft_weight<R>(nufft_ring(l, q, mask), t, two_over_w, beta);
            const uint32_t j = a.perm[i];
            sr += k * (R)cr[j];
            if (!REAL) si += k * (R)ci[j];
        }
        if (wraps) {
            i0 = 0;
            i1 = a.cell_start[end - grid];
        }
    }
    ((T *)a.out_re)[g] = (T)sr;
    ((T *)a.out_im)[g] = (T)si;
}

// c[b out_dist + perm[i]] = sum over the w grid points l under sorted point i of phi(2 (l - n_g x_i) / w) g[b n_g + l mod n_g]
template <typename T>
__global__ void __launch_bounds__(256) nufft_interp_kernel(NufftArgs a) {
    using R = typename NufftReal<T>::type;
    const unsigned long long g = global_group(a);
    if (g >= a.groups) return;
    unsigned long long b = g / a.m;
    const unsigned long long i = g - b * a.m;
    const unsigned long long mask = (1ull << a.log_g) - 1;
    const T *gr = (const T *)a.in_re + (b << a.log_g), *gi = (const T *)a.in_im + (b << a.log_g);
    const double two_over_w = 2.0 / a.w;
    const R beta = (R)nufft_beta(a.w);
    double t;
    const long long q = nufft_cell(a.xs[i], (double)(mask + 1), &t);
    const long long first = nufft_first(a.w, t);
    R sr = 0, si = 0;
    for (int s = 0; s < a.w; ++s) {
        const long long dq = first + s;
        const unsigned long long l = (unsigned long long)(q + dq) & mask;
        const R k = nufft_weight<R>(dq, t, two_over_w, beta);
        sr += k * (R)gr[l];
        si += k * (R)gi[l];
    }
    const unsigned long long o = b * a.out_dist + a.perm[i];
    ((T *)a.out_re)[o] = (T)sr;
    ((T *)a.out_im)[o] = (T)si;
}

// g^[b n_g + slot(m)] = F[b in_dist + m] / phi^(k(m)) for m < N, exact zeros in every other slot.  REAL: no imaginary plane
template <typename T, bool VEC, bool REAL>
__global__ void __launch_bounds__(256) nufft_pre_kernel(NufftArgs a) {
    using V = typename AnyVec<T>::type;
    constexpr int W = AnyVec<T>::N;
    const unsigned long long g = global_group(a);
    if (g >= a.groups) return;
    const unsigned long long grid = 1ull << a.log_g;
    const unsigned log_gpt = a.log_g - (W == 2 ? 1 : 2);
    const unsigned long long b = g >> log_gpt, s0 = (g & ((1ull << log_gpt) - 1)) * W;
    const unsigned long long pos = (a.n + 1) / 2, neg = grid - (a.n - pos);  // slots [0, pos) and [neg, n_g) hold modes
    const T *fr = (const T *)a.in_re + b * a.in_dist;
    const T *fi = REAL ? nullptr : (const T *)a.in_im + b * a.in_dist;
    const T *p = (const T *)a.inv_hat;
    T orr[W], oi[W];
    // the mode of slot s0 where the whole group lies in one of the two runs of modes
    const bool low = s0 + W <= pos, high = s0 >= neg;
    const unsigned long long m0 = low ? s0 : s0 - (grid - a.n);
    if (VEC && (low || high) && m0 % W == 0) {
        const V vr = __builtin_nontemporal_load((const V *)(fr + m0));
        const V vp = *(const V *)(p + m0);
        V vi = vr;
        if (!REAL) vi = __builtin_nontemporal_load((const V *)(fi + m0));
#pragma unroll
        for (int j = 0; j < W; ++j) {
            orr[j] = vr[j] * vp[j];
            oi[j] = REAL ? T(0) : vi[j] * vp[j];
        }
    } else {
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const unsigned long long s = s0 + j;
            const bool in = s < pos || s >= neg;
            const unsigned long long m = s < pos ? s : s - (grid - a.n);
            const T pm = in ? p[m] : T(0);
            orr[j] = in ? __builtin_nontemporal_load(fr + m) * pm : T(0);
            oi[j] = in && !REAL ? __builtin_nontemporal_load(fi + m) * pm : T(0);
        }
    }
    T *wr = (T *)a.out_re + (b << a.log_g) + s0, *wi = (T *)a.out_im + (b << a.log_g) + s0;
    if (VEC) {
        V vr, vi;
#pragma unroll
        for (int j = 0; j < W; ++j) {
            vr[j] = orr[j];
            vi[j] = oi[j];
        }
        *(V *)wr = vr;
        *(V *)wi = vi;
    } else {
#pragma unroll
        for (int j = 0; j < W; ++j) {
            wr[j] = orr[j];
            wi[j] = oi[j];
        }
    }
}

// F[b out_dist + m] = g^[b n_g + slot(m)] / phi^(k(m)) for m < N
template <typename T, bool VEC>
__global__ void __launch_bounds__(256) nufft_deconv_kernel(NufftArgs a) {
    using V = typename AnyVec<T>::type;
    constexpr int W = AnyVec<T>::N;
    const unsigned long long g = global_group(a);
    if (g >= a.groups) return;
    unsigned long long b;
    const unsigned long long m0 = split_group(g, a.gpt, &b) * W;
    const unsigned long long grid = 1ull << a.log_g, pos = (a.n + 1) / 2;
    const T *gr = (const T *)a.in_re + (b << a.log_g), *gi = (const T *)a.in_im + (b << a.log_g);
    const T *p = (const T *)a.inv_hat;
    T *fr = (T *)a.out_re + b * a.out_dist, *fi = (T *)a.out_im + b * a.out_dist;
    // the whole group in one run of modes and inside N: its slots are consecutive
    const bool low = m0 + W <= pos, high = m0 >= pos && m0 + W <= a.n;
    const unsigned long long s0 = nufft_slot(m0, a.n, grid);
    if (VEC && (low || high) && s0 % W == 0) {
        const V vp = *(const V *)(p + m0);
        const V vr = *(const V *)(gr + s0) * vp, vi = *(const V *)(gi + s0) * vp;
        __builtin_nontemporal_store(vr, (V *)(fr + m0));
        __builtin_nontemporal_store(vi, (V *)(fi + m0));
    } else {
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const unsigned long long m = m0 + j;
            if (m < a.n) {
                const unsigned long long s = nufft_slot(m, a.n, grid);
                const T pm = p[m];
                __builtin_nontemporal_store(gr[s] * pm, fr + m);
                __builtin_nontemporal_store(gi[s] * pm, fi + m);
            }
        }
    }
}

template <typename T> hipError_t launch_nufft(int kind, bool vec, const NufftArgs &a0, hipStream_t stream) {
    NufftArgs a = a0;
    const bool real = a.in_im == nullptr;
    return launch_in_slices(a.groups, [&](dim3 grid, unsigned long long g0) {
        a.g0 = g0;
        if (kind == 0 && real)
            hipLaunchKernelGGL((nufft_spread_kernel<T, true>), grid, dim3(256), 0, stream, a);
        else if (kind == 0)
            hipLaunchKernelGGL((nufft_spread_kernel<T, false>), grid, dim3(256), 0, stream, a);
        else if (kind == 1)
            hipLaunchKernelGGL(nufft_interp_kernel<T>, grid, dim3(256), 0, stream, a);
        else if (kind == 2 && vec && real)
            hipLaunchKernelGGL((nufft_pre_kernel<T, true, true>), grid, dim3(256), 0, stream, a);
        else if (kind == 2 && vec)
            hipLaunchKernelGGL((nufft_pre_kernel<T, true, false>), grid, dim3(256), 0, stream, a);
        else if (kind == 2 && real)
            hipLaunchKernelGGL((nufft_pre_kernel<T, false, true>), grid, dim3(256), 0, stream, a);
        else if (kind == 2)
            hipLaunchKernelGGL((nufft_pre_kernel<T, false, false>), grid, dim3(256), 0, stream, a);
        else if (vec)
            hipLaunchKernelGGL((nufft_deconv_kernel<T, true>), grid, dim3(256), 0, stream, a);
        else
            hipLaunchKernelGGL((nufft_deconv_kernel<T, false>), grid, dim3(256), 0, stream, a);
    });
}

template hipError_t launch_nufft<double>(int, bool, const NufftArgs &, hipStream_t);
template hipError_t launch_nufft<float>(int, bool, const NufftArgs &, hipStream_t);

}  // namespace phast
