// nufft2d.hip -- the four kernels of the two-dimensional non-uniform FFT (nufft2d.hpp has the algorithm).
//
// spread and interpolate are data-dependent gathers over the point set sorted by the combined grid cell q1 g2 + q2: one thread
// per fine-grid point (spread; l2 fastest across threads) or per sorted point (interpolate) and transform, element accesses,
// every sum in registers in a fixed order and ONE store per output -- no atomics, no LDS, so the bits depend on nothing but the
// points and the data.  Every kernel value is the product nufft_weight(dq1, t1) * nufft_weight(dq2, t2) in R (double for f64,
// float for f32), formed the same way in both kernels: type 2 Reverse is the adjoint of type 1 Forward to rounding.
//
// pre and deconvolve are streaming sweeps built like nufft.hip's, along axis 2: one group of 16 bytes per plane per thread,
// 256-thread workgroups in address order, launch_in_slices, and an element-access variant for planes (or a workspace) that do
// not allow 16-byte accesses, for rows of the caller's planes that do not start on a 16-byte boundary (N2 no multiple of the
// group) and for groups that straddle the positive / negative run of modes.
#include "nufft2d.hpp"

namespace phast {

template <typename T> struct Nufft2dReal { typedef double type; };
template <> struct Nufft2dReal<float> { typedef float type; };

// the signed distance l - q of two cells around a ring of mask + 1 cells, in [-(mask + 1) / 2, (mask + 1) / 2)
__device__ inline long long nufft2d_ring(unsigned long long l, long long q, unsigned long long mask) {
    const long long half = (long long)((mask + 1) >> 1);
    return (long long)(((unsigned long long)((long long)l - q + half)) & mask) - half;
}

// g[b G + l1 g2 + l2] = sum_j phi1 phi2 c[b in_dist + j] over the points of the cells (l1 - h .. l1 + h - 1) x (l2 - h .. l2 + h - 1)
// (mod g1, g2), h = ceil(w / 2): cell row by cell row in that order, each row's cells one run of the sorted tables (two where
// the columns wrap past the end of the grid: the cells up to the end first), in sorted order.  REAL: no imaginary plane
template <typename T, bool REAL>
__global__ void __launch_bounds__(256) nufft2d_spread_kernel(Nufft2dArgs a) {
    using R = typename Nufft2dReal<T>::type;
    const unsigned long long g = global_group(a);
    if (g >= a.groups) return;
    const unsigned log_g = a.log_g1 + a.log_g2;
    const unsigned long long g1 = 1ull << a.log_g1, g2 = 1ull << a.log_g2, mask1 = g1 - 1, mask2 = g2 - 1;
    const unsigned long long b = g >> log_g, l = g & ((1ull << log_g) - 1), l1 = l >> a.log_g2, l2 = l & mask2;
    const T *cr = (const T *)a.in_re + b * a.in_dist;
    const T *ci = REAL ? nullptr : (const T *)a.in_im + b * a.in_dist;
    const unsigned long long h = (unsigned long long)((a.w + 1) / 2);
    const double dg1 = (double)g1, dg2 = (double)g2, two_over_w = 2.0 / a.w;
    const R beta = (R)nufft_beta(a.w);
    const unsigned long long lo2 = (l2 - h) & mask2, end2 = lo2 + 2 * h;  // 2h <= g2 columns from lo2
    const bool wraps = end2 > g2;
    R sr = 0, si = 0;
    for (unsigned long long rr = 0; rr < 2 * h; ++rr) {  // 2h <= g1 distinct cell rows
        const uint32_t *row = a.cell_start + (((l1 - h + rr) & mask1) << a.log_g2);
        uint32_t i0 = row[lo2], i1 = row[wraps ? g2 : end2];
        for (int run = 0; run < (wraps ? 2 : 1); ++run) {
            for (uint32_t i = i0; i < i1; ++i) {
                double t1, t2;
                const long long q1 = nufft_cell(a.xs[i], dg1, &t1), q2 = nufft_cell(a.ys[i], dg2, &t2);
                const R k = nufft_weight<R>(nufft2d_ring(l1, q1, mask1), t1, two_over_w, beta) *
                            nufft_weight<R>(nufft2d_ring(l2, q2, mask2), t2, two_over_w, beta);
                const uint32_t j = a.perm[i];
                sr += k * (R)cr[j];
                if (!REAL) si += k * (R)ci[j];
            }
            if (wraps) {
                i0 = row[0];
                i1 = row[end2 - g2];
            }
        }
    }
    ((T *)a.out_re)[g] = (T)sr;
    ((T *)a.out_im)[g] = (T)si;
}

// c[b out_dist + perm[i]] = sum over the w x w grid points under sorted point i of phi1 phi2 g[b G + l1 g2 + l2]: rows
// (q1 + first1 + s) mod g1, s outer, columns (q2 + first2 + u) mod g2, u inner.  The w axis-2 kernel values are formed once, into
// registers: the loops over u are unrolled to kNufftMaxWidth with static indices and a `u < w` guard (an array indexed at run
// time would live in scratch memory)
template <typename T>
__global__ void __launch_bounds__(256) nufft2d_interp_kernel(Nufft2dArgs a) {
    using R = typename Nufft2dReal<T>::type;
    const unsigned long long g = global_group(a);
    if (g >= a.groups) return;
    const unsigned long long b = g / a.m, i = g - b * a.m;
    const unsigned log_g = a.log_g1 + a.log_g2;
    const unsigned long long mask1 = (1ull << a.log_g1) - 1, mask2 = (1ull << a.log_g2) - 1;
    const T *gr = (const T *)a.in_re + (b << log_g), *gi = (const T *)a.in_im + (b << log_g);
    const double two_over_w = 2.0 / a.w;
    const R beta = (R)nufft_beta(a.w);
    double t1, t2;
    const long long q1 = nufft_cell(a.xs[i], (double)(mask1 + 1), &t1), q2 = nufft_cell(a.ys[i], (double)(mask2 + 1), &t2);
    const long long first1 = nufft_first(a.w, t1), first2 = nufft_first(a.w, t2);
    R k2[kNufftMaxWidth];
#pragma unroll
    for (int u = 0; u < kNufftMaxWidth; ++u) k2[u] = u < a.w ? nufft_weight<R>(first2 + u, t2, two_over_w, beta) : R(0);
    R sr = 0, si = 0;
    for (int s = 0; s < a.w; ++s) {
        const long long dq1 = first1 + s;
        const R k1 = nufft_weight<R>(dq1, t1, two_over_w, beta);
        const unsigned long long row = ((unsigned long long)(q1 + dq1) & mask1) << a.log_g2;
#pragma unroll
        for (int u = 0; u < kNufftMaxWidth; ++u) {
            if (u < a.w) {
                const unsigned long long l = row + ((unsigned long long)(q2 + first2 + u) & mask2);
                const R k = k1 * k2[u];
                sr += k * (R)gr[l];
                si += k * (R)gi[l];
            }
        }
    }
    const unsigned long long o = b * a.out_dist + a.perm[i];
    ((T *)a.out_re)[o] = (T)sr;
    ((T *)a.out_im)[o] = (T)si;
}

// g^[b G + slot1(m1) g2 + slot2(m2)] = F[b in_dist + m1 N2 + m2] inv1[m1] inv2[m2], exact zeros in every other slot of the
// whole grid.  REAL: no imaginary plane
template <typename T, bool VEC, bool REAL>
__global__ void __launch_bounds__(256) nufft2d_pre_kernel(Nufft2dArgs a) {
    using V = typename AnyVec<T>::type;
    constexpr int W = AnyVec<T>::N;
    constexpr unsigned LW = W == 2 ? 1 : 2;
    const unsigned long long g = global_group(a);
    if (g >= a.groups) return;
    const unsigned log_g = a.log_g1 + a.log_g2, log_gpr = a.log_g2 - LW;  // groups per row of the grid (g2 >= 8)
    const unsigned long long g1 = 1ull << a.log_g1, g2 = 1ull << a.log_g2;
    const unsigned long long b = g >> (log_g - LW), rem = g & ((1ull << (log_g - LW)) - 1);
    const unsigned long long r1 = rem >> log_gpr, s0 = (rem & ((1ull << log_gpr) - 1)) * W;
    const unsigned long long pos1 = (a.n1 + 1) / 2, neg1 = g1 - (a.n1 - pos1);  // rows [0, pos1) and [neg1, g1) hold modes
    const unsigned long long pos2 = (a.n2 + 1) / 2, neg2 = g2 - (a.n2 - pos2);  // and so the columns
    const bool row_in = r1 < pos1 || r1 >= neg1;
    const unsigned long long m1 = r1 < pos1 ? r1 : r1 - (g1 - a.n1);
    T orr[W], oi[W];
#pragma unroll
    for (int j = 0; j < W; ++j) orr[j] = oi[j] = T(0);
    if (row_in) {
        const T *fr = (const T *)a.in_re + b * a.in_dist + m1 * a.n2;
        const T *fi = REAL ? nullptr : (const T *)a.in_im + b * a.in_dist + m1 * a.n2;
        const T *p = (const T *)a.inv2;
        const T p1 = ((const T *)a.inv1)[m1];
        // the mode of slot s0 where the whole group lies in one of the two runs of modes
        const bool low = s0 + W <= pos2, high = s0 >= neg2;
        const unsigned long long m0 = low ? s0 : s0 - (g2 - a.n2);
        if (VEC && (low || high) && m0 % W == 0 && (m1 * a.n2) % W == 0) {
            const V vr = __builtin_nontemporal_load((const V *)(fr + m0));
            const V vp = *(const V *)(p + m0);
            V vi = vr;
            if (!REAL) vi = __builtin_nontemporal_load((const V *)(fi + m0));
#pragma unroll
            for (int j = 0; j < W; ++j) {
                orr[j] = vr[j] * p1 * vp[j];
                oi[j] = REAL ? T(0) : vi[j] * p1 * vp[j];
            }
        } else {
#pragma unroll
            for (int j = 0; j < W; ++j) {
                const unsigned long long s = s0 + j;
                const bool in = s < pos2 || s >= neg2;
                const unsigned long long m = s < pos2 ? s : s - (g2 - a.n2);
                const T pm = in ? p[m] : T(0);
                orr[j] = in ? __builtin_nontemporal_load(fr + m) * p1 * pm : T(0);
                oi[j] = in && !REAL ? __builtin_nontemporal_load(fi + m) * p1 * pm : T(0);
            }
        }
    }
    const unsigned long long at = (b << log_g) + (r1 << a.log_g2) + s0;
    T *wr = (T *)a.out_re + at, *wi = (T *)a.out_im + at;
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

// F[b out_dist + m1 N2 + m2] = g^[b G + slot1(m1) g2 + slot2(m2)] inv1[m1] inv2[m2]
template <typename T, bool VEC>
__global__ void __launch_bounds__(256) nufft2d_deconv_kernel(Nufft2dArgs a) {
    using V = typename AnyVec<T>::type;
    constexpr int W = AnyVec<T>::N;
    const unsigned long long g = global_group(a);
    if (g >= a.groups) return;
    unsigned long long b, m1;
    const unsigned gpr = (unsigned)((a.n2 + W - 1) / W);  // groups per row of modes
    const unsigned long long rem = split_group(g, a.gpt, &b);
    const unsigned long long m0 = split_group(rem, gpr, &m1) * W;
    const unsigned log_g = a.log_g1 + a.log_g2;
    const unsigned long long g1 = 1ull << a.log_g1, g2 = 1ull << a.log_g2, pos2 = (a.n2 + 1) / 2;
    const unsigned long long row = (b << log_g) + (nufft_slot(m1, a.n1, g1) << a.log_g2);
    const T *gr = (const T *)a.in_re + row, *gi = (const T *)a.in_im + row;
    const T *p = (const T *)a.inv2;
    const T p1 = ((const T *)a.inv1)[m1];
    T *fr = (T *)a.out_re + b * a.out_dist + m1 * a.n2, *fi = (T *)a.out_im + b * a.out_dist + m1 * a.n2;
    // the whole group in one run of modes and inside N2: its slots are consecutive
    const bool low = m0 + W <= pos2, high = m0 >= pos2 && m0 + W <= a.n2;
    const unsigned long long s0 = nufft_slot(m0, a.n2, g2);
    if (VEC && (low || high) && s0 % W == 0 && (m1 * a.n2) % W == 0) {
        const V vp = *(const V *)(p + m0);
        const V vr = *(const V *)(gr + s0) * p1 * vp, vi = *(const V *)(gi + s0) * p1 * vp;
        __builtin_nontemporal_store(vr, (V *)(fr + m0));
        __builtin_nontemporal_store(vi, (V *)(fi + m0));
    } else {
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const unsigned long long m = m0 + j;
            if (m < a.n2) {
                const unsigned long long s = nufft_slot(m, a.n2, g2);
                const T pm = p[m];
                __builtin_nontemporal_store(gr[s] * p1 * pm, fr + m);
                __builtin_nontemporal_store(gi[s] * p1 * pm, fi + m);
            }
        }
    }
}

template <typename T> hipError_t launch_nufft2d(int kind, bool vec, const Nufft2dArgs &a0, hipStream_t stream) {
    Nufft2dArgs a = a0;
    const bool real = a.in_im == nullptr;
    return launch_in_slices(a.groups, [&](dim3 grid, unsigned long long g0) {
        a.g0 = g0;
        if (kind == 0 && real)
            hipLaunchKernelGGL((nufft2d_spread_kernel<T, true>), grid, dim3(256), 0, stream, a);
        else if (kind == 0)
            hipLaunchKernelGGL((nufft2d_spread_kernel<T, false>), grid, dim3(256), 0, stream, a);
        else if (kind == 1)
            hipLaunchKernelGGL(nufft2d_interp_kernel<T>, grid, dim3(256), 0, stream, a);
        else if (kind == 2 && vec && real)
            hipLaunchKernelGGL((nufft2d_pre_kernel<T, true, true>), grid, dim3(256), 0, stream, a);
        else if (kind == 2 && vec)
            hipLaunchKernelGGL((nufft2d_pre_kernel<T, true, false>), grid, dim3(256), 0, stream, a);
        else if (kind == 2 && real)
            hipLaunchKernelGGL((nufft2d_pre_kernel<T, false, true>), grid, dim3(256), 0, stream, a);
        else if (kind == 2)
            hipLaunchKernelGGL((nufft2d_pre_kernel<T, false, false>), grid, dim3(256), 0, stream, a);
        else if (vec)
            hipLaunchKernelGGL((nufft2d_deconv_kernel<T, true>), grid, dim3(256), 0, stream, a);
        else
            hipLaunchKernelGGL((nufft2d_deconv_kernel<T, false>), grid, dim3(256), 0, stream, a);
    });
}

template hipError_t launch_nufft2d<double>(int, bool, const Nufft2dArgs &, hipStream_t);
template hipError_t launch_nufft2d<float>(int, bool, const Nufft2dArgs &, hipStream_t);

}  // namespace phast
