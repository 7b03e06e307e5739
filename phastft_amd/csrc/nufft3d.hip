// nufft3d.hip -- the four kernels of the three-dimensional non-uniform FFT (nufft3d.hpp has the algorithm).
//
// spread is a gather by tiles: a 256-thread workgroup owns kNufft3dTile1 x kNufft3dTile2 x kNufft3dTile3 points of the fine grid of
// one transform (l3 fastest across the threads).  The points that can reach the tile are those of the cells within the kernel's
// reach of it on every axis; with the points sorted by the combined cell (q1 g2 + q2) g3 + q3 every (cell row 1, cell row 2) pair
// of that neighbourhood is one run of the sorted tables, or two where axis 3 wraps.  The workgroup walks the runs in a fixed order
// and stages the points through LDS, kNufft3dChunk at a time: the threads share the loads of the positions, of perm and of the
// values behind perm, then share the kernel values -- per staged point ONE value of nufft_weight for each of the tile's 4 + 8 + 8
// coordinates (0 outside the support), formed once for the whole tile -- and after a barrier every thread adds every staged point
// to its own grid point in registers: (k1 k2) k3 in R, exactly as the interpolation kernel forms it, so type 2 Reverse stays the
// adjoint of type 1 Forward to rounding.  One store per output, no atomics, no cross-lane operations; the order in which a thread
// adds depends on the tile and the point set alone, so the bits depend on nothing but the points and the data.  Every loop that
// holds a barrier runs on the tile's coordinates and on cell_start values that all threads read alike.
//
// interpolate is one thread per sorted point and transform over w^3 grid values, as nufft2d.hip's with one more loop.  pre and
// deconvolve are streaming sweeps along axis 3 built like nufft2d.hip's: one group of 16 bytes per plane per thread, 256-thread
// workgroups in address order, launch_in_slices, and an element-access variant for planes (or a workspace) that do not allow
// 16-byte accesses, for rows of the caller's planes that do not start on a 16-byte boundary and for groups that straddle the
// positive / negative run of modes.  Every path multiplies ((v inv1) inv2) inv3.
#include "nufft3d.hpp"

namespace phast {

template <typename T> struct Nufft3dReal { typedef double type; };
template <> struct Nufft3dReal<float> { typedef float type; };

// the signed distance l - q of two cells around a ring of mask + 1 cells, in [-(mask + 1) / 2, (mask + 1) / 2)
__device__ inline long long nufft3d_ring(unsigned long long l, long long q, unsigned long long mask) {
    const long long half = (long long)((mask + 1) >> 1);
    return (long long)(((unsigned long long)((long long)l - q + half)) & mask) - half;
}

// the cells of one axis whose points can reach a tile of `tile` grid points from `lo`: lo - h .. lo + tile + h - 2 (mod g), that
// is `*count` cells from `*first`; the whole ring, once, from cell 0 where they would meet themselves
__device__ inline void nufft3d_reach(unsigned long long lo, unsigned tile, unsigned long long h, unsigned long long g,
                                     unsigned long long *first, unsigned long long *count) {
    const unsigned long long e = tile + 2 * h - 1;
    *first = e >= g ? 0 : (lo - h) & (g - 1);
    *count = e >= g ? g : e;
}

// g[b G + (l1 g2 + l2) g3 + l3] = sum_j (phi1 phi2) phi3 c[b in_dist + j] over the points of the cells round the tile: cell row 1
// outer, cell row 2 in the middle (both from the first cell of the reach, in ring order), the cells of axis 3 up to the end of
// the grid before those past the wrap, each run in sorted order.  REAL: no imaginary plane
template <typename T, bool REAL>
__global__ void __launch_bounds__(256) nufft3d_spread_kernel(Nufft3dArgs a) {
    using R = typename Nufft3dReal<T>::type;
    constexpr unsigned T1 = kNufft3dTile1, T2 = kNufft3dTile2, T3 = kNufft3dTile3, P = kNufft3dChunk, NW = T1 + T2 + T3;
    static_assert(T1 * T2 * T3 == 256 && P <= 256, "a tile is one workgroup; a thread stages at most one point per pass");
    __shared__ double s_pos[3][P];  // the staged positions, turns
    __shared__ R s_val[2][P];       // the staged values
    __shared__ R s_k[P][NW];        // per staged point the kernel values at the tile's T1, T2 and T3 coordinates
    const unsigned tid = threadIdx.x;
    const unsigned long long tile = (a.g0 >> 8) + blockIdx.x;  // of the launch's transforms: the whole workgroup leaves together
    if ((tile << 8) >= a.groups) return;
    const unsigned log_g = a.log_g1 + a.log_g2 + a.log_g3;
    const unsigned long long g1 = 1ull << a.log_g1, g2 = 1ull << a.log_g2, g3 = 1ull << a.log_g3;
    const unsigned long long b = tile >> (log_g - 8), in_b = tile & ((1ull << (log_g - 8)) - 1);
    const unsigned long long n3t = g3 / T3, n2t = g2 / T2;
    const unsigned long long lo3 = (in_b % n3t) * T3, lo2 = (in_b / n3t % n2t) * T2, lo1 = (in_b / n3t / n2t) * T1;
    const unsigned c3 = tid % T3, c2 = tid / T3 % T2, c1 = tid / (T3 * T2);
    const T *cr = (const T *)a.in_re + b * a.in_dist;
    const T *ci = REAL ? nullptr : (const T *)a.in_im + b * a.in_dist;
    const unsigned long long h = (unsigned long long)((a.w + 1) / 2);
    const double two_over_w = 2.0 / a.w;
    const R beta = (R)nufft_beta(a.w);
    unsigned long long f1, e1, f2, e2, f3, e3;
    nufft3d_reach(lo1, T1, h, g1, &f1, &e1);
    nufft3d_reach(lo2, T2, h, g2, &f2, &e2);
    nufft3d_reach(lo3, T3, h, g3, &f3, &e3);
    const bool wraps = f3 + e3 > g3;
    R sr = 0, si = 0;
    unsigned fill = 0;  // staged points not yet added; the same in every thread
    const unsigned rows = (unsigned)(e1 * e2), per2 = (unsigned)e2;
    for (unsigned rr = 0; rr <= rows; ++rr) {  // one pass more than there are rows: it adds what is still staged
        const bool last = rr == rows;
        uint32_t i0 = 0, i1 = 0, j0 = 0, j1 = 0;  // the run up to the end of the grid and the one past the wrap
        if (!last) {
            const unsigned long long q1 = (f1 + rr / per2) & (g1 - 1), q2 = (f2 + rr % per2) & (g2 - 1);
            const uint32_t *row = a.cell_start + (((q1 << a.log_g2) + q2) << a.log_g3);
            i0 = row[f3];
            i1 = row[wraps ? g3 : f3 + e3];
            if (wraps) {
                j0 = row[0];
                j1 = row[f3 + e3 - g3];
            }
        }
        for (;;) {
            if (i0 == i1) {
                i0 = j0;
                i1 = j1;
                j0 = j1 = 0;
            }
            const unsigned take = i1 - i0 < P - fill ? i1 - i0 : P - fill;
            if (tid < take) {
                const uint32_t i = i0 + tid, j = a.perm[i];
                s_pos[0][fill + tid] = a.xs[i];
                s_pos[1][fill + tid] = a.ys[i];
                s_pos[2][fill + tid] = a.zs[i];
                s_val[0][fill + tid] = (R)cr[j];
                if (!REAL) s_val[1][fill + tid] = (R)ci[j];
            }
            i0 += take;
            fill += take;
            if (fill == P || (last && fill)) {
                __syncthreads();  // the positions and values are staged
                // the staged points' kernel values, shared among the threads
                for (unsigned e = tid; e < fill * NW; e += 256) {
                    const unsigned p = e / NW, k = e % NW;
                    const unsigned axis = k < T1 ? 0 : k < T1 + T2 ? 1 : 2;
                    const unsigned long long l = axis == 0 ? lo1 + k : axis == 1 ? lo2 + (k - T1) : lo3 + (k - T1 - T2);
                    const unsigned long long g = axis == 0 ? g1 : axis == 1 ? g2 : g3;
                    double t;
                    const long long q = nufft_cell(s_pos[axis][p], (double)g, &t);
                    s_k[p][k] = nufft_weight<R>(nufft3d_ring(l, q, g - 1), t, two_over_w, beta);
                }
                __syncthreads();
                for (unsigned p = 0; p < fill; ++p) {  // every point into every thread's sums
                    const R k = (s_k[p][c1] * s_k[p][T1 + c2]) * s_k[p][T1 + T2 + c3];
                    sr += k * s_val[0][p];
                    if (!REAL) si += k * s_val[1][p];
                }
                __syncthreads();  // before the next pass overwrites what this one read
                fill = 0;
            }
            if (i0 == i1 && j0 == j1) break;
        }
    }
    const unsigned long long o = (b << log_g) + ((((lo1 + c1) << a.log_g2) + lo2 + c2) << a.log_g3) + lo3 + c3;
    ((T *)a.out_re)[o] = (T)sr;
    ((T *)a.out_im)[o] = (T)si;
}

// c[b out_dist + perm[i]] = sum over the w^3 grid points under sorted point i of (phi1 phi2) phi3 g[...]: planes
// (q1 + first1 + s) mod g1, s outer, rows (q2 + first2 + v) mod g2 in the middle, columns (q3 + first3 + u) mod g3 inner.  The w
// axis-3 kernel values are formed once, into registers: the loops over u are unrolled to kNufftMaxWidth with static indices and a
// `u < w` guard (an array indexed at run time would live in scratch memory); the axis-1 and axis-2 values are formed in their loops
template <typename T>
__global__ void __launch_bounds__(256) nufft3d_interp_kernel(Nufft3dArgs a) {
    using R = typename Nufft3dReal<T>::type;
    const unsigned long long g = global_group(a);
    if (g >= a.groups) return;
    const unsigned long long b = g / a.m, i = g - b * a.m;
    const unsigned log_g = a.log_g1 + a.log_g2 + a.log_g3;
    const unsigned long long mask1 = (1ull << a.log_g1) - 1, mask2 = (1ull << a.log_g2) - 1, mask3 = (1ull << a.log_g3) - 1;
    const T *gr = (const T *)a.in_re + (b << log_g), *gi = (const T *)a.in_im + (b << log_g);
    const double two_over_w = 2.0 / a.w;
    const R beta = (R)nufft_beta(a.w);
    double t1, t2, t3;
    const long long q1 = nufft_cell(a.xs[i], (double)(mask1 + 1), &t1), q2 = nufft_cell(a.ys[i], (double)(mask2 + 1), &t2);
    const long long q3 = nufft_cell(a.zs[i], (double)(mask3 + 1), &t3);
    const long long first1 = nufft_first(a.w, t1), first2 = nufft_first(a.w, t2), first3 = nufft_first(a.w, t3);
    R k3[kNufftMaxWidth];
#pragma unroll
    for (int u = 0; u < kNufftMaxWidth; ++u) k3[u] = u < a.w ? nufft_weight<R>(first3 + u, t3, two_over_w, beta) : R(0);
    R sr = 0, si = 0;
    for (int s = 0; s < a.w; ++s) {
        const long long dq1 = first1 + s;
        const R k1 = nufft_weight<R>(dq1, t1, two_over_w, beta);
        const unsigned long long plane = ((unsigned long long)(q1 + dq1) & mask1) << a.log_g2;
        for (int v = 0; v < a.w; ++v) {
            const long long dq2 = first2 + v;
            const R k12 = k1 * nufft_weight<R>(dq2, t2, two_over_w, beta);
            const unsigned long long row = (plane + ((unsigned long long)(q2 + dq2) & mask2)) << a.log_g3;
#pragma unroll
            for (int u = 0; u < kNufftMaxWidth; ++u) {
                if (u < a.w) {
                    const unsigned long long l = row + ((unsigned long long)(q3 + first3 + u) & mask3);
                    const R k = k12 * k3[u];
                    sr += k * (R)gr[l];
                    si += k * (R)gi[l];
                }
            }
        }
    }
    const unsigned long long o = b * a.out_dist + a.perm[i];
    ((T *)a.out_re)[o] = (T)sr;
    ((T *)a.out_im)[o] = (T)si;
}

// g^[b G + (slot1(m1) g2 + slot2(m2)) g3 + slot3(m3)] = F[b in_dist + (m1 N2 + m2) N3 + m3] inv1[m1] inv2[m2] inv3[m3], exact
// zeros in every other slot of the whole grid.  REAL: no imaginary plane
template <typename T, bool VEC, bool REAL>
__global__ void __launch_bounds__(256) nufft3d_pre_kernel(Nufft3dArgs a) {
    using V = typename AnyVec<T>::type;
    constexpr int W = AnyVec<T>::N;
    constexpr unsigned LW = W == 2 ? 1 : 2;
    const unsigned long long g = global_group(a);
    if (g >= a.groups) return;
    const unsigned log_g = a.log_g1 + a.log_g2 + a.log_g3, log_gpr = a.log_g3 - LW;  // groups per row of the grid (g3 >= 8)
    const unsigned long long g1 = 1ull << a.log_g1, g2 = 1ull << a.log_g2, g3 = 1ull << a.log_g3;
    const unsigned long long b = g >> (log_g - LW), rem = g & ((1ull << (log_g - LW)) - 1);
    const unsigned long long rows = rem >> log_gpr, s0 = (rem & ((1ull << log_gpr) - 1)) * W;
    const unsigned long long r1 = rows >> a.log_g2, r2 = rows & (g2 - 1);
    const unsigned long long pos1 = (a.n1 + 1) / 2, neg1 = g1 - (a.n1 - pos1);  // planes [0, pos1) and [neg1, g1) hold modes,
    const unsigned long long pos2 = (a.n2 + 1) / 2, neg2 = g2 - (a.n2 - pos2);  // and so the rows
    const unsigned long long pos3 = (a.n3 + 1) / 2, neg3 = g3 - (a.n3 - pos3);  // and the columns
    const bool row_in = (r1 < pos1 || r1 >= neg1) && (r2 < pos2 || r2 >= neg2);
    const unsigned long long m1 = r1 < pos1 ? r1 : r1 - (g1 - a.n1), m2 = r2 < pos2 ? r2 : r2 - (g2 - a.n2);
    T orr[W], oi[W];
#pragma unroll
    for (int j = 0; j < W; ++j) orr[j] = oi[j] = T(0);
    if (row_in) {
        const unsigned long long base = (m1 * a.n2 + m2) * a.n3;
        const T *fr = (const T *)a.in_re + b * a.in_dist + base;
        const T *fi = REAL ? nullptr : (const T *)a.in_im + b * a.in_dist + base;
        const T *p = (const T *)a.inv3;
        const T p1 = ((const T *)a.inv1)[m1], p2 = ((const T *)a.inv2)[m2];
        // the mode of slot s0 where the whole group lies in one of the two runs of modes
        const bool low = s0 + W <= pos3, high = s0 >= neg3;
        const unsigned long long m0 = low ? s0 : s0 - (g3 - a.n3);
        if (VEC && (low || high) && m0 % W == 0 && base % W == 0) {
            const V vr = __builtin_nontemporal_load((const V *)(fr + m0));
            const V vp = *(const V *)(p + m0);
            V vi = vr;
            if (!REAL) vi = __builtin_nontemporal_load((const V *)(fi + m0));
#pragma unroll
            for (int j = 0; j < W; ++j) {
                orr[j] = vr[j] * p1 * p2 * vp[j];
                oi[j] = REAL ? T(0) : vi[j] * p1 * p2 * vp[j];
            }
        } else {
#pragma unroll
            for (int j = 0; j < W; ++j) {
                const unsigned long long s = s0 + j;
                const bool in = s < pos3 || s >= neg3;
                const unsigned long long m = s < pos3 ? s : s - (g3 - a.n3);
                const T pm = in ? p[m] : T(0);
                orr[j] = in ? __builtin_nontemporal_load(fr + m) * p1 * p2 * pm : T(0);
                oi[j] = in && !REAL ? __builtin_nontemporal_load(fi + m) * p1 * p2 * pm : T(0);
            }
        }
    }
    const unsigned long long at = (b << log_g) + (rows << a.log_g3) + s0;
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

// F[b out_dist + (m1 N2 + m2) N3 + m3] = g^[b G + (slot1(m1) g2 + slot2(m2)) g3 + slot3(m3)] inv1[m1] inv2[m2] inv3[m3]
template <typename T, bool VEC>
__global__ void __launch_bounds__(256) nufft3d_deconv_kernel(Nufft3dArgs a) {
    using V = typename AnyVec<T>::type;
    constexpr int W = AnyVec<T>::N;
    const unsigned long long g = global_group(a);
    if (g >= a.groups) return;
    unsigned long long b, mrow, m1;
    const unsigned gpr = (unsigned)((a.n3 + W - 1) / W);  // groups per row of modes
    const unsigned long long rem = split_group(g, a.gpt, &b);
    const unsigned long long m0 = split_group(rem, gpr, &mrow) * W;
    const unsigned long long m2 = split_group(mrow, (unsigned)a.n2, &m1);
    const unsigned log_g = a.log_g1 + a.log_g2 + a.log_g3;
    const unsigned long long g1 = 1ull << a.log_g1, g2 = 1ull << a.log_g2, g3 = 1ull << a.log_g3, pos3 = (a.n3 + 1) / 2;
    const unsigned long long row = (b << log_g) + (((nufft_slot(m1, a.n1, g1) << a.log_g2) + nufft_slot(m2, a.n2, g2)) << a.log_g3);
    const T *gr = (const T *)a.in_re + row, *gi = (const T *)a.in_im + row;
    const T *p = (const T *)a.inv3;
    const T p1 = ((const T *)a.inv1)[m1], p2 = ((const T *)a.inv2)[m2];
    const unsigned long long base = mrow * a.n3;
    T *fr = (T *)a.out_re + b * a.out_dist + base, *fi = (T *)a.out_im + b * a.out_dist + base;
    // the whole group in one run of modes and inside N3: its slots are consecutive
    const bool low = m0 + W <= pos3, high = m0 >= pos3 && m0 + W <= a.n3;
    const unsigned long long s0 = nufft_slot(m0, a.n3, g3);
    if (VEC && (low || high) && s0 % W == 0 && base % W == 0) {
        const V vp = *(const V *)(p + m0);
        const V vr = *(const V *)(gr + s0) * p1 * p2 * vp, vi = *(const V *)(gi + s0) * p1 * p2 * vp;
        __builtin_nontemporal_store(vr, (V *)(fr + m0));
        __builtin_nontemporal_store(vi, (V *)(fi + m0));
    } else {
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const unsigned long long m = m0 + j;
            if (m < a.n3) {
                const unsigned long long s = nufft_slot(m, a.n3, g3);
                const T pm = p[m];
                __builtin_nontemporal_store(gr[s] * p1 * p2 * pm, fr + m);
                __builtin_nontemporal_store(gi[s] * p1 * p2 * pm, fi + m);
            }
        }
    }
}

template <typename T> hipError_t launch_nufft3d(int kind, bool vec, const Nufft3dArgs &a0, hipStream_t stream) {
    Nufft3dArgs a = a0;
    const bool real = a.in_im == nullptr;
    return launch_in_slices(a.groups, [&](dim3 grid, unsigned long long g0) {
        a.g0 = g0;
        if (kind == 0 && real)
            hipLaunchKernelGGL((nufft3d_spread_kernel<T, true>), grid, dim3(256), 0, stream, a);
        else if (kind == 0)
            hipLaunchKernelGGL((nufft3d_spread_kernel<T, false>), grid, dim3(256), 0, stream, a);
        else if (kind == 1)
            hipLaunchKernelGGL(nufft3d_interp_kernel<T>, grid, dim3(256), 0, stream, a);
        else if (kind == 2 && vec && real)
            hipLaunchKernelGGL((nufft3d_pre_kernel<T, true, true>), grid, dim3(256), 0, stream, a);
        else if (kind == 2 && vec)
            hipLaunchKernelGGL((nufft3d_pre_kernel<T, true, false>), grid, dim3(256), 0, stream, a);
        else if (kind == 2 && real)
            hipLaunchKernelGGL((nufft3d_pre_kernel<T, false, true>), grid, dim3(256), 0, stream, a);
        else if (kind == 2)
            hipLaunchKernelGGL((nufft3d_pre_kernel<T, false, false>), grid, dim3(256), 0, stream, a);
        else if (vec)
            hipLaunchKernelGGL((nufft3d_deconv_kernel<T, true>), grid, dim3(256), 0, stream, a);
        else
            hipLaunchKernelGGL((nufft3d_deconv_kernel<T, false>), grid, dim3(256), 0, stream, a);
    });
}

template hipError_t launch_nufft3d<double>(int, bool, const Nufft3dArgs &, hipStream_t);
template hipError_t launch_nufft3d<float>(int, bool, const Nufft3dArgs &, hipStream_t);

}  // namespace phast
