// nufft_nd.hip -- the four kernels of the non-uniform FFT in D = 2 and 3 dimensions (nufft_nd.hpp has the algorithm).  pre,
// deconvolve and interpolate are written once for every rank; only spreading differs, and has one body per rank.
//
// spread in two dimensions is a gather per grid point over the point set sorted by the combined cell q1 g2 + q2: one thread per
// fine-grid point and transform (l2 fastest across threads), element accesses, every sum in registers in a fixed order and ONE
// store per output -- no atomics, no LDS, so the bits depend on nothing but the points and the data.
//
// spread in three dimensions is a gather by tiles: a 256-thread workgroup owns kNufft3dTile1 x kNufft3dTile2 x kNufft3dTile3
// points of the fine grid of one transform (l3 fastest across the threads).  The points that can reach the tile are those of the
// cells within the kernel's reach of it on every axis; with the points sorted by the combined cell (q1 g2 + q2) g3 + q3 every
// (cell row 1, cell row 2) pair of that neighbourhood is one run of the sorted tables, or two where axis 3 wraps.  The workgroup
// walks the runs in a fixed order and stages the points through LDS, kNufft3dChunk at a time: the threads share the loads of the
// positions, of perm and of the values behind perm, then share the kernel values -- per staged point ONE value of nufft_weight
// for each of the tile's 4 + 8 + 8 coordinates (0 outside the support), formed once for the whole tile -- and after a barrier
// every thread adds every staged point to its own grid point in registers: (k1 k2) k3 in R, exactly as the interpolation kernel
// forms it.  One store per output, no atomics, no cross-lane operations; the order in which a thread adds depends on the tile
// and the point set alone, so the bits depend on nothing but the points and the data.  Every loop that holds a barrier runs on
// the tile's coordinates and on cell_start values that all threads read alike.
//
// Every kernel value is a product of nufft_weight(dq_i, t_i) in R (double for f64, float for f32), multiplied left to right and
// formed the same way in spread and interpolate: type 2 Reverse is the adjoint of type 1 Forward to rounding.
//
// interpolate is one thread per sorted point and transform over w^D grid values.  pre and deconvolve are streaming sweeps built
// like nufft.hip's, along the last axis: one group of 16 bytes per plane per thread, 256-thread workgroups in address order,
// launch_in_slices, and an element-access variant for planes (or a workspace) that do not allow 16-byte accesses, for rows of the
// caller's planes that do not start on a 16-byte boundary (N_D no multiple of the group) and for groups that straddle the
// positive / negative run of modes.  Every path multiplies ((v inv1) inv2) inv3.
#include "nufft_nd.hpp"

namespace phast {

// log2 G
template <size_t D> __device__ inline unsigned nufft_nd_log_cells(const NufftNdArgs<D> &a) {
    unsigned log_g = 0;
#pragma unroll
    for (size_t d = 0; d < D; ++d) log_g += a.log_g[d];
    return log_g;
}

// v inv1 .. inv(D-1), multiplied left to right; V: T or a group of T
template <typename V, typename T, size_t L> __device__ inline V nufft_nd_scaled(V v, const T (&pr)[L]) {
#pragma unroll
    for (size_t d = 0; d < L; ++d) v = v * pr[d];
    return v;
}

// the cells of one axis whose points can reach a tile of `tile` grid points from `lo`: lo - h .. lo + tile + h - 2 (mod g), that
// is `*count` cells from `*first`; the whole ring, once, from cell 0 where they would meet themselves
__device__ inline void nufft3d_reach(unsigned long long lo, unsigned tile, unsigned long long h, unsigned long long g,
                                     unsigned long long *first, unsigned long long *count) {
    const unsigned long long e = tile + 2 * h - 1;
    *first = e >= g ? 0 : (lo - h) & (g - 1);
    *count = e >= g ? g : e;
}

// Spreading: per grid point in two dimensions, per tile in three.  REAL: no imaginary plane.
//
// 2-D: g[b G + l1 g2 + l2] = sum_j phi1 phi2 c[b in_dist + j] over the points of the cells (l1 - h .. l1 + h - 1) x
// (l2 - h .. l2 + h - 1) (mod g1, g2), h = ceil(w / 2): cell row by cell row in that order, each row's cells one run of the
// sorted tables (two where the columns wrap past the end of the grid: the cells up to the end first), in sorted order
//
// 3-D: g[b G + (l1 g2 + l2) g3 + l3] = sum_j (phi1 phi2) phi3 c[b in_dist + j] over the points of the cells round the tile: cell
// row 1 outer, cell row 2 in the middle (both from the first cell of the reach, in ring order), the cells of axis 3 up to the end
// of the grid before those past the wrap, each run in sorted order
template <typename T, size_t D, bool REAL>
__global__ void __launch_bounds__(256) nufft_nd_spread_kernel(NufftNdArgs<D> a) {
    using R = typename NufftReal<T>::type;
    if constexpr (D == 2) {
        const unsigned long long g = global_group(a);
        if (g >= a.groups) return;
        const unsigned log_g = a.log_g[0] + a.log_g[1];
        const unsigned long long g1 = 1ull << a.log_g[0], g2 = 1ull << a.log_g[1], mask1 = g1 - 1, mask2 = g2 - 1;
        const unsigned long long b = g >> log_g, l = g & ((1ull << log_g) - 1), l1 = l >> a.log_g[1], l2 = l & mask2;
        const T *cr = (const T *)a.in_re + b * a.in_dist;
        const T *ci = REAL ? nullptr : (const T *)a.in_im + b * a.in_dist;
        const unsigned long long h = (unsigned long long)((a.w + 1) / 2);
        const double dg1 = (double)g1, dg2 = (double)g2, two_over_w = 2.0 / a.w;
        const R beta = (R)nufft_beta(a.w);
        const unsigned long long lo2 = (l2 - h) & mask2, end2 = lo2 + 2 * h;  // 2h <= g2 columns from lo2
        const bool wraps = end2 > g2;
        R sr = 0, si = 0;
        for (unsigned long long rr = 0; rr < 2 * h; ++rr) {  // 2h <= g1 distinct cell rows
            const uint32_t *row = a.cell_start + (((l1 - h + rr) & mask1) << a.log_g[1]);
            uint32_t i0 = row[lo2], i1 = row[wraps ? g2 : end2];
            for (int run = 0; run < (wraps ? 2 : 1); ++run) {
                for (uint32_t i = i0; i < i1; ++i) {
                    double t1, t2;
                    const long long q1 = nufft_cell(a.xs[0][i], dg1, &t1), q2 = nufft_cell(a.xs[1][i], dg2, &t2);
                    const R k = nufft_weight<R>(nufft_ring(l1, q1, mask1), t1, two_over_w, beta) *
                                nufft_weight<R>(nufft_ring(l2, q2, mask2), t2, two_over_w, beta);
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
    } else {
        constexpr unsigned T1 = kNufft3dTile1, T2 = kNufft3dTile2, T3 = kNufft3dTile3, P = kNufft3dChunk, NW = T1 + T2 + T3;
        static_assert(T1 * T2 * T3 == 256 && P <= 256, "a tile is one workgroup; a thread stages at most one point per pass");
        __shared__ double s_pos[3][P];  // the staged positions, turns
        __shared__ R s_val[2][P];       // the staged values
        __shared__ R s_k[P][NW];        // per staged point the kernel values at the tile's T1, T2 and T3 coordinates
        const unsigned tid = threadIdx.x;
        const unsigned long long tile = (a.g0 >> 8) + blockIdx.x;  // of the launch's transforms: the whole workgroup leaves together
        if ((tile << 8) >= a.groups) return;
        const unsigned log_g = a.log_g[0] + a.log_g[1] + a.log_g[2];
        const unsigned long long g1 = 1ull << a.log_g[0], g2 = 1ull << a.log_g[1], g3 = 1ull << a.log_g[2];
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
                const uint32_t *row = a.cell_start + (((q1 << a.log_g[1]) + q2) << a.log_g[2]);
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
                    s_pos[0][fill + tid] = a.xs[0][i];
                    s_pos[1][fill + tid] = a.xs[1][i];
                    s_pos[2][fill + tid] = a.xs[2][i];
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
                        s_k[p][k] = nufft_weight<R>(nufft_ring(l, q, g - 1), t, two_over_w, beta);
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
        const unsigned long long o = (b << log_g) + ((((lo1 + c1) << a.log_g[1]) + lo2 + c2) << a.log_g[2]) + lo3 + c3;
        ((T *)a.out_re)[o] = (T)sr;
        ((T *)a.out_im)[o] = (T)si;
    }
}

// c[b out_dist + perm[i]] = sum over the w^D grid points under sorted point i of (phi1 phi2) phi3 g[...]: the cells
// (q_i + first_i + s) mod g_i of every axis, axis 1 outermost and the last axis innermost.  The w kernel values of the last axis
// are formed once, into registers: the loops over u are unrolled to kNufftMaxWidth with static indices and a `u < w` guard (an
// array indexed at run time would live in scratch memory); the values of the other axes are formed in their loops.  The loop
// between the first and the last axis is written out for D <= 3: a recursion over the axes costs the f64 kernel of three
// dimensions 0.3 to 0.8 % of its time, an odometer over w^(D-2) cells 23 VGPRs and a wave of occupancy
template <typename T, size_t D>
__global__ void __launch_bounds__(256) nufft_nd_interp_kernel(NufftNdArgs<D> a) {
    using R = typename NufftReal<T>::type;
    static_assert(D == 2 || D == 3, "the loop over the middle axis is written for at most one");
    constexpr size_t L = D - 1;  // the last axis
    const unsigned long long g = global_group(a);
    if (g >= a.groups) return;
    const unsigned long long b = g / a.m, i = g - b * a.m;
    const unsigned log_g = nufft_nd_log_cells(a);
    const T *gr = (const T *)a.in_re + (b << log_g), *gi = (const T *)a.in_im + (b << log_g);
    const double two_over_w = 2.0 / a.w;
    const R beta = (R)nufft_beta(a.w);
    unsigned long long mask[D];
    long long q[D], first[D];
    double t[D];
#pragma unroll
    for (size_t d = 0; d < D; ++d) {
        mask[d] = (1ull << a.log_g[d]) - 1;
        q[d] = nufft_cell(a.xs[d][i], (double)(mask[d] + 1), &t[d]);
        first[d] = nufft_first(a.w, t[d]);
    }
    R kl[kNufftMaxWidth];
#pragma unroll
    for (int u = 0; u < kNufftMaxWidth; ++u) kl[u] = u < a.w ? nufft_weight<R>(first[L] + u, t[L], two_over_w, beta) : R(0);
    R sr = 0, si = 0;
    for (int s = 0; s < a.w; ++s) {
        const long long dq1 = first[0] + s;
        const R k1 = nufft_weight<R>(dq1, t[0], two_over_w, beta);
        const unsigned long long plane = ((unsigned long long)(q[0] + dq1) & mask[0]) << a.log_g[1];
        for (int v = 0; v < (D == 3 ? a.w : 1); ++v) {  // the middle axis of three dimensions; one pass in two
            R km = k1;
            unsigned long long row = plane;
            if constexpr (D == 3) {
                const long long dq2 = first[1] + v;
                km = k1 * nufft_weight<R>(dq2, t[1], two_over_w, beta);
                row = (plane + ((unsigned long long)(q[1] + dq2) & mask[1])) << a.log_g[2];
            }
#pragma unroll
            for (int u = 0; u < kNufftMaxWidth; ++u) {
                if (u < a.w) {
                    const unsigned long long l = row + ((unsigned long long)(q[L] + first[L] + u) & mask[L]);
                    const R k = km * kl[u];
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
template <typename T, size_t D, bool VEC, bool REAL>
__global__ void __launch_bounds__(256) nufft_nd_pre_kernel(NufftNdArgs<D> a) {
    using V = typename AnyVec<T>::type;
    constexpr int W = AnyVec<T>::N;
    constexpr unsigned LW = W == 2 ? 1 : 2;
    constexpr size_t L = D - 1;  // the sweep runs along the last axis
    const unsigned long long g = global_group(a);
    if (g >= a.groups) return;
    const unsigned log_g = nufft_nd_log_cells(a), log_gpr = a.log_g[L] - LW;  // groups per row of the grid (g_D >= 8)
    const unsigned long long gl = 1ull << a.log_g[L];
    const unsigned long long b = g >> (log_g - LW), rem = g & ((1ull << (log_g - LW)) - 1);
    const unsigned long long rows = rem >> log_gpr, s0 = (rem & ((1ull << log_gpr) - 1)) * W;
    // the row of the grid as cells (r1, .., r(D-1)): the cells [0, pos_i) and [neg_i, g_i) of an axis hold modes
    bool row_in = true;
    unsigned long long m[L], rest = rows;
#pragma unroll
    for (size_t d = L; d-- > 0;) {
        const unsigned long long gd = 1ull << a.log_g[d], r = d ? rest & (gd - 1) : rest;
        rest >>= a.log_g[d];
        const unsigned long long pos = (a.n[d] + 1) / 2, neg = gd - (a.n[d] - pos);
        row_in = row_in && (r < pos || r >= neg);
        m[d] = r < pos ? r : r - (gd - a.n[d]);
    }
    const unsigned long long posl = (a.n[L] + 1) / 2, negl = gl - (a.n[L] - posl);  // and so the columns
    T orr[W], oi[W];
#pragma unroll
    for (int j = 0; j < W; ++j) orr[j] = oi[j] = T(0);
    if (row_in) {
        unsigned long long base = 0;  // of the row of modes: (m1 N2 + m2) N3
        T pr[L];
#pragma unroll
        for (size_t d = 0; d < L; ++d) {
            base = base * a.n[d] + m[d];
            pr[d] = ((const T *)a.inv[d])[m[d]];
        }
        base *= a.n[L];
        const T *fr = (const T *)a.in_re + b * a.in_dist + base;
        const T *fi = REAL ? nullptr : (const T *)a.in_im + b * a.in_dist + base;
        const T *p = (const T *)a.inv[L];
        // the mode of slot s0 where the whole group lies in one of the two runs of modes
        const bool low = s0 + W <= posl, high = s0 >= negl;
        const unsigned long long m0 = low ? s0 : s0 - (gl - a.n[L]);
        if (VEC && (low || high) && m0 % W == 0 && base % W == 0) {
            const V vr = __builtin_nontemporal_load((const V *)(fr + m0));
            const V vp = *(const V *)(p + m0);
            V vi = vr;
            if (!REAL) vi = __builtin_nontemporal_load((const V *)(fi + m0));
            const V ur = nufft_nd_scaled(vr, pr), ui = nufft_nd_scaled(vi, pr);
#pragma unroll
            for (int j = 0; j < W; ++j) {
                orr[j] = ur[j] * vp[j];
                oi[j] = REAL ? T(0) : ui[j] * vp[j];
            }
        } else {
#pragma unroll
            for (int j = 0; j < W; ++j) {
                const unsigned long long s = s0 + j;
                const bool in = s < posl || s >= negl;
                const unsigned long long ml = s < posl ? s : s - (gl - a.n[L]);
                const T pm = in ? p[ml] : T(0);
                orr[j] = in ? nufft_nd_scaled(__builtin_nontemporal_load(fr + ml), pr) * pm : T(0);
                oi[j] = in && !REAL ? nufft_nd_scaled(__builtin_nontemporal_load(fi + ml), pr) * pm : T(0);
            }
        }
    }
    const unsigned long long at = (b << log_g) + (rows << a.log_g[L]) + s0;
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
template <typename T, size_t D, bool VEC>
__global__ void __launch_bounds__(256) nufft_nd_deconv_kernel(NufftNdArgs<D> a) {
    using V = typename AnyVec<T>::type;
    constexpr int W = AnyVec<T>::N;
    constexpr size_t L = D - 1;  // the sweep runs along the last axis
    const unsigned long long g = global_group(a);
    if (g >= a.groups) return;
    unsigned long long b, mrow;
    const unsigned gpr = (unsigned)((a.n[L] + W - 1) / W);  // groups per row of modes
    const unsigned long long rem = split_group(g, a.gpt, &b);
    const unsigned long long m0 = split_group(rem, gpr, &mrow) * W;
    // the row of modes mrow = m1 N2 + m2 as (m1, .., m(D-1)), its row of the grid and its D - 1 factors
    unsigned long long m[L], rest = mrow;
#pragma unroll
    for (size_t d = L; d-- > 1;) m[d] = split_group(rest, (unsigned)a.n[d], &rest);
    m[0] = rest;
    unsigned long long row = 0;
    T pr[L];
#pragma unroll
    for (size_t d = 0; d < L; ++d) {
        row = (row << a.log_g[d]) + nufft_slot(m[d], a.n[d], 1ull << a.log_g[d]);
        pr[d] = ((const T *)a.inv[d])[m[d]];
    }
    row = (b << nufft_nd_log_cells(a)) + (row << a.log_g[L]);
    const unsigned long long gl = 1ull << a.log_g[L], posl = (a.n[L] + 1) / 2;
    const T *gr = (const T *)a.in_re + row, *gi = (const T *)a.in_im + row;
    const T *p = (const T *)a.inv[L];
    const unsigned long long base = mrow * a.n[L];
    T *fr = (T *)a.out_re + b * a.out_dist + base, *fi = (T *)a.out_im + b * a.out_dist + base;
    // the whole group in one run of modes and inside N_D: its slots are consecutive
    const bool low = m0 + W <= posl, high = m0 >= posl && m0 + W <= a.n[L];
    const unsigned long long s0 = nufft_slot(m0, a.n[L], gl);
    if (VEC && (low || high) && s0 % W == 0 && base % W == 0) {
        const V vp = *(const V *)(p + m0);
        const V vr = nufft_nd_scaled(*(const V *)(gr + s0), pr) * vp, vi = nufft_nd_scaled(*(const V *)(gi + s0), pr) * vp;
        __builtin_nontemporal_store(vr, (V *)(fr + m0));
        __builtin_nontemporal_store(vi, (V *)(fi + m0));
    } else {
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const unsigned long long ml = m0 + j;
            if (ml < a.n[L]) {
                const unsigned long long s = nufft_slot(ml, a.n[L], gl);
                const T pm = p[ml];
                __builtin_nontemporal_store(nufft_nd_scaled(gr[s], pr) * pm, fr + ml);
                __builtin_nontemporal_store(nufft_nd_scaled(gi[s], pr) * pm, fi + ml);
            }
        }
    }
}

template <typename T, size_t D> hipError_t launch_nufft_nd(int kind, bool vec, const NufftNdArgs<D> &a0, hipStream_t stream) {
    NufftNdArgs<D> a = a0;
    const bool real = a.in_im == nullptr;
    return launch_in_slices(a.groups, [&](dim3 grid, unsigned long long g0) {
        a.g0 = g0;
        if (kind == 0 && real)
            hipLaunchKernelGGL((nufft_nd_spread_kernel<T, D, true>), grid, dim3(256), 0, stream, a);
        else if (kind == 0)
            hipLaunchKernelGGL((nufft_nd_spread_kernel<T, D, false>), grid, dim3(256), 0, stream, a);
        else if (kind == 1)
            hipLaunchKernelGGL((nufft_nd_interp_kernel<T, D>), grid, dim3(256), 0, stream, a);
        else if (kind == 2 && vec && real)
            hipLaunchKernelGGL((nufft_nd_pre_kernel<T, D, true, true>), grid, dim3(256), 0, stream, a);
        else if (kind == 2 && vec)
            hipLaunchKernelGGL((nufft_nd_pre_kernel<T, D, true, false>), grid, dim3(256), 0, stream, a);
        else if (kind == 2 && real)
            hipLaunchKernelGGL((nufft_nd_pre_kernel<T, D, false, true>), grid, dim3(256), 0, stream, a);
        else if (kind == 2)
            hipLaunchKernelGGL((nufft_nd_pre_kernel<T, D, false, false>), grid, dim3(256), 0, stream, a);
        else if (vec)
            hipLaunchKernelGGL((nufft_nd_deconv_kernel<T, D, true>), grid, dim3(256), 0, stream, a);
        else
            hipLaunchKernelGGL((nufft_nd_deconv_kernel<T, D, false>), grid, dim3(256), 0, stream, a);
    });
}

template hipError_t launch_nufft_nd<double, 2>(int, bool, const NufftNdArgs<2> &, hipStream_t);
template hipError_t launch_nufft_nd<float, 2>(int, bool, const NufftNdArgs<2> &, hipStream_t);
template hipError_t launch_nufft_nd<double, 3>(int, bool, const NufftNdArgs<3> &, hipStream_t);
template hipError_t launch_nufft_nd<float, 3>(int, bool, const NufftNdArgs<3> &, hipStream_t);

}  // namespace phast
