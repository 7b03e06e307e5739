// nufft_nd.hpp -- non-uniform FFTs of types 1 and 2 in D = 2 or 3 dimensions.  M points (x1_j, .., xD_j) in
// turns (reduced mod 1 per coordinate), N1 x .. x ND modes, row-major (the last axis fastest), each axis in numpy fftfreq
// order; k_i pairs with x_i:
//
//     type 1 (points -> modes)   F[m1, .., mD] = sum_j c_j exp(-+2 pi i (k1(m1) x1_j + .. + kD(mD) xD_j))
//     type 2 (modes -> points)   c_j = sum_m F[m1, .., mD] exp(-+2 pi i (k1(m1) x1_j + .. + kD(mD) xD_j))   (- Forward, + Reverse)
//
// The schedule is nufft.hpp's, per axis: the same width w, beta, kernel value (nufft_weight), support (nufft_first), slot
// (nufft_slot) and quadrature (NufftQuad), on a fine grid of g1 x .. x gD points, g_i = nufft_grid(N_i, w):
//
//     stage   type 1                                                  type 2
//     a       spread with the product kernel (phi1 phi2) phi3         pre: g^[slot1, .., slotD] = F inv1 .. invD, 0 elsewhere
//     b       the D-dimensional FFT of (g1, .., gD) in place (NdPlanner, always Forward: Reverse swaps the planes)
//     c       deconvolve  F = g^[slot1, .., slotD] inv1 .. invD       interpolate over the w^D grid points under a point
//
// The points are sorted once, on the host, by the combined cell (q1 g2 + q2) g3 + q3, so the cells of one row of cells along the
// last axis are one contiguous run of the sorted tables.  In two dimensions spreading is a gather per grid point, as in one
// dimension.  In three it is a gather by TILES of the fine grid (nufft_nd.hip): a workgroup owns kNufft3dTile1 x kNufft3dTile2 x
// kNufft3dTile3 grid points, stages the points of the cells round the tile through LDS kNufft3dChunk at a time and forms their
// kernel values once for the whole tile.
//
// The top of this header has no HIP dependency: tests/test_nufft2d_cpu.py and tests/test_nufft3d_cpu.py compile it with g++.
#pragma once

#include "nufft.hpp"

namespace phast {

constexpr unsigned long long kNufftNdMaxGrid = 1ull << 28;  // G = g1 .. gD: cell_start stays below 1 GiB, one f64 transform below 8 GiB
// the 3-D spread kernel's tile of fine-grid points (axis 3 fastest across the 256 threads) and the points it stages per pass
// through LDS.  Powers of two <= 8: every grid is whole tiles, g_i >= 8
constexpr unsigned kNufft3dTile1 = 4, kNufft3dTile2 = 8, kNufft3dTile3 = 8;
constexpr unsigned kNufft3dChunk = 128;

// N_i >= 1, G = g1 .. gD <= 2^28, 1 <= M <= 2^30, eps in [1e-14, 1e-1] (f64) or [1e-6, 1e-1] (f32), every coordinate finite.
// n, x: D entries each, axis 1 first.  The part that does not read the points (they may be in device memory: nufft_sort.hpp)
template <size_t D> bool nufft_nd_bad_sizes(const size_t *n, const double *const *x, size_t m, double eps, bool f32) {
    for (size_t i = 0; i < D; ++i)
        if (n[i] == 0 || n[i] > kNufftNdMaxGrid || !x[i]) return true;
    if (m == 0 || m > kNufftMaxPoints) return true;
    if (!(eps >= (f32 ? 1e-6 : 1e-14) && eps <= 1e-1)) return true;
    const int w = nufft_width(eps);
    unsigned long long room = kNufftNdMaxGrid;  // what the axes still to come may take: every g_i is a power of two <= 2^29
    for (size_t i = 0; i < D; ++i) {
        const unsigned long long g = nufft_grid(n[i], w);
        if (g > room) return true;
        room /= g;
    }
    return false;
}
template <size_t D> bool nufft_nd_bad_args(const size_t *n, const double *const *x, size_t m, double eps, bool f32) {
    if (nufft_nd_bad_sizes<D>(n, x, m, eps, f32)) return true;
    for (size_t j = 0; j < m; ++j)
        for (size_t i = 0; i < D; ++i)
            if (!std::isfinite(x[i][j])) return true;
    return false;
}

// Sorts the points by the combined cell (q1 g2 + q2) g3 + q3 (axis 1 most significant), q_i the top log_g_i bits of the
// coordinate mod 1: a stable counting sort, the original index the tie-break.  xs[a][i]: the i-th sorted position along axis a
// in turns; perm[i]: its original index; cell_start[q] .. cell_start[q + 1]: the sorted range of cell q (G + 1 entries).
template <size_t D>
void nufft_nd_bin(const double *const *x, size_t m, const unsigned *log_g, double *const *xs, uint32_t *perm, uint32_t *cell_start) {
    unsigned log_cells = 0;
    for (size_t a = 0; a < D; ++a) log_cells += log_g[a];
    const size_t cells = (size_t)1 << log_cells;
    std::vector<uint32_t> cell(m);
    for (size_t q = 0; q <= cells; ++q) cell_start[q] = 0;
    for (size_t j = 0; j < m; ++j) {
        uint32_t q = 0;
        for (size_t a = 0; a < D; ++a) q = (q << log_g[a]) | (uint32_t)(czt_frac(x[a][j], 0).hi >> (64 - log_g[a]));
        cell[j] = q;
        ++cell_start[q + 1];
    }
    for (size_t q = 0; q < cells; ++q) cell_start[q + 1] += cell_start[q];
    std::vector<uint32_t> at(cell_start, cell_start + cells);
    for (size_t j = 0; j < m; ++j) {
        const uint32_t i = at[cell[j]]++;
        perm[i] = (uint32_t)j;
        for (size_t a = 0; a < D; ++a) xs[a][i] = nufft_turns(czt_frac(x[a][j], 0));
    }
}

}  // namespace phast

#if defined(__HIPCC__)
namespace phast {

// one launch of one of the four kernels over `c` transforms (nufft_nd.hip); G = g1 .. gD.  The arrays have axis 1 first
template <size_t D> struct NufftNdArgs {
    const void *in_re;  // spread / pre: the caller's planes (transform b at b * in_dist); deconvolve / interpolate: the
    const void *in_im;  // workspace (b * G).  spread / pre: null for real data
    void *out_re;       // spread / pre: the workspace; deconvolve / interpolate: the caller's planes (b * out_dist)
    void *out_im;
    const double *xs[D];         // [M] sorted positions per axis, turns in [0, 1)
    const uint32_t *perm;        // [M] original index of sorted point i
    const uint32_t *cell_start;  // [G + 1], cell (q1 g2 + q2) g3 + q3
    const void *inv[D];          // [N_i]: 1 / phi^(k_i(m_i)) on g_i points, rounded to T
    unsigned long long in_dist, out_dist;
    unsigned long long n[D], m;  // N1 x .. x ND modes, M points
    unsigned long long groups;   // spread: c G threads (3-D: a tile per workgroup); interpolate: c M; pre: c G / V groups; deconvolve: c gpt
    unsigned long long g0;       // first group of this launch (launches split at 2^31 - 1 workgroups)
    unsigned log_g[D];           // g_i = 2^log_g_i
    unsigned gpt;                // deconvolve: groups per transform, N1 .. N(D-1) ceil(ND / V)
    int w;                       // kernel width in cells
};
// kind: 0 spread (2-D: one thread per grid point; 3-D: a tile of 256 grid points per workgroup), 1 interpolate (one thread per
// point; both element accesses); 2 pre, 3 deconvolve (streaming sweeps along the last axis; `vec`: the caller's planes AND the
// workspace allow 16-byte accesses)
template <typename T, size_t D> hipError_t launch_nufft_nd(int kind, bool vec, const NufftNdArgs<D> &a, hipStream_t stream);

}  // namespace phast
#endif
