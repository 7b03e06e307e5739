// nufft3d.hpp -- non-uniform FFTs of types 1 and 2 in three dimensions.  M points (x_j, y_j, z_j) in turns (reduced
// mod 1 per coordinate), N1 x N2 x N3 modes, row-major (index (m1 N2 + m2) N3 + m3), each axis in numpy fftfreq order; k1 pairs with
// x, k2 with y, k3 with z:
//
//     type 1 (points -> modes)   F[m1, m2, m3] = sum_j c_j exp(-+2 pi i (k1(m1) x_j + k2(m2) y_j + k3(m3) z_j))
//     type 2 (modes -> points)   c_j = sum_m F[m1, m2, m3] exp(-+2 pi i (k1(m1) x_j + k2(m2) y_j + k3(m3) z_j))   (- Forward, + Reverse)
//
// The schedule is nufft.hpp's, per axis: the same width w, beta, kernel value (nufft_weight), support (nufft_first), slot
// (nufft_slot) and quadrature (NufftQuad), on a fine grid of g1 x g2 x g3 points, g_i = nufft_grid(N_i, w):
//
//     stage   type 1                                                  type 2
//     a       spread with the product kernel (phi1 phi2) phi3         pre: g^[slot1, slot2, slot3] = F inv1 inv2 inv3, 0 elsewhere
//     b       the 3-D FFT of (g1, g2, g3) in place (NdPlanner, always Forward: Reverse swaps the planes)
//     c       deconvolve  F = g^[slot1, slot2, slot3] inv1 inv2 inv3  interpolate over the w^3 grid points under a point
//
// The points are sorted once, on the host, by the combined cell (q1 g2 + q2) g3 + q3, so the cells (r1, r2, a .. b) of one pair of
// cell rows are one contiguous run of the sorted tables.  Spreading is a gather by TILES of the fine grid (nufft3d.hip): a
// workgroup owns kNufft3dTile1 x kNufft3dTile2 x kNufft3dTile3 grid points, stages the points of the cells round the tile through
// LDS kNufft3dChunk at a time and forms their kernel values once for the whole tile.
//
// The top of this header has no HIP dependency: tests/test_nufft3d_cpu.py compiles it with g++.
#pragma once

#include "nufft.hpp"

namespace phast {

constexpr unsigned long long kNufft3dMaxGrid = 1ull << 28;  // G = g1 g2 g3: cell_start stays below 1 GiB
// the spread kernel's tile of fine-grid points (axis 3 fastest across the 256 threads) and the points it stages per pass through
// LDS.  Powers of two <= 8: every grid is whole tiles, g_i >= 8
constexpr unsigned kNufft3dTile1 = 4, kNufft3dTile2 = 8, kNufft3dTile3 = 8;
constexpr unsigned kNufft3dChunk = 128;

// N_i >= 1, G = g1 g2 g3 <= 2^28, 1 <= M <= 2^30, eps in [1e-14, 1e-1] (f64) or [1e-6, 1e-1] (f32), every coordinate finite
// the part that does not read the points (they may be in device memory: nufft_sort.hpp)
inline bool nufft3d_bad_sizes(unsigned long long n1, unsigned long long n2, unsigned long long n3, unsigned long long m, const double *x,
                              const double *y, const double *z, double eps, bool f32) {
    if (n1 == 0 || n2 == 0 || n3 == 0 || n1 > kNufft3dMaxGrid || n2 > kNufft3dMaxGrid || n3 > kNufft3dMaxGrid) return true;
    if (m == 0 || m > kNufftMaxPoints || !x || !y || !z) return true;
    if (!(eps >= (f32 ? 1e-6 : 1e-14) && eps <= 1e-1)) return true;
    const int w = nufft_width(eps);
    // each is a power of two <= 2^29: neither quotient nor comparison overflows
    const unsigned long long room = kNufft3dMaxGrid / nufft_grid(n1, w);
    return room == 0 || nufft_grid(n2, w) > room || nufft_grid(n3, w) > room / nufft_grid(n2, w);
}
inline bool nufft3d_bad_args(unsigned long long n1, unsigned long long n2, unsigned long long n3, unsigned long long m, const double *x,
                             const double *y, const double *z, double eps, bool f32) {
    if (nufft3d_bad_sizes(n1, n2, n3, m, x, y, z, eps, f32)) return true;
    for (unsigned long long j = 0; j < m; ++j)
        if (!std::isfinite(x[j]) || !std::isfinite(y[j]) || !std::isfinite(z[j])) return true;
    return false;
}

// Sorts the points by the combined cell (q1 g2 + q2) g3 + q3, q_i the top log_g_i bits of the coordinate mod 1: a stable counting
// sort, the original index the tie-break.  xs[i], ys[i], zs[i]: the i-th sorted position in turns; perm[i]: its original index;
// cell_start[q] .. cell_start[q + 1]: the sorted range of cell q (g1 g2 g3 + 1 entries).
inline void nufft3d_bin(const double *x, const double *y, const double *z, size_t m, unsigned log_g1, unsigned log_g2, unsigned log_g3,
                        double *xs, double *ys, double *zs, uint32_t *perm, uint32_t *cell_start) {
    const size_t cells = (size_t)1 << (log_g1 + log_g2 + log_g3);
    std::vector<uint32_t> cell(m);
    for (size_t q = 0; q <= cells; ++q) cell_start[q] = 0;
    for (size_t j = 0; j < m; ++j) {
        const uint32_t q1 = (uint32_t)(czt_frac(x[j], 0).hi >> (64 - log_g1)), q2 = (uint32_t)(czt_frac(y[j], 0).hi >> (64 - log_g2));
        const uint32_t q3 = (uint32_t)(czt_frac(z[j], 0).hi >> (64 - log_g3));
        cell[j] = (((q1 << log_g2) | q2) << log_g3) | q3;
        ++cell_start[cell[j] + 1];
    }
    for (size_t q = 0; q < cells; ++q) cell_start[q + 1] += cell_start[q];
    std::vector<uint32_t> at(cell_start, cell_start + cells);
    for (size_t j = 0; j < m; ++j) {
        const uint32_t i = at[cell[j]]++;
        perm[i] = (uint32_t)j;
        xs[i] = nufft_turns(czt_frac(x[j], 0));
        ys[i] = nufft_turns(czt_frac(y[j], 0));
        zs[i] = nufft_turns(czt_frac(z[j], 0));
    }
}

}  // namespace phast

#if defined(__HIPCC__)
namespace phast {

// one launch of one of the four kernels over `c` transforms (nufft3d.hip); G = g1 g2 g3
struct Nufft3dArgs {
    const void *in_re;  // spread / pre: the caller's planes (transform b at b * in_dist); deconvolve / interpolate: the
    const void *in_im;  // workspace (b * G).  spread / pre: null for real data
    void *out_re;       // spread / pre: the workspace; deconvolve / interpolate: the caller's planes (b * out_dist)
    void *out_im;
    const double *xs, *ys, *zs;      // [M] sorted positions, turns in [0, 1)
    const uint32_t *perm;            // [M] original index of sorted point i
    const uint32_t *cell_start;      // [G + 1], cell (q1 g2 + q2) g3 + q3
    const void *inv1, *inv2, *inv3;  // [N1], [N2], [N3]: 1 / phi^(k_i(m_i)) on g_i points, rounded to T
    unsigned long long in_dist, out_dist;
    unsigned long long n1, n2, n3, m;  // N1 x N2 x N3 modes, M points
    unsigned long long groups;         // spread: c G threads (a tile per workgroup); interpolate: c M; pre: c G / V groups; deconvolve: c gpt
    unsigned long long g0;             // first group of this launch (launches split at 2^31 - 1 workgroups)
    unsigned log_g1, log_g2, log_g3;   // g_i = 2^log_g_i
    unsigned gpt;                      // deconvolve: groups per transform, N1 N2 ceil(N3 / V)
    int w;                             // kernel width in cells
};
// kind: 0 spread (a tile of 256 grid points per workgroup), 1 interpolate (one thread per point; both element accesses); 2 pre,
// 3 deconvolve (streaming sweeps along axis 3; `vec`: the caller's planes AND the workspace allow 16-byte accesses)
template <typename T> hipError_t launch_nufft3d(int kind, bool vec, const Nufft3dArgs &a, hipStream_t stream);

}  // namespace phast
#endif
