// nufft2d.hpp -- non-uniform FFTs of types 1 and 2 in two dimensions.  M points (x_j, y_j) in turns (reduced mod 1
// per coordinate), N1 x N2 modes, row-major (index m1 N2 + m2), each axis in numpy fftfreq order; k1 pairs with x, k2 with y:
//
//     type 1 (points -> modes)   F[m1, m2] = sum_j c_j exp(-+2 pi i (k1(m1) x_j + k2(m2) y_j))
//     type 2 (modes -> points)   c_j = sum_{m1, m2} F[m1, m2] exp(-+2 pi i (k1(m1) x_j + k2(m2) y_j))     (- Forward, + Reverse)
//
// The schedule is nufft.hpp's, per axis: the same width w, beta, kernel value (nufft_weight), support (nufft_first), slot
// (nufft_slot) and quadrature (NufftQuad), on a fine grid of g1 x g2 points, g_i = nufft_grid(N_i, w):
//
//     stage   type 1                                                  type 2
//     a       spread with the product kernel phi1 phi2                pre: g^[slot1, slot2] = F inv1 inv2, 0 elsewhere
//     b       the 2-D FFT of (g1, g2) in place (NdPlanner, always Forward: Reverse swaps the planes)
//     c       deconvolve  F = g^[slot1, slot2] inv1 inv2              interpolate over the w x w grid points under a point
//
// The points are sorted once, on the host, by the combined cell q1 g2 + q2, so the cells (r, a .. b) of one cell row are one
// contiguous run of the sorted tables and spreading is a gather, as in one dimension.
//
// The top of this header has no HIP dependency: tests/test_nufft2d_cpu.py compiles it with g++.
#pragma once

#include "nufft.hpp"

namespace phast {

constexpr unsigned long long kNufft2dMaxGrid = 1ull << 28;  // G = g1 g2: cell_start stays below 1 GiB, one f64 transform below 8 GiB

// N1, N2 >= 1, G = g1 g2 <= 2^28, 1 <= M <= 2^30, eps in [1e-14, 1e-1] (f64) or [1e-6, 1e-1] (f32), every coordinate finite
// the part that does not read the points (they may be in device memory: nufft_sort.hpp)
inline bool nufft2d_bad_sizes(unsigned long long n1, unsigned long long n2, unsigned long long m, const double *x, const double *y,
                              double eps, bool f32) {
    if (n1 == 0 || n2 == 0 || n1 > kNufft2dMaxGrid || n2 > kNufft2dMaxGrid) return true;
    if (m == 0 || m > kNufftMaxPoints || !x || !y) return true;
    if (!(eps >= (f32 ? 1e-6 : 1e-14) && eps <= 1e-1)) return true;
    const int w = nufft_width(eps);
    return nufft_grid(n1, w) > kNufft2dMaxGrid / nufft_grid(n2, w);  // both are powers of two <= 2^29
}
inline bool nufft2d_bad_args(unsigned long long n1, unsigned long long n2, unsigned long long m, const double *x, const double *y,
                             double eps, bool f32) {
    if (nufft2d_bad_sizes(n1, n2, m, x, y, eps, f32)) return true;
    for (unsigned long long j = 0; j < m; ++j)
        if (!std::isfinite(x[j]) || !std::isfinite(y[j])) return true;
    return false;
}

// Sorts the points by the combined cell q1 g2 + q2, q_i the top log_g_i bits of the coordinate mod 1: a stable counting sort,
// the original index the tie-break.  xs[i], ys[i]: the i-th sorted position in turns; perm[i]: its original index;
// cell_start[q] .. cell_start[q + 1]: the sorted range of cell q (g1 g2 + 1 entries).
inline void nufft2d_bin(const double *x, const double *y, size_t m, unsigned log_g1, unsigned log_g2, double *xs, double *ys,
                        uint32_t *perm, uint32_t *cell_start) {
    const size_t cells = (size_t)1 << (log_g1 + log_g2);
    std::vector<uint32_t> cell(m);
    for (size_t q = 0; q <= cells; ++q) cell_start[q] = 0;
    for (size_t j = 0; j < m; ++j) {
        const uint32_t q1 = (uint32_t)(czt_frac(x[j], 0).hi >> (64 - log_g1)), q2 = (uint32_t)(czt_frac(y[j], 0).hi >> (64 - log_g2));
        cell[j] = (q1 << log_g2) | q2;
        ++cell_start[cell[j] + 1];
    }
    for (size_t q = 0; q < cells; ++q) cell_start[q + 1] += cell_start[q];
    std::vector<uint32_t> at(cell_start, cell_start + cells);
    for (size_t j = 0; j < m; ++j) {
        const uint32_t i = at[cell[j]]++;
        perm[i] = (uint32_t)j;
        xs[i] = nufft_turns(czt_frac(x[j], 0));
        ys[i] = nufft_turns(czt_frac(y[j], 0));
    }
}

}  // namespace phast

#if defined(__HIPCC__)
namespace phast {

// one launch of one of the four kernels over `c` transforms (nufft2d.hip); G = g1 g2
struct Nufft2dArgs {
    const void *in_re;  // spread / pre: the caller's planes (transform b at b * in_dist); deconvolve / interpolate: the
    const void *in_im;  // workspace (b * G).  spread / pre: null for real data
    void *out_re;       // spread / pre: the workspace; deconvolve / interpolate: the caller's planes (b * out_dist)
    void *out_im;
    const double *xs, *ys;       // [M] sorted positions, turns in [0, 1)
    const uint32_t *perm;        // [M] original index of sorted point i
    const uint32_t *cell_start;  // [G + 1], cell q1 g2 + q2
    const void *inv1, *inv2;     // [N1], [N2]: 1 / phi^(k_i(m_i)) on g_i points, rounded to T
    unsigned long long in_dist, out_dist;
    unsigned long long n1, n2, m;  // N1 x N2 modes, M points
    unsigned long long groups;     // spread: c G threads; interpolate: c M; pre: c G / V groups; deconvolve: c gpt
    unsigned long long g0;         // first group of this launch (launches split at 2^31 - 1 workgroups)
    unsigned log_g1, log_g2;       // g_i = 2^log_g_i
    unsigned gpt;                  // deconvolve: groups per transform, N1 ceil(N2 / V)
    int w;                         // kernel width in cells
};
// kind: 0 spread, 1 interpolate (one thread per element, element accesses); 2 pre, 3 deconvolve (streaming sweeps along axis 2;
// `vec`: the caller's planes AND the workspace allow 16-byte accesses)
template <typename T> hipError_t launch_nufft2d(int kind, bool vec, const Nufft2dArgs &a, hipStream_t stream);

}  // namespace phast
#endif
