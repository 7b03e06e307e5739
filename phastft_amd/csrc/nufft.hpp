// nufft.hpp -- non-uniform FFTs of types 1 and 2 in one dimension.  M points x_j in turns (reduced mod 1),
// N modes in numpy fftfreq order, k(m) = m for m < ceil(N / 2) and m - N otherwise:
//
//     type 1 (points -> modes)   F[m] = sum_j c_j exp(-+2 pi i k(m) x_j)
//     type 2 (modes -> points)   c_j  = sum_m F[m] exp(-+2 pi i k(m) x_j)        (- Forward, + Reverse; no scaling)
//
// through a fine grid of n_g = 2^ceil(log2 max(2N, 2w, 8)) points and the "exponential of semicircle" kernel
// phi(z) = exp(beta (sqrt(1 - z^2) - 1)) on |z| < 1, w grid cells wide, beta = 2.30 w:
//
//     stage   type 1                                              type 2
//     a       spread    g[l] = sum_j phi(2 (l - n_g x_j) / w) c_j       pre       g^[k mod n_g] = F[m] / phi^(k), 0 elsewhere
//     b       FFT_{n_g} in place on the engine (the swap trick gives the + sign)
//     c       deconvolve  F[m] = g^[k mod n_g] / phi^(k)                interpolate  c_j = sum_l phi(2 (l - n_g x_j) / w) g[l]
//
// No floating-point atomics: the points are sorted by grid cell once, on the host, and the spread kernel GATHERS -- one thread
// per grid point walks the points of the cells within ceil(w / 2) of it in sorted order.  With n_g a power of two the exact
// fraction of a turn of czt.hpp IS the grid position: the cell is its top log2 n_g bits.
//
// The top of this header has no HIP dependency: tests/test_nufft_cpu.py compiles it with g++.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "czt.hpp"  // CztFrac, czt_frac: x mod 1 exactly

namespace phast {

constexpr unsigned long long kNufftMaxModes = 1ull << 28;   // n_g = 2^29 at most: inside the f64 engine's 2^30
constexpr unsigned long long kNufftMaxPoints = 1ull << 30;  // perm and cell_start are 32-bit
constexpr int kNufftMinWidth = 2, kNufftMaxWidth = 16;

// w = clamp(ceil(log10(1 / eps)) + 1, 2, 16).  A decade that log10 returns a hair off an integer counts as that integer.
inline int nufft_width(double eps) {
    double d = -std::log10(eps);
    const double r = std::nearbyint(d);
    if (std::fabs(d - r) < 1e-9) d = r;
    const int w = (int)std::ceil(d) + 1;
    return w < kNufftMinWidth ? kNufftMinWidth : w > kNufftMaxWidth ? kNufftMaxWidth : w;
}

PHAST_HD double nufft_beta(int w) { return 2.30 * w; }

// the fine grid: the smallest power of two >= max(2N, 2w, 8).  >= 2w: a point never meets a grid point twice across the wrap
inline unsigned long long nufft_grid(unsigned long long n, int w) {
    unsigned long long g = 8;
    while (g < 2 * n || g < 2ull * w) g <<= 1;
    return g;
}

// 1 <= N <= 2^28, 1 <= M <= 2^30, eps in [1e-14, 1e-1] (f64) or [1e-6, 1e-1] (f32), every x_j finite
// the part that does not read the points (they may be in device memory: nufft_sort.hpp)
inline bool nufft_bad_sizes(unsigned long long n, unsigned long long m, const double *x, double eps, bool f32) {
    if (n == 0 || n > kNufftMaxModes || m == 0 || m > kNufftMaxPoints || !x) return true;
    return !(eps >= (f32 ? 1e-6 : 1e-14) && eps <= 1e-1);
}
inline bool nufft_bad_args(unsigned long long n, unsigned long long m, const double *x, double eps, bool f32) {
    if (nufft_bad_sizes(n, m, x, eps, f32)) return true;
    for (unsigned long long j = 0; j < m; ++j)
        if (!std::isfinite(x[j])) return true;
    return false;
}

// phi at z^2 = z2 (0 outside the support), evaluated in R = double or float
template <typename R> PHAST_HD R nufft_phi(R z2, R beta) {
    if (!(z2 < R(1))) return R(0);
    if constexpr (sizeof(R) == 8)
        return exp(beta * (sqrt(R(1) - z2) - R(1)));
    else
        return expf(beta * (sqrtf(R(1) - z2) - R(1)));
}

// A sorted position p = n_g x in [0, n_g) as (cell, offset in [0, 1)): exact, n_g being a power of two and x < 1
PHAST_HD long long nufft_cell(double x, double grid, double *t) {
    const double p = x * grid;
    const long long q = (long long)p;
    *t = p - (double)q;
    return q;
}

// One kernel value: the grid point `dq` cells above the cell of a point at in-cell offset t lies dq - t cells from it.  The
// spread and the interpolation kernels both come through here, so type 2 Reverse is the adjoint of type 1 Forward to rounding.
template <typename R> PHAST_HD R nufft_weight(long long dq, double t, double two_over_w, R beta) {
    const double z = ((double)dq - t) * two_over_w;
    return nufft_phi<R>((R)(z * z), beta);
}

// the first of the w grid points under a point at (q, t), relative to q: every l with |l - q - t| < w / 2 is among
// q + first .. q + first + w - 1 (the one that may lie exactly on the edge of the support has phi = 0)
PHAST_HD long long nufft_first(int w, double t) {
    const int h = (w + 1) / 2;
    return 1 - h + ((w & 1) && t >= 0.5 ? 1 : 0);
}

// the grid slot of mode index m < N (k >= 0 at the bottom, k < 0 at the top)
PHAST_HD unsigned long long nufft_slot(unsigned long long m, unsigned long long n, unsigned long long grid) {
    return m < (n + 1) / 2 ? m : m + grid - n;
}

// a fraction of a turn as a double in [0, 1), TRUNCATED to 53 significant bits (rounding could reach 1.0); the top
// log2 n_g <= 29 bits -- the cell -- are kept whatever the leading zeros.  The double is put together from its bits (the 53
// leading bits of the fraction, the exponent from the count of zeros above them), so host and device code share it
PHAST_HD double nufft_turns(CztFrac f) {
    unsigned long long hi = f.hi, lo = f.lo;
    int exp2 = 0;
    if (hi == 0) {
        hi = lo;
        lo = 0;
        exp2 = -64;
    }
    if (hi == 0) return 0.0;
    const int lz = __builtin_clzll(hi);
    if (lz) hi = (hi << lz) | (lo >> (64 - lz));
    // (hi >> 11) 2^(exp2 - lz - 53) with hi >> 11 in [2^52, 2^53): the exponent field is 1022 + exp2 - lz >= 895
    const unsigned long long bits = ((unsigned long long)(1022 + exp2 - lz) << 52) | ((hi >> 11) & 0xfffffffffffffull);
    double r;
    __builtin_memcpy(&r, &bits, sizeof r);
    return r;
}

// Gauss-Legendre nodes and weights on [-1, 1] (Newton's iteration on P_n from the Chebyshev guess)
inline void nufft_gauss_legendre(int n, std::vector<double> &x, std::vector<double> &wt) {
    x.assign(n, 0.0);
    wt.assign(n, 0.0);
    const double pi = 3.141592653589793238462643383279502884;
    for (int i = 0; i < (n + 1) / 2; ++i) {
        double z = std::cos(pi * (i + 0.75) / (n + 0.5)), dp = 1;
        for (int it = 0; it < 100; ++it) {
            double p0 = 1, p1 = z;
            for (int k = 2; k <= n; ++k) {
                const double p2 = ((2 * k - 1) * z * p1 - (k - 1) * p0) / k;
                p0 = p1;
                p1 = p2;
            }
            dp = n * (z * p1 - p0) / (z * z - 1);
            const double dz = p1 / dp;
            z -= dz;
            if (std::fabs(dz) < 1e-16) break;
        }
        x[i] = -z;
        x[n - 1 - i] = z;
        wt[i] = wt[n - 1 - i] = 2 / ((1 - z * z) * dp * dp);
    }
}

// phi^(k), the Fourier transform of the kernel on the fine grid,
//     phi^(k) = int_{-w/2}^{w/2} phi(2 t / w) cos(2 pi k t / n_g) dt = w int_0^{pi/2} e^{beta (cos th - 1)} cos(a sin th) cos th dth,
// a = pi w k / n_g, by Gauss-Legendre quadrature in th: z = sin th takes the square-root ends of phi away, the integrand in
// th is entire and the rule converges geometrically.  kNufftQuadNodes nodes leave < 1e-14 of phi^(0) for every w <= 16 and
// |k| <= n_g / 4 (tests/test_nufft_cpu.py holds it against a tanh-sinh trapezoid sum).
constexpr int kNufftQuadNodes = 32;
struct NufftQuad {
    std::vector<double> s, f;  // sin th_i and w wt_i e^{beta (cos th_i - 1)} cos th_i
    double a1 = 0;             // pi w / n_g
    NufftQuad(int w, unsigned long long grid) {
        std::vector<double> x, wt;
        nufft_gauss_legendre(kNufftQuadNodes, x, wt);
        const double q = 0.78539816339744830961566084581987572, beta = nufft_beta(w);  // pi / 4
        for (int i = 0; i < kNufftQuadNodes; ++i) {
            const double th = q * (x[i] + 1);
            s.push_back(std::sin(th));
            f.push_back((double)w * q * wt[i] * std::exp(beta * (std::cos(th) - 1)) * std::cos(th));
        }
        a1 = 4 * q * (double)w / (double)grid;
    }
    double operator()(long long k) const { return at((double)k); }
    // the same rule at a real argument: phi^ at k / n_g turns per cell, |k| <= n_g / 4 (nufft_t3.hpp)
    double at(double k) const {
        const double a = a1 * k;
        double acc = 0;
        for (size_t i = 0; i < s.size(); ++i) acc += f[i] * std::cos(a * s[i]);
        return acc;
    }
};

// Sorts the points by grid cell: a stable counting sort on the top log_g bits of x_j mod 1, the original index the tie-break.
// xs[i]: the i-th sorted position in turns; perm[i]: its original index; cell_start[q] .. cell_start[q + 1]: the sorted
// range of cell q (n_g + 1 entries).
inline void nufft_bin(const double *x, size_t m, unsigned log_g, double *xs, uint32_t *perm, uint32_t *cell_start) {
    const size_t grid = (size_t)1 << log_g;
    std::vector<uint32_t> cell(m);
    for (size_t q = 0; q <= grid; ++q) cell_start[q] = 0;
    for (size_t j = 0; j < m; ++j) {
        cell[j] = (uint32_t)(czt_frac(x[j], 0).hi >> (64 - log_g));
        ++cell_start[cell[j] + 1];
    }
    for (size_t q = 0; q < grid; ++q) cell_start[q + 1] += cell_start[q];
    std::vector<uint32_t> at(cell_start, cell_start + grid);
    for (size_t j = 0; j < m; ++j) {
        const uint32_t i = at[cell[j]]++;
        perm[i] = (uint32_t)j;
        xs[i] = nufft_turns(czt_frac(x[j], 0));
    }
}

}  // namespace phast

#if defined(__HIPCC__)
#include "any_len.hpp"

namespace phast {

// one launch of one of the four kernels over `c` transforms (nufft.hip)
struct NufftArgs {
    const void *in_re;  // spread / pre: the caller's planes (transform b at b * in_dist); deconvolve / interpolate: the
    const void *in_im;  // workspace (b * n_g).  spread / pre: null for real data
    void *out_re;       // spread / pre: the workspace; deconvolve / interpolate: the caller's planes (b * out_dist)
    void *out_im;
    const double *xs;            // [M] sorted positions, turns in [0, 1)
    const uint32_t *perm;        // [M] original index of sorted point i
    const uint32_t *cell_start;  // [n_g + 1]
    const void *inv_hat;         // [N] 1 / phi^(k(m)), rounded to T
    unsigned long long in_dist, out_dist;
    unsigned long long n, m;    // N modes, M points
    unsigned long long groups;  // spread: c n_g threads; interpolate: c M; pre: c n_g / V groups; deconvolve: c gpt
    unsigned long long g0;      // first group of this launch (launches split at 2^31 - 1 workgroups)
    unsigned log_g;             // n_g = 2^log_g
    unsigned gpt;               // deconvolve: groups per transform, ceil(N / V)
    int w;                      // kernel width in cells
};
// kind: 0 spread, 1 interpolate (one thread per element, element accesses); 2 pre, 3 deconvolve (streaming sweeps; `vec`:
// the caller's planes AND the workspace allow 16-byte accesses)
template <typename T> hipError_t launch_nufft(int kind, bool vec, const NufftArgs &a, hipStream_t stream);

// the type the kernel values and the sums of spread and interpolate are formed in
template <typename T> struct NufftReal { typedef double type; };
template <> struct NufftReal<float> { typedef float type; };

// the signed distance l - q of two cells around a ring of mask + 1 cells, in [-(mask + 1) / 2, (mask + 1) / 2)
__device__ inline long long nufft_ring(unsigned long long l, long long q, unsigned long long mask) {
    const long long half = (long long)((mask + 1) >> 1);
    return (long long)(((unsigned long long)((long long)l - q + half)) & mask) - half;
}

}  // namespace phast
#endif
