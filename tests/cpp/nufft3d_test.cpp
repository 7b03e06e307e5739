// nufft3d_test.cpp -- the host half of csrc/nufft_nd.hpp at D = 3 behind a C interface: the argument check, the binning by the
// combined cell and the constants of the spread kernel's tile.  Plain g++, no HIP: tests/test_nufft3d_cpu.py builds it as a
// shared library and holds both against Python integers.
#include "nufft_nd.hpp"

extern "C" {

int nufft3d_t_bad_args(unsigned long long n1, unsigned long long n2, unsigned long long n3, unsigned long long m, const double *x,
                       const double *y, const double *z, double eps, int f32) {
    const size_t n[3] = {(size_t)n1, (size_t)n2, (size_t)n3};
    const double *const p[3] = {x, y, z};
    return phast::nufft_nd_bad_args<3>(n, p, (size_t)m, eps, f32 != 0);
}
void nufft3d_t_bin(const double *x, const double *y, const double *z, size_t m, unsigned log_g1, unsigned log_g2, unsigned log_g3,
                   double *xs, double *ys, double *zs, uint32_t *perm, uint32_t *cell_start) {
    const double *const p[3] = {x, y, z};
    const unsigned log_g[3] = {log_g1, log_g2, log_g3};
    double *const s[3] = {xs, ys, zs};
    phast::nufft_nd_bin<3>(p, m, log_g, s, perm, cell_start);
}
// (tile extent on axis 1, 2, 3, points per pass through LDS)
void nufft3d_t_tile(unsigned *out) {
    out[0] = phast::kNufft3dTile1;
    out[1] = phast::kNufft3dTile2;
    out[2] = phast::kNufft3dTile3;
    out[3] = phast::kNufft3dChunk;
}
}
