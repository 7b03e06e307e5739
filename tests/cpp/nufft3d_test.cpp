// nufft3d_test.cpp -- the host half of csrc/nufft3d.hpp behind a C interface: the argument check, the binning by the combined
// cell and the constants of the spread kernel's tile.  Plain g++, no HIP: tests/test_nufft3d_cpu.py builds it as a shared library
// and holds both against Python integers.
#include "nufft3d.hpp"

extern "C" {

int nufft3d_t_bad_args(unsigned long long n1, unsigned long long n2, unsigned long long n3, unsigned long long m, const double *x,
                       const double *y, const double *z, double eps, int f32) {
    return phast::nufft3d_bad_args(n1, n2, n3, m, x, y, z, eps, f32 != 0);
}
void nufft3d_t_bin(const double *x, const double *y, const double *z, size_t m, unsigned log_g1, unsigned log_g2, unsigned log_g3,
                   double *xs, double *ys, double *zs, uint32_t *perm, uint32_t *cell_start) {
    phast::nufft3d_bin(x, y, z, m, log_g1, log_g2, log_g3, xs, ys, zs, perm, cell_start);
}
// (tile extent on axis 1, 2, 3, points per pass through LDS)
void nufft3d_t_tile(unsigned *out) {
    out[0] = phast::kNufft3dTile1;
    out[1] = phast::kNufft3dTile2;
    out[2] = phast::kNufft3dTile3;
    out[3] = phast::kNufft3dChunk;
}
}
