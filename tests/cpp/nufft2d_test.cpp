// nufft2d_test.cpp -- the host half of csrc/nufft2d.hpp behind a C interface: the argument check and the binning by the
// combined cell.  Plain g++, no HIP: tests/test_nufft2d_cpu.py builds it as a shared library and holds both against Python
// integers.
#include "nufft2d.hpp"

extern "C" {

int nufft2d_t_bad_args(unsigned long long n1, unsigned long long n2, unsigned long long m, const double *x, const double *y,
                       double eps, int f32) {
    return phast::nufft2d_bad_args(n1, n2, m, x, y, eps, f32 != 0);
}
void nufft2d_t_bin(const double *x, const double *y, size_t m, unsigned log_g1, unsigned log_g2, double *xs, double *ys,
                   uint32_t *perm, uint32_t *cell_start) {
    phast::nufft2d_bin(x, y, m, log_g1, log_g2, xs, ys, perm, cell_start);
}
}
