// nufft2d_test.cpp -- the host half of csrc/nufft_nd.hpp at D = 2 behind a C interface: the argument check and the binning by
// the combined cell.  Plain g++, no HIP: tests/test_nufft2d_cpu.py builds it as a shared library and holds both against Python
// integers.
#include "nufft_nd.hpp"

extern "C" {

int nufft2d_t_bad_args(unsigned long long n1, unsigned long long n2, unsigned long long m, const double *x, const double *y,
                       double eps, int f32) {
    const size_t n[2] = {(size_t)n1, (size_t)n2};
    const double *const p[2] = {x, y};
    return phast::nufft_nd_bad_args<2>(n, p, (size_t)m, eps, f32 != 0);
}
void nufft2d_t_bin(const double *x, const double *y, size_t m, unsigned log_g1, unsigned log_g2, double *xs, double *ys,
                   uint32_t *perm, uint32_t *cell_start) {
    const double *const p[2] = {x, y};
    const unsigned log_g[2] = {log_g1, log_g2};
    double *const s[2] = {xs, ys};
    phast::nufft_nd_bin<2>(p, m, log_g, s, perm, cell_start);
}
}
