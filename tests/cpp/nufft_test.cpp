// nufft_test.cpp -- the host half of csrc/nufft.hpp behind a C interface: the argument check, the width and grid rules, the
// quadrature of phi^, the truncated position and the binning.  Plain g++, no HIP: tests/test_nufft_cpu.py builds it as a shared
// library and holds every function against Python integers and numpy.
#include "nufft.hpp"

extern "C" {

int nufft_t_bad_args(unsigned long long n, unsigned long long m, const double *x, double eps, int f32) {
    return phast::nufft_bad_args(n, m, x, eps, f32 != 0);
}
int nufft_t_width(double eps) { return phast::nufft_width(eps); }
unsigned long long nufft_t_grid(unsigned long long n, int w) { return phast::nufft_grid(n, w); }
unsigned long long nufft_t_slot(unsigned long long m, unsigned long long n, unsigned long long grid) { return phast::nufft_slot(m, n, grid); }
long long nufft_t_first(int w, double t) { return phast::nufft_first(w, t); }
double nufft_t_turns(double x) { return phast::nufft_turns(phast::czt_frac(x, 0)); }
double nufft_t_weight(long long dq, double t, int w) { return phast::nufft_weight<double>(dq, t, 2.0 / w, phast::nufft_beta(w)); }
// out[i] = phi^(k[i]) on a grid of `grid` points
void nufft_t_phi_hat(int w, unsigned long long grid, const long long *k, size_t count, double *out) {
    const phast::NufftQuad hat(w, grid);
    for (size_t i = 0; i < count; ++i) out[i] = hat(k[i]);
}
void nufft_t_bin(const double *x, size_t m, unsigned log_g, double *xs, uint32_t *perm, uint32_t *cell_start) {
    phast::nufft_bin(x, m, log_g, xs, perm, cell_start);
}
}
