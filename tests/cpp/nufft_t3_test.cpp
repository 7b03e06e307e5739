// nufft_t3_test.cpp -- the host half of csrc/nufft_t3.hpp behind a C interface: the argument check, the grid rule, the
// positions and targets, the exact phases, the two tables and phi^ at a real argument.  Plain g++, no HIP:
// tests/test_nufft_t3_cpu.py builds it as a shared library and holds every function against Python fractions and numpy.
#include "nufft_t3.hpp"

extern "C" {

int nufft_t3_t_bad_args(const double *x, unsigned long long m, const double *s, unsigned long long k, double eps, int f32) {
    return phast::nufft_t3_bad_args(x, m, s, k, eps, f32 != 0);
}
// out: cx, cs, X, S, h; returns n_f (0: none); *w the width
unsigned long long nufft_t3_t_grid(const double *x, unsigned long long m, const double *s, unsigned long long k, double eps,
                                   double *out, int *w) {
    const phast::NufftT3Grid g = phast::nufft_t3_grid(x, m, s, k, eps);
    out[0] = g.cx, out[1] = g.cs, out[2] = g.X, out[3] = g.S, out[4] = g.h;
    *w = g.w;
    return g.nf;
}
// u[M]: the sources as fractions of the outer grid; t[K]: the targets in turns per cell
void nufft_t3_t_points(const double *x, unsigned long long m, const double *s, unsigned long long k, double eps, double *u,
                       double *t) {
    const phast::NufftT3Grid g = phast::nufft_t3_grid(x, m, s, k, eps);
    phast::nufft_t3_positions(g, x, m, u);
    phast::nufft_t3_targets(g, s, k, t);
}
void nufft_t3_t_phase64(double a, double b, double *c, double *s) { phast::nufft_t3_phase<double>(a, b, c, s); }
void nufft_t3_t_phase32(double a, double b, float *c, float *s) { phast::nufft_t3_phase<float>(a, b, c, s); }
// the tables of a plan as the planner builds them: xs, perm, cell_start [n_f + 1], pre [2 M], d_re, d_im [K] (f64)
void nufft_t3_t_tables(const double *x, unsigned long long m, const double *s, unsigned long long k, double eps, double *xs,
                       uint32_t *perm, uint32_t *cell_start, double *pre, double *d_re, double *d_im) {
    const phast::NufftT3Grid g = phast::nufft_t3_grid(x, m, s, k, eps);
    std::vector<double> u(m), t(k);
    phast::nufft_t3_positions(g, x, m, u.data());
    phast::nufft_t3_targets(g, s, k, t.data());
    phast::nufft_bin(u.data(), m, g.log_f, xs, perm, cell_start);
    phast::nufft_t3_pre_table<double>(g, x, perm, m, pre);
    phast::nufft_t3_post_table<double>(g, s, t.data(), k, d_re, d_im);
}
// out[i] = phi^_outer(xi[i])
void nufft_t3_t_phi_hat(int w, const double *xi, size_t count, double *out) {
    const phast::NufftT3Hat hat(w);
    for (size_t i = 0; i < count; ++i) out[i] = hat(xi[i]);
}
}
