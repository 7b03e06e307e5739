// lomb_tables_test.cpp -- the host-only top of csrc/lomb.hpp behind a C interface for tests/test_lomb_cpu.py (g++, no HIP).
#include "lomb.hpp"

using namespace phast;

extern "C" {

int lomb_t_bad_args(const double *t, unsigned long long m, const double *f, unsigned long long k, const double *w) {
    return lomb_bad_args(t, m, f, k, w);
}
unsigned long long lomb_t_slab_len(unsigned long long m) { return lomb_slab_len(m); }
unsigned long long lomb_t_slabs(unsigned long long m) { return lomb_slabs(m, lomb_slab_len(m)); }
double lomb_t_epsneg(int f32) { return lomb_epsneg(f32 != 0); }
void lomb_t_weights(const double *w, unsigned long long m, double *out) { lomb_weights(w, m, out); }

// out[0..3][k] = cos tau, sin tau, CCt, SSt from the sums a0 = (c, s) and a2 = (c2, s2)
void lomb_t_tables(const double *c, const double *s, const double *c2, const double *s2, unsigned long long k, int floating_mean,
                   int f32, double *out) {
    for (unsigned long long i = 0; i < k; ++i)
        lomb_table(c[i], s[i], c2[i], s2[i], floating_mean, lomb_epsneg(f32 != 0), out + i, out + k + i, out + 2 * k + i, out + 3 * k + i);
}

// out[0..2][k] = P, a, b from A1 = (ar, ai) and the tables (CCt and SSt, not their reciprocals)
void lomb_t_post(const double *ar, const double *ai, const double *tab, unsigned long long k, double *out) {
    for (unsigned long long i = 0; i < k; ++i)
        out[i] = lomb_post(ar[i], ai[i], tab[i], tab[k + i], 1.0 / tab[2 * k + i], 1.0 / tab[3 * k + i], out + k + i, out + 2 * k + i);
}
}
