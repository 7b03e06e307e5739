// dwt_geom_test.cpp -- the host-only top of csrc/dwt.hpp behind a C interface for tests/test_dwt_cpu.py (g++, no HIP).
#include "dwt.hpp"

using namespace phast;

extern "C" {

unsigned long long dwt_t_level_len(unsigned long long n, unsigned f, int mode) { return dwt_level_len(n, f, mode); }
unsigned long long dwt_t_synth_len(unsigned long long m, unsigned f, int mode) { return dwt_synth_len(m, f, mode); }
unsigned dwt_t_max_level(unsigned long long len, unsigned f) { return dwt_max_level(len, f); }
long long dwt_t_ext_index(int mode, long long n, long long t) { return dwt_ext_index(mode, n, t); }
long long dwt_t_synth_index(int mode, long long m, long long k) { return dwt_synth_index(mode, m, k); }
int dwt_t_bad_args(unsigned long long len, unsigned long long f, unsigned long long levels, int mode) { return dwt_bad_args(len, f, levels, mode); }
// n[0 .. J], off[0 .. J], then coeff_len, row_a, row_b, tile
void dwt_t_geom(unsigned long long len, unsigned f, unsigned levels, int mode, unsigned long long *n, unsigned long long *off,
                unsigned long long *rest) {
    const DwtGeom g = dwt_geom(len, f, levels, mode);
    for (unsigned l = 0; l <= levels; ++l) {
        n[l] = g.n[l];
        off[l] = g.off[l];
    }
    rest[0] = g.coeff_len;
    rest[1] = g.row_a;
    rest[2] = g.row_b;
    rest[3] = g.tile;
}
void dwt_t_analysis_span(unsigned long long i0, unsigned long long n, unsigned f, int mode, long long *lo, unsigned long long *count) {
    dwt_analysis_span(i0, n, f, mode, lo, count);
}
void dwt_t_synth_pairs(unsigned long long out_len, unsigned f, int mode, long long *q_first, unsigned long long *pairs) {
    dwt_synth_pairs(out_len, f, mode, q_first, pairs);
}
void dwt_t_synth_span(long long q0, unsigned long long n, unsigned f, long long *lo, unsigned long long *count) {
    dwt_synth_span(q0, n, f, lo, count);
}
long long dwt_t_shift(int synth, unsigned f, int mode) { return synth ? dwt_synth_shift(f, mode) : dwt_analysis_shift(f, mode); }
unsigned dwt_t_const(int which) {
    const unsigned c[] = {kDwtTile, kDwtPerThread, kDwtHalfLds, kDwtMaxFilter, kDwtMaxLevel};
    return c[which];
}
}
