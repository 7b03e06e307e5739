// synthesizer_geom_test.cpp -- the host-only top of csrc/synthesizer.hpp behind a C interface for tests/test_synthesizer_cpu.py
// (g++, no HIP).
#include "synthesizer.hpp"

using namespace phast;

extern "C" {

unsigned long long sy_t_full_len(unsigned long long f, unsigned long long k, unsigned long long d) { return synth_full_len(f, k, d); }
unsigned long long sy_t_m_lo(unsigned long long n, unsigned long long k, unsigned long long d) { return synth_m_lo(n, k, d); }
long long sy_t_m_hi(unsigned long long n, unsigned long long f, unsigned long long d) { return synth_m_hi(n, f, d); }
unsigned long long sy_t_col(unsigned long long n, unsigned long long m) { return synth_col(n, m); }
// out[0..8) = tile, per, terms, sq, sr, sm, kq, kr
void sy_t_geom(unsigned long long k, unsigned long long m, unsigned long long d, unsigned *out) {
    const SynthGeom g = synth_geom(k, m, d);
    out[0] = g.tile;
    out[1] = g.per;
    out[2] = g.terms;
    out[3] = g.sq;
    out[4] = g.sr;
    out[5] = g.sm;
    out[6] = g.kq;
    out[7] = g.kr;
}
int sy_t_bad_args(unsigned long long f, unsigned long long k, unsigned long long m, unsigned long long d, unsigned long long first,
                  unsigned long long out_len) {
    return synth_bad_args(f, k, m, d, first, out_len);
}
unsigned sy_t_const(int which) {
    const unsigned c[] = {kSynthPer, kSynthTile};
    return c[which];
}
}
