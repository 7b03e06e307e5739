// channelizer_geom_test.cpp -- the host-only top of csrc/channelizer.hpp behind a C interface for tests/test_channelizer_cpu.py
// (g++, no HIP).
#include "channelizer.hpp"

using namespace phast;

extern "C" {

unsigned long long ch_t_full_frames(unsigned long long len, unsigned long long k, unsigned long long d) { return chan_full_frames(len, k, d); }
unsigned long long ch_t_t(unsigned long long k, unsigned long long m) { return chan_t(k, m); }
unsigned long long ch_t_r0(unsigned long long fr, unsigned long long p, unsigned long long m, unsigned long long d) { return chan_r0(fr, p, m, d); }
// out[0..7) = cols, fpp, per, frames, span, jc, rows
void ch_t_geom(unsigned long long k, unsigned long long m, unsigned long long d, unsigned *out) {
    const ChanGeom g = chan_geom(k, m, d);
    out[0] = g.cols;
    out[1] = g.fpp;
    out[2] = g.per;
    out[3] = g.frames;
    out[4] = g.span;
    out[5] = g.jc;
    out[6] = g.rows;
}
void ch_t_span(unsigned long long m0, unsigned long long n, unsigned long long p0, unsigned long long c, unsigned long long m,
               unsigned long long d, unsigned long long j0, unsigned long long jc, long long *q_lo, unsigned long long *count) {
    chan_span(m0, n, p0, c, m, d, j0, jc, q_lo, count);
}
int ch_t_bad_args(unsigned long long len, unsigned long long k, unsigned long long m, unsigned long long d, unsigned long long first,
                  unsigned long long out_frames) {
    return chan_bad_args(len, k, m, d, first, out_frames);
}
unsigned ch_t_const(int which) {
    const unsigned c[] = {kChanLds, kChanMaxCols, kChanPerThread};
    return c[which];
}
}
