// resample_geom_test.cpp -- the host-only top of csrc/resample.hpp behind a C interface for tests/test_resample_cpu.py (g++, no
// HIP).
#include "resample.hpp"

using namespace phast;

extern "C" {

unsigned long long rs_t_full_len(unsigned long long len, unsigned long long k, unsigned long long up, unsigned long long down) {
    return upfirdn_full_len(len, k, up, down);
}
unsigned long long rs_t_kp(unsigned long long k, unsigned long long up) { return upfirdn_kp(k, up); }
// out[0..5) = rows, jc, stride, tile, by_phase
void rs_t_geom(unsigned long long k, unsigned long long up, unsigned long long down, unsigned *out) {
    const UpfirdnGeom g = upfirdn_geom(k, up, down);
    out[0] = g.rows;
    out[1] = g.jc;
    out[2] = g.stride;
    out[3] = g.tile;
    out[4] = (unsigned)g.by_phase;
}
void rs_t_span(unsigned long long m0, unsigned long long n, unsigned long long up, unsigned long long down, unsigned long long j0,
               unsigned long long jc, long long *lo, unsigned long long *count) {
    upfirdn_span(m0, n, up, down, j0, jc, lo, count);
}
int rs_t_upfirdn_bad_args(unsigned long long len, unsigned long long k, unsigned long long up, unsigned long long down,
                          unsigned long long first, unsigned long long out_len) {
    return upfirdn_bad_args(len, k, up, down, first, out_len);
}
int rs_t_resample_bad_args(unsigned long long len, unsigned long long num) { return resample_bad_args(len, num); }
unsigned long long rs_t_bins(unsigned long long len, unsigned long long num) { return resample_bins(len, num); }
double rs_t_nyquist(unsigned long long len, unsigned long long num) { return resample_nyquist(len, num); }
unsigned rs_t_const(int which) {
    const unsigned c[] = {kResampleTapLds, kResampleTapPad, kResampleSigLds, kResampleMaxTile, kResamplePerThread, kResampleMaxRows};
    return c[which];
}
}
