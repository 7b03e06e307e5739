// cwt_geom_test.cpp -- the host-only top of csrc/cwt.hpp behind a C interface for tests/test_cwt_cpu.py (g++, no HIP).
#include "cwt.hpp"

using namespace phast;
using u64 = unsigned long long;

extern "C" {

// out[0..8) = v, tile, group, tiles, ngrp, bins, xd, rd
void cw_t_geom(u64 p, u64 s, int real_input, unsigned elem_size, u64 *out) {
    const CwtGeom g = cwt_geom(p, s, real_input, elem_size);
    out[0] = g.v;
    out[1] = g.tile;
    out[2] = g.group;
    out[3] = g.tiles;
    out[4] = g.ngrp;
    out[5] = g.bins;
    out[6] = g.xd;
    out[7] = g.rd;
}
u64 cw_t_first_signal(u64 row0, u64 s) { return cwt_first_signal(row0, s); }
u64 cw_t_signals(u64 row0, u64 r, u64 s) { return cwt_signals(row0, r, s); }
u64 cw_t_max_signals(u64 r, u64 s, u64 batch) { return cwt_max_signals(r, s, batch); }
u64 cw_t_first_group(u64 row0, u64 s, u64 ngrp) { return cwt_first_group(row0, s, ngrp); }
u64 cw_t_groups(u64 row0, u64 r, u64 s, u64 ngrp) { return cwt_groups(row0, r, s, ngrp); }
u64 cw_t_need(u64 r, u64 s, u64 batch, u64 sig_per, u64 row_per, unsigned v) { return cwt_need(r, s, batch, sig_per, row_per, v); }
u64 cw_t_rows_per_chunk(u64 len, u64 total, u64 s, u64 batch, u64 sig_per, u64 row_per, unsigned v) {
    return cwt_rows_per_chunk(len, total, s, batch, sig_per, row_per, v);
}
long long cw_t_signed_bin(u64 k, u64 p) { return cwt_signed_bin(k, p); }
double cw_t_step_gain(u64 k, u64 p) { return cwt_step_gain(k, p); }
int cw_t_bad_args(u64 l, u64 p, u64 s, int family, double param, int norm) { return cwt_bad_args(l, p, s, family, param, norm); }
int cw_t_bad_scale(double s) { return cwt_bad_scale(s); }
double cw_t_family_const(int family, double param) { return cwt_family_const(family, param); }
double cw_t_family_peak(int family, double param) { return cwt_family_peak(family, param); }
double cw_t_gain(int family, double param, int norm, double scale) { return cwt_gain(family, param, norm, scale); }
unsigned cw_t_group_const() { return kCwtGroup; }
}
