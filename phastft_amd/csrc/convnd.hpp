// convnd.hpp -- convolution and correlation of real arrays of rank 1 .. 3 by overlap-save along every axis, around one real
// N-d transform of the tile shape.
//
// x is a row-major real array [L_0 .. L_{r-1}], h one of the same rank [K_0 .. K_{r-1}].  full[t] = sum_j g[j] x[t - j],
// t_i in [0, L_i + K_i - 1), with g = h (convolution) or h reversed along every axis (correlation); out[i] = full[t0 + i].
// Per axis t0_i = conv_t0(K_i, mode) and out_i = conv_out_len(L_i, K_i, mode): the rules of conv.hpp, axis by axis.  These
// are scipy.signal.convolve / correlate(x, h, mode, method="direct").  Per axis a block B_i >= K_i, a hop S_i = B_i - K_i + 1
// and segs_i = ceil(out_i / S_i); tiles = prod segs_i, numbered row-major over (s_0 .. s_{r-1}):
//     tile      tile s = x~[t0_i + s_i S_i - (K_i - 1) + j_i], j_i < B_i; x~ is x inside the array, 0 outside   kConvNdTile
//     R2C       X[s] = rfftn_B(tile s)                                                  RealNdPlanner (unchanged)
//     spectrum  X[s] *= H^, H^ = rfftn_B(g zero-padded to B), unscaled (the C2R scales by 1 / prod B)   kConvSpectrum (conv.hip)
//     C2R       y[s] = irfftn_B(X[s])                                                   RealNdPlanner (unchanged)
//     save      out[s_i S_i + a_i] = y[s][K_i - 1 + a_i], a_i < min(S_i, out_i - s_i S_i)                       kConvNdSave
//
// An axis with L_i = K_i = 1 does nothing and is dropped (the last one stays if nothing else does); what is left is padded
// in front with such axes to rank 3, which is the one form the geometry and the kernels know.
//
// The top of this header (geometry, automatic block, argument rules) has no HIP dependency: tests/test_convnd_cpu.py
// compiles it with g++.
#pragma once

#include "conv.hpp"

namespace phast {

constexpr unsigned kConvNdMaxRank = 3;
constexpr unsigned long long kConvNdMaxPoints = 1ull << 30;      // prod L and prod out
constexpr unsigned long long kConvNdMaxTilePoints = 1ull << 28;  // prod B

// the automatic block of one axis of an array of `rank` axes that count (1 .. 3): the smallest power of two
// >= max(4 (K - 1), floor), floor = 1024 for rank 1 (§16) and 64 for rank 2 and 3 (§13: the transpose reaches its rate only
// when both sides are >= 64); or the smallest power of two >= out + K - 1 (one tile spans the axis) where that is smaller
PHAST_HD unsigned long long convnd_auto_block(unsigned long long len, unsigned long long k, int mode, unsigned rank) {
    const unsigned long long floor_b = rank <= 1 ? 1024 : 64;
    unsigned long long b = conv_pow2_ceil(4 * (k - 1) > floor_b ? 4 * (k - 1) : floor_b);
    if (b > kConvMaxLen) b = kConvMaxLen;
    const unsigned long long whole = conv_pow2_ceil(conv_out_len(len, k, mode) + k - 1);
    return whole < b ? whole : b;
}

// the geometry of a planner, always of rank 3: the caller's axes that count, behind axes of L = K = B = 1
struct ConvNdGeom {
    unsigned rank;                   // the axes that count (1 .. 3): they are the last `rank` entries
    unsigned axis_of[kConvNdMaxRank];  // the caller's axis behind entry i (entries in front of the counted ones: unused)
    unsigned long long len[kConvNdMaxRank], k[kConvNdMaxRank], b[kConvNdMaxRank], s[kConvNdMaxRank];
    unsigned long long t0[kConvNdMaxRank], out[kConvNdMaxRank], segs[kConvNdMaxRank];
    unsigned long long sig_pts, out_pts, tile_pts, tiles;  // prod L, prod out, prod B, prod segs
};

// The argument rules of a planner, before the device is touched: 0 when the arguments are legal for elements of which `vec`
// fill 16 bytes, and then *g is the geometry.  block: null, or per caller's axis 0 = the automatic block.
PHAST_HD int convnd_bad_args(const size_t *sig_dims, const size_t *tap_dims, size_t rank, int mode, int flip,
                             const size_t *block, unsigned long long vec, ConvNdGeom *g) {
    if (!sig_dims || !tap_dims || !g || rank < 1 || rank > kConvNdMaxRank) return 1;
    if (mode != kConvFull && mode != kConvSame && mode != kConvValid) return 1;
    if (flip != 0 && flip != 1) return 1;
    if (vec != 2 && vec != 4) return 1;
    unsigned kept[kConvNdMaxRank], q = 0;
    for (size_t i = 0; i < rank; ++i) {
        if (sig_dims[i] < 1 || sig_dims[i] > kConvMaxLen || tap_dims[i] < 1 || tap_dims[i] > kConvMaxLen) return 1;
        if (block && block[i] > kConvMaxLen) return 1;
        if (mode == kConvValid && sig_dims[i] < tap_dims[i]) return 1;
        if (sig_dims[i] > 1 || tap_dims[i] > 1 || (q == 0 && i + 1 == rank)) kept[q++] = (unsigned)i;
    }
    g->rank = q;
    g->sig_pts = g->out_pts = g->tile_pts = g->tiles = 1;
    const unsigned lead = kConvNdMaxRank - q;
    for (unsigned i = 0; i < kConvNdMaxRank; ++i) {
        const bool unit = i < lead;
        const unsigned ax = unit ? 0 : kept[i - lead];
        g->axis_of[i] = ax;
        const unsigned long long len = unit ? 1 : sig_dims[ax], k = unit ? 1 : tap_dims[ax];
        unsigned long long b = unit ? 1 : block ? block[ax] : 0;
        if (!b) b = convnd_auto_block(len, k, mode, q);
        if (b < k || b > kConvMaxLen) return 1;
        g->len[i] = len;
        g->k[i] = k;
        g->b[i] = b;
        g->s[i] = b - k + 1;
        g->t0[i] = conv_t0(k, mode);
        g->out[i] = conv_out_len(len, k, mode);
        g->segs[i] = conv_segments(g->out[i], k, b);
        g->sig_pts *= len;  // every factor <= 2^29 and every product checked <= 2^30: no overflow
        g->out_pts *= g->out[i];
        g->tile_pts *= b;
        g->tiles *= g->segs[i];
        if (g->out[i] < 1 || g->sig_pts > kConvNdMaxPoints || g->out_pts > kConvNdMaxPoints) return 1;
        if (g->tile_pts > kConvNdMaxTilePoints) return 1;
    }
    return 0;
}

// first sample of the array that tile coordinate s reads along entry i (may be negative), and the samples it yields there
PHAST_HD long long convnd_src0(const ConvNdGeom &g, unsigned i, unsigned long long s) {
    return (long long)(g.t0[i] + s * g.s[i]) - (long long)(g.k[i] - 1);
}
PHAST_HD unsigned long long convnd_yield(const ConvNdGeom &g, unsigned i, unsigned long long s) {
    const unsigned long long left = g.out[i] - s * g.s[i];
    return left < g.s[i] ? left : g.s[i];
}
// groups of `vec` elements of an output row that the run of one tile can touch, wherever the row starts in memory
PHAST_HD unsigned long long convnd_save_groups(unsigned long long s_last, unsigned long long vec) {
    return (s_last + vec - 1) / vec + 1;
}

}  // namespace phast

#if defined(__HIPCC__)

namespace phast {

enum ConvNdKind { kConvNdTile = 0, kConvNdSave = 1 };

// one sweep over `groups` thread groups of V = 16 / sizeof(T) elements: of a workspace tile (tile sweep), or of the caller's
// output along its last axis (save sweep).  All axis values are < 2^30: the kernels divide in 32 bits.
struct ConvNdArgs {
    const void *in;  // tile: the caller's arrays; save: the workspace tiles y
    void *out;       // tile: the workspace tiles; save: the caller's outputs
    unsigned long long sig_dist, out_dist;  // elements between the caller's arrays / outputs
    unsigned long long fd;                  // elements between workspace tiles
    unsigned long long q0, q1;  // the flattened (array, tile) indices [q0, q1) of this chunk; workspace tile 0 is q0
    unsigned long long groups;  // groups in this launch
    unsigned long long g0;      // first group of this launch (launches split at 2^31 - 1 workgroups)
    unsigned gpt;               // groups per workspace tile (tile: fd / V; save: S_0 S_1 gpr)
    unsigned gpr;               // save: groups per output row of a tile, convnd_save_groups(S_2, V)
    unsigned tiles, pts;        // prod segs, prod B
    unsigned len[3], k1[3], b[3], s[3], t0[3], n_out[3], segs[3];  // k1 = K - 1
};
template <typename T> hipError_t launch_convnd(int kind, const ConvNdArgs &a, hipStream_t stream);

}  // namespace phast
#endif
