// convnd.hip -- the gather and scatter sweeps of N-d overlap-save convolution (convnd.hpp has the definitions; the multiply by
// the filter's spectrum is conv.hip's spectrum sweep, a tile's half spectrum being one of its rows).
//
// Built as conv.hip is: 256-thread workgroups in address order, launches split at 2^31 - 1 workgroups, a thread owns one group
// of V = 16 / sizeof(T) consecutive elements on the side it writes.  The workspace side moves in aligned 16-byte accesses; the
// caller's side is read as one 16-byte load of element alignment (Unaligned<T>) or written as one aligned 16-byte store where
// a whole group lies inside the array (tile sweep) or inside one tile's run of an output row (save sweep), and by element at
// the edges.  The caller's arrays are accessed non-temporally: the input is streamed prod (B_i / S_i) times, the output
// once.  No LDS, no atomics: an output sample has exactly one source.
#include "convnd.hpp"

namespace phast {

// ---- tile: tile r of the workspace = x~[t0_i + s_i S_i - (K_i - 1) + j_i], j_i < B_i, of tile q0 + r; zeros in the padding
// up to fd ----
template <typename T>
__global__ void __launch_bounds__(256) convnd_tile_kernel(ConvNdArgs a) {
    using V = typename AnyVec<T>::type;
    using VU = typename Unaligned<T>::type;
    constexpr int L = AnyVec<T>::N;
    const unsigned long long g = global_group(a);
    if (g >= a.groups) return;
    unsigned long long r;
    const unsigned f0 = (unsigned)split_group(g, a.gpt, &r) * L;  // the group's first element in the tile: fd <= 2^28 + 3
    unsigned long long arr;
    unsigned t = (unsigned)split_group(a.q0 + r, a.tiles, &arr);  // tiles <= 2^30
    const unsigned s2 = t % a.segs[2];
    t /= a.segs[2];
    const unsigned s1 = t % a.segs[1], s0 = t / a.segs[1];
    unsigned j2 = f0 % a.b[2], j1 = f0 / a.b[2];
    unsigned j0 = j1 / a.b[1];
    j1 -= j0 * a.b[1];
    // the array's sample of tile element (0, 0, 0); every term < 2^30
    const int o0 = (int)(a.t0[0] + s0 * a.s[0]) - (int)a.k1[0], o1 = (int)(a.t0[1] + s1 * a.s[1]) - (int)a.k1[1],
              o2 = (int)(a.t0[2] + s2 * a.s[2]) - (int)a.k1[2];
    const T *x = (const T *)a.in + arr * a.sig_dist;
    const int i0 = o0 + (int)j0, i1 = o1 + (int)j1, i2 = o2 + (int)j2;
    V v;
    if (f0 < a.pts && j2 + L <= a.b[2] && i0 >= 0 && i0 < (int)a.len[0] && i1 >= 0 && i1 < (int)a.len[1] && i2 >= 0 &&
        i2 + L <= (int)a.len[2]) {  // an interior group: one tile row, its source run inside the array on every axis
        const VU u = __builtin_nontemporal_load((const VU *)(x + ((unsigned long long)i0 * a.len[1] + i1) * a.len[2] + i2));
#pragma unroll
        for (int e = 0; e < L; ++e) v[e] = u[e];
    } else {  // an edge of the array, the padding up to fd, or a group that straddles two tile rows
#pragma unroll
        for (int e = 0; e < L; ++e) {
            const int c0 = o0 + (int)j0, c1 = o1 + (int)j1, c2 = o2 + (int)j2;
            const bool inside = f0 + e < a.pts && c0 >= 0 && c0 < (int)a.len[0] && c1 >= 0 && c1 < (int)a.len[1] && c2 >= 0 &&
                                c2 < (int)a.len[2];
            v[e] = inside ? __builtin_nontemporal_load(x + ((unsigned long long)c0 * a.len[1] + c1) * a.len[2] + c2) : T(0);
            if (++j2 == a.b[2]) {  // the next tile row
                j2 = 0;
                if (++j1 == a.b[1]) {
                    j1 = 0;
                    ++j0;
                }
            }
        }
    }
    *(V *)((T *)a.out + r * a.fd + f0) = v;
}

// ---- save: out[s_i S_i + a_i] = y[K_i - 1 + a_i] of every tile of the chunk.  A thread owns one aligned 16-byte group of the
// caller's output in the run of one tile along the last axis, in output row (a_0, a_1) of that tile ----
template <typename T>
__global__ void __launch_bounds__(256) convnd_save_kernel(ConvNdArgs a) {
    using V = typename AnyVec<T>::type;
    using VU = typename Unaligned<T>::type;
    constexpr int L = AnyVec<T>::N;
    const unsigned long long g = global_group(a);
    if (g >= a.groups) return;
    unsigned long long r;
    unsigned w = (unsigned)split_group(g, a.gpt, &r);  // gpt = S_0 S_1 gpr < 2^30
    const unsigned m = w % a.gpr;
    w /= a.gpr;
    const unsigned a1 = w % a.s[1], a0 = w / a.s[1];
    unsigned long long arr;
    unsigned t = (unsigned)split_group(a.q0 + r, a.tiles, &arr);
    const unsigned s2 = t % a.segs[2];
    t /= a.segs[2];
    const unsigned s1 = t % a.segs[1], s0 = t / a.segs[1];
    const unsigned r0 = s0 * a.s[0] + a0, r1 = s1 * a.s[1] + a1;  // the output row
    if (r0 >= a.n_out[0] || r1 >= a.n_out[1]) return;              // the last tile of an axis yields fewer rows
    const unsigned c_lo = s2 * a.s[2];                              // the tile's run [c_lo, c_hi) of the row
    const unsigned c_hi = c_lo + a.s[2] < a.n_out[2] ? c_lo + a.s[2] : a.n_out[2];
    T *row = (T *)a.out + arr * a.out_dist + ((unsigned long long)r0 * a.n_out[1] + r1) * a.n_out[2];
    const T *y = (const T *)a.in + r * a.fd + ((unsigned long long)(a.k1[0] + a0) * a.b[1] + (a.k1[1] + a1)) * a.b[2] + a.k1[2];
    // the row's element 0 lies `mis` elements into a 16-byte group: group m of the run starts at row element e
    const unsigned mis = (unsigned)(reinterpret_cast<unsigned long long>(row) / sizeof(T)) & (unsigned)(L - 1);
    const long long e = (long long)((c_lo + mis) / L + m) * L - (long long)mis;
    if (e >= (long long)c_hi) return;
    if (e >= (long long)c_lo && e + L <= (long long)c_hi) {  // the whole group in this tile's run
        const VU u = *(const VU *)(y + (e - c_lo));
        V v;
#pragma unroll
        for (int k = 0; k < L; ++k) v[k] = u[k];
        __builtin_nontemporal_store(v, (V *)(row + e));
        return;
    }
#pragma unroll
    for (int k = 0; k < L; ++k) {  // a ragged end: the neighbouring tile, or nobody, writes the rest of the group
        const long long c = e + k;
        if (c >= (long long)c_lo && c < (long long)c_hi) __builtin_nontemporal_store(y[c - c_lo], row + c);
    }
}

template <typename T> hipError_t launch_convnd(int kind, const ConvNdArgs &a0, hipStream_t stream) {
    if (kind != kConvNdTile && kind != kConvNdSave) return hipErrorInvalidValue;
    ConvNdArgs a = a0;
    return launch_in_slices(a.groups, [&](dim3 grid, unsigned long long g0) {
        a.g0 = g0;
        const dim3 block(256);
        if (kind == kConvNdTile) hipLaunchKernelGGL((convnd_tile_kernel<T>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((convnd_save_kernel<T>), grid, block, 0, stream, a);
    });
}

template hipError_t launch_convnd<double>(int, const ConvNdArgs &, hipStream_t);
template hipError_t launch_convnd<float>(int, const ConvNdArgs &, hipStream_t);

}  // namespace phast
