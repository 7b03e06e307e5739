// nufft_sort.hpp -- the point tables of the non-uniform FFT planners (nufft.hpp, nufft_nd.hpp) built on the device from
// coordinates in device memory: the same perm, cell_start and sorted positions as nufft_bin and
// nufft_nd_bin give on the host, bit for bit.  Three stages, shared by one, two and three dimensions and by f64 and f32 (the points
// are doubles in both):
//
//     keys     one thread per point: the combined cell (((q1 << log_g2) | q2) << log_g3) | q3, q_i the top log_g_i bits of
//              czt_frac(coordinate, 0); a flag is raised if a coordinate is not finite
//     pairs    a stable least-significant-digit radix sort of (key, original index), kNufftSortBits bits per pass and only as
//              many passes as the key has digits; per pass a histogram per workgroup of kNufftSortBlock keys, an exclusive scan
//              of the (digit, workgroup) counts, and a scatter that ranks every key inside its workgroup through LDS
//     tables   perm[i] = the sorted index, xs[i] = nufft_turns(czt_frac(x[perm[i]], 0)) (ys, zs alike), and cell_start[q] = the
//              first sorted position whose key is >= q, by a boundary search: one writer per entry
//
// The order never comes from the arrival order of anything: the kernels use no atomics at all.  A thread counts the digits of its
// own kNufftSortPerThread CONSECUTIVE keys into a column of LDS that it alone writes; an exclusive scan of the counts in (digit,
// thread) order then gives every (digit, thread) its first slot, and the thread hands its keys their slots in ascending order --
// equal keys keep the order of their original indices, as in the host's counting sort.  Workgroups meet at kernel boundaries
// only, and the kernels use no cross-lane operations (tests/test_nufft_sort_emulator.py runs them on tests/emu/block_shim.hpp).
//
// The scan of the n = 2^kNufftSortBits * ceil(M / kNufftSortBlock) counts is hierarchical, S = kNufftSortScan entries (and threads)
// per workgroup: reduce every workgroup's entries to one partial, scan the partials (the same way, while they are more than one
// workgroup's), then scan every workgroup's entries in place on top of its partial.  The counts are few beside the keys (M / 256
// of them), so S is small: the scan has a level of partials above S entries (M > 16 Ki points), a second one above S^2 (M > 1 Mi
// points, which a host run of the kernels can still afford) and a third above S^3 entries (M > 64 Mi).
//
// The top of this header has no HIP dependency.
#pragma once

#include "nufft.hpp"

namespace phast {

constexpr unsigned kNufftSortBits = 4, kNufftSortRadix = 1u << kNufftSortBits;  // one digit
constexpr unsigned kNufftSortThreads = 256, kNufftSortPerThread = 16;
constexpr unsigned kNufftSortBlock = kNufftSortThreads * kNufftSortPerThread;  // B: keys per workgroup
constexpr unsigned kNufftSortScan = 64;                                        // S: entries per workgroup of one scan level

inline unsigned nufft_sort_passes(unsigned key_bits) { return (key_bits + kNufftSortBits - 1) / kNufftSortBits; }
inline unsigned long long nufft_sort_groups(unsigned long long m) { return (m + kNufftSortBlock - 1) / kNufftSortBlock; }
// 32-bit entries of the histogram buffer: the (digit, workgroup) counts, then the partials of every scan level
inline unsigned long long nufft_sort_hist_len(unsigned long long m) {
    unsigned long long n = kNufftSortRadix * nufft_sort_groups(m), total = n;
    while (n > kNufftSortScan) {
        n = (n + kNufftSortScan - 1) / kNufftSortScan;
        total += n;
    }
    return total;
}
// the temporary device memory of one sort of M points: two key and two index arrays, the histogram and the flag, every part
// 256-byte aligned -- 16 M bytes and a little
inline unsigned long long nufft_sort_part(unsigned long long bytes) { return (bytes + 255) & ~255ull; }
inline unsigned long long nufft_sort_temp_bytes(unsigned long long m) {
    return 4 * nufft_sort_part(4 * m) + nufft_sort_part(4 * nufft_sort_hist_len(m)) + 256;
}

}  // namespace phast

#if defined(__HIPCC__)
namespace phast {

struct NufftSortArgs {
    const double *x, *y, *z;          // [M] device coordinates in turns; y null in 1-D, z null below 3-D
    unsigned long long m;             // M points
    unsigned log_g1, log_g2, log_g3;  // the grid per axis; 0 for an axis that is not there
    uint32_t *key[2], *idx[2];        // [M] each: the ping-pong buffers of the pairs
    uint32_t *hist;                   // [nufft_sort_hist_len(M)]
    uint32_t *flag;                   // [1], zero before the keys stage; nonzero after it: a coordinate was not finite
    uint32_t *perm, *cell_start;      // the planner's tables: [M], [2^(log_g1 + log_g2 + log_g3) + 1]
    double *xs, *ys, *zs;             // [M] each (ys, zs as y, z)
};
// keys: a.x, a.y, a.z -> a.key[0], a.flag
hipError_t launch_nufft_sort_keys(const NufftSortArgs &a, hipStream_t stream);
// pairs: a.key[0] (and the implied indices 0 .. M - 1) -> a.key[*side], a.idx[*side] in sorted order
hipError_t launch_nufft_sort_pairs(const NufftSortArgs &a, int *side, hipStream_t stream);
// tables: a.key[side], a.idx[side] and the coordinates -> a.perm, a.cell_start, a.xs, a.ys, a.zs
hipError_t launch_nufft_sort_tables(const NufftSortArgs &a, int side, hipStream_t stream);

}  // namespace phast
#endif
