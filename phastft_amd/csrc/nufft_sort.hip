// nufft_sort.hip -- the kernels that build the point tables of the non-uniform FFT planners on the device (nufft_sort.hpp has the
// algorithm and the rules).  No atomics, no cross-lane operations, workgroups meet at kernel boundaries only.
#include "nufft_sort.hpp"

namespace phast {

constexpr unsigned kSortR = kNufftSortRadix, kSortT = kNufftSortThreads, kSortP = kNufftSortPerThread, kSortS = kNufftSortScan;
static_assert(kSortR * kSortR == kSortT, "a thread sums kSortR entries of the counts and a second step sums kSortR of those");
static_assert(kSortP == kSortR, "a thread scans as many entries of the counts as it has keys");

// the position of a point in turns: the exact fraction TRUNCATED to 53 significant bits, as nufft_bin stores it
__device__ inline double nufft_sort_position(double v) { return nufft_turns(czt_frac(v, 0)); }

// the cell of a coordinate on an axis of 2^log_g cells (0 where the axis is not there); *bad if it is not finite
__device__ inline uint32_t nufft_sort_cell(const double *c, unsigned long long j, unsigned log_g, bool *bad) {
    if (!c) return 0;
    const double v = c[j];
    unsigned long long bits = 0;
    __builtin_memcpy(&bits, &v, sizeof bits);
    if (((bits >> 52) & 0x7ffull) == 0x7ffull) {
        *bad = true;
        return 0;
    }
    return (uint32_t)(czt_frac(v, 0).hi >> (64 - log_g));
}

// keys: one thread per point
__global__ void __launch_bounds__(256) nufft_sort_key_kernel(NufftSortArgs a) {
    const unsigned long long j = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= a.m) return;
    bool bad = false;
    const uint32_t q1 = nufft_sort_cell(a.x, j, a.log_g1, &bad), q2 = nufft_sort_cell(a.y, j, a.log_g2, &bad);
    const uint32_t q3 = nufft_sort_cell(a.z, j, a.log_g3, &bad);
    a.key[0][j] = (((q1 << a.log_g2) | q2) << a.log_g3) | q3;
    if (bad) *a.flag = 1u;  // every writer writes the same value
}

// one pass of the sort over the digit at `shift`
struct NufftSortPass {
    const uint32_t *key_in, *idx_in;  // idx_in is not read by the first pass: the index is the position
    uint32_t *key_out, *idx_out;
    uint32_t *hist;  // [digit * groups + workgroup]: counts after the histogram kernel, first slots after the scan
    unsigned long long m, groups;
    unsigned shift;
};

// The thread's keys (n of them, from `base` on) into registers, and their digits counted into column t of cnt[digit][thread]: the
// column is this thread's alone
__device__ inline void nufft_sort_count(const NufftSortPass &p, uint32_t *cnt, unsigned t, unsigned long long base, unsigned n,
                                        uint32_t (&key)[kSortP]) {
#pragma unroll
    for (unsigned d = 0; d < kSortR; ++d) cnt[d * kSortT + t] = 0;
    if (n == kSortP) {
#pragma unroll
        for (unsigned j = 0; j < kSortP; ++j) key[j] = p.key_in[base + j];
    } else {
#pragma unroll
        for (unsigned j = 0; j < kSortP; ++j) key[j] = j < n ? p.key_in[base + j] : 0u;
    }
#pragma unroll
    for (unsigned j = 0; j < kSortP; ++j)
        if (j < n) cnt[((key[j] >> p.shift) & (kSortR - 1)) * kSortT + t] += 1;
}

__device__ inline unsigned nufft_sort_own(const NufftSortPass &p, unsigned t, unsigned long long *base) {
    *base = (unsigned long long)blockIdx.x * kNufftSortBlock + (unsigned long long)t * kSortP;
    return *base >= p.m ? 0u : p.m - *base < kSortP ? (unsigned)(p.m - *base) : kSortP;
}

// histogram: hist[d * groups + workgroup] = the keys of this workgroup whose digit is d
__global__ void __launch_bounds__(kSortT) nufft_sort_hist_kernel(NufftSortPass p) {
    __shared__ uint32_t cnt[kSortR * kSortT];
    __shared__ uint32_t part[kSortT];
    const unsigned t = threadIdx.x;
    unsigned long long base;
    const unsigned n = nufft_sort_own(p, t, &base);
    uint32_t key[kSortP];
    nufft_sort_count(p, cnt, t, base, n, key);
    __syncthreads();
    uint32_t s = 0;  // entries t * kSortR ..: digit t / kSortR, threads (t % kSortR) * kSortR ..
#pragma unroll
    for (unsigned k = 0; k < kSortR; ++k) s += cnt[t * kSortR + k];
    part[t] = s;
    __syncthreads();
    if (t < kSortR) {
        uint32_t total = 0;
#pragma unroll
        for (unsigned k = 0; k < kSortR; ++k) total += part[t * kSortR + k];
        p.hist[t * p.groups + blockIdx.x] = total;
    }
}

// scatter: every key of the workgroup to hist[digit][workgroup] (after the scan: the first slot of this workgroup's keys of that
// digit) + its rank among the workgroup's keys of the same digit, in the order of their positions
template <bool FIRST>
__global__ void __launch_bounds__(kSortT) nufft_sort_scatter_kernel(NufftSortPass p) {
    __shared__ uint32_t cnt[kSortR * kSortT];
    __shared__ uint32_t sums[2][kSortT];
    __shared__ uint32_t off[kSortR];
    const unsigned t = threadIdx.x;
    unsigned long long base;
    const unsigned n = nufft_sort_own(p, t, &base);
    uint32_t key[kSortP], idx[kSortP];
    nufft_sort_count(p, cnt, t, base, n, key);
#pragma unroll
    for (unsigned j = 0; j < kSortP; ++j) idx[j] = FIRST ? (uint32_t)(base + j) : j < n ? p.idx_in[base + j] : 0u;
    __syncthreads();  // every column is counted before the scan reads across the columns
    // the exclusive scan of the counts in (digit, thread) order: this thread's kSortR entries, then the threads' sums
    uint32_t s = 0;
#pragma unroll
    for (unsigned k = 0; k < kSortR; ++k) s += cnt[t * kSortR + k];
    sums[0][t] = s;
    unsigned cur = 0;
    for (unsigned step = 1; step < kSortT; step <<= 1) {
        __syncthreads();
        sums[cur ^ 1][t] = sums[cur][t] + (t >= step ? sums[cur][t - step] : 0u);
        cur ^= 1;
    }
    __syncthreads();
    uint32_t run = sums[cur][t] - s;
    // entry t * kSortR is the first of digit t / kSortR where t % kSortR == 0: what to add to a rank to get the slot
    if (t % kSortR == 0) off[t / kSortR] = p.hist[(t / kSortR) * p.groups + blockIdx.x] - run;
#pragma unroll
    for (unsigned k = 0; k < kSortR; ++k) {
        const uint32_t c = cnt[t * kSortR + k];
        cnt[t * kSortR + k] = run;
        run += c;
    }
    __syncthreads();
    // the rank: column t now holds the rank of this thread's first key of each digit
#pragma unroll
    for (unsigned k = 0; k < kSortP; ++k) {
        const unsigned j = k;  // ascending: equal digits keep the order of their positions (the tie-break)
        if (j < n) {
            const unsigned d = (key[j] >> p.shift) & (kSortR - 1);
            const uint32_t r = cnt[d * kSortT + t];
            cnt[d * kSortT + t] = r + 1;
            const uint32_t slot = off[d] + r;
            p.key_out[slot] = key[j];
            p.idx_out[slot] = idx[j];
        }
    }
}

// the inclusive scan of one value per thread of a workgroup of kSortS threads through sums[2][kSortS]
__device__ inline uint32_t nufft_sort_scan_block(uint32_t (*sums)[kSortS], unsigned t, uint32_t v) {
    sums[0][t] = v;
    unsigned cur = 0;
    for (unsigned step = 1; step < kSortS; step <<= 1) {
        __syncthreads();
        sums[cur ^ 1][t] = sums[cur][t] + (t >= step ? sums[cur][t - step] : 0u);
        cur ^= 1;
    }
    __syncthreads();
    return sums[cur][t];
}

// partial[workgroup] = the sum of the workgroup's kSortS entries of data[0 .. n)
__global__ void __launch_bounds__(kSortS) nufft_sort_reduce_kernel(const uint32_t *data, unsigned long long n, uint32_t *partial) {
    __shared__ uint32_t sums[2][kSortS];
    const unsigned t = threadIdx.x;
    const unsigned long long e = (unsigned long long)blockIdx.x * kSortS + t;
    const uint32_t total = nufft_sort_scan_block(sums, t, e < n ? data[e] : 0u);
    if (t == kSortS - 1) partial[blockIdx.x] = total;
}

// data[e] = (partial ? partial[workgroup] : 0) + the sum of the workgroup's entries before e, in place; partial holds the
// exclusive scan of the workgroups' sums
__global__ void __launch_bounds__(kSortS) nufft_sort_scan_kernel(uint32_t *data, unsigned long long n, const uint32_t *partial) {
    __shared__ uint32_t sums[2][kSortS];
    const unsigned t = threadIdx.x;
    const unsigned long long e = (unsigned long long)blockIdx.x * kSortS + t;
    const uint32_t v = e < n ? data[e] : 0u;
    const uint32_t incl = nufft_sort_scan_block(sums, t, v);
    if (e < n) data[e] = incl - v + (partial ? partial[blockIdx.x] : 0u);
}

// tables: the sorted index and the positions of sorted point i
__global__ void __launch_bounds__(256) nufft_sort_table_kernel(NufftSortArgs a, const uint32_t *idx) {
    const unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.m) return;
    const uint32_t j = idx[i];
    a.perm[i] = j;
    a.xs[i] = nufft_sort_position(a.x[j]);
    if (a.y) a.ys[i] = nufft_sort_position(a.y[j]);
    if (a.z) a.zs[i] = nufft_sort_position(a.z[j]);
}

// cell_start[q] = the first sorted position whose key is >= q, q <= cells: a boundary search, one thread and one store per entry
__global__ void __launch_bounds__(256) nufft_sort_cell_kernel(const uint32_t *key, unsigned long long m, unsigned long long cells,
                                                              uint32_t *cell_start) {
    const unsigned long long q = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (q > cells) return;
    unsigned long long lo = 0, hi = m;  // key[i] < q for i < lo, key[i] >= q for i >= hi
    while (lo < hi) {
        const unsigned long long mid = (lo + hi) >> 1;
        if (key[mid] < q)
            lo = mid + 1;
        else
            hi = mid;
    }
    cell_start[q] = (uint32_t)lo;
}

hipError_t launch_nufft_sort_keys(const NufftSortArgs &a, hipStream_t stream) {
    hipLaunchKernelGGL(nufft_sort_key_kernel, dim3((unsigned)((a.m + 255) / 256)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

// the exclusive scan of data[0 .. n) in place; `partial`: room for the partials of every level above
static void nufft_sort_scan(uint32_t *data, unsigned long long n, uint32_t *partial, hipStream_t stream) {
    const unsigned long long groups = (n + kSortS - 1) / kSortS;
    if (groups > 1) {
        hipLaunchKernelGGL(nufft_sort_reduce_kernel, dim3((unsigned)groups), dim3(kSortS), 0, stream, (const uint32_t *)data, n, partial);
        nufft_sort_scan(partial, groups, partial + groups, stream);
    }
    hipLaunchKernelGGL(nufft_sort_scan_kernel, dim3((unsigned)groups), dim3(kSortS), 0, stream, data, n,
                       (const uint32_t *)(groups > 1 ? partial : nullptr));
}

hipError_t launch_nufft_sort_pairs(const NufftSortArgs &a, int *side, hipStream_t stream) {
    const unsigned passes = nufft_sort_passes(a.log_g1 + a.log_g2 + a.log_g3);
    NufftSortPass p{};
    p.m = a.m;
    p.groups = nufft_sort_groups(a.m);
    p.hist = a.hist;
    const unsigned long long n = kSortR * p.groups;
    int from = 0;
    for (unsigned pass = 0; pass < passes; ++pass, from ^= 1) {
        p.key_in = a.key[from];
        p.idx_in = a.idx[from];
        p.key_out = a.key[from ^ 1];
        p.idx_out = a.idx[from ^ 1];
        p.shift = pass * kNufftSortBits;
        hipLaunchKernelGGL(nufft_sort_hist_kernel, dim3((unsigned)p.groups), dim3(kSortT), 0, stream, p);
        nufft_sort_scan(a.hist, n, a.hist + n, stream);
        if (pass == 0)
            hipLaunchKernelGGL(nufft_sort_scatter_kernel<true>, dim3((unsigned)p.groups), dim3(kSortT), 0, stream, p);
        else
            hipLaunchKernelGGL(nufft_sort_scatter_kernel<false>, dim3((unsigned)p.groups), dim3(kSortT), 0, stream, p);
    }
    *side = from;
    return hipGetLastError();
}

hipError_t launch_nufft_sort_tables(const NufftSortArgs &a, int side, hipStream_t stream) {
    const unsigned long long cells = 1ull << (a.log_g1 + a.log_g2 + a.log_g3);
    hipLaunchKernelGGL(nufft_sort_table_kernel, dim3((unsigned)((a.m + 255) / 256)), dim3(256), 0, stream, a, (const uint32_t *)a.idx[side]);
    hipLaunchKernelGGL(nufft_sort_cell_kernel, dim3((unsigned)(cells / 256 + 1)), dim3(256), 0, stream, (const uint32_t *)a.key[side], a.m,
                       cells, a.cell_start);
    return hipGetLastError();
}

}  // namespace phast
