// nufft_sort_emu_test.cpp -- the kernels that build the point tables of the NUFFT planners on the device (csrc/nufft_sort.hip), run
// on the host under AddressSanitizer and UndefinedBehaviorSanitizer (tests/test_nufft_sort_emulator.py builds and runs it).  The
// histogram and the scatter count, scan and rank through LDS between barriers, so the program stands on tests/emu/block_shim.hpp:
// a workgroup's threads are fibers that run from one __syncthreads() to the next in ascending or in descending order, and every
// case runs in BOTH orders.  One translation unit with its own main, linked without the HIP runtime.  nufft_sort.hip is #included
// as it stands (it uses no atomics, so there is none to define here) and every kernel is driven through its own launchers,
// launch_nufft_sort_keys, _pairs and _tables, as planner_nufft_sort.hpp drives them.
//
// Buffers: the coordinates, the two key and two index arrays, the histogram (nufft_sort_hist_len entries), the flag and the
// tables are heap allocations of exactly the bytes the contract covers.
//
// The reference is the host path itself: nufft_bin and nufft_nd_bin on the same points.  perm, cell_start and
// xs / ys / zs must be EQUAL, bit for bit.
//
// Point sets: (u) uniform in [-3, 3); (c) clumped, every point within 1e-7 of 0.3; (d) duplicates, five distinct values; (e)
// the edge list (signed zeros, the smallest subnormals, -2^-130, which is cut to 0, -2^-60, which lands at 1 - 2^-53, 1 - 2^-53,
// +-1, 0.25, 0.5, +-(2^52 + 0.5), +-1e300, and q / n_g for a few q with the doubles just below and above) padded with (u).
//
// Sizes, with B = kNufftSortBlock and S = kNufftSortScan from the header: M = 1, 2, B - 1, B, B + 1, 3 B + 17, one M whose counts
// are two workgroups of the scan, and (argument "all") one M above S^2 B / 2^kNufftSortBits, where the scan of the counts has more
// than one workgroup at both levels below its top.  Grids: 1-D of 3, 8 and 9 bits (one, two and three passes: the sorted pairs end in either buffer), 2-D of 3 + 3 and
// 4 + 6 bits, 3-D of 3 + 5 + 4 bits, and ("all") 1-D of 20 bits.
#include <hip/hip_runtime.h>

#include "block_shim.hpp"

#include <cmath>
// any_len.hpp's chirp() (on nufft.hpp's include path, never called by these kernels) names the device's sincospi: a host
// overload so that the header compiles here
inline void sincospi(double t, double *s, double *c) {
    *s = std::sin(3.141592653589793238462643383279502884 * t);
    *c = std::cos(3.141592653589793238462643383279502884 * t);
}

#include "nufft_sort.hip"

#include "nufft_nd.hpp"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sanitizer_exit.hpp"

namespace {

using namespace phast;

int g_fails = 0;
unsigned long long g_compared = 0;
char g_case[256] = "";

void fail(const char *what, const char *fmt, ...) {
    if (++g_fails > 12) return;
    std::printf("FAIL %s [%s]: ", what, g_case);
    va_list ap;
    va_start(ap, fmt);
    std::vprintf(fmt, ap);
    va_end(ap);
    std::printf("\n");
}

double rnd(unsigned long long seed, unsigned long long i) {  // uniform in [0, 1)
    unsigned long long x = seed * 0x9E3779B97F4A7C15ull + i * 0xD1B54A32D192ED03ull + 0x2545F4914F6CDD1Dull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    x ^= x >> 31;
    return (double)(x >> 11) * 0x1p-53;
}

// exactly n elements on the heap
template <typename E> struct Buf {
    E *p;
    size_t n;
    explicit Buf(size_t n_) : p((E *)std::malloc(n_ ? n_ * sizeof(E) : 1)), n(n_) {
        if (!p) std::abort();
        std::memset(p, 0xCD, n * sizeof(E));
    }
    ~Buf() { std::free(p); }
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
};

std::vector<double> edge_list(unsigned log_g) {
    const double g = std::ldexp(1.0, (int)log_g);
    std::vector<double> e = {0.0,  -0.0,          5e-324,         -5e-324, -0x1p-130,     -0x1p-60, 1.0 - 0x1p-53, 1.0,
                             -1.0, 0.25,          0.5,            0x1p52 + 0.5, -(0x1p52 + 0.5), 1e300,    -1e300};
    for (double q : {1.0, 2.0, g / 2, g - 1}) {
        const double v = q / g;
        e.push_back(v);
        e.push_back(std::nextafter(v, -1.0));
        e.push_back(std::nextafter(v, 2.0));
    }
    return e;
}

// coordinate `axis` of point j of the set
void fill(char set, unsigned axis, unsigned log_g, double *x, size_t m) {
    const std::vector<double> e = edge_list(log_g);
    const double five[5] = {0.1, -0.7, 2.3, 1.1, 0.999};
    for (size_t j = 0; j < m; ++j) {
        const double u = rnd(17 + axis, j);
        if (set == 'u')
            x[j] = 6.0 * u - 3.0;
        else if (set == 'c')
            x[j] = 0.3 + (2.0 * u - 1.0) * 1e-7;
        else if (set == 'd')
            x[j] = five[(size_t)(u * 5.0) % 5];
        else
            x[j] = j < e.size() ? e[(j + 5 * axis) % e.size()] : 6.0 * u - 3.0;
    }
}

template <typename E> void same(const char *what, const E *got, const E *want, size_t n) {
    g_compared += n;
    if (std::memcmp(got, want, n * sizeof(E)) == 0) return;
    for (size_t i = 0; i < n; ++i)
        if (std::memcmp(got + i, want + i, sizeof(E)) != 0) {
            if (sizeof(E) == 8) {
                unsigned long long a, b;
                std::memcpy(&a, got + i, 8);
                std::memcpy(&b, want + i, 8);
                fail(what, "entry %zu of %zu is %016llx, the host path has %016llx", i, n, a, b);
            } else {
                unsigned a, b;
                std::memcpy(&a, got + i, 4);
                std::memcpy(&b, want + i, 4);
                fail(what, "entry %zu of %zu is %u, the host path has %u", i, n, a, b);
            }
            return;
        }
}

void run_case(unsigned dims, const unsigned (&lg)[3], size_t m, char set, block_shim::Order order) {
    std::snprintf(g_case, sizeof g_case, "%uD bits %u+%u+%u M=%zu set %c %s", dims, lg[0], lg[1], lg[2], m, set,
                  order == block_shim::kAscending ? "ascending" : "descending");
    block_shim::order = order;
    const size_t cells = (size_t)1 << (lg[0] + lg[1] + lg[2]);
    Buf<double> x(m), y(dims > 1 ? m : 0), z(dims > 2 ? m : 0);
    fill(set, 0, lg[0], x.p, m);
    if (dims > 1) fill(set, 1, lg[1], y.p, m);
    if (dims > 2) fill(set, 2, lg[2], z.p, m);
    // the host path
    std::vector<double> rxs(m), rys(m), rzs(m);
    std::vector<uint32_t> rperm(m), rcell(cells + 1);
    const double *const xin[3] = {x.p, y.p, z.p};
    double *const rs[3] = {rxs.data(), rys.data(), rzs.data()};
    if (dims == 1)
        nufft_bin(x.p, m, lg[0], rxs.data(), rperm.data(), rcell.data());
    else if (dims == 2)
        nufft_nd_bin<2>(xin, m, lg, rs, rperm.data(), rcell.data());
    else
        nufft_nd_bin<3>(xin, m, lg, rs, rperm.data(), rcell.data());
    // the device path
    Buf<uint32_t> k0(m), k1(m), i0(m), i1(m), hist(nufft_sort_hist_len(m)), flag(1), perm(m), cell(cells + 1);
    Buf<double> xs(m), ys(dims > 1 ? m : 0), zs(dims > 2 ? m : 0);
    NufftSortArgs a{};
    a.x = x.p;
    a.y = dims > 1 ? y.p : nullptr;
    a.z = dims > 2 ? z.p : nullptr;
    a.m = m;
    a.log_g1 = lg[0];
    a.log_g2 = lg[1];
    a.log_g3 = lg[2];
    a.key[0] = k0.p;
    a.key[1] = k1.p;
    a.idx[0] = i0.p;
    a.idx[1] = i1.p;
    a.hist = hist.p;
    a.flag = flag.p;
    a.perm = perm.p;
    a.cell_start = cell.p;
    a.xs = xs.p;
    a.ys = dims > 1 ? ys.p : nullptr;
    a.zs = dims > 2 ? zs.p : nullptr;
    flag.p[0] = 0;
    int side = -1;
    if (launch_nufft_sort_keys(a, nullptr) != hipSuccess || launch_nufft_sort_pairs(a, &side, nullptr) != hipSuccess) fail("launch", "error");
    if (flag.p[0] != 0) fail("flag", "raised for finite points");
    if (side != (int)(nufft_sort_passes(lg[0] + lg[1] + lg[2]) & 1)) fail("side", "the pairs ended in buffer %d", side);
    if (side != 0 && side != 1) return;
    if (launch_nufft_sort_tables(a, side, nullptr) != hipSuccess) fail("launch", "error");
    same("perm", perm.p, rperm.data(), m);
    same("cell_start", cell.p, rcell.data(), cells + 1);
    same("xs", xs.p, rxs.data(), m);
    if (dims > 1) same("ys", ys.p, rys.data(), m);
    if (dims > 2) same("zs", zs.p, rzs.data(), m);
}

// a coordinate that is not finite, at the first, a middle and the last point of each array: the flag, and nothing out of bounds
void run_flag(unsigned dims, size_t m) {
    const unsigned lg[3] = {4, dims > 1 ? 3u : 0u, dims > 2 ? 5u : 0u};
    const double bad[3] = {std::nan(""), HUGE_VAL, -HUGE_VAL};
    for (unsigned axis = 0; axis < dims; ++axis)
        for (size_t at : {(size_t)0, m / 2, m - 1}) {
            std::snprintf(g_case, sizeof g_case, "%uD M=%zu not finite: axis %u point %zu", dims, m, axis, at);
            Buf<double> x(m), y(dims > 1 ? m : 0), z(dims > 2 ? m : 0);
            fill('u', 0, lg[0], x.p, m);
            if (dims > 1) fill('u', 1, lg[1], y.p, m);
            if (dims > 2) fill('u', 2, lg[2], z.p, m);
            (axis == 0 ? x.p : axis == 1 ? y.p : z.p)[at] = bad[(axis + at) % 3];
            Buf<uint32_t> k0(m), flag(1);
            NufftSortArgs a{};
            a.x = x.p;
            a.y = dims > 1 ? y.p : nullptr;
            a.z = dims > 2 ? z.p : nullptr;
            a.m = m;
            a.log_g1 = lg[0];
            a.log_g2 = lg[1];
            a.log_g3 = lg[2];
            a.key[0] = k0.p;
            a.flag = flag.p;
            flag.p[0] = 0;
            launch_nufft_sort_keys(a, nullptr);
            ++g_compared;
            if (flag.p[0] == 0) fail("flag", "not raised");
        }
}

}  // namespace

// "small": the sizes up to 3 B + 17 on the small grids; "all" (the default): also the grid of 2^20 cells and the M that gives the scan
// of the counts a second level of partials
int main(int argc, char **argv) {
    const bool all = argc < 2 || !std::strcmp(argv[1], "all");
    if (!all && std::strcmp(argv[1], "small")) {
        std::printf("usage: %s [all|small]\n", argv[0]);
        return 2;
    }
    const size_t B = kNufftSortBlock, S = kNufftSortScan;
    std::printf("block %zu scan %zu bits %u\n", B, S, kNufftSortBits);
    const unsigned grids[][4] = {{1, 3, 0, 0}, {1, 8, 0, 0}, {1, 9, 0, 0}, {2, 3, 3, 0}, {2, 4, 6, 0}, {3, 3, 5, 4}};
    const size_t sizes[] = {1, 2, B - 1, B, B + 1, 3 * B + 17, (S / kNufftSortRadix + 1) * B + 1};  // the last: two workgroups of counts
    for (const auto &g : grids) {
        const unsigned lg[3] = {g[1], g[2], g[3]};
        for (size_t m : sizes)
            for (char set : {'u', 'c', 'd', 'e'})
                for (block_shim::Order order : {block_shim::kAscending, block_shim::kDescending}) run_case(g[0], lg, m, set, order);
    }
    for (unsigned dims = 1; dims <= 3; ++dims) run_flag(dims, B + 3);
    if (all) {
        const unsigned wide[3] = {20, 0, 0}, two[3] = {5, 0, 0};
        for (block_shim::Order order : {block_shim::kAscending, block_shim::kDescending}) {
            run_case(1, wide, 3 * B + 17, order == block_shim::kAscending ? 'e' : 'u', order);
            // 2^bits (M / B) counts > S^2: the partials of the first level are themselves more than one workgroup's
            const size_t big = S * S / kNufftSortRadix * B + 5;
            std::printf("scan: %llu counts, %llu and %llu partials\n", (unsigned long long)(kNufftSortRadix * nufft_sort_groups(big)),
                        (unsigned long long)((kNufftSortRadix * nufft_sort_groups(big) + S - 1) / S),
                        (unsigned long long)(((kNufftSortRadix * nufft_sort_groups(big) + S - 1) / S + S - 1) / S));
            run_case(1, two, big, order == block_shim::kAscending ? 'd' : 'u', order);
        }
    }
    block_shim::order = block_shim::kAscending;
    // every kernel was reached
    const char *const kernels[] = {"nufft_sort_key_kernel", "nufft_sort_hist_kernel", "nufft_sort_scatter_kernel<true>",
                                   "nufft_sort_scatter_kernel<false>", "nufft_sort_reduce_kernel", "nufft_sort_scan_kernel",
                                   "nufft_sort_table_kernel", "nufft_sort_cell_kernel"};
    std::snprintf(g_case, sizeof g_case, "coverage");
    for (const char *k : kernels) {
        unsigned long long n = 0;
        for (const auto &r : block_shim::ran)
            if (r.first.rfind(k, 0) == 0) n += r.second;
        std::printf("  ran %-34s %llu\n", k, n);
        if (n == 0) fail("coverage", "%s was never launched", k);
    }
    std::printf("launches %llu threads %llu barriers %llu elements %llu\n", block_shim::launches, block_shim::threads_run, block_shim::barriers,
                g_compared);
    std::printf("nufft_sort: %s (%d failures)\n", g_fails ? "FAILED" : "ok", g_fails);
    phast_test_exit(g_fails ? 1 : 0);
}
