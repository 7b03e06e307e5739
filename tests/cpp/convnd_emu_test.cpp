// convnd_emu_test.cpp -- the tile and save sweeps of N-d overlap-save convolution (csrc/convnd.hip, #included as it stands), run on
// the host under AddressSanitizer and UndefinedBehaviorSanitizer (tests/test_convnd_emulator.py builds and runs it;
// tests/emu/sweep_shim.hpp turns a launch into a serial loop).  A stand-alone program: no GPU, no HIP runtime.
//
// Both kernels are driven through launch_convnd with arguments built as ConvNdPlanner::dev builds them, from the geometry of
// convnd_bad_args, per chunk of tiles.  Arrays and taps hold small integers, so every sum below is exact in float and in double
// and the checks are bit for bit:
//     tile sweep   every element of every workspace tile against x~ of the definition, zeros in the padding up to fd;
//     (transforms) y = the cyclic convolution of the tile with g in the tile's shape, summed here in long double: what the R2C,
//                  the spectrum sweep and the C2R compute between the two sweeps;
//     save sweep   the caller's output, after all chunks, against full[t0 + i] of the definition summed directly.
// Buffers are heap allocations of exactly the bytes the contract covers (one element too far is an AddressSanitizer report);
// an "unaligned" buffer is one element longer and used from element 1.  Outputs and workspaces start as a NaN bit pattern: an
// element the contract names must have lost it, every other one (the lead-in, the gaps between the arrays of a batch) must
// have kept its exact bits.  The spectrum sweep between the two is conv.hip's: tests/cpp/sweep_emu_test.cpp has it.
#include <hip/hip_runtime.h>

#include "sweep_shim.hpp"

#include "convnd.hip"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sanitizer_exit.hpp"

using namespace phast;

namespace {

using ld = long double;

template <typename T> struct Fp;
template <> struct Fp<double> {
    using bits = unsigned long long;
    static constexpr bits sentinel = 0x7ff8dead5eed0001ull;  // a quiet NaN no kernel produces
    static constexpr size_t V = 2;
    static const char *name() { return "f64"; }
};
template <> struct Fp<float> {
    using bits = unsigned;
    static constexpr bits sentinel = 0x7fc5eed1u;
    static constexpr size_t V = 4;
    static const char *name() { return "f32"; }
};

int g_fails = 0;
unsigned long long g_compared = 0;
char g_case[320] = "";

void set_case(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(g_case, sizeof g_case, fmt, ap);
    va_end(ap);
}
void fail(const char *kernel, const char *fmt, ...) {
    if (++g_fails > 12) return;
    std::printf("FAIL %s [%s]: ", kernel, g_case);
    va_list ap;
    va_start(ap, fmt);
    std::vprintf(fmt, ap);
    va_end(ap);
    std::printf("\n");
}

// an allocation of exactly n elements of T behind `off` elements of lead-in (off = 1: an element-aligned pointer)
template <typename T> struct Buf {
    using bits = typename Fp<T>::bits;
    T *base = nullptr, *p = nullptr;
    size_t n, off;
    Buf(size_t n_, size_t off_ = 0) : n(n_), off(off_) {
        void *q = nullptr;
        const size_t bytes = (n + off) * sizeof(T);
        if (posix_memalign(&q, 16, bytes ? bytes : 1)) std::abort();
        base = (T *)q;
        p = base + off;
        for (size_t i = 0; i < n + off; ++i) std::memcpy(base + i, &Fp<T>::sentinel, sizeof(T));
    }
    ~Buf() { std::free(base); }
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    bool is_sentinel(long long i) const {  // i >= -off
        bits b;
        std::memcpy(&b, p + i, sizeof(T));
        return b == Fp<T>::sentinel;
    }
};

unsigned long long mix(unsigned long long seed, unsigned long long i) {
    unsigned long long x = seed * 0x9E3779B97F4A7C15ull + i * 0xD1B54A32D192ED03ull + 0x2545F4914F6CDD1Dull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
int small_int(unsigned long long seed, unsigned long long i, int amp) {  // in [-amp, amp], never 0: a zero fill cannot pass for data
    const int v = (int)(mix(seed, i) % (unsigned)(2 * amp)) - amp;
    return v >= 0 ? v + 1 : v;
}

struct Shape {
    size_t rank, len[3], k[3], b[3];
};

// ConvNdPlanner::dev's arguments for the geometry g
ConvNdArgs args_of(const ConvNdGeom &g, size_t fd, size_t sig_dist, size_t out_dist) {
    ConvNdArgs a{};
    a.sig_dist = sig_dist;
    a.out_dist = out_dist;
    a.fd = fd;
    a.tiles = (unsigned)g.tiles;
    a.pts = (unsigned)g.tile_pts;
    for (unsigned i = 0; i < kConvNdMaxRank; ++i) {
        a.len[i] = (unsigned)g.len[i];
        a.k1[i] = (unsigned)(g.k[i] - 1);
        a.b[i] = (unsigned)g.b[i];
        a.s[i] = (unsigned)g.s[i];
        a.t0[i] = (unsigned)g.t0[i];
        a.n_out[i] = (unsigned)g.out[i];
        a.segs[i] = (unsigned)g.segs[i];
    }
    return a;
}

template <typename T> void run_case(const Shape &sh, int mode, int flip, size_t batch, size_t off, size_t rows) {
    constexpr size_t V = Fp<T>::V;
    ConvNdGeom g{};
    const bool bad = convnd_bad_args(sh.len, sh.k, sh.rank, mode, flip, sh.b, V, &g) != 0;
    set_case("%s L=%llu,%llu,%llu K=%llu,%llu,%llu B=%llu,%llu,%llu mode=%d flip=%d batch=%zu off=%zu chunk=%zu", Fp<T>::name(), g.len[0],
             g.len[1], g.len[2], g.k[0], g.k[1], g.k[2], g.b[0], g.b[1], g.b[2], mode, flip, batch, off, rows);
    if (bad) {  // every case the caller sends is legal
        fail("convnd_bad_args", "rejects a shape of the table (rank %zu, first axis %zu)", sh.rank, sh.len[0]);
        return;
    }
    const size_t L0 = g.len[0], L1 = g.len[1], L2 = g.len[2], K0 = g.k[0], K1 = g.k[1], K2 = g.k[2];
    const size_t B0 = g.b[0], B1 = g.b[1], B2 = g.b[2], O0 = g.out[0], O1 = g.out[1], O2 = g.out[2];
    const size_t sig_pts = g.sig_pts, out_pts = g.out_pts, pts = g.tile_pts, tiles = g.tiles, fd = conv_row(pts, V);
    const size_t sd = batch == 1 ? sig_pts : sig_pts + 1, od = batch == 1 ? out_pts : out_pts + 3, total = batch * tiles;
    Buf<T> x((batch - 1) * sd + sig_pts, off), out((batch - 1) * od + out_pts, off);
    std::vector<int> taps(K0 * K1 * K2);
    for (size_t i = 0; i < taps.size(); ++i) taps[i] = small_int(31 * K2 + K0, i, 4);
    for (size_t b = 0; b < batch; ++b)
        for (size_t i = 0; i < sig_pts; ++i) x.p[b * sd + i] = (T)small_int(17 * L2 + b, i, 8);
    auto xt = [&](size_t b, long long i0, long long i1, long long i2) -> ld {  // x~ of array b
        if (i0 < 0 || i0 >= (long long)L0 || i1 < 0 || i1 >= (long long)L1 || i2 < 0 || i2 >= (long long)L2) return 0;
        return (ld)x.p[b * sd + ((size_t)i0 * L1 + (size_t)i1) * L2 + (size_t)i2];
    };
    auto gt = [&](size_t j0, size_t j1, size_t j2) -> ld {  // g: the taps, reversed along every axis for correlation
        return (ld)(flip ? taps[((K0 - 1 - j0) * K1 + (K1 - 1 - j1)) * K2 + (K2 - 1 - j2)] : taps[(j0 * K1 + j1) * K2 + j2]);
    };
    ConvNdArgs a = args_of(g, fd, sd, od);
    const unsigned gpr = (unsigned)convnd_save_groups(g.s[2], V);
    for (size_t q0 = 0; q0 < total; q0 += rows) {
        const size_t c = total - q0 < rows ? total - q0 : rows;
        Buf<T> w(c * fd);
        a.q0 = q0;
        a.q1 = q0 + c;
        a.in = x.p;
        a.out = w.p;
        a.gpt = (unsigned)(fd / V);
        a.groups = c * a.gpt;
        if (launch_convnd<T>(kConvNdTile, a, nullptr) != hipSuccess) fail("convnd_tile_kernel", "the launcher failed");
        std::vector<ld> y(c * pts);
        for (size_t r = 0; r < c; ++r) {
            const size_t b = (q0 + r) / tiles, t = (q0 + r) % tiles, s2 = t % g.segs[2], s1 = t / g.segs[2] % g.segs[1],
                         s0 = t / g.segs[2] / g.segs[1];
            const long long o0 = convnd_src0(g, 0, s0), o1 = convnd_src0(g, 1, s1), o2 = convnd_src0(g, 2, s2);
            for (size_t f = 0; f < fd; ++f) {  // the tile sweep's contract
                const size_t j2 = f % B2, j1 = f / B2 % B1, j0 = f / B2 / B1;
                const ld want = f < pts ? xt(b, o0 + (long long)j0, o1 + (long long)j1, o2 + (long long)j2) : 0;
                ++g_compared;
                if (w.is_sentinel((long long)(r * fd + f))) fail("convnd_tile_kernel", "tile %zu element %zu was not written", r, f);
                else if (!((ld)w.p[r * fd + f] == want))
                    fail("convnd_tile_kernel", "tile %zu element %zu = %.9Lg, must be exactly %.9Lg", r, f, (ld)w.p[r * fd + f], want);
            }
            // what the transforms make of the tile: its cyclic convolution with g.  Only the saved corner is needed
            for (size_t a0 = 0; a0 < convnd_yield(g, 0, s0); ++a0)
                for (size_t a1 = 0; a1 < convnd_yield(g, 1, s1); ++a1)
                    for (size_t a2 = 0; a2 < convnd_yield(g, 2, s2); ++a2) {
                        ld acc = 0;
                        for (size_t j0 = 0; j0 < K0; ++j0)
                            for (size_t j1 = 0; j1 < K1; ++j1)
                                for (size_t j2 = 0; j2 < K2; ++j2)
                                    acc += gt(j0, j1, j2) * (ld)w.p[r * fd + ((K0 - 1 + a0 - j0) * B1 + (K1 - 1 + a1 - j1)) * B2 + (K2 - 1 + a2 - j2)];
                        y[r * pts + ((K0 - 1 + a0) * B1 + (K1 - 1 + a1)) * B2 + (K2 - 1 + a2)] = acc;
                    }
        }
        for (size_t r = 0; r < c; ++r)  // the C2R's output in the workspace rows; what is never saved is poison
            for (size_t f = 0; f < fd; ++f) {
                const size_t j2 = f % B2, j1 = f / B2 % B1, j0 = f / B2 / B1;
                const bool corner = f < pts && j0 >= K0 - 1 && j1 >= K1 - 1 && j2 >= K2 - 1;
                w.p[r * fd + f] = corner ? (T)y[r * pts + f] : (T)1e30;
            }
        a.in = w.p;
        a.out = out.p;
        a.gpr = gpr;
        a.gpt = (unsigned)(g.s[0] * g.s[1] * gpr);
        a.groups = c * a.gpt;
        if (launch_convnd<T>(kConvNdSave, a, nullptr) != hipSuccess) fail("convnd_save_kernel", "the launcher failed");
    }
    // after all chunks: every output sample against the definition, summed directly; the gaps and the lead-in untouched
    for (size_t b = 0; b < batch; ++b) {
        for (size_t i0 = 0; i0 < O0; ++i0)
            for (size_t i1 = 0; i1 < O1; ++i1)
                for (size_t i2 = 0; i2 < O2; ++i2) {
                    ld want = 0;
                    for (size_t j0 = 0; j0 < K0; ++j0)
                        for (size_t j1 = 0; j1 < K1; ++j1)
                            for (size_t j2 = 0; j2 < K2; ++j2)
                                want += gt(j0, j1, j2) * xt(b, (long long)(g.t0[0] + i0) - (long long)j0, (long long)(g.t0[1] + i1) - (long long)j1,
                                                            (long long)(g.t0[2] + i2) - (long long)j2);
                    const size_t i = b * od + (i0 * O1 + i1) * O2 + i2;
                    ++g_compared;
                    if (out.is_sentinel((long long)i)) fail("convnd_save_kernel", "out[%zu,%zu,%zu] of array %zu was not written", i0, i1, i2, b);
                    else if (!((ld)out.p[i] == want))
                        fail("convnd_save_kernel", "out[%zu,%zu,%zu] of array %zu = %.9Lg, must be exactly %.9Lg", i0, i1, i2, b, (ld)out.p[i], want);
                }
        if (b + 1 < batch)
            for (size_t i = out_pts; i < od; ++i)
                if (!out.is_sentinel((long long)(b * od + i))) fail("convnd_save_kernel", "the gap behind output %zu was written", b);
    }
    for (size_t i = 1; i <= off; ++i)
        if (!out.is_sentinel(-(long long)i)) fail("convnd_save_kernel", "the element in front of the output was written");
}

}  // namespace

int main(int argc, char **argv) {
    // the shapes the schedule was first tried on and (70,300; 17,5; 64,32); one whose odd tile rows straddle 16-byte groups
    // well inside a wide array (the fast path's row condition decides there, not the array's edge); and a rank-3 one with an
    // odd number of tile points, whose padding up to fd continues into rows that lie inside the array
    const Shape shapes[] = {{2, {9, 7}, {3, 4}, {4, 4}},       {2, {20, 13}, {5, 3}, {8, 8}},  {2, {12, 10}, {1, 4}, {1, 8}},
                            {2, {5, 6}, {7, 9}, {8, 16}},      {2, {10, 11}, {4, 5}, {6, 17}}, {3, {6, 5, 7}, {2, 3, 2}, {4, 4, 4}},
                            {2, {70, 300}, {17, 5}, {64, 32}}, {2, {6, 40}, {2, 3}, {3, 7}},   {3, {5, 4, 6}, {2, 2, 3}, {3, 3, 5}}};
    const bool quick = argc > 1 && !std::strcmp(argv[1], "quick");  // the self-tests of the checker: the small shapes only
    for (const Shape &sh : shapes) {
        const bool large = sh.len[1] >= 300;
        if (quick && large) continue;
        for (int mode = 0; mode < 3; ++mode) {
            bool has = true;
            for (size_t i = 0; i < sh.rank; ++i) has = has && (mode != kConvValid || sh.len[i] >= sh.k[i]);
            if (!has) continue;
            for (int flip = 0; flip < 2; ++flip)
                for (size_t rows : {(size_t)1 << 20, (size_t)1, (size_t)2})
                    for (size_t off = 0; off < 2; ++off) {
                        if (large && (flip != (mode & 1) || (rows == 1 && off))) continue;  // the direct sums of the large shape take time
                        run_case<double>(sh, mode, flip, 1, off, rows);
                        run_case<float>(sh, mode, flip, 1, off, rows);
                        if (!large) {
                            run_case<double>(sh, mode, flip, 2, off, rows);
                            run_case<float>(sh, mode, flip, 2, off, rows);
                        }
                    }
        }
    }
    std::printf("convnd: launches %llu threads %llu elements %llu bit-exact\n", sweep_shim::launches, sweep_shim::threads_run, g_compared);
    std::printf("convnd: %s (%d failures)\n", g_fails ? "FAILED" : "ok", g_fails);
    phast_test_exit(g_fails ? 1 : 0);
}
