// block_emu_test.cpp -- the kernels that move data through LDS between barriers (nd.hip, bitrev.hip, twiddle.hip and the digest of
// fill.hip), run on the host under AddressSanitizer and UndefinedBehaviorSanitizer (tests/test_block_emulator.py builds and runs it;
// tests/emu/block_shim.hpp runs a workgroup as fibers that meet at __syncthreads()).  One translation unit per product file
// (BLOCK_PART = 1..4, the file #included as it stands) and one for main (BLOCK_PART = 0).  argv[1] names the part; argv[2] may narrow nd to
// one element type or to the quotient check, and bitrev to the cases of one kernel (the checker's self-tests do: a mutant is caught
// by a part of a part).
//
// Every case: buffers of exactly the bytes the contract covers, each a heap block of its own, so one element too far is an
// AddressSanitizer report; outputs start as a sentinel bit pattern; the inputs of the pure data movers are distinct integers
// stored as bit patterns, so one misplaced element is visible, and they are compared as bits.  Every case runs twice, with the
// threads of a workgroup in ascending and in descending order between two barriers: a barrier that is missing gives wrong bits
// in at least one of them.
#ifndef BLOCK_PART
#error "compile with -DBLOCK_PART=0 (main) .. 4"
#endif

#if BLOCK_PART == 0
// ------------------------------------------------------------------------------------------------------------ main
#include <cstdio>
#include <cstring>

#include "sanitizer_exit.hpp"

int block_nd(const char *only);
int block_bitrev(const char *only);
int block_twiddle(const char *only);
int block_digest(const char *only);

int main(int argc, char **argv) {
    struct Part {
        const char *name;
        int (*run)(const char *);
    };
    const Part parts[] = {{"nd", block_nd}, {"bitrev", block_bitrev}, {"twiddle", block_twiddle}, {"digest", block_digest}};
    int fails = 0, ran = 0;
    for (const Part &p : parts) {
        if (argc > 1 && std::strcmp(argv[1], p.name) != 0) continue;
        ++ran;
        const int f = p.run(argc > 2 ? argv[2] : "");
        std::printf("%s: %s (%d failures)\n", p.name, f ? "FAILED" : "ok", f);
        fails += f;
    }
    if (!ran) {
        std::printf("usage: %s [nd [f64|f32|fdiv] | bitrev [kernel] | twiddle | digest]\n", argv[0]);
        phast_test_exit(2);
    }
    phast_test_exit(fails ? 1 : 0);
}

#else
// ------------------------------------------------------------------------------------------------------------ a part
#include <hip/hip_runtime.h>

#include "block_shim.hpp"

#if BLOCK_PART == 1
#include "nd.hip"
#elif BLOCK_PART == 2
#include "bitrev.hip"
#elif BLOCK_PART == 3
#include "twiddle.hip"
#include "plan.hpp"  // host_tw3, tw3_bits_for: the tables as TwiddleGrid uploads them
#elif BLOCK_PART == 4
#include "fill.hip"
#endif

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

namespace {

using ld = long double;
using u64 = unsigned long long;
using u32 = unsigned;

template <typename T> struct Fp;
template <> struct Fp<double> {
    using bits = u64;
    [[maybe_unused]] static constexpr ld u = 0x1p-53L;
    [[maybe_unused]] static constexpr bits sentinel = 0x7ff8dead5eed0001ull;  // a quiet NaN no kernel produces
    [[maybe_unused]] static constexpr size_t V = 2;
    static const char *name() { return "f64"; }
};
template <> struct Fp<float> {
    using bits = u32;
    [[maybe_unused]] static constexpr ld u = 0x1p-24L;
    [[maybe_unused]] static constexpr bits sentinel = 0x7fc5eed1u;
    [[maybe_unused]] static constexpr size_t V = 4;
    static const char *name() { return "f32"; }
};

char g_case[320] = "";
int g_fails = 0, g_printed = 0;

void set_case(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(g_case, sizeof g_case, fmt, ap);
    va_end(ap);
}
// FAIL <kernel instantiation> [case]: ...; the first few are printed, the count is in the summary line
void fail(const std::string &kernel, const char *fmt, ...) {
    ++g_fails;
    if (++g_printed > 40) return;
    std::printf("FAIL %s [%s]: ", kernel.c_str(), g_case);
    va_list ap;
    va_start(ap, fmt);
    std::vprintf(fmt, ap);
    va_end(ap);
    std::printf("\n");
}
const char *order_name() { return block_shim::order == block_shim::kAscending ? "ascending" : "descending"; }

// an allocation of exactly n elements of T behind `off` elements of lead-in (off = 1: one element off a 16-byte boundary);
// the elements are handled as bit patterns
template <typename T> struct Buf {
    using bits = typename Fp<T>::bits;
    T *base = nullptr, *p = nullptr;
    size_t n;
    explicit Buf(size_t n_, size_t off = 0) : n(n_) {
        void *q = nullptr;
        const size_t bytes = (n + off) * sizeof(T);
        if (posix_memalign(&q, 16, bytes ? bytes : 1)) std::abort();
        base = (T *)q;
        p = base + off;
        for (size_t i = 0; i < off; ++i) std::memcpy(base + i, &Fp<T>::sentinel, sizeof(T));
    }
    ~Buf() { std::free(base); }
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    bits get(size_t i) const {
        bits b;
        std::memcpy(&b, p + i, sizeof(T));
        return b;
    }
    void set(size_t i, bits b) { std::memcpy(p + i, &b, sizeof(T)); }
    Buf &sentinel() {
        for (size_t i = 0; i < n; ++i) set(i, Fp<T>::sentinel);
        return *this;
    }
};

int report(const char *prefix) {
    for (const auto &kv : block_shim::ran)
        if (kv.first.find(prefix) != std::string::npos || !*prefix) std::printf("  ran %-64s %6llu launches\n", kv.first.c_str(), kv.second);
    block_shim::print_counters();
    return g_fails;
}
// every name of `must` has been launched: the shim's launch knows the instantiation
void require_ran(const std::vector<std::string> &must) {
    set_case("coverage");
    for (const std::string &k : must) {
        bool found = false;
        for (const auto &kv : block_shim::ran) found |= kv.first.find(k) != std::string::npos;
        if (!found) fail(k, "this instantiation was never launched: the cases no longer reach it");
    }
}

}  // namespace

// ============================================================================================================ nd.hip
#if BLOCK_PART == 1
namespace {
using namespace phast;

// the launcher's span, written a second time: wide-side entries per narrow tile
template <typename T> size_t span_of(size_t S, bool vw) {
    constexpr size_t TS = 256 / sizeof(T), E = TS * TS, V = 16 / sizeof(T);
    const size_t pitch = S | 1;
    return (vw ? E * V / (V * pitch + 1) : E / pitch) & ~(size_t)7;
}

// one matrix shape and one buffer arrangement, in both thread orders.  dist_kind: 0 = R C (batch 1), 1 = a multiple of V with a
// gap, 2 = odd with a gap
template <typename T> void nd_case(size_t R, size_t C, size_t batch, int dist_kind, size_t src_off, size_t dst_off) {
    using bits = typename Fp<T>::bits;
    constexpr size_t V = Fp<T>::V;
    const size_t rc = R * C;
    size_t sd = rc, dd = rc;
    if (dist_kind == 1) {
        sd = (rc + V - 1) / V * V + V;
        dd = (rc + V - 1) / V * V + 2 * V;
    } else if (dist_kind == 2) {
        sd = (rc + 2) | 1;
        dd = (rc + 4) | 1;
    }
    const size_t sn = (batch - 1) * sd + rc, dn = (batch - 1) * dd + rc;
    Buf<T> sre(sn, src_off), sim(sn, src_off), dre(dn, dst_off), dim_(dn, dst_off);
    for (size_t i = 0; i < sn; ++i) {
        sre.set(i, (bits)(1 + i));
        sim.set(i, (bits)(0x40000001u + i));
    }
    for (int ord = 0; ord < 2; ++ord) {
        block_shim::order = ord ? block_shim::kDescending : block_shim::kAscending;
        set_case("%s R=%zu C=%zu batch=%zu src_dist=%zu dst_dist=%zu src_off=%zu dst_off=%zu %s", Fp<T>::name(), R, C, batch, sd, dd,
                 src_off, dst_off, order_name());
        dre.sentinel();
        dim_.sentinel();
        const hipError_t e = launch_nd_transpose<T>(sre.p, sim.p, dre.p, dim_.p, batch, R, C, sd, dd, nullptr);
        const std::string k = block_shim::last_kernel;
        if (e != hipSuccess) fail(k, "the launcher returned %d", (int)e);
        for (int pl = 0; pl < 2; ++pl) {
            const Buf<T> &s = pl ? sim : sre, &d = pl ? dim_ : dre;
            const bits tag = pl ? 0x40000001u : 1u;
            for (size_t i = 0; i < sn; ++i)
                if (s.get(i) != (bits)(tag + i)) fail(k, "source %s[%zu] was changed", pl ? "im" : "re", i);
            std::vector<char> named(dn, 0);
            for (size_t b = 0; b < batch; ++b)
                for (size_t r = 0; r < R; ++r)
                    for (size_t c = 0; c < C; ++c) {
                        const size_t at = b * dd + c * R + r;
                        named[at] = 1;
                        const bits want = s.get(b * sd + r * C + c), got = d.get(at);
                        if (got != want)
                            fail(k, "%s: dst[b=%zu][c=%zu][r=%zu] holds %#llx, must hold src[b][r][c] = %#llx%s", pl ? "im" : "re", b, c, r,
                                 (u64)got, (u64)want, got == Fp<T>::sentinel ? " (never written)" : "");
                    }
            for (size_t i = 0; i < dn; ++i)
                if (!named[i] && d.get(i) != Fp<T>::sentinel) fail(k, "%s: the gap element dst[%zu] between matrices was written", pl ? "im" : "re", i);
        }
    }
}

// the buffer arrangements of one shape: batch 1 with every plane aligned / one element off (the four combinations reach the
// four (wide side, flat run) vectorisations of the narrow kernels independently), batch 2 at a distance that is a multiple of V
// and at an odd one
template <typename T> void nd_shape(size_t R, size_t C, bool batches) {
    nd_case<T>(R, C, 1, 0, 0, 0);
    nd_case<T>(R, C, 1, 0, 1, 1);
    nd_case<T>(R, C, 1, 0, 0, 1);
    nd_case<T>(R, C, 1, 0, 1, 0);
    if (!batches) return;
    nd_case<T>(R, C, 2, 1, 0, 0);
    nd_case<T>(R, C, 2, 1, 1, 1);
    nd_case<T>(R, C, 2, 2, 0, 0);
}

template <typename T> void nd_all() {
    constexpr size_t TS = 256 / sizeof(T), V = Fp<T>::V;
    // narrow, every S: the wide side from the span the launcher will compute.  (The vectorised span is the smaller one; a wide
    // side that is a multiple of V is laid out from it, and is then at least as many tiles under the element-wise span's cases.)
    for (size_t S = 1; S < TS; ++S) {
        const size_t sv = span_of<T>(S, true), se = span_of<T>(S, false);
        // less than one span (W >= S keeps S the narrow side; where span - V < S that is S itself, below the element-wise span)
        const size_t w_less = sv - V >= S ? sv - V : S;
        const size_t w_vtail = 2 * sv + 3 * V;  // two spans and a ragged tail that is a multiple of V
        const size_t w_odd = 2 * se + 5;        // two spans and an odd tail
        for (int orient = 0; orient < 2; ++orient) {
            nd_shape<T>(orient ? S : w_less, orient ? w_less : S, false);
            nd_shape<T>(orient ? S : w_vtail, orient ? w_vtail : S, true);
            nd_shape<T>(orient ? S : w_odd, orient ? w_odd : S, true);
        }
    }
    // square: ragged tiles on either edge
    const size_t sides[4] = {TS, TS + 1, 2 * TS - 1, 2 * TS + V};
    for (size_t R : sides)
        for (size_t C : sides) nd_shape<T>(R, C, true);
}

// fdiv(x, 1.0f / d) == x / d for every divisor the kernels can form and every x below the largest tile's E (host IEEE
// arithmetic: the device's own rounding of 1.0f / d is checked on the device, tests/test_gpu_nd.py)
void fdiv_all() {
    std::set<unsigned> divisors;
    for (unsigned S = 1; S < 64; ++S) {
        divisors.insert(S);
        if (S < 32) {
            divisors.insert((unsigned)(span_of<double>(S, true) / 2));
            divisors.insert((unsigned)span_of<double>(S, false));
        }
        divisors.insert((unsigned)(span_of<float>(S, true) / 4));
        divisors.insert((unsigned)span_of<float>(S, false));
    }
    unsigned long long checked = 0;
    for (unsigned d : divisors) {
        const float inv = 1.0f / (float)d;
        for (unsigned x = 0; x < 4096; ++x, ++checked)
            if (fdiv(x, inv) != x / d) {
                set_case("x=%u d=%u", x, d);
                fail("fdiv", "fdiv(x, 1.0f / d) = %u, x / d = %u", fdiv(x, inv), x / d);
                goto done;  // the first (x, d) names the defect
            }
    }
done:
    std::printf("  fdiv: %zu divisors (1 .. %u), %llu quotients\n", divisors.size(), *divisors.rbegin(), checked);
}

}  // namespace

int block_nd(const char *only) {
    auto on = [&](const char *what) { return !*only || !std::strcmp(only, what); };
    if (!on("f64") && !on("f32") && !on("fdiv")) fail("nd", "no such selection: %s", only);
    if (!*only || on("fdiv")) fdiv_all();
    if (on("f64")) nd_all<double>();
    if (on("f32")) nd_all<float>();
    std::vector<std::string> must;
    for (const char *t : {"double", "float"})
        if (on(t[0] == 'd' ? "f64" : "f32"))
        for (const char *a : {"true", "false"})
            for (const char *b : {"true", "false"}) {
                must.push_back(std::string("nd_transpose_square<") + t + ", " + a + ", " + b + ">");
                for (const char *c : {"true", "false"}) must.push_back(std::string("nd_transpose_narrow<") + t + ", " + a + ", " + b + ", " + c + ">");
            }
    require_ran(must);  // all 24 instantiations, 12 per type
    return report("nd_transpose");
}
#endif

// ============================================================================================================ bitrev.hip
#if BLOCK_PART == 2
namespace {
using namespace phast;

unsigned rev_bits(unsigned x, unsigned bits) {
    unsigned r = 0;
    for (unsigned i = 0; i < bits; ++i) r |= ((x >> i) & 1u) << (bits - 1 - i);
    return r;
}

// {tile(p) : p < pairs} is every t with t <= rev(t), once
void pair_enum_all() {
    for (unsigned m = 0; m <= 20; ++m) {
        set_case("tile bits m=%u", m);
        const PairEnum pe(m);
        std::vector<char> seen((size_t)1 << m, 0);
        unsigned long long want = 0;
        for (unsigned t = 0; t < (1u << m); ++t) want += t <= rev_bits(t, m);
        if (pe.pairs != want) fail("PairEnum", "pairs = %llu, there are %llu tiles with t <= rev(t)", pe.pairs, want);
        for (unsigned long long p = 0; p < pe.pairs; ++p) {
            const unsigned t = pe.tile((unsigned)p);
            if (t >= (1u << m)) fail("PairEnum", "tile(%llu) = %u is no tile", p, t);
            else if (t > rev_bits(t, m)) fail("PairEnum", "tile(%llu) = %u > rev = %u: the pair's other name", p, t, rev_bits(t, m));
            else if (seen[t]++) fail("PairEnum", "tile(%llu) = %u comes twice", p, t);
        }
        for (unsigned t = 0; t < (1u << m); ++t)
            if (t <= rev_bits(t, m) && !seen[t]) fail("PairEnum", "the pair of tile %u is never enumerated", t);
    }
}

// `run(data, log_n, batch, dist)` permutes `batch` arrays in place: out[i] = in[rev(i)], gaps and neighbours untouched
const char *g_only = "";
template <typename U, typename Run> void bitrev_case(const char *what, unsigned log_n, size_t batch, size_t dist, Run run) {
    if (*g_only && !std::strstr(what, g_only)) return;
    const size_t n = (size_t)1 << log_n, total = (batch - 1) * dist + n;
    constexpr U kSentinel = (U)0xdead5eed0badc0deull;
    for (int ord = 0; ord < 2; ++ord) {
        block_shim::order = ord ? block_shim::kDescending : block_shim::kAscending;
        set_case("%s u%zu log_n=%u batch=%zu dist=%zu %s", what, 8 * sizeof(U), log_n, batch, dist, order_name());
        void *q = nullptr;
        if (posix_memalign(&q, 16, total * sizeof(U))) std::abort();
        U *x = (U *)q;
        for (size_t i = 0; i < total; ++i) x[i] = kSentinel;
        for (size_t b = 0; b < batch; ++b)
            for (size_t i = 0; i < n; ++i) x[b * dist + i] = (U)(((b + 1) << 24) + i);
        const unsigned long long before = block_shim::launches;
        const hipError_t e = run(x, log_n, batch, dist);
        const std::string k = block_shim::last_kernel;
        if (e != hipSuccess) fail(k, "the launcher returned %d", (int)e);
        if (block_shim::launches == before) fail(what, "nothing was launched");
        std::vector<char> named(total, 0);
        for (size_t b = 0; b < batch; ++b)
            for (size_t i = 0; i < n; ++i) {
                named[b * dist + i] = 1;
                const U want = (U)(((b + 1) << 24) + rev_bits((unsigned)i, log_n)), got = x[b * dist + i];
                if (got != want) fail(k, "array %zu: out[%zu] = %#llx, must be in[rev] = %#llx", b, i, (u64)got, (u64)want);
            }
        for (size_t i = 0; i < total; ++i)
            if (!named[i] && x[i] != kSentinel) fail(k, "the gap element [%zu] between arrays was written", i);
        std::free(x);
    }
}

// batch 1, and 3 at n + 2 (and at n + 1 where the kernel moves single elements)
template <typename U, typename Run> void bitrev_sizes(const char *what, unsigned lo, unsigned hi, bool elementwise, Run run) {
    for (unsigned log_n = lo; log_n <= hi; ++log_n) {
        const size_t n = (size_t)1 << log_n;
        bitrev_case<U>(what, log_n, 1, n, run);
        bitrev_case<U>(what, log_n, 3, n + 2, run);
        if (elementwise) bitrev_case<U>(what, log_n, 3, n + 1, run);
    }
}

// a persistent kernel launched with FEWER workgroups than work items, so that every workgroup walks several pairs: the
// prefetch of the next pair and the barrier that waits for the previous pair's readers do something only then
template <typename U, int BETA, typename Launch> void shrunken(const char *what, unsigned log_n, Launch launch) {
    bitrev_case<U>(what, log_n, 3, ((size_t)1 << log_n) + 2, [&](U *x, unsigned ln, size_t batch, size_t dist) {
        const unsigned tiles = 1u << (ln - 2 * BETA);
        const unsigned long long total = PairEnum(ln - 2 * BETA).pairs * batch;
        if (total < 10) fail(what, "only %llu work items: the grid of 3 does not walk", total);
        launch(x, ln, dist, tiles, total);
        return hipSuccess;
    });
}

}  // namespace

int block_bitrev(const char *only) {
    g_only = only;
    if (!*only) pair_enum_all();
    auto simple64 = [](u64 *x, unsigned l, size_t b, size_t d) { return launch_bitrev_u<u64, 6, 512>(x, l, b, d, nullptr); };
    auto simple32 = [](u32 *x, unsigned l, size_t b, size_t d) { return launch_bitrev_u<u32, 6, 512>(x, l, b, d, nullptr); };
    bitrev_sizes<u64>("simple", 1, 11, true, simple64);
    bitrev_sizes<u32>("simple", 1, 11, true, simple32);
    bitrev_sizes<u64>("tiled", 10, 11, true, [](u64 *x, unsigned l, size_t b, size_t d) { return launch_bitrev_u<u64, 5, 256>(x, l, b, d, nullptr); });
    // launch_bitrev<float> hands launch_bitrev_u<unsigned, 6, 512> only sizes below 2^12, which the simple kernel takes: the
    // tiled instantiation it carries is reached through the launcher template itself
    bitrev_sizes<u32>("tiled", 12, 13, true, simple32);
    bitrev_sizes<u64>("persistent1", 12, 17, true,
                      [](u64 *x, unsigned l, size_t b, size_t d) { return launch_bitrev_persistent<u64, 6, 512>(x, l, b, d, nullptr, 4); });
    bitrev_sizes<u32>("persistent1", 12, 17, true,
                      [](u32 *x, unsigned l, size_t b, size_t d) { return launch_bitrev_persistent<u32, 6, 512>(x, l, b, d, nullptr, 4); });
    bitrev_sizes<u64>("persistent2", 12, 17, false,
                      [](u64 *x, unsigned l, size_t b, size_t d) { return launch_bitrev_persistent2<u64, 6, 256, true>(x, l, b, d, nullptr, 4); });
    bitrev_sizes<u64>("persistent3", 14, 19, false,
                      [](u64 *x, unsigned l, size_t b, size_t d) { return launch_bitrev_persistent3<u64, 7, 1024>(x, l, b, d, nullptr); });
    // the public launchers, at the sizes where they stay small
    bitrev_sizes<u64>("launch_bitrev<double>", 9, 12, true,
                      [](u64 *x, unsigned l, size_t b, size_t d) { return launch_bitrev<double>(reinterpret_cast<double *>(x), l, b, d, nullptr); });
    bitrev_sizes<u32>("launch_bitrev<float>", 11, 12, true,
                      [](u32 *x, unsigned l, size_t b, size_t d) { return launch_bitrev<float>(reinterpret_cast<float *>(x), l, b, d, nullptr); });

    shrunken<u64, 6>("persistent1 grid=3", 15, [](u64 *x, unsigned l, size_t d, unsigned tiles, u64 total) {
        hipLaunchKernelGGL((phast::bitrev_persistent_kernel<unsigned long long, 6, 512>), dim3(3), dim3(512), 0, nullptr, x, l, d, tiles, total);
    });
    shrunken<u32, 6>("persistent1 grid=3", 15, [](u32 *x, unsigned l, size_t d, unsigned tiles, u64 total) {
        hipLaunchKernelGGL((phast::bitrev_persistent_kernel<unsigned int, 6, 512>), dim3(3), dim3(512), 0, nullptr, x, l, d, tiles, total);
    });
    shrunken<u64, 6>("persistent2 grid=3", 15, [](u64 *x, unsigned l, size_t d, unsigned tiles, u64 total) {
        hipLaunchKernelGGL((phast::bitrev_persistent2_kernel<unsigned long long, 6, 256, true>), dim3(3), dim3(256), 0, nullptr, x, l, d, tiles, total);
    });
    shrunken<u64, 7>("persistent3 grid=3", 17, [](u64 *x, unsigned l, size_t d, unsigned tiles, u64 total) {
        hipLaunchKernelGGL((phast::bitrev_persistent3_kernel<unsigned long long, 7, 1024>), dim3(3), dim3(1024), sizeof(u64) * 128 * 129, nullptr, x,
                           l, d, tiles, total);
    });

    if (!*only)
        require_ran({"bitrev_simple_kernel<unsigned long long>", "bitrev_simple_kernel<unsigned int>", "bitrev_tiled_kernel<unsigned long long, 5, 256>",
                     "bitrev_tiled_kernel<unsigned int, 6, 512>", "bitrev_persistent_kernel<unsigned long long, 6, 512>",
                     "bitrev_persistent_kernel<unsigned int, 6, 512>", "bitrev_persistent2_kernel<unsigned long long, 6, 256, true>",
                     "bitrev_persistent3_kernel<unsigned long long, 7, 1024>", "launch_bitrev_persistent3"});
    return report("");
}
#endif

// ============================================================================================================ twiddle.hip
#if BLOCK_PART == 3
namespace {
using namespace phast;

ld rnd(u64 seed, u64 i) {  // uniform in [-1, 1), exact in float
    u64 x = seed * 0x9E3779B97F4A7C15ull + i * 0xD1B54A32D192ED03ull + 0x2545F4914F6CDD1Dull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    x ^= x >> 31;
    return (ld)(long long)(x >> 43) * 0x1p-20L - 1.0L;
}

// block (r, c) *= W_N^((row0 + r)(col0 + c)), in place, rows at row_pitch.  The gate is that of one complex multiply by a
// table twiddle as tests/cpp/sweep_emu_test.cpp counts it (r2c_gate there): the twiddle is a product of three table entries of
// unit modulus, 7 roundings, the two products with it 1 and their sum 1: (9 + 2) u_T times the magnitude of the operand
template <typename T> void twiddle_case(unsigned log_n, size_t rows, size_t cols, size_t pitch, size_t row0, size_t col0) {
    using bits = typename Fp<T>::bits;
    const ld kPi = 3.141592653589793238462643383279502884L, gate_k = (ld)(9 + 2) * Fp<T>::u;
    const unsigned tw_bits = tw3_bits_for(log_n);
    const std::vector<cx_t<T>> tab = host_tw3<T>(log_n, tw_bits);
    // the kernel reads the table through `tw3`: a heap block of exactly its bytes
    Buf<T> tabbuf(2 * tab.size());
    std::memcpy(tabbuf.p, tab.data(), tab.size() * sizeof(cx_t<T>));
    const size_t total = (rows - 1) * pitch + cols;
    const u64 N = 1ull << log_n;
    for (int ord = 0; ord < 2; ++ord) {
        block_shim::order = ord ? block_shim::kDescending : block_shim::kAscending;
        set_case("%s log_n=%u rows=%zu cols=%zu pitch=%zu row0=%zu col0=%zu %s", Fp<T>::name(), log_n, rows, cols, pitch, row0, col0, order_name());
        Buf<T> re(total), im(total);
        re.sentinel();
        im.sentinel();
        std::vector<ld> xr(total), xi(total);
        for (size_t r = 0; r < rows; ++r)
            for (size_t c = 0; c < cols; ++c) {
                const size_t at = r * pitch + c;
                re.p[at] = (T)(xr[at] = rnd(7 * rows + cols, at));
                im.p[at] = (T)(xi[at] = rnd(11 * rows + cols, at));
            }
        TwiddleGridArgs a{};
        a.re = re.p;
        a.im = im.p;
        a.tw3 = tabbuf.p;
        a.rows = rows;
        a.cols = cols;
        a.row_pitch = pitch;
        a.row0 = row0;
        a.col0 = col0;
        a.log_n = log_n;
        a.tw_bits = tw_bits;
        const hipError_t e = launch_twiddle_grid<T>(a, nullptr);
        const std::string k = block_shim::last_kernel;
        if (e != hipSuccess) fail(k, "the launcher returned %d", (int)e);
        double worst = 0;
        for (size_t r = 0; r < rows; ++r)
            for (size_t c = 0; c < pitch && r * pitch + c < total; ++c) {
                const size_t at = r * pitch + c;
                if (c >= cols) {
                    if (re.get(at) != Fp<T>::sentinel || im.get(at) != Fp<T>::sentinel) fail(k, "the pad element [%zu][%zu] between rows was written", r, c);
                    continue;
                }
                const u64 ex = ((row0 + r) * (col0 + c)) % N;
                const ld t = 2 * kPi * (ld)ex / (ld)N, wr = cosl(t), wi = -sinl(t);
                const ld rr = xr[at] * wr - xi[at] * wi, ri = xr[at] * wi + xi[at] * wr, gate = gate_k * (fabsl(xr[at]) + fabsl(xi[at]));
                const ld er = fabsl((ld)re.p[at] - rr), ei = fabsl((ld)im.p[at] - ri);
                if (re.get(at) == (bits)Fp<T>::sentinel) fail(k, "[%zu][%zu] was not written", r, c);
                else if (!(er <= gate) || !(ei <= gate))
                    fail(k, "[%zu][%zu] = (%.17Lg, %.17Lg), reference (%.17Lg, %.17Lg): error %.3Lg > gate %.3Lg", r, c, (ld)re.p[at], (ld)im.p[at], rr,
                         ri, er > ei ? er : ei, gate);
                else if (gate > 0 && (double)((er > ei ? er : ei) / gate) > worst) worst = (double)((er > ei ? er : ei) / gate);
            }
        std::printf("  %s [%s]: worst error / gate %.3f\n", k.c_str(), g_case, worst);
    }
}

}  // namespace

int block_twiddle(const char *) {
    // rows x cols no multiple of the grid (2 x 5 workgroups of 256 columns); then one that makes every thread walk the columns
    // (more than 64 x 256 of them) with a table of three levels
    twiddle_case<double>(12, 5, 300, 307, 3, 1000);
    twiddle_case<float>(12, 5, 300, 307, 3, 1000);
    twiddle_case<double>(20, 3, 16500, 16503, 37, 20000);
    twiddle_case<float>(20, 3, 16500, 16503, 37, 20000);
    require_ran({"twiddle_grid_kernel<double>", "twiddle_grid_kernel<float>"});
    return report("");
}
#endif

// ============================================================================================================ fill.hip
#if BLOCK_PART == 4
namespace {
using namespace phast;

// digest[b] = {sum re, sum im, sum (re^2 + im^2), re[probe]}.  The inputs are positive, so every sum is the sum of its terms'
// magnitudes and the bound of an f64 summation of n terms in any order, (n - 1) u (1 + O(u)) relative, is within n 2^-52
template <typename T> void digest_case(size_t n, size_t batch, size_t dist, size_t probe) {
    const size_t total = (batch - 1) * dist + n;
    Buf<T> re(total), im(total);
    re.sentinel();
    im.sentinel();
    u64 x = 0x9E3779B97F4A7C15ull * (n + 1);
    auto next = [&]() {
        x ^= x << 13;
        x ^= x >> 7;
        x ^= x << 17;
        return (T)((ld)(x >> 11) * 0x1p-53L + 0x1p-30L);  // (0, 1]
    };
    for (size_t b = 0; b < batch; ++b)
        for (size_t i = 0; i < n; ++i) {
            re.p[b * dist + i] = next();
            im.p[b * dist + i] = next();
        }
    for (int ord = 0; ord < 2; ++ord) {
        block_shim::order = ord ? block_shim::kDescending : block_shim::kAscending;
        set_case("%s n=%zu batch=%zu dist=%zu probe=%zu %s", Fp<T>::name(), n, batch, dist, probe, order_name());
        Buf<double> dg(4 * batch);
        dg.sentinel();
        const hipError_t e = launch_digest<T>(re.p, im.p, n, batch, dist, probe, dg.p, nullptr);
        const std::string k = block_shim::last_kernel;
        if (e != hipSuccess) fail(k, "the launcher returned %d", (int)e);
        for (size_t b = 0; b < batch; ++b) {
            ld s[3] = {0, 0, 0};
            for (size_t i = 0; i < n; ++i) {
                const ld a = (ld)re.p[b * dist + i], c = (ld)im.p[b * dist + i];
                s[0] += a;
                s[1] += c;
                s[2] += a * a + c * c;
            }
            for (int j = 0; j < 3; ++j) {
                const ld got = (ld)dg.p[4 * b + j], err = fabsl(got - s[j]), gate = (ld)n * 0x1p-52L * s[j];
                if (dg.get(4 * b + j) == Fp<double>::sentinel) fail(k, "digest[%zu][%d] was not written", b, j);
                else if (!(err <= gate)) fail(k, "digest[%zu][%d] = %.17Lg, reference %.17Lg: error %.3Lg > gate %.3Lg", b, j, got, s[j], err, gate);
            }
            const double want = (double)re.p[b * dist + (probe < n ? probe : 0)];
            if (std::memcmp(&want, dg.p + 4 * b + 3, sizeof want)) fail(k, "digest[%zu][3] = %.17g, the probe re[%zu] = %.17g", b, dg.p[4 * b + 3], probe, want);
        }
    }
}

}  // namespace

int block_digest(const char *) {
    for (size_t n : {1, 255, 256, 257, 1000})
        for (size_t probe : {(size_t)0, n / 2, n - 1, n + 5}) {
            digest_case<double>(n, 3, n + 3, probe);
            digest_case<float>(n, 3, n + 3, probe);
        }
    require_ran({"digest_kernel<double>", "digest_kernel<float>"});
    return report("");
}
#endif

#endif  // BLOCK_PART != 0
