// synthesizer_emu_test.cpp -- the unfold of the polyphase synthesis bank (csrc/synthesizer.hip, #included as it stands), run on
// the host under AddressSanitizer and UndefinedBehaviorSanitizer (tests/test_synthesizer_emulator.py builds and runs it;
// tests/emu/block_shim.hpp runs a workgroup as fibers).  A stand-alone program: no GPU, no HIP runtime.
//
// The kernels are driven through their launchers with arguments built as SynthesizerPlanner::unfold builds them: one plane
// (real output) and two planes (complex output) of rows of M rounded up to 16 bytes -- and, for M = 1, of the caller's dense
// rows --, aligned and one element off, for batches of 1 and 3 at an odd output distance, on heap blocks of exactly the
// contract's elements (one element too far is an AddressSanitizer report), in both fiber orders.  Taps and rows are m 2^-e with
// small integers m (never 0) and e in 0 .. 40: the products are exact, the sums round, so their bits depend on the order --
// compared bit for bit with acc = fma(tab[n - m D], v[m][n mod M], acc), m = m_lo .. m_hi ascending from 0.  Outputs start as a
// NaN bit pattern: a sample the contract names must have lost it, every other element must have kept it.  The copy sweep (two
// planes into padded rows; one plane with two columns zeroed) is checked the same way.
#include <hip/hip_runtime.h>

#include "block_shim.hpp"

#include <cmath>
// any_len.hpp's chirp() (on synthesizer.hpp's include path, never called by these kernels) names the device's sincospi: a host
// overload so that the header compiles here
inline void sincospi(double t, double *s, double *c) {
    *s = std::sin(3.141592653589793238462643383279502884 * t);
    *c = std::cos(3.141592653589793238462643383279502884 * t);
}

#include "synthesizer.hip"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sanitizer_exit.hpp"

using namespace phast;

namespace {

using ld = long double;
using u64 = unsigned long long;

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

int g_fails = 0, g_fails_rot0 = 0;  // all; those in shapes whose hop is a multiple of M
u64 g_compared = 0;
char g_case[320] = "";

void set_case(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(g_case, sizeof g_case, fmt, ap);
    va_end(ap);
}
void fail(const char *fmt, ...) {
    if (std::strstr(g_case, "rot=0")) ++g_fails_rot0;
    if (++g_fails > 12) return;
    std::printf("FAIL synth_unfold [%s]: ", g_case);
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
template <typename T> bool same_bits(T a, T b) { return std::memcmp(&a, &b, sizeof(T)) == 0; }

u64 mix(u64 seed, u64 i) {
    u64 x = seed * 0x9E3779B97F4A7C15ull + i * 0xD1B54A32D192ED03ull + 0x2545F4914F6CDD1Dull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
int small_int(u64 seed, u64 i, int amp) {  // in [-amp, amp], never 0: a zero fill cannot pass for data
    const int v = (int)(mix(seed, i) % (unsigned)(2 * amp)) - amp;
    return v >= 0 ? v + 1 : v;
}
// m 2^-e: exact products, sums that round
template <typename T> T wide(u64 seed, u64 i) { return (T)std::ldexp((double)small_int(seed, i, 8), -(int)(mix(seed + 1, i) % 41)); }

struct Shape {
    size_t f, k, m, d, first, out_len;  // out_len 0: full_len - first
};

// planes: 1 or 2; dense: rows of M (the M = 1 path of complex output), else rows of M rounded up to 16 bytes
template <typename T> void run_unfold(const Shape &s, int planes, size_t batch, size_t off, bool dense) {
    constexpr size_t V = Fp<T>::V;
    set_case("%s F=%zu K=%zu M=%zu D=%zu rot=%d first=%zu out=%zu planes=%d batch=%zu off=%zu dense=%d", Fp<T>::name(), s.f, s.k, s.m,
             s.d, s.d % s.m ? 1 : 0, s.first, s.out_len, planes, batch, off, (int)dense);
    if (synth_bad_args(s.f, s.k, s.m, s.d, s.first, s.out_len)) {
        fail("the shape is refused");
        return;
    }
    // SynthesizerPlanner::init
    const size_t full = (size_t)synth_full_len(s.f, s.k, s.d), n_out = s.out_len ? s.out_len : full - s.first, M = s.m;
    const SynthGeom g = synth_geom(s.k, s.m, s.d);
    const size_t tiles = (n_out + g.tile - 1) / g.tile;
    const size_t ld_ = dense ? M : (M + V - 1) / V * V;
    Buf<T> table(s.k);
    for (size_t i = 0; i < s.k; ++i) table.p[i] = wide<T>(5 * s.k + M, i);
    // the rows: every element of a row's padding keeps the sentinel (a NaN: a read of it poisons the sum)
    const size_t rows = batch * s.f;
    Buf<T> v0((rows - 1) * ld_ + M, off), v1((rows - 1) * ld_ + M, off);
    for (size_t r = 0; r < rows; ++r)
        for (size_t p = 0; p < M; ++p) {
            v0.p[r * ld_ + p] = wide<T>(7 * s.f + r, p);
            v1.p[r * ld_ + p] = wide<T>(11 * s.f + r, p);
        }
    const std::vector<T> keep0(v0.base, v0.base + v0.n + v0.off), keep1(v1.base, v1.base + v1.n + v1.off);
    const size_t od = batch == 1 ? n_out : (n_out + 3) | 1;
    for (int order = 0; order < 2; ++order) {
        block_shim::order = order ? block_shim::kDescending : block_shim::kAscending;
        Buf<T> o0((batch - 1) * od + n_out, off), o1(planes == 2 ? (batch - 1) * od + n_out : 0, off);
        SynthArgs a{};  // SynthesizerPlanner::unfold
        a.v[0] = v0.p;
        a.v[1] = planes == 2 ? v1.p : nullptr;
        a.out[0] = o0.p;
        a.out[1] = planes == 2 ? o1.p : nullptr;
        a.taps = table.p;
        a.ld = ld_;
        a.out_dist = od;
        a.f = s.f;
        a.k = s.k;
        a.m = M;
        a.d = s.d;
        a.first = s.first;
        a.out_len = n_out;
        a.count = batch;
        a.tiles = tiles;
        a.groups = (u64)planes * batch * tiles * 256;
        a.geom = g;
        if (launch_synth_unfold<T>(a, nullptr) != hipSuccess) fail("the launcher failed");
        for (int pl = 0; pl < planes; ++pl) {
            const Buf<T> &v = pl ? v1 : v0, &o = pl ? o1 : o0;
            for (size_t b = 0; b < batch; ++b) {
                for (size_t i = 0; i < n_out; ++i) {
                    const u64 n = s.first + i;
                    const long long lo = (long long)synth_m_lo(n, s.k, s.d), hi = synth_m_hi(n, s.f, s.d);
                    T acc = T(0);
                    for (long long m = lo; m <= hi; ++m)
                        acc = std::fma(table.p[n - (u64)m * s.d], v.p[(b * s.f + (size_t)m) * ld_ + n % M], acc);
                    ++g_compared;
                    const T got = o.p[b * od + i];
                    if (!same_bits(got, acc))
                        fail("plane %d sample %zu of signal %zu = %.17Lg, must be exactly %.17Lg (thread order %d)", pl, i, b, (ld)got,
                             (ld)acc, order);
                    if (n >= full && !same_bits(got, T(0))) fail("sample %zu of signal %zu, beyond full_len, is not 0", i, b);
                }
                if (b + 1 < batch)
                    for (size_t i = n_out; i < od; ++i)
                        if (!o.is_sentinel((long long)(b * od + i))) fail("the gap behind signal %zu was written at %zu", b, i);
            }
            for (size_t e = 1; e <= off; ++e)
                if (!o.is_sentinel(-(long long)e)) fail("the element in front of the signals was written");
        }
    }
    block_shim::order = block_shim::kAscending;
    if (std::memcmp(keep0.data(), v0.base, keep0.size() * sizeof(T)) || std::memcmp(keep1.data(), v1.base, keep1.size() * sizeof(T)))
        fail("the rows were written");
}

// the copy sweep: dense rows of M of two planes into rows of M rounded up to 16 bytes; the padding keeps the sentinel.
// zero: one plane into dense rows with the columns 0 and M / 2 written as 0
template <typename T> void run_copy(size_t rows, size_t M, size_t off, bool zero) {
    constexpr size_t V = Fp<T>::V;
    set_case("%s copy rows=%zu M=%zu rot=0 off=%zu zero=%d", Fp<T>::name(), rows, M, off, (int)zero);
    const size_t ld_ = zero ? M : (M + V - 1) / V * V;
    const int planes = zero ? 1 : 2;
    Buf<T> i0(rows * M, off), i1(rows * M, off), o0((rows - 1) * ld_ + M), o1((rows - 1) * ld_ + M);
    for (size_t e = 0; e < rows * M; ++e) {
        i0.p[e] = wide<T>(13 * M, e);
        i1.p[e] = wide<T>(17 * M, e);
    }
    SynthCopyArgs a{};
    a.in[0] = i0.p;
    a.in[1] = i1.p;
    a.out[0] = o0.p;
    a.out[1] = o1.p;
    a.n = M;
    a.in_ld = M;
    a.out_ld = ld_;
    a.rows = rows;
    a.zero_a = zero ? 0 : M;
    a.zero_b = zero ? M / 2 : M;
    if (zero) a.in[1] = a.out[1] = nullptr;
    a.groups = (u64)planes * rows * M;
    if (launch_synth_copy<T>(a, nullptr) != hipSuccess) fail("the launcher failed");
    for (int pl = 0; pl < planes; ++pl) {
        const Buf<T> &in = pl ? i1 : i0, &o = pl ? o1 : o0;
        for (size_t r = 0; r < rows; ++r)
            for (size_t p = 0; p < ld_ && r * ld_ + p < o.n; ++p) {
                ++g_compared;
                const T want = p >= M || (zero && (p == 0 || p == M / 2)) ? T(0) : in.p[r * M + p];
                if (p >= M ? !o.is_sentinel((long long)(r * ld_ + p)) : !same_bits(o.p[r * ld_ + p], want))
                    fail("plane %d row %zu column %zu is wrong", pl, r, p);
            }
    }
}

}  // namespace

int main() {
    // tests/synthesizer_reference.py's cases, the long ones with fewer frames, and windows around the tile: one less, exactly
    // one, one more, past full_len
    const Shape shapes[] = {
        {1, 1, 1, 1, 0, 0},      {1, 1, 1, 1, 1, 1025},     {5, 24, 8, 8, 0, 0},      {5, 24, 8, 8, 3, 1023},     {7, 25, 8, 4, 0, 0},
        {7, 25, 8, 4, 3, 1025},  {6, 21, 6, 4, 0, 0},       {6, 21, 6, 4, 3, 1024},   {4, 50, 7, 3, 0, 0},        {4, 50, 7, 3, 3, 58},
        {5, 5, 8, 8, 0, 0},      {6, 32, 8, 12, 0, 0},      {9, 4, 3, 1, 0, 0},       {9, 4, 3, 1, 12, 2},        {4, 1030, 257, 257, 0, 0},
        {4, 1030, 257, 257, 3, 1800}, {14, 2048, 256, 192, 0, 0}, {14, 2048, 256, 192, 3, 4543}, {6, 4100, 1024, 1024, 0, 0},
        {300, 8200, 4, 4, 0, 0}, {300, 8200, 4, 4, 3, 1025}, {50, 9, 300, 7, 0, 0},   {40, 3, 2, 1000, 0, 0},     {3000, 40, 16, 40, 0, 0},
        {700, 3, 5, 300, 200000, 5000},
    };
    for (const Shape &s : shapes) {
        for (size_t batch = 1; batch <= 3; batch += 2)
            for (size_t off = 0; off < 2; ++off) {
                if (s.k > 1000 && batch != 1 + 2 * off) continue;  // the long filters: batch 1 aligned, batch 3 one element off
                for (int planes = 1; planes <= 2; ++planes) {
                    run_unfold<double>(s, planes, batch, off, false);
                    run_unfold<float>(s, planes, batch, off, false);
                }
                if (s.m == 1) {
                    run_unfold<double>(s, 2, batch, off, true);
                    run_unfold<float>(s, 2, batch, off, true);
                }
            }
    }
    for (size_t off = 0; off < 2; ++off)
        for (size_t m : {(size_t)1, (size_t)3, (size_t)8, (size_t)257})
            for (size_t rows : {(size_t)1, (size_t)5, (size_t)300}) {
                for (bool zero : {false, true}) {
                    run_copy<double>(rows, m, off, zero);
                    run_copy<float>(rows, m, off, zero);
                }
            }
    std::printf("synthesizer: ");
    block_shim::print_counters();
    std::printf("synthesizer: elements %llu checked\n", g_compared);
    std::printf("synthesizer: %s (%d failures, %d of them at D mod M = 0)\n", g_fails ? "FAILED" : "ok", g_fails, g_fails_rot0);
    phast_test_exit(g_fails ? 1 : 0);
}
