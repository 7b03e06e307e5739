// channelizer_emu_test.cpp -- the fold of the polyphase channelizer (csrc/channelizer.hip, #included as it stands), run on the
// host under AddressSanitizer and UndefinedBehaviorSanitizer (tests/test_channelizer_emulator.py builds and runs it;
// tests/emu/block_shim.hpp runs a workgroup as fibers that meet at __syncthreads(): the kernel stages the signal through LDS).
// A stand-alone program: no GPU, no HIP runtime.
//
// The kernel is driven through its launcher with arguments built as ChannelizerPlanner::fold builds them: one plane into rows
// of M rounded up to 16 bytes (real signals; whole, and in chunks of 1 and of 5 rows of the flattened frame index) and two
// planes into rows of M (complex signals), aligned and one element off, for batches of 1 and 3, on heap blocks of exactly the
// contract's elements (one element too far is an AddressSanitizer report), in both fiber orders.  Taps and samples are
// m 2^-e with small integers m (never 0) and e in 0 .. 40: the products are exact, the sums round, so their bits depend on the
// order -- compared bit for bit with acc = fma(h[r0 + j M], x[m D - r0 - j M], acc), j = 0 .. T - 1 ascending from 0,
// r0 = (m D - p) mod M, taps beyond K and samples outside [0, L) zero.  Outputs start as a NaN bit pattern: an element the
// contract names must have lost it, every other one must have kept it.
#include <hip/hip_runtime.h>

#include "block_shim.hpp"

#include <cmath>
// any_len.hpp's chirp() (on channelizer.hpp's include path, never called by this kernel) names the device's sincospi: a host
// overload so that the header compiles here
inline void sincospi(double t, double *s, double *c) {
    *s = std::sin(3.141592653589793238462643383279502884 * t);
    *c = std::cos(3.141592653589793238462643383279502884 * t);
}

#include "channelizer.hip"

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
    std::printf("FAIL chan_fold [%s]: ", g_case);
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
    size_t len, k, m, d, first, out_frames;  // out_frames 0: full_frames - first
};

// planes: 1 (rows of fd, chunks of `chunk` rows; 0: whole) or 2 (rows of M, whole)
template <typename T> void run_fold(const Shape &s, int planes, size_t batch, size_t chunk, size_t off) {
    constexpr size_t V = Fp<T>::V;
    set_case("%s L=%zu K=%zu M=%zu D=%zu rot=%d first=%zu frames=%zu planes=%d batch=%zu chunk=%zu off=%zu", Fp<T>::name(), s.len, s.k,
             s.m, s.d, s.d % s.m ? 1 : 0, s.first, s.out_frames, planes, batch, chunk, off);
    if (chan_bad_args(s.len, s.k, s.m, s.d, s.first, s.out_frames)) {
        fail("the shape is refused");
        return;
    }
    // ChannelizerPlanner::init
    const size_t full = (size_t)chan_full_frames(s.len, s.k, s.d), n_out = s.out_frames ? s.out_frames : full - s.first;
    const size_t t = (size_t)chan_t(s.k, s.m), M = s.m;
    const ChanGeom g = chan_geom(s.k, s.m, s.d);
    const size_t ftiles = (n_out + g.frames - 1) / g.frames, ctiles = (M + g.cols - 1) / g.cols;
    const size_t ld_ = planes == 2 ? M : (M + V - 1) / V * V;
    Buf<T> table(t * M);
    for (size_t i = 0; i < t * M; ++i) table.p[i] = i < s.k ? wide<T>(5 * s.k + M, i) : T(0);
    const size_t sd = batch == 1 ? s.len : s.len + 3;
    Buf<T> x0((batch - 1) * sd + s.len, off), x1((batch - 1) * sd + s.len, off);
    for (size_t b = 0; b < batch; ++b)
        for (size_t j = 0; j < s.len; ++j) {
            x0.p[b * sd + j] = wide<T>(7 * s.len + b, j);
            x1.p[b * sd + j] = wide<T>(11 * s.len + b, j);
        }
    const std::vector<T> keep0(x0.base, x0.base + x0.n + x0.off), keep1(x1.base, x1.base + x1.n + x1.off);
    const size_t total = batch * n_out, rows = chunk ? chunk : total;
    for (int order = 0; order < 2; ++order) {
        block_shim::order = order ? block_shim::kDescending : block_shim::kAscending;
        for (size_t q0 = 0; q0 < total; q0 += rows) {
            const size_t c = total - q0 < rows ? total - q0 : rows;
            Buf<T> o0(c * ld_, off), o1(planes == 2 ? c * ld_ : 0, off);
            ChanArgs a{};  // ChannelizerPlanner::fold
            a.x[0] = x0.p;
            a.x[1] = planes == 2 ? x1.p : nullptr;
            a.out[0] = o0.p;
            a.out[1] = planes == 2 ? o1.p : nullptr;
            a.taps = table.p;
            a.sig_dist = sd;
            a.ld = ld_;
            a.len = s.len;
            a.t = t;
            a.m = M;
            a.d = s.d;
            a.first = s.first;
            a.out_frames = n_out;
            a.q0 = q0;
            a.count = c;
            const size_t q1 = q0 + c - 1;
            a.ft0 = q0 / n_out * ftiles + q0 % n_out / g.frames;
            a.ftn = q1 / n_out * ftiles + q1 % n_out / g.frames - a.ft0 + 1;
            a.ftiles = ftiles;
            a.ctiles = ctiles;
            a.groups = (u64)planes * a.ftn * ctiles * 256;
            a.dqv = (unsigned)(g.frames > 1 ? s.d / M : 0);
            a.dm = (unsigned)(s.d % M);
            a.sq = (unsigned)(g.per > 1 ? g.fpp * s.d / M : 0);
            a.sm = (unsigned)(g.per > 1 ? g.fpp * s.d % M : 0);
            a.geom = g;
            if (launch_chan_fold<T>(a, nullptr) != hipSuccess) fail("the launcher failed");
            for (int pl = 0; pl < planes; ++pl) {
                const Buf<T> &x = pl ? x1 : x0, &o = pl ? o1 : o0;
                for (size_t r = 0; r < c; ++r) {
                    const size_t b = (q0 + r) / n_out, i = (q0 + r) % n_out;
                    const long long md = (long long)((s.first + i) * s.d);
                    for (size_t p = 0; p < ld_; ++p) {
                        if (p >= M) {
                            if (!o.is_sentinel((long long)(r * ld_ + p))) fail("the padding of row %zu was written at %zu", r, p);
                            continue;
                        }
                        long long r0 = (md - (long long)p) % (long long)M;
                        if (r0 < 0) r0 += (long long)M;
                        T acc = T(0);
                        for (size_t j = 0; j < t; ++j) {
                            const size_t ti = (size_t)r0 + j * M;
                            const long long n = md - r0 - (long long)(j * M);
                            const T h = ti < s.k ? table.p[ti] : T(0);
                            const T v = n >= 0 && n < (long long)s.len ? x.p[b * sd + n] : T(0);
                            acc = std::fma(h, v, acc);
                        }
                        ++g_compared;
                        const T got = o.p[r * ld_ + p];
                        if (!same_bits(got, acc))
                            fail("plane %d frame %zu of signal %zu column %zu = %.17Lg, must be exactly %.17Lg (thread order %d)", pl, i, b, p,
                                 (ld)got, (ld)acc, order);
                        if (s.first + i >= full && !same_bits(got, T(0))) fail("frame %zu of signal %zu, beyond full_frames, is not 0", i, b);
                    }
                }
                for (size_t e = 1; e <= off; ++e)
                    if (!o.is_sentinel(-(long long)e)) fail("the element in front of the rows was written");
            }
        }
    }
    block_shim::order = block_shim::kAscending;
    if (std::memcmp(keep0.data(), x0.base, keep0.size() * sizeof(T)) || std::memcmp(keep1.data(), x1.base, keep1.size() * sizeof(T)))
        fail("the signals were written");
}

// the geometry the kernel trusts: rows x cols within LDS, for the shapes here and a sweep of small ones
void check_geom(size_t k, size_t m, size_t d) {
    const ChanGeom g = chan_geom(k, m, d);
    if (g.frames != g.fpp * g.per || g.rows != g.span + g.jc - 1 || (u64)g.rows * g.cols > kChanLds || g.jc < 1 || g.fpp * g.cols > 256 ||
        g.per > kChanPerThread || g.span < ((g.frames - 1) * (u64)d + m - 1) / m + 2) {
        set_case("K=%zu M=%zu D=%zu", k, m, d);
        fail("the geometry does not fit: cols %u fpp %u per %u span %u jc %u rows %u", g.cols, g.fpp, g.per, g.span, g.jc, g.rows);
    }
}

}  // namespace

int main() {
    // tests/channelizer_reference.py's cases, the long ones on shorter signals, and windows around the tile: one less, exactly
    // one, one more, past full_frames
    const Shape shapes[] = {
        {1, 1, 1, 1, 0, 0},        {1, 1, 1, 1, 1, 1025},      {37, 24, 8, 8, 0, 0},        {37, 24, 8, 8, 3, 127},     {37, 24, 8, 4, 0, 0},
        {37, 24, 8, 4, 3, 129},    {41, 21, 6, 4, 0, 0},       {41, 21, 6, 4, 3, 168},      {30, 50, 7, 3, 0, 0},       {30, 50, 7, 3, 3, 145},
        {20, 5, 8, 8, 0, 0},       {33, 17, 5, 5, 0, 0},       {64, 32, 8, 12, 0, 0},       {9, 4, 3, 1, 0, 0},         {9, 4, 3, 1, 3, 341},
        {600, 1030, 257, 257, 0, 0}, {600, 1030, 257, 257, 3, 5}, {900, 2048, 256, 192, 0, 0}, {900, 2048, 256, 192, 3, 3},
        {1500, 4100, 1024, 1024, 0, 0}, {1100, 8200, 4, 4, 0, 0}, {1100, 8200, 4, 4, 3, 257},  {50, 9, 300, 7, 0, 0},    {40, 3, 2, 1000, 0, 0},
        {5000, 40, 16, 40, 0, 0},
    };
    for (const Shape &s : shapes) {
        check_geom(s.k, s.m, s.d);
        for (size_t batch = 1; batch <= 3; batch += 2)
            for (size_t off = 0; off < 2; ++off) {
                if (s.k > 1000 && batch != 1 + 2 * off) continue;  // the long filters: batch 1 aligned, batch 3 one element off
                run_fold<double>(s, 2, batch, 0, off);
                run_fold<float>(s, 2, batch, 0, off);
                for (size_t chunk : {(size_t)0, (size_t)1, (size_t)5}) {
                    if (chunk && (s.k > 1000 || s.out_frames > 200)) continue;
                    run_fold<double>(s, 1, batch, chunk, off);
                    run_fold<float>(s, 1, batch, chunk, off);
                }
            }
    }
    for (size_t m = 1; m <= 600; m += (m < 20 ? 1 : 37))
        for (size_t d : {(size_t)1, (size_t)3, m, 2 * m + 1, (size_t)5000, (size_t)1 << 29})
            for (size_t k : {(size_t)1, 4 * m + 1, (size_t)1 << 20}) check_geom(k, m, d);
    std::printf("channelizer: ");
    block_shim::print_counters();
    std::printf("channelizer: elements %llu checked\n", g_compared);
    std::printf("channelizer: %s (%d failures, %d of them at D mod M = 0)\n", g_fails ? "FAILED" : "ok", g_fails, g_fails_rot0);
    phast_test_exit(g_fails ? 1 : 0);
}
