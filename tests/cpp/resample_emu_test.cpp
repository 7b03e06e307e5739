// resample_emu_test.cpp -- the kernels of sample-rate conversion (csrc/resample.hip, #included as it stands), run on the host
// under AddressSanitizer and UndefinedBehaviorSanitizer (tests/test_resample_emulator.py builds and runs it; tests/emu/block_shim.hpp
// runs a workgroup as fibers that meet at __syncthreads(): the polyphase kernel stages taps and samples through LDS).  A
// stand-alone program: no GPU, no HIP runtime.
//
// Both kernels are driven through their launchers with arguments built as UpfirdnPlanner::dev and ResamplePlanner::dev build
// them, aligned and one element off, for batches of 1 and 3 (whole, and for the spectrum sweep also in chunks of one signal),
// on heap blocks of exactly the contract's elements (one element too far is an AddressSanitizer report), in both fiber orders.
//     upfirdn   taps and samples m 2^-e with small integers m (never 0) and e in 0 .. 40: the products are exact, the sums
//               round, so their bits depend on the order -- compared bit for bit with acc = fma(row[j], x[q - j], acc),
//               j = 0 .. Kp - 1 ascending from 0, over the phase-major rows formed here; x = 0 outside [0, L)
//     spectrum  small integers, a scale that is a power of two: every product is exact, compared with the definition; the
//               planes of X carry NaN behind their bins, which must not reach Y
// Outputs start as a NaN bit pattern: an element the contract names must have lost it, every other one must have kept it.
#include <hip/hip_runtime.h>

#include "block_shim.hpp"

#include <cmath>
// any_len.hpp's chirp() (on resample.hpp's include path, never called by these kernels) names the device's sincospi: a host
// overload so that the header compiles here
inline void sincospi(double t, double *s, double *c) {
    *s = std::sin(3.141592653589793238462643383279502884 * t);
    *c = std::cos(3.141592653589793238462643383279502884 * t);
}

#include "resample.hip"

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

int g_fails = 0;
u64 g_compared = 0;
char g_case[320] = "";

void set_case(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(g_case, sizeof g_case, fmt, ap);
    va_end(ap);
}
void fail(const char *kernel, const char *fmt, ...) {
    static const char *names[16];
    static int counts[16];
    ++g_fails;
    int i = 0;
    while (i < 15 && names[i] && std::strcmp(names[i], kernel)) ++i;
    names[i] = kernel;
    if (++counts[i] > 6) return;  // six lines per kernel: one kernel's failures do not hide another's
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
    size_t len, k, up, down, first, out_len;  // out_len 0: full_len - first
};

template <typename T> void run_upfirdn(const Shape &s, size_t batch, size_t off) {
    set_case("%s L=%zu K=%zu up=%zu down=%zu first=%zu out_len=%zu batch=%zu off=%zu", Fp<T>::name(), s.len, s.k, s.up, s.down, s.first,
             s.out_len, batch, off);
    if (upfirdn_bad_args(s.len, s.k, s.up, s.down, s.first, s.out_len)) {
        fail("upfirdn", "the shape is refused");
        return;
    }
    // UpfirdnPlanner::init
    const size_t full = (size_t)upfirdn_full_len(s.len, s.k, s.up, s.down), n_out = s.out_len ? s.out_len : full - s.first;
    const size_t kp = (size_t)upfirdn_kp(s.k, s.up);
    const UpfirdnGeom g = upfirdn_geom(s.k, s.up, s.down);
    const size_t tiles = (n_out + g.tile - 1) / g.tile;
    const size_t ts = (size_t)upfirdn_table_stride(kp);
    Buf<T> table(s.up * ts);
    for (size_t i = 0; i < s.up * ts; ++i) table.p[i] = T(0);
    for (size_t i = 0; i < s.k; ++i) table.p[(i % s.up) * ts + i / s.up] = wide<T>(5 * s.k + s.up, i);
    const size_t sd = batch == 1 ? s.len : s.len + 3, od = batch == 1 ? n_out : n_out + 5;
    Buf<T> x((batch - 1) * sd + s.len, off);
    for (size_t b = 0; b < batch; ++b)
        for (size_t j = 0; j < s.len; ++j) x.p[b * sd + j] = wide<T>(7 * s.len + b, j);
    const std::vector<T> x0(x.base, x.base + x.n + x.off);
    for (int order = 0; order < 2; ++order) {
        block_shim::order = order ? block_shim::kDescending : block_shim::kAscending;
        Buf<T> out((batch - 1) * od + n_out, off);
        UpfirdnArgs a{};  // UpfirdnPlanner::dev
        a.x = x.p;
        a.out = out.p;
        a.taps = table.p;
        a.sig_dist = sd;
        a.out_dist = od;
        a.len = s.len;
        a.kp = kp;
        a.ts = ts;
        a.up = s.up;
        a.down = s.down;
        a.first = s.first;
        a.out_len = n_out;
        a.tiles = tiles;
        a.groups = batch * tiles * 256;
        a.dq = 256 * s.down / s.up;
        a.dp = 256 * s.down % s.up;
        a.geom = g;
        if (launch_upfirdn<T>(a, nullptr) != hipSuccess) fail("upfirdn", "the launcher failed");
        for (size_t b = 0; b < batch; ++b) {
            for (size_t i = 0; i < n_out; ++i) {
                const u64 md = (u64)(s.first + i) * s.down, q = md / s.up, p = md % s.up;
                T acc = T(0);
                for (size_t j = 0; j < kp; ++j) {
                    const long long n = (long long)q - (long long)j;
                    const T v = n >= 0 && n < (long long)s.len ? x.p[b * sd + n] : T(0);
                    acc = std::fma(table.p[p * ts + j], v, acc);
                }
                ++g_compared;
                const T got = out.p[b * od + i];
                if (!same_bits(got, acc))
                    fail("upfirdn", "output %zu of signal %zu = %.17Lg, must be exactly %.17Lg (thread order %d)", i, b, (ld)got, (ld)acc, order);
                if (s.first + i >= full && !same_bits(got, T(0))) fail("upfirdn", "output %zu of signal %zu, beyond full_len, is not 0", i, b);
            }
            if (b + 1 < batch)
                for (size_t i = n_out; i < od; ++i)
                    if (!out.is_sentinel((long long)(b * od + i))) fail("upfirdn", "element %zu of output row %zu was written", i, b);
        }
        for (size_t e = 1; e <= off; ++e)
            if (!out.is_sentinel(-(long long)e)) fail("upfirdn", "the element in front of the outputs was written");
    }
    block_shim::order = block_shim::kAscending;
    if (std::memcmp(x0.data(), x.base, x0.size() * sizeof(T))) fail("upfirdn", "the signals were written");
}

template <typename T> void run_spectrum(size_t len, size_t num, size_t batch, bool chunked, size_t off) {
    constexpr size_t V = Fp<T>::V;
    set_case("%s L=%zu num=%zu batch=%zu %s off=%zu", Fp<T>::name(), len, num, batch, chunked ? "chunks of 1" : "whole", off);
    // ResamplePlanner::init, with a scale that is a power of two in place of num / L
    const size_t xd = (len / 2 + 1 + V - 1) / V * V, yd = (num / 2 + 1 + V - 1) / V * V, bins = (size_t)resample_bins(len, num);
    const double scale = 0.25, last = scale * resample_nyquist(len, num);
    const size_t chunk = chunked ? 1 : batch;
    const size_t need = 2 * chunk * (xd + yd) + (V - 1);
    Buf<T> work(need, off);
    const size_t skip = ((16 - (reinterpret_cast<uintptr_t>(work.p) & 15u)) & 15u) / sizeof(T);
    T *w = work.p + skip;
    for (size_t b0 = 0; b0 < batch; b0 += chunk) {
        const size_t c = batch - b0 < chunk ? batch - b0 : chunk;
        T *x_re = w, *x_im = x_re + c * xd, *y_re = x_im + c * xd, *y_im = y_re + c * yd;
        for (size_t i = 0; i < 2 * c * (xd + yd); ++i) std::memcpy(w + i, &Fp<T>::sentinel, sizeof(T));
        auto xr = [&](size_t b, size_t k) { return (T)small_int(31 * len + b0 + b, k, 9); };
        auto xi = [&](size_t b, size_t k) { return (T)small_int(37 * len + b0 + b, k, 9); };
        for (size_t b = 0; b < c; ++b)
            for (size_t k = 0; k < len / 2 + 1; ++k) {  // the bins of X; NaN behind them
                x_re[b * xd + k] = xr(b, k);
                x_im[b * xd + k] = xi(b, k);
            }
        ResampleArgs a{};  // ResamplePlanner::dev
        a.x_re = x_re;
        a.x_im = x_im;
        a.y_re = y_re;
        a.y_im = y_im;
        a.xd = xd;
        a.yd = yd;
        a.bins = bins;
        a.zero_im = num % 2 ? ~0ull : num / 2;
        a.scale = scale;
        a.last = last;
        a.gpt = (unsigned)(yd / V);
        a.groups = c * a.gpt;
        if (launch_resample_spectrum<T>(a, nullptr) != hipSuccess) fail("resample_spectrum", "the launcher failed");
        for (size_t b = 0; b < c; ++b)
            for (size_t k = 0; k < yd; ++k) {
                const double f = k + 1 == bins ? last : scale;
                const T want_re = k < bins ? (T)((double)xr(b, k) * f) : T(0);
                const T want_im = k < bins && k != 0 && !(num % 2 == 0 && k == num / 2) ? (T)((double)xi(b, k) * f) : T(0);
                ++g_compared;
                if (!same_bits(y_re[b * yd + k], want_re))
                    fail("resample_spectrum", "Re Y[%zu] of signal %zu = %.9Lg, must be exactly %.9Lg", k, b0 + b, (ld)y_re[b * yd + k], (ld)want_re);
                if (!same_bits(y_im[b * yd + k], want_im))
                    fail("resample_spectrum", "Im Y[%zu] of signal %zu = %.9Lg, must be exactly %.9Lg", k, b0 + b, (ld)y_im[b * yd + k], (ld)want_im);
            }
        for (size_t b = 0; b < c; ++b)
            for (size_t k = 0; k < xd; ++k) {
                const bool named = k < len / 2 + 1;
                if (work.is_sentinel((long long)(x_re + b * xd + k - work.p)) == named || work.is_sentinel((long long)(x_im + b * xd + k - work.p)) == named)
                    fail("resample_spectrum", "the planes of X were written at bin %zu of signal %zu", k, b0 + b);
            }
    }
    for (size_t e = 1; e <= off; ++e)
        if (!work.is_sentinel(-(long long)e)) fail("resample_spectrum", "the element in front of the workspace was written");
}

}  // namespace

int main() {
    // tests/resample_reference.py's cases, the long ones on shorter signals, and windows around the tile: one less, exactly
    // one, one more, two and three more, past full_len
    const Shape shapes[] = {
        {1, 1, 1, 1, 0, 0},        {5, 3, 5, 1, 0, 0},         {17, 7, 3, 2, 0, 0},        {17, 7, 3, 2, 3, 40},      {40, 33, 2, 3, 0, 0},
        {9, 4, 1, 7, 0, 0},        {9, 4, 1, 7, 2, 9},         {3, 50, 4, 5, 0, 0},        {60, 3201, 160, 147, 0, 0}, {60, 3201, 147, 160, 5, 0},
        {40, 4200, 7, 5, 0, 0},    {20, 6000, 300, 7, 0, 0},   {20, 6000, 300, 7, 3, 515}, {300, 5000, 1, 1, 2000, 1100},
        {1200, 5, 1, 1, 0, 1023},  {1200, 5, 1, 1, 1, 1024},   {1200, 5, 1, 1, 3, 1025},   {1200, 5, 1, 1, 3, 2051},  {700, 9, 3, 1, 0, 0},
        {5000, 9, 1, 5, 0, 0},     {2000, 64, 1, 4, 0, 0},     {3, 2, 1000, 999, 0, 0},
    };
    for (const Shape &s : shapes)
        for (size_t batch = 1; batch <= 3; batch += 2)
            for (size_t off = 0; off < 2; ++off) {
                if (s.k > 1000 && batch != 1 + 2 * off) continue;  // the long filters: batch 1 aligned, batch 3 one element off
                run_upfirdn<double>(s, batch, off);
                run_upfirdn<float>(s, batch, off);
            }
    const size_t pairs[][2] = {{1, 1}, {1, 5}, {5, 1}, {8, 8}, {8, 5}, {8, 6}, {8, 12}, {8, 13}, {9, 4}, {9, 6}, {9, 14}, {2, 1}, {6, 4},
                               {1000, 441}, {441, 1000}, {2100, 1024}};
    for (const auto &p : pairs)
        for (size_t batch = 1; batch <= 3; batch += 2)
            for (int chunked = 0; chunked < 2; ++chunked)
                for (size_t off = 0; off < 2; ++off) {
                    run_spectrum<double>(p[0], p[1], batch, chunked != 0, off);
                    run_spectrum<float>(p[0], p[1], batch, chunked != 0, off);
                }
    std::printf("resample: ");
    block_shim::print_counters();
    std::printf("resample: elements %llu checked\n", g_compared);
    std::printf("resample: %s (%d failures)\n", g_fails ? "FAILED" : "ok", g_fails);
    phast_test_exit(g_fails ? 1 : 0);
}
