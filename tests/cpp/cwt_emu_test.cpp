// cwt_emu_test.cpp -- the bank kernel of the continuous wavelet transform and the pad / crop sweep (csrc/cwt.hip, #included as
// it stands), run on the host under AddressSanitizer and UndefinedBehaviorSanitizer (tests/test_cwt_emulator.py builds and runs
// it; tests/emu/block_shim.hpp runs a workgroup as fibers).  A stand-alone program: no GPU, no HIP runtime.
//
// The kernels are driven through their launchers with arguments built as CwtPlanner::dev builds them: the spectra of the
// signals a chunk touches in planes xd apart, the rows either in the caller's planes (P = L: L apart, the signals an odd
// distance apart) or in workspace rows rd apart (P > L), whole calls and chunks of 1 and of 3 rows (which straddle signals and
// scale groups), aligned and one element off, on heap blocks of exactly the contract's elements (one element too far is an
// AddressSanitizer report), in both fiber orders.  Every element is compared bit for bit with the expression order cwt.hpp
// documents, written out again here; outputs start as a NaN bit pattern: an element the contract names must have lost it,
// every other element must have kept it.
#include <hip/hip_runtime.h>

#include "block_shim.hpp"

#include <cmath>
// any_len.hpp's chirp() (on cwt.hpp's include path, never called by these kernels) names the device's sincospi: a host
// overload so that the header compiles here
inline void sincospi(double t, double *s, double *c) {
    *s = std::sin(3.141592653589793238462643383279502884 * t);
    *c = std::cos(3.141592653589793238462643383279502884 * t);
}

#include "cwt.hip"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sanitizer_exit.hpp"

using namespace phast;

namespace {

using u64 = unsigned long long;

template <typename T> struct Fp;
template <> struct Fp<double> {
    using bits = unsigned long long;
    static constexpr bits sentinel = 0x7ff8dead5eed0001ull;  // a quiet NaN no kernel produces
    static constexpr size_t V = 2;
    static const char *name() { return "f64"; }
    static double E(double a) { return std::exp(a); }
};
template <> struct Fp<float> {
    using bits = unsigned;
    static constexpr bits sentinel = 0x7fc5eed1u;
    static constexpr size_t V = 4;
    static const char *name() { return "f32"; }
    static double E(double a) { return std::exp(a); }
};

int g_fails = 0;
u64 g_compared = 0, g_mirrored = 0, g_zero_filled = 0;
char g_case[320] = "";

void set_case(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(g_case, sizeof g_case, fmt, ap);
    va_end(ap);
}
void fail(const char *fmt, ...) {
    if (++g_fails > 12) return;
    std::printf("FAIL cwt [%s]: ", g_case);
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
// in (-1, 1), never 0 (a zero fill cannot pass for data), every mantissa bit in use (the products round)
template <typename T> T value(u64 seed, u64 i) {
    const double v = (double)(mix(seed, i) >> 11) / 9007199254740992.0;  // [0, 1)
    return (T)((mix(seed + 7, i) & 1 ? 1.0 : -1.0) * (0.0625 + 0.9 * v));
}

// ---- the documented expression order (cwt.hpp), written out again ----
double ipow(double y, unsigned m) {
    double r = 1.0;
    for (unsigned e = m; e; e >>= 1) {
        if (e & 1) r *= y;
        y *= y;
    }
    return r;
}
template <typename T> T filter(int family, double param, double s, double g, u64 k, u64 P) {
    if (family == kCwtStep) return (T)(k == 0 || 2 * k == P ? 1.0 : 2 * k < P ? 2.0 : 0.0);
    const long long kk = k <= P / 2 ? (long long)k : (long long)k - (long long)P;
    const double x = s * ((6.283185307179586 * (double)kk) / (double)P);
    const unsigned m = (unsigned)param;
    double h;
    if (family == kCwtMorlet) {
        const double d = x - param;
        h = x > 0 ? g * Fp<T>::E(-0.5 * d * d) : 0.0;
    } else if (family == kCwtPaul) {
        const double e = Fp<T>::E(-x / (double)m);
        h = x > 0 && e > 0 ? g * ipow(x * e, m) : 0.0;
    } else {
        const double e = Fp<T>::E(-(x * x) / (double)(2 * m));
        h = e > 0 ? g * ipow(x * e, m) : 0.0;
    }
    return (T)h;
}

struct Shape {
    size_t l, p, s;
    int family;
    double param;
    int real_input;
};

// one chunk [row0, row0 + r) of a call of `batch` signals; rows in the caller's planes (P = L) or in workspace rows (P > L)
template <typename T> void run_bank(const Shape &sh, size_t batch, size_t row0, size_t r, size_t off) {
    const size_t P = sh.p, S = sh.s, L = sh.l, half = P / 2;
    const bool padded = P > L, analytic = sh.family != kCwtDog;
    set_case("%s L=%zu P=%zu S=%zu family=%d param=%g real=%d batch=%zu rows=%zu+%zu off=%zu", Fp<T>::name(), L, P, S, sh.family, sh.param,
             sh.real_input, batch, row0, r, off);
    if (cwt_bad_args(L, P, S, sh.family, sh.param, kCwtL2)) {
        fail("the shape is refused");
        return;
    }
    const CwtGeom g = cwt_geom(P, S, sh.real_input, sizeof(T));
    const size_t b0 = (size_t)cwt_first_signal(row0, S), ns = (size_t)cwt_signals(row0, r, S);
    // the tables, as CwtPlanner::init builds them
    std::vector<double> scales(S), gains(S);
    for (size_t j = 0; j < S; ++j) {
        scales[j] = 0.6 * std::pow(1.7, (double)((j * 5) % S));  // any order
        gains[j] = cwt_gain(sh.family, sh.param, j & 1 ? kCwtPeak : kCwtL2, scales[j]);
    }
    // the spectra of the signals the chunk touches: exactly (ns - 1) xd + bins elements; the padding of a row keeps the sentinel
    Buf<T> x0((ns - 1) * g.xd + g.bins, off), x1((ns - 1) * g.xd + g.bins, off);
    for (size_t b = 0; b < ns; ++b)
        for (size_t k = 0; k < g.bins; ++k) {
            x0.p[b * g.xd + k] = value<T>(3 * P + b0 + b, k);
            x1.p[b * g.xd + k] = value<T>(5 * P + b0 + b, k);
        }
    const std::vector<T> keep0(x0.base, x0.base + x0.n + x0.off), keep1(x1.base, x1.base + x1.n + x1.off);
    const size_t od = batch == 1 ? S * L : (S * L + 3) | 1;  // the caller's signals, an odd distance apart
    for (int order = 0; order < 2; ++order) {
        block_shim::order = order ? block_shim::kDescending : block_shim::kAscending;
        const size_t out_n = padded ? (r - 1) * g.rd + P : (batch - 1) * od + S * L;
        Buf<T> o0(out_n, off), o1(out_n, off);
        CwtArgs a{};  // CwtPlanner::dev
        a.x[0] = x0.p;
        a.x[1] = x1.p;
        a.out[0] = o0.p;
        a.out[1] = o1.p;
        a.scales = scales.data();
        a.gains = gains.data();
        a.xd = g.xd;
        a.out_sig = padded ? S * g.rd : od;
        a.out_row = padded ? g.rd : L;
        a.out_off = padded ? row0 * g.rd : 0;
        a.p = P;
        a.s = S;
        a.row0 = row0;
        a.rows = r;
        a.sig0 = b0;
        a.tiles = g.tiles;
        a.ngrp = g.ngrp;
        a.grp0 = cwt_first_group(row0, S, g.ngrp);
        a.groups = g.tiles * cwt_groups(row0, r, S, g.ngrp) * 256;
        a.param = sh.param;
        a.family = sh.family;
        a.real_input = sh.real_input;
        if (launch_cwt_bank<T>(a, nullptr) != hipSuccess) fail("the launcher failed");
        std::vector<char> named(out_n, 0);
        for (size_t row = row0; row < row0 + r; ++row) {
            const size_t b = row / S, j = row % S;
            const T *xr = x0.p + (b - b0) * g.xd, *xi = x1.p + (b - b0) * g.xd;
            const size_t at = padded ? (row - row0) * g.rd : b * od + j * L;
            for (size_t k = 0; k < P; ++k) {
                T re, im, wr, wi;
                named[at + k] = 1;
                ++g_compared;
                if (analytic && k > half) {
                    wr = wi = T(0);
                    ++g_zero_filled;
                } else {
                    if (!sh.real_input || k <= half) {
                        re = xr[k];
                        im = xi[k];
                    } else {
                        re = xr[P - k];
                        im = -xi[P - k];
                        ++g_mirrored;
                    }
                    const T h = filter<T>(sh.family, sh.param, scales[j], gains[j], k, P);
                    const T pr = re * h, pi = im * h;
                    const unsigned unit = sh.family == kCwtDog ? (unsigned)sh.param & 3 : 2;
                    wr = unit == 0 ? -pr : unit == 1 ? -pi : unit == 2 ? pr : pi;
                    wi = unit == 0 ? -pi : unit == 1 ? pr : unit == 2 ? pi : -pr;
                }
                if (!same_bits(o0.p[at + k], wr) || !same_bits(o1.p[at + k], wi))
                    fail("row (%zu, %zu) bin %zu = (%.17g, %.17g), must be exactly (%.17g, %.17g) (thread order %d)", b, j, k,
                         (double)o0.p[at + k], (double)o1.p[at + k], (double)wr, (double)wi, order);
            }
        }
        for (size_t e = 0; e < out_n; ++e)
            if (!named[e] && (!o0.is_sentinel((long long)e) || !o1.is_sentinel((long long)e))) fail("element %zu, outside the chunk's rows, was written", e);
        for (size_t e = 1; e <= off; ++e)
            if (!o0.is_sentinel(-(long long)e) || !o1.is_sentinel(-(long long)e)) fail("the element in front of the rows was written");
    }
    block_shim::order = block_shim::kAscending;
    if (std::memcmp(keep0.data(), x0.base, keep0.size() * sizeof(T)) || std::memcmp(keep1.data(), x1.base, keep1.size() * sizeof(T)))
        fail("the spectra were written");
}

// the pad: `batch` signals of L points an odd distance apart into rows of P points `ld` apart, zeros behind the signal
template <typename T> void run_pad(size_t L, size_t P, size_t batch, size_t b0, size_t ns, size_t off, int planes) {
    constexpr size_t V = Fp<T>::V;
    set_case("%s pad L=%zu P=%zu batch=%zu signals=%zu+%zu off=%zu planes=%d", Fp<T>::name(), L, P, batch, b0, ns, off, planes);
    const size_t ld = (P + V - 1) / V * V, sd = batch == 1 ? L : (L + 3) | 1;
    Buf<T> i0((batch - 1) * sd + L, off), i1((batch - 1) * sd + L, off), o0((ns - 1) * ld + P, off), o1((ns - 1) * ld + P, off);
    for (size_t e = 0; e < i0.n; ++e) {
        i0.p[e] = value<T>(13 * L, e);
        i1.p[e] = value<T>(17 * L, e);
    }
    CwtCopyArgs a{};
    a.in[0] = i0.p;
    a.in[1] = planes == 2 ? i1.p : nullptr;
    a.out[0] = o0.p;
    a.out[1] = planes == 2 ? o1.p : nullptr;
    a.n_in = L;
    a.n_out = P;
    a.s = 1;
    a.row0 = b0;
    a.rows = ns;
    a.in_sig = sd;
    a.out_sig = ld;
    a.out_off = b0 * ld;
    a.groups = (u64)planes * ns * P;
    if (launch_cwt_copy<T>(a, nullptr) != hipSuccess) fail("the launcher failed");
    for (int pl = 0; pl < planes; ++pl) {
        const Buf<T> &in = pl ? i1 : i0, &o = pl ? o1 : o0;
        for (size_t b = 0; b < ns; ++b)
            for (size_t c = 0; c < ld && b * ld + c < o.n; ++c) {
                ++g_compared;
                const T want = c < L ? in.p[(b0 + b) * sd + c] : T(0);
                if (c >= P ? !o.is_sentinel((long long)(b * ld + c)) : !same_bits(o.p[b * ld + c], want)) fail("plane %d row %zu column %zu is wrong", pl, b, c);
            }
    }
    if (planes == 1)
        for (size_t e = 0; e < o1.n; ++e)
            if (!o1.is_sentinel((long long)e)) fail("the plane the call does not have was written");
}

// the crop: the first L of the workspace rows [row0, row0 + r) into the caller's planes
template <typename T> void run_crop(size_t L, size_t P, size_t S, size_t batch, size_t row0, size_t r, size_t off) {
    constexpr size_t V = Fp<T>::V;
    set_case("%s crop L=%zu P=%zu S=%zu batch=%zu rows=%zu+%zu off=%zu", Fp<T>::name(), L, P, S, batch, row0, r, off);
    const size_t rd = (P + V - 1) / V * V, od = batch == 1 ? S * L : (S * L + 3) | 1;
    Buf<T> i0((r - 1) * rd + P, off), i1((r - 1) * rd + P, off), o0((batch - 1) * od + S * L, off), o1((batch - 1) * od + S * L, off);
    for (size_t q = 0; q < r; ++q)
        for (size_t c = 0; c < P; ++c) {
            i0.p[q * rd + c] = value<T>(19 * P + q, c);
            i1.p[q * rd + c] = value<T>(23 * P + q, c);
        }
    CwtCopyArgs a{};
    a.in[0] = i0.p;
    a.in[1] = i1.p;
    a.out[0] = o0.p;
    a.out[1] = o1.p;
    a.n_in = a.n_out = L;
    a.s = S;
    a.row0 = row0;
    a.rows = r;
    a.in_sig = S * rd;
    a.in_row = rd;
    a.in_off = row0 * rd;
    a.out_sig = od;
    a.out_row = L;
    a.groups = (u64)2 * r * L;
    if (launch_cwt_copy<T>(a, nullptr) != hipSuccess) fail("the launcher failed");
    for (int pl = 0; pl < 2; ++pl) {
        const Buf<T> &in = pl ? i1 : i0, &o = pl ? o1 : o0;
        std::vector<char> named(o.n, 0);
        for (size_t row = row0; row < row0 + r; ++row)
            for (size_t c = 0; c < L; ++c) {
                const size_t at = row / S * od + row % S * L + c;
                named[at] = 1;
                ++g_compared;
                if (!same_bits(o.p[at], in.p[(row - row0) * rd + c])) fail("plane %d row %zu column %zu is wrong", pl, row, c);
            }
        for (size_t e = 0; e < o.n; ++e)
            if (!named[e] && !o.is_sentinel((long long)e)) fail("plane %d element %zu, outside the chunk's rows, was written", pl, e);
    }
}

}  // namespace

int main() {
    // P = 1, 2, 7, 8 (both Nyquist cases); one bin below, at and above a tile of bins (512 in f64, 1024 in f32); S = 1 and one
    // below, at and above a scale group; L < P
    std::vector<Shape> shapes;
    const int fams[] = {kCwtMorlet, kCwtPaul, kCwtDog, kCwtDog, kCwtDog, kCwtDog, kCwtStep};
    const double pars[] = {6.0, 4.0, 1.0, 2.0, 3.0, 4.0, 0.0};
    for (int real = 0; real < 2; ++real)
        for (int f = 0; f < 7; ++f) {
            for (size_t p : {(size_t)1, (size_t)2, (size_t)7, (size_t)8}) shapes.push_back({p, p, 3, fams[f], pars[f], real});
            shapes.push_back({5, 8, 2, fams[f], pars[f], real});
            shapes.push_back({5, 7, 2, fams[f], pars[f], real});
        }
    for (int real = 0; real < 2; ++real) {
        for (size_t p : {(size_t)511, (size_t)512, (size_t)513, (size_t)1023, (size_t)1024, (size_t)1025}) {
            shapes.push_back({p, p, 1, kCwtMorlet, 6.0, real});
            shapes.push_back({p - 200, p, 2, kCwtDog, 3.0, real});
        }
        for (size_t s : {(size_t)1, (size_t)7, (size_t)8, (size_t)9}) {
            shapes.push_back({9, 9, s, kCwtPaul, 2.0, real});
            shapes.push_back({6, 10, s, kCwtDog, 1.0, real});
        }
    }
    for (const Shape &s : shapes)
        for (size_t off = 0; off < 2; ++off) {
            const size_t batch = 1 + 2 * off;  // batch 1 aligned, batch 3 one element off
            const size_t total = batch * s.s;
            run_bank<double>(s, batch, 0, total, off);
            run_bank<float>(s, batch, 0, total, off);
            if (s.p > 100) continue;
            for (size_t r : {(size_t)1, (size_t)3}) {
                if (r >= total) continue;
                for (size_t row0 = 0; row0 < total; row0 += r) {
                    const size_t rr = total - row0 < r ? total - row0 : r;
                    run_bank<double>(s, batch, row0, rr, off);
                    run_bank<float>(s, batch, row0, rr, off);
                }
            }
        }
    for (size_t off = 0; off < 2; ++off)
        for (size_t lp : {(size_t)0x00010001, (size_t)0x00050007, (size_t)0x00050008, (size_t)0x00640083, (size_t)0x012c0200}) {
            const size_t L = lp >> 16, P = lp & 0xffff;
            for (int planes = 1; planes <= 2; ++planes) {
                run_pad<double>(L, P, 1, 0, 1, off, planes);
                run_pad<float>(L, P, 1, 0, 1, off, planes);
                run_pad<double>(L, P, 3, 0, 3, off, planes);
                run_pad<float>(L, P, 3, 1, 2, off, planes);
            }
            if (P == L) continue;
            for (size_t S : {(size_t)1, (size_t)3}) {
                run_crop<double>(L, P, S, 1, 0, S, off);
                run_crop<float>(L, P, S, 3, 0, 3 * S, off);
                run_crop<double>(L, P, S, 3, 1, 3 * S - 2, off);
                run_crop<float>(L, P, S, 3, 3 * S - 1, 1, off);
            }
        }
    std::printf("cwt: ");
    block_shim::print_counters();
    std::printf("cwt: elements %llu checked, %llu of them mirrored reads, %llu zero fills\n", g_compared, g_mirrored, g_zero_filled);
    std::printf("cwt: %s (%d failures)\n", g_fails ? "FAILED" : "ok", g_fails);
    phast_test_exit(g_fails ? 1 : 0);
}
