// sweep_emu_test.cpp -- the streaming sweep kernels of the composite transforms, run on the host under AddressSanitizer and
// UndefinedBehaviorSanitizer (tests/test_sweep_emulator.py builds and runs it; tests/emu/sweep_shim.hpp turns a launch into a
// serial loop).  One translation unit per product file (SWEEP_PART = 1..8, the file #included as it stands) and one for main
// (SWEEP_PART = 0).  Every kernel is driven through the product's own launch_* function with arguments built as the planner
// that launches it builds them, and every element of every output is compared with a long double statement of the kernel's
// contract, written here a second time on purpose.
//
// Buffers: every caller-side buffer and every workspace is a heap allocation of exactly the bytes the contract covers, so one
// element too far is an AddressSanitizer report; an "unaligned" buffer is one element longer and used from element 1, so its
// end still is the allocation's end.  Outputs and workspaces start as a NaN bit pattern (the sentinel): an element the
// contract names must have lost it, every other element must have kept its exact bits.  A 16-byte access through a pointer
// that is not 16-byte aligned is UBSan's "misaligned address", or, where the access is a non-temporal builtin that UBSan does
// not instrument, the host's own alignment fault (the aligned SSE move), which AddressSanitizer reports as SEGV.
//
// The numeric gate is derived, not measured: per element k * u_T * (sum of the magnitudes of the terms), u_T the unit
// roundoff of T (2^-53, 2^-24), k the roundings of the kernel's expression (counted beside each case) plus 2.  The sweeps
// compute in double and round once to T, so a count is given as (roundings in T, roundings in double): the gate of an f32
// sweep is (nT + 2) u_f32 + nD u_f64, that of an f64 sweep (nT + nD + 2) u_f64.  A twiddle's phase is one rounding of an angle
// of up to 2 pi (any_len.hpp: t = -r / N in (-2, 0] half turns), which moves up to 2 pi u between the cosine and the sine:
// it is counted as 7 roundings, and because it moves weight from one product to the other the magnitude of a twiddled term
// is that of its operand (|twiddle| = 1).  The host sincospi is not the device's: this says nothing about device accuracy.
#ifndef SWEEP_PART
#error "compile with -DSWEEP_PART=0 (main) .. 8"
#endif

#if SWEEP_PART == 0
// ------------------------------------------------------------------------------------------------------------ main
#include <cstdio>
#include <cstring>

#include "sanitizer_exit.hpp"

int sweep_any_len();
int sweep_any_real();
int sweep_dct();
int sweep_stft();
int sweep_conv();
int sweep_czt();
int sweep_complex_nums();
int sweep_r2c();

int main(int argc, char **argv) {
    struct Part {
        const char *name;
        int (*run)();
    };
    const Part parts[] = {{"any_len", sweep_any_len}, {"any_real", sweep_any_real}, {"dct", sweep_dct},
                          {"stft", sweep_stft},       {"conv", sweep_conv},         {"czt", sweep_czt},
                          {"complex_nums", sweep_complex_nums}, {"r2c", sweep_r2c}};
    int fails = 0, ran = 0;
    for (const Part &p : parts) {
        if (argc > 1 && std::strcmp(argv[1], p.name) != 0) continue;
        ++ran;
        const int f = p.run();
        std::printf("%s: %s (%d failures)\n", p.name, f ? "FAILED" : "ok", f);
        fails += f;
    }
    if (!ran) {
        std::printf("usage: %s [any_len|any_real|dct|stft|conv|czt|complex_nums|r2c]\n", argv[0]);
        phast_test_exit(2);
    }
    phast_test_exit(fails ? 1 : 0);
}

#else
// ------------------------------------------------------------------------------------------------------------ a part
#include <hip/hip_runtime.h>

#include "sweep_shim.hpp"

#if SWEEP_PART == 1
#include "any_len.hip"
#elif SWEEP_PART == 2
#include "any_real.hip"
#elif SWEEP_PART == 3
#include "dct.hip"
#elif SWEEP_PART == 4
#include "stft.hip"
#elif SWEEP_PART == 5
#include "conv.hip"
#elif SWEEP_PART == 6
#include "czt.hip"
#elif SWEEP_PART == 7
#include "complex_nums.hip"
#elif SWEEP_PART == 8
#include "r2c.hip"
#include "plan.hpp"  // host_tw3, tw3_bits_for: the tables as planner_r2c.hpp uploads them
#endif

#include <complex>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <vector>

namespace {

using ld = long double;
using cld = std::complex<long double>;
constexpr ld kPi = 3.141592653589793238462643383279502884L;
constexpr ld kUD = 0x1p-53L;

template <typename T> struct Fp;
template <> struct Fp<double> {
    using bits = unsigned long long;
    static constexpr ld u = 0x1p-53L;
    static constexpr bits sentinel = 0x7ff8dead5eed0001ull;  // a quiet NaN no kernel produces
    static constexpr size_t V = 2;
    static const char *name() { return "f64"; }
};
template <> struct Fp<float> {
    using bits = unsigned;
    static constexpr ld u = 0x1p-24L;
    static constexpr bits sentinel = 0x7fc5eed1u;
    static constexpr size_t V = 4;
    static const char *name() { return "f32"; }
};
// the gate's factor of a kernel with nT roundings in T and nD in double (the header has the rule)
template <typename T> ld gate_k(int nT, int nD) { return (ld)(nT + 2) * Fp<T>::u + (ld)nD * kUD; }

struct Stat {
    const char *kernel;
    double worst = 0;  // err / gate
    unsigned long long compared = 0, exact = 0, launches = 0;
    int fails = 0;
};
std::deque<Stat> g_stats;
char g_case[320] = "";
int g_fails = 0;

Stat &stat_of(const char *kernel) {
    for (Stat &s : g_stats)
        if (!std::strcmp(s.kernel, kernel)) return s;
    g_stats.push_back(Stat{kernel});
    return g_stats.back();
}
void set_case(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(g_case, sizeof g_case, fmt, ap);
    va_end(ap);
}
void fail(Stat &s, const char *fmt, ...) {
    ++s.fails;
    ++g_fails;
    if (s.fails > 6) return;  // the first few name the kernel and the case; the count is in the summary line
    std::printf("FAIL %s [%s]: ", s.kernel, g_case);
    va_list ap;
    va_start(ap, fmt);
    std::vprintf(fmt, ap);
    va_end(ap);
    std::printf("\n");
}
int report() {
    for (const Stat &s : g_stats)
        std::printf("  %-28s launches %5llu  elements %8llu (bit-exact %8llu)  worst error / gate %.3f%s\n", s.kernel, s.launches,
                    s.compared, s.exact, s.worst, s.fails ? "  FAILED" : "");
    return g_fails;
}
void launched(Stat &s, hipError_t rc) {
    ++s.launches;
    if (rc != hipSuccess) fail(s, "the launcher returned %d", (int)rc);
}

ld rnd(unsigned long long seed, unsigned long long i) {  // uniform in [-1, 1), exact in float
    unsigned long long x = seed * 0x9E3779B97F4A7C15ull + i * 0xD1B54A32D192ED03ull + 0x2545F4914F6CDD1Dull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    x ^= x >> 31;
    return (ld)(long long)(x >> 43) * 0x1p-20L - 1.0L;  // 21 bits
}

// an allocation of exactly n elements of T behind `off` elements of lead-in (off = 1: an element-aligned pointer)
template <typename T> struct Buf {
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
    T &operator[](size_t i) { return p[i]; }
    ld at(size_t i) const { return (ld)p[i]; }
    Buf &random(unsigned long long seed, ld amp = 1.0L) {
        for (size_t i = 0; i < n; ++i) p[i] = (T)(amp * rnd(seed, i));
        return *this;
    }
    Buf &sentinel() {
        for (size_t i = 0; i < n; ++i) std::memcpy(p + i, &Fp<T>::sentinel, sizeof(T));
        return *this;
    }
};
bool al16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// what a buffer a kernel may write must look like afterwards: ref and gate per element; gate < 0: the contract does not
// name the element (it keeps its bits), gate = 0: bit-equal, gate > 0: |value - ref| <= gate
template <typename T> struct Expect {
    using bits = typename Fp<T>::bits;
    Buf<T> &buf;
    const char *what;
    std::vector<bits> before;
    std::vector<ld> ref, gate;
    bool bad_test = false;
    Expect(Buf<T> &b, const char *what_) : buf(b), what(what_), before(b.n), ref(b.n, 0), gate(b.n, -1) {
        for (size_t i = 0; i < b.n; ++i) std::memcpy(&before[i], b.p + i, sizeof(T));
    }
    void name(size_t i, ld r, ld g) {
        if (i >= buf.n || gate[i] >= 0) {
            bad_test = true;  // the test's own statement of the contract names an element twice or outside the buffer
            return;
        }
        ref[i] = r;
        gate[i] = g;
    }
    void exact(size_t i, ld r) { name(i, r, 0); }
    void verify(Stat &s) {
        if (bad_test) fail(s, "%s: the test named an element twice or out of range", what);
        for (size_t i = 0; i < buf.n; ++i) {
            bits now;
            std::memcpy(&now, buf.p + i, sizeof(T));
            if (gate[i] < 0) {
                if (now != before[i]) fail(s, "%s[%zu] lies outside the contract and was written (%.9Lg)", what, i, buf.at(i));
                continue;
            }
            ++s.compared;
            if (now == Fp<T>::sentinel) {
                fail(s, "%s[%zu] is named by the contract and was not written", what, i);
                continue;
            }
            const ld v = buf.at(i);
            if (gate[i] == 0) {
                ++s.exact;
                if (!(v == ref[i])) fail(s, "%s[%zu] = %.17Lg, must be exactly %.17Lg", what, i, v, ref[i]);
                continue;
            }
            const ld err = v > ref[i] ? v - ref[i] : ref[i] - v;
            if (!(err <= gate[i])) fail(s, "%s[%zu] = %.17Lg, reference %.17Lg: error %.3Lg > gate %.3Lg", what, i, v, ref[i], err, gate[i]);
            else if ((double)(err / gate[i]) > s.worst) s.worst = (double)(err / gate[i]);
        }
    }
};

unsigned ilog2_of(unsigned long long v) {
    unsigned l = 0;
    while ((1ull << l) < v) ++l;
    return l;
}
size_t round_up(size_t n, size_t v) { return (n + v - 1) / v * v; }
size_t span(size_t batch, size_t dist, size_t n) { return batch ? (batch - 1) * dist + n : 0; }

// (batch, dist, off) of a caller-side array of n elements per transform: batch 1 and 3, distances n, n + 1 (odd or even, never a
// multiple of V together with n) and n rounded up to V, base offset 0 and 1 element.  A planner sets dist = n for one transform.
struct Layout {
    size_t batch, dist, off;
};
std::vector<Layout> layouts(size_t n, size_t v) {
    std::vector<Layout> out;
    for (size_t off = 0; off < 2; ++off) {
        out.push_back({1, n, off});
        out.push_back({3, n, off});
        out.push_back({3, n + 1, off});
        if (round_up(n, v) != n) out.push_back({3, round_up(n, v), off});
        else out.push_back({3, n + v, off});
    }
    return out;
}

// w_n[k] = exp(-i pi k^2 / n): k^2 is reduced mod 2n in integers, the angle is below 2 pi
cld chirp_ref(unsigned long long k, unsigned long long n) {
    const unsigned long long r = (k * k) % (2 * n);
    const ld t = kPi * (ld)r / (ld)n;
    return cld(cosl(t), -sinl(t));
}
// exp(-2 pi i k / n)
cld root_ref(unsigned long long k, unsigned long long n) {
    const ld t = 2 * kPi * (ld)(k % n) / (ld)n;
    return cld(cosl(t), -sinl(t));
}
ld mag(cld z) { return fabsl(z.real()) + fabsl(z.imag()); }

}  // namespace

using namespace phast;

// ============================================================================================================ any_len.hip
#if SWEEP_PART == 1
namespace {

// no power of two: those never reach the sweeps (AnyPlanner::pow2); 12 and 20 stand in for the residue 0 mod V they would give
// (only full 16-byte groups, and a packed batch, dist == n, on the 16-byte path)
const size_t kLens[] = {3, 5, 7, 9, 12, 15, 17, 20, 33, 258};

// the planner's call of one chunk: AnyPlanner::run_chunk
template <typename T> void any_len_case(size_t n, const Layout &lay) {
    constexpr size_t V = Fp<T>::V;
    const size_t m = (size_t)any_conv_len(n), c = lay.batch, dist = lay.dist;
    const unsigned log_m = ilog2_of(m);
    Buf<T> xr(span(c, dist, n), lay.off), xi(span(c, dist, n), lay.off);
    xr.random(11 * n + c);
    xi.random(13 * n + c);
    const bool planner_vec = al16(xr.p) && al16(xi.p) && dist % V == 0;
    for (int vec = planner_vec ? 1 : 0; vec >= 0; --vec) {  // the element path is legal wherever the 16-byte path is
        set_case("%s N=%zu M=%zu batch=%zu dist=%zu off=%zu vec=%d", Fp<T>::name(), n, m, c, dist, lay.off, vec);
        {  // chirp-pad: a[b M + k] = x[b dist + k] w[k] (k < N), 0 up to M
            Stat &s = stat_of(vec ? "any_pre_kernel<VEC>" : "any_pre_kernel");
            Buf<T> w(2 * c * m);
            w.sentinel();
            Expect<T> e(w, "workspace");
            AnySweepArgs a{};
            a.n = n;
            a.log_m = log_m;
            a.in_dist = a.out_dist = dist;
            a.in_re = xr.p;
            a.in_im = xi.p;
            a.out_re = w.p;
            a.out_im = w.p + c * m;
            a.groups = c * (m / V);
            launched(s, launch_any_sweep<T>(0, vec != 0, a, nullptr));
            // roundings: phase 7, cos and sin 2, two products 2, their sum 1 in double; the conversion to T
            const ld g = gate_k<T>(1, 12);
            for (size_t b = 0; b < c; ++b)
                for (size_t k = 0; k < m; ++k) {
                    if (k >= n) {
                        e.exact(b * m + k, 0);
                        e.exact(c * m + b * m + k, 0);
                        continue;
                    }
                    const cld x(xr.at(b * dist + k), xi.at(b * dist + k)), y = x * chirp_ref(k, n);
                    e.name(b * m + k, y.real(), g * mag(x));
                    e.name(c * m + b * m + k, y.imag(), g * mag(x));
                }
            e.verify(s);
        }
        for (int inverse = 0; inverse < 2; ++inverse) {  // chirp-post: X[b dist + k] = w[k] c[b M + k] * scale (k < N)
            Stat &s = stat_of(vec ? "any_post_kernel<VEC>" : "any_post_kernel");
            Buf<T> w(2 * c * m), outr(span(c, dist, n), lay.off), outi(span(c, dist, n), lay.off);
            w.random(17 * n + c);
            outr.sentinel();
            outi.sentinel();
            Expect<T> er(outr, "re"), ei(outi, "im");
            AnySweepArgs a{};
            a.n = n;
            a.log_m = log_m;
            a.in_dist = a.out_dist = dist;
            a.in_re = w.p;
            a.in_im = w.p + c * m;
            a.out_re = outr.p;
            a.out_im = outi.p;
            a.gpt = (unsigned)((n + V - 1) / V);
            a.groups = c * a.gpt;
            a.scale = inverse ? 1.0 / (double)n : 1.0;
            launched(s, launch_any_sweep<T>(2, vec != 0, a, nullptr));
            // roundings: the scale on either part 2, phase 7, cos and sin 2, two products 2, their sum 1; the conversion
            const ld g = gate_k<T>(1, 14);
            for (size_t b = 0; b < c; ++b)
                for (size_t k = 0; k < n; ++k) {
                    const cld v = cld(w.at(b * m + k), w.at(c * m + b * m + k)) * (ld)a.scale, y = v * chirp_ref(k, n);
                    er.name(b * dist + k, y.real(), g * mag(v));
                    ei.name(b * dist + k, y.imag(), g * mag(v));
                }
            er.verify(s);
            ei.verify(s);
        }
    }
    if (lay.off == 0 && dist == n) {  // the workspace sweeps do not see the caller's layout
        set_case("%s N=%zu M=%zu batch=%zu", Fp<T>::name(), n, m, c);
        Stat &s = stat_of("any_spectrum_kernel");  // A[b M + k] *= Bh[k]: ConvCore::convolve
        Buf<T> w(2 * c * m), bh(2 * m);
        w.random(19 * n + c);
        bh.random(23 * n);
        Expect<T> e(w, "workspace");
        AnySweepArgs a{};
        a.out_re = w.p;
        a.out_im = w.p + c * m;
        a.bh_re = bh.p;
        a.bh_im = bh.p + m;
        a.log_m = log_m;
        a.groups = c * (m / V);
        const ld g = gate_k<T>(3, 0);  // two products and their difference / sum, in T
        for (size_t b = 0; b < c; ++b)
            for (size_t k = 0; k < m; ++k) {
                const ld ar = w.at(b * m + k), ai = w.at(c * m + b * m + k), br = bh.at(k), bi = bh.at(m + k);
                e.name(b * m + k, ar * br - ai * bi, g * (fabsl(ar * br) + fabsl(ai * bi)));
                e.name(c * m + b * m + k, ar * bi + ai * br, g * (fabsl(ar * bi) + fabsl(ai * br)));
            }
        launched(s, launch_any_sweep<T>(1, true, a, nullptr));
        e.verify(s);
    }
}

void chirp_b_case(size_t n) {  // b[k] = conj(w[k]) (k < N), b[M - k] = b[k] (0 < k < N), 0 elsewhere: AnyPlanner::init
    const size_t m = (size_t)any_conv_len(n);
    set_case("f64 N=%zu M=%zu", n, m);
    Stat &s = stat_of("any_chirp_b_kernel");
    Buf<double> re(m), im(m);
    re.sentinel();
    im.sentinel();
    Expect<double> er(re, "re"), ei(im, "im");
    launched(s, launch_any_chirp_b(re.p, im.p, n, ilog2_of(m), nullptr));
    const ld g = gate_k<double>(0, 8);  // phase 7, the cosine or the sine 1
    for (size_t i = 0; i < m; ++i) {
        const size_t lag = i < n ? i : m - i;
        if (lag >= n) {
            er.exact(i, 0);
            ei.exact(i, 0);
            continue;
        }
        const cld b = std::conj(chirp_ref(lag, n));
        er.name(i, b.real(), g);
        ei.name(i, b.imag(), g);
    }
    er.verify(s);
    ei.verify(s);
}

void round_case(size_t count) {  // out[i] = (float)in[i]: ConvCore::make_table
    set_case("count=%zu", count);
    Stat &s = stat_of("any_round_kernel");
    Buf<double> in(count);
    Buf<float> out(count);
    in.random(29 + count, 3.0L);
    out.sentinel();
    Expect<float> e(out, "out");
    for (size_t i = 0; i < count; ++i) e.exact(i, (ld)(float)in.p[i]);
    launched(s, launch_any_round(in.p, out.p, count, nullptr));
    e.verify(s);
}

}  // namespace

int sweep_any_len() {
    for (size_t n : kLens) {
        for (const Layout &lay : layouts(n, 2)) any_len_case<double>(n, lay);
        for (const Layout &lay : layouts(n, 4)) any_len_case<float>(n, lay);
        chirp_b_case(n);
    }
    for (size_t count : {1, 2, 3, 16, 255, 256, 257, 1030}) round_case(count);
    return report();
}
#endif

// ============================================================================================================ any_real.hip
#if SWEEP_PART == 2
namespace {

// one chunk as AnyRealPlanner::run_chunk launches it; kind by kind.  `hd`: the distance of the half-spectrum planes
template <typename T> AnyRealArgs real_args(size_t n, size_t l, size_t m, size_t in_dist, size_t out_dist) {
    AnyRealArgs a{};
    a.n = n;
    a.l = l;
    a.log_m = ilog2_of(m);
    a.in_dist = in_dist;
    a.out_dist = out_dist;
    return a;
}

template <typename T> void real_even_case(size_t n, const Layout &sig, const Layout &spec) {
    constexpr size_t V = Fp<T>::V;
    const size_t h = n / 2, m = (size_t)any_conv_len(h), c = sig.batch, bins = h + 1;
    // ---- R2C: pack + chirp-pad, a[b M + k] = (x[2k] + i x[2k+1]) w_H[k] (k < H), 0 up to M
    {
        Buf<T> x(span(c, sig.dist, n), sig.off);
        x.random(31 * n + c);
        const bool planner_vec = al16(x.p) && (c == 1 || sig.dist % V == 0);
        for (int vec = planner_vec ? 1 : 0; vec >= 0; --vec) {
            set_case("%s N=%zu H=%zu M=%zu batch=%zu dist=%zu off=%zu vec=%d", Fp<T>::name(), n, h, m, c, sig.dist, sig.off, vec);
            Stat &s = stat_of(vec ? "any_r2c_pack_kernel<VEC>" : "any_r2c_pack_kernel");
            Buf<T> w(2 * c * m);
            w.sentinel();
            Expect<T> e(w, "workspace");
            AnyRealArgs a = real_args<T>(n, h, m, sig.dist, spec.dist);
            a.in_re = x.p;
            a.in_im = nullptr;
            a.out_re = w.p;
            a.out_im = w.p + c * m;
            a.groups = c * (m / V);
            launched(s, launch_any_real<T>(kR2cPack, vec != 0, a, nullptr));
            const ld g = gate_k<T>(1, 12);  // as any_pre_kernel: phase 7, cos / sin 2, products 2, sum 1; the conversion
            for (size_t b = 0; b < c; ++b)
                for (size_t k = 0; k < m; ++k) {
                    if (k >= h) {
                        e.exact(b * m + k, 0);
                        e.exact(c * m + b * m + k, 0);
                        continue;
                    }
                    const cld z(x.at(b * sig.dist + 2 * k), x.at(b * sig.dist + 2 * k + 1)), y = z * chirp_ref(k, h);
                    e.name(b * m + k, y.real(), g * mag(z));
                    e.name(c * m + b * m + k, y.imag(), g * mag(z));
                }
            e.verify(s);
        }
    }
    // ---- R2C: chirp-post + untangle, Z = w_H c; X[k] = (Z[k] + conj Z[H-k]) / 2 - i W^k (Z[k] - conj Z[H-k]) / 2, k <= H,
    // Z[H] = Z[0]; Im X[0] = Im X[H] = 0 exactly
    {
        Buf<T> w(2 * c * m);
        w.random(37 * n + c);
        Buf<T> probe_r(span(c, spec.dist, bins), spec.off), probe_i(span(c, spec.dist, bins), spec.off);
        const bool planner_vec = al16(probe_r.p) && al16(probe_i.p) && (c == 1 || spec.dist % V == 0);
        for (int vec = planner_vec ? 1 : 0; vec >= 0; --vec) {
            set_case("%s N=%zu H=%zu M=%zu batch=%zu dist=%zu off=%zu vec=%d", Fp<T>::name(), n, h, m, c, spec.dist, spec.off, vec);
            Stat &s = stat_of(vec ? "any_r2c_untangle_kernel<VEC>" : "any_r2c_untangle_kernel");
            Buf<T> outr(span(c, spec.dist, bins), spec.off), outi(span(c, spec.dist, bins), spec.off);
            outr.sentinel();
            outi.sentinel();
            Expect<T> er(outr, "re"), ei(outi, "im");
            AnyRealArgs a = real_args<T>(n, h, m, sig.dist, spec.dist);
            a.in_re = w.p;
            a.in_im = w.p + c * m;
            a.out_re = outr.p;
            a.out_im = outi.p;
            a.gpt = (unsigned)((h / 2 + 1 + V - 1) / V);
            a.groups = c * a.gpt;
            launched(s, launch_any_real<T>(kR2cUntangle, vec != 0, a, nullptr));
            // roundings: Z (phase 7, cos / sin 2, products 2, sum 1) 12, the half sum / difference 1, W^k (phase pi: 4, value 1) 5,
            // its two products and their sum 3, the last sum 1; the conversion.  Every term of the last sum carries the factor 1/2
            const ld g = gate_k<T>(1, 22);
            for (size_t b = 0; b < c; ++b)
                for (size_t k = 0; k <= h; ++k) {
                    const size_t k1 = k % h, k2 = (h - k1) % h;
                    const cld c1(w.at(b * m + k1), w.at(c * m + b * m + k1)), c2(w.at(b * m + k2), w.at(c * m + b * m + k2));
                    const cld z1 = c1 * chirp_ref(k1, h), z2 = std::conj(c2 * chirp_ref(k2, h));
                    const cld xk = (z1 + z2) * 0.5L - cld(0, 1) * root_ref(k, n) * (z1 - z2) * 0.5L;
                    er.name(b * spec.dist + k, xk.real(), g * 0.5L * (mag(c1) + mag(c2)));
                    if (k == 0 || k == h) ei.exact(b * spec.dist + k, 0);
                    else ei.name(b * spec.dist + k, xk.imag(), g * 0.5L * (mag(c1) + mag(c2)));
                }
            er.verify(s);
            ei.verify(s);
        }
    }
    // ---- C2R: preprocess + pad, z~[k] = (A + conj B) / 2 + i conj(W^k) (A - conj B) / 2, A = X[k], B = X[H - k];
    // a[b M + k] = (Im z~[k] + i Re z~[k]) w_H[k] (k < H), 0 up to M
    {
        Buf<T> xr(span(c, spec.dist, bins), spec.off), xi(span(c, spec.dist, bins), spec.off);
        xr.random(41 * n + c);
        xi.random(43 * n + c);
        const bool planner_vec = al16(xr.p) && al16(xi.p) && (c == 1 || spec.dist % V == 0);
        for (int vec = planner_vec ? 1 : 0; vec >= 0; --vec) {
            set_case("%s N=%zu H=%zu M=%zu batch=%zu dist=%zu off=%zu vec=%d", Fp<T>::name(), n, h, m, c, spec.dist, spec.off, vec);
            Stat &s = stat_of(vec ? "any_c2r_pre_kernel<VEC>" : "any_c2r_pre_kernel");
            Buf<T> w(2 * c * m);
            w.sentinel();
            Expect<T> e(w, "workspace");
            AnyRealArgs a = real_args<T>(n, h, m, spec.dist, sig.dist);
            a.in_re = xr.p;
            a.in_im = xi.p;
            a.out_re = w.p;
            a.out_im = w.p + c * m;
            a.groups = c * (m / V);
            launched(s, launch_any_real<T>(kC2rPre, vec != 0, a, nullptr));
            // roundings: W^k 5, sum / difference 1, two products and their sum 3, the sum into z~ 1, the chirp 9, its products
            // and sum 3; the conversion.  Every term of z~ carries the factor 1/2
            const ld g = gate_k<T>(1, 22);
            for (size_t b = 0; b < c; ++b)
                for (size_t k = 0; k < m; ++k) {
                    if (k >= h) {
                        e.exact(b * m + k, 0);
                        e.exact(c * m + b * m + k, 0);
                        continue;
                    }
                    const cld A(xr.at(b * spec.dist + k), xi.at(b * spec.dist + k));
                    const cld B(xr.at(b * spec.dist + h - k), xi.at(b * spec.dist + h - k));
                    const cld zt = (A + std::conj(B)) * 0.5L + cld(0, 1) * std::conj(root_ref(k, n)) * (A - std::conj(B)) * 0.5L;
                    const cld y = cld(zt.imag(), zt.real()) * chirp_ref(k, h);
                    e.name(b * m + k, y.real(), g * 0.5L * (mag(A) + mag(B)));
                    e.name(c * m + b * m + k, y.imag(), g * 0.5L * (mag(A) + mag(B)));
                }
            e.verify(s);
        }
    }
    // ---- C2R: chirp-post + interleave, Y = w_H c / H; x[2k] = Im Y[k], x[2k+1] = Re Y[k], k < H
    {
        Buf<T> w(2 * c * m);
        w.random(47 * n + c);
        Buf<T> probe(span(c, sig.dist, n), sig.off);
        const bool planner_vec = al16(probe.p) && (c == 1 || sig.dist % V == 0);
        for (int vec = planner_vec ? 1 : 0; vec >= 0; --vec) {
            set_case("%s N=%zu H=%zu M=%zu batch=%zu dist=%zu off=%zu vec=%d", Fp<T>::name(), n, h, m, c, sig.dist, sig.off, vec);
            Stat &s = stat_of(vec ? "any_c2r_interleave_kernel<VEC>" : "any_c2r_interleave_kernel");
            Buf<T> x(span(c, sig.dist, n), sig.off);
            x.sentinel();
            Expect<T> e(x, "signal");
            AnyRealArgs a = real_args<T>(n, h, m, spec.dist, sig.dist);
            a.in_re = w.p;
            a.in_im = w.p + c * m;
            a.out_re = x.p;
            a.out_im = nullptr;
            a.scale = 1.0 / (double)h;
            a.gpt = (unsigned)((h + V - 1) / V);
            a.groups = c * a.gpt;
            launched(s, launch_any_real<T>(kC2rInterleave, vec != 0, a, nullptr));
            const ld g = gate_k<T>(1, 14);  // as any_post_kernel: scale 2, phase 7, cos / sin 2, products 2, sum 1; the conversion
            for (size_t b = 0; b < c; ++b)
                for (size_t k = 0; k < h; ++k) {
                    const cld v = cld(w.at(b * m + k), w.at(c * m + b * m + k)) * (ld)a.scale, y = v * chirp_ref(k, h);
                    e.name(b * sig.dist + 2 * k, y.imag(), g * mag(v));
                    e.name(b * sig.dist + 2 * k + 1, y.real(), g * mag(v));
                }
            e.verify(s);
        }
    }
}

template <typename T> void real_odd_case(size_t n, const Layout &sig, const Layout &spec) {
    constexpr size_t V = Fp<T>::V;
    const size_t m = (size_t)any_conv_len(n), c = sig.batch, q = (n - 1) / 2, bins = q + 1;
    {  // ---- R2C: a[b M + k] = x[k] w_N[k] (k < N), 0 up to M
        Buf<T> x(span(c, sig.dist, n), sig.off);
        x.random(53 * n + c);
        const bool planner_vec = al16(x.p) && (c == 1 || sig.dist % V == 0);
        for (int vec = planner_vec ? 1 : 0; vec >= 0; --vec) {
            set_case("%s N=%zu M=%zu batch=%zu dist=%zu off=%zu vec=%d", Fp<T>::name(), n, m, c, sig.dist, sig.off, vec);
            Stat &s = stat_of(vec ? "any_r2c_odd_pad_kernel<VEC>" : "any_r2c_odd_pad_kernel");
            Buf<T> w(2 * c * m);
            w.sentinel();
            Expect<T> e(w, "workspace");
            AnyRealArgs a = real_args<T>(n, n, m, sig.dist, spec.dist);
            a.in_re = x.p;
            a.out_re = w.p;
            a.out_im = w.p + c * m;
            a.groups = c * (m / V);
            launched(s, launch_any_real<T>(kR2cOddPad, vec != 0, a, nullptr));
            const ld g = gate_k<T>(1, 9);  // phase 7, the cosine or the sine 1, one product 1; the conversion
            for (size_t b = 0; b < c; ++b)
                for (size_t k = 0; k < m; ++k) {
                    if (k >= n) {
                        e.exact(b * m + k, 0);
                        e.exact(c * m + b * m + k, 0);
                        continue;
                    }
                    const ld v = x.at(b * sig.dist + k);
                    const cld y = v * chirp_ref(k, n);
                    e.name(b * m + k, y.real(), g * fabsl(v));
                    e.name(c * m + b * m + k, y.imag(), g * fabsl(v));
                }
            e.verify(s);
        }
    }
    {  // ---- R2C: X[k] = w_N[k] c[k], k <= (N - 1) / 2; Im X[0] = 0 exactly
        Buf<T> w(2 * c * m);
        w.random(59 * n + c);
        Buf<T> probe_r(span(c, spec.dist, bins), spec.off), probe_i(span(c, spec.dist, bins), spec.off);
        const bool planner_vec = al16(probe_r.p) && al16(probe_i.p) && (c == 1 || spec.dist % V == 0);
        for (int vec = planner_vec ? 1 : 0; vec >= 0; --vec) {
            set_case("%s N=%zu M=%zu batch=%zu dist=%zu off=%zu vec=%d", Fp<T>::name(), n, m, c, spec.dist, spec.off, vec);
            Stat &s = stat_of(vec ? "any_r2c_odd_post_kernel<VEC>" : "any_r2c_odd_post_kernel");
            Buf<T> outr(span(c, spec.dist, bins), spec.off), outi(span(c, spec.dist, bins), spec.off);
            outr.sentinel();
            outi.sentinel();
            Expect<T> er(outr, "re"), ei(outi, "im");
            AnyRealArgs a = real_args<T>(n, n, m, sig.dist, spec.dist);
            a.in_re = w.p;
            a.in_im = w.p + c * m;
            a.out_re = outr.p;
            a.out_im = outi.p;
            a.gpt = (unsigned)((bins + V - 1) / V);
            a.groups = c * a.gpt;
            launched(s, launch_any_real<T>(kR2cOddPost, vec != 0, a, nullptr));
            const ld g = gate_k<T>(1, 12);  // phase 7, cos / sin 2, products 2, sum 1; the conversion
            for (size_t b = 0; b < c; ++b)
                for (size_t k = 0; k <= q; ++k) {
                    const cld v(w.at(b * m + k), w.at(c * m + b * m + k)), y = v * chirp_ref(k, n);
                    er.name(b * spec.dist + k, y.real(), g * mag(v));
                    if (k == 0) ei.exact(b * spec.dist, 0);
                    else ei.name(b * spec.dist + k, y.imag(), g * mag(v));
                }
            er.verify(s);
            ei.verify(s);
        }
    }
    {  // ---- C2R: Xh[k] = X[k] (k <= (N-1)/2, Im X[0] taken as 0), conj X[N - k] above; a = (Im Xh + i Re Xh) w_N (k < N), 0 up to M
        Buf<T> xr(span(c, spec.dist, bins), spec.off), xi(span(c, spec.dist, bins), spec.off);
        xr.random(61 * n + c);
        xi.random(67 * n + c);
        const bool planner_vec = al16(xr.p) && al16(xi.p) && (c == 1 || spec.dist % V == 0);
        for (int vec = planner_vec ? 1 : 0; vec >= 0; --vec) {
            set_case("%s N=%zu M=%zu batch=%zu dist=%zu off=%zu vec=%d", Fp<T>::name(), n, m, c, spec.dist, spec.off, vec);
            Stat &s = stat_of(vec ? "any_c2r_odd_pad_kernel<VEC>" : "any_c2r_odd_pad_kernel");
            Buf<T> w(2 * c * m);
            w.sentinel();
            Expect<T> e(w, "workspace");
            AnyRealArgs a = real_args<T>(n, n, m, spec.dist, sig.dist);
            a.in_re = xr.p;
            a.in_im = xi.p;
            a.out_re = w.p;
            a.out_im = w.p + c * m;
            a.groups = c * (m / V);
            launched(s, launch_any_real<T>(kC2rOddPad, vec != 0, a, nullptr));
            const ld g = gate_k<T>(1, 12);
            for (size_t b = 0; b < c; ++b)
                for (size_t k = 0; k < m; ++k) {
                    if (k >= n) {
                        e.exact(b * m + k, 0);
                        e.exact(c * m + b * m + k, 0);
                        continue;
                    }
                    const size_t src = k <= q ? k : n - k;
                    cld xh(xr.at(b * spec.dist + src), xi.at(b * spec.dist + src));
                    if (k > q) xh = std::conj(xh);
                    if (k == 0) xh = cld(xh.real(), 0);
                    const cld y = cld(xh.imag(), xh.real()) * chirp_ref(k, n);
                    e.name(b * m + k, y.real(), g * mag(xh));
                    e.name(c * m + b * m + k, y.imag(), g * mag(xh));
                }
            e.verify(s);
        }
    }
    {  // ---- C2R: x[k] = Im(w_N[k] c[k]) / N, k < N
        Buf<T> w(2 * c * m);
        w.random(71 * n + c);
        Buf<T> probe(span(c, sig.dist, n), sig.off);
        const bool planner_vec = al16(probe.p) && (c == 1 || sig.dist % V == 0);
        for (int vec = planner_vec ? 1 : 0; vec >= 0; --vec) {
            set_case("%s N=%zu M=%zu batch=%zu dist=%zu off=%zu vec=%d", Fp<T>::name(), n, m, c, sig.dist, sig.off, vec);
            Stat &s = stat_of(vec ? "any_c2r_odd_post_kernel<VEC>" : "any_c2r_odd_post_kernel");
            Buf<T> x(span(c, sig.dist, n), sig.off);
            x.sentinel();
            Expect<T> e(x, "signal");
            AnyRealArgs a = real_args<T>(n, n, m, spec.dist, sig.dist);
            a.in_re = w.p;
            a.in_im = w.p + c * m;
            a.out_re = x.p;
            a.scale = 1.0 / (double)n;
            a.gpt = (unsigned)((n + V - 1) / V);
            a.groups = c * a.gpt;
            launched(s, launch_any_real<T>(kC2rOddPost, vec != 0, a, nullptr));
            const ld g = gate_k<T>(1, 13);  // phase 7, cos / sin 2, products 2, sum 1, scale 1; the conversion
            for (size_t b = 0; b < c; ++b)
                for (size_t k = 0; k < n; ++k) {
                    const cld v(w.at(b * m + k), w.at(c * m + b * m + k)), y = v * chirp_ref(k, n) * (ld)a.scale;
                    e.name(b * sig.dist + k, y.imag(), g * mag(v) * (ld)a.scale);
                }
            e.verify(s);
        }
    }
}

// N = 1, 2: AnyRealPlanner::run_tiny
template <typename T> void real_tiny_case(size_t n, const Layout &sig, const Layout &spec) {
    const size_t c = sig.batch, bins = n / 2 + 1;
    {
        set_case("%s r2c N=%zu batch=%zu dist=%zu/%zu off=%zu/%zu", Fp<T>::name(), n, c, sig.dist, spec.dist, sig.off, spec.off);
        Stat &s = stat_of("any_real_tiny_kernel(r2c)");
        Buf<T> x(span(c, sig.dist, n), sig.off), outr(span(c, spec.dist, bins), spec.off), outi(span(c, spec.dist, bins), spec.off);
        x.random(73 * n + c);
        outr.sentinel();
        outi.sentinel();
        Expect<T> er(outr, "re"), ei(outi, "im");
        AnyRealArgs a{};
        a.n = n;
        a.in_re = x.p;
        a.out_re = outr.p;
        a.out_im = outi.p;
        a.in_dist = sig.dist;
        a.out_dist = spec.dist;
        a.groups = c;
        launched(s, launch_any_real<T>(kR2cTiny, false, a, nullptr));
        const ld g = gate_k<T>(1, 0);  // one sum in T
        for (size_t b = 0; b < c; ++b) {
            const ld x0 = x.at(b * sig.dist), x1 = n == 2 ? x.at(b * sig.dist + 1) : 0;
            if (n == 1) er.exact(b * spec.dist, x0);
            else {
                er.name(b * spec.dist, x0 + x1, g * (fabsl(x0) + fabsl(x1)));
                er.name(b * spec.dist + 1, x0 - x1, g * (fabsl(x0) + fabsl(x1)));
                ei.exact(b * spec.dist + 1, 0);
            }
            ei.exact(b * spec.dist, 0);
        }
        er.verify(s);
        ei.verify(s);
    }
    {
        set_case("%s c2r N=%zu batch=%zu dist=%zu/%zu off=%zu/%zu", Fp<T>::name(), n, c, spec.dist, sig.dist, spec.off, sig.off);
        Stat &s = stat_of("any_real_tiny_kernel(c2r)");
        Buf<T> xr(span(c, spec.dist, bins), spec.off), x(span(c, sig.dist, n), sig.off);
        xr.random(79 * n + c);
        x.sentinel();
        Expect<T> e(x, "signal");
        AnyRealArgs a{};
        a.n = n;
        a.in_re = xr.p;
        a.out_re = x.p;
        a.out_im = nullptr;
        a.in_dist = spec.dist;
        a.out_dist = sig.dist;
        a.groups = c;
        launched(s, launch_any_real<T>(kC2rTiny, false, a, nullptr));
        const ld g = gate_k<T>(1, 1);  // one sum in double (the half is exact); the conversion
        for (size_t b = 0; b < c; ++b) {
            const ld r0 = xr.at(b * spec.dist), r1 = n == 2 ? xr.at(b * spec.dist + 1) : 0;
            if (n == 1) e.exact(b * sig.dist, r0);
            else {
                e.name(b * sig.dist, 0.5L * (r0 + r1), g * 0.5L * (fabsl(r0) + fabsl(r1)));
                e.name(b * sig.dist + 1, 0.5L * (r0 - r1), g * 0.5L * (fabsl(r0) + fabsl(r1)));
            }
        }
        e.verify(s);
    }
}

// the signal's layouts paired with the half spectrum's: distances h + 1 and (h + 2) | 1 for the planes (h = N / 2)
template <typename T, typename F> void real_layouts(size_t n, size_t bins, F &&f) {
    const size_t hh = n / 2;
    for (const Layout &sig : layouts(n, Fp<T>::V)) {
        Layout spec{sig.batch, bins, sig.off};
        if (sig.batch > 1 && sig.dist != n) spec.dist = sig.dist == n + 1 ? ((hh + 2) | 1) : round_up(bins, Fp<T>::V);
        f(sig, spec);
    }
}

}  // namespace

int sweep_any_real() {
    for (size_t n : {6, 10, 12, 14, 18, 24, 30, 34, 40, 66, 516}) {  // even, no power of two: H = 3, 5, 6, 7, 9, 12, 15, 17, 20, 33, 258
        real_layouts<double>(n, n / 2 + 1, [&](const Layout &a, const Layout &b) { real_even_case<double>(n, a, b); });
        real_layouts<float>(n, n / 2 + 1, [&](const Layout &a, const Layout &b) { real_even_case<float>(n, a, b); });
    }
    for (size_t n : {3, 5, 7, 9, 15, 17, 33, 1031}) {
        real_layouts<double>(n, (n - 1) / 2 + 1, [&](const Layout &a, const Layout &b) { real_odd_case<double>(n, a, b); });
        real_layouts<float>(n, (n - 1) / 2 + 1, [&](const Layout &a, const Layout &b) { real_odd_case<float>(n, a, b); });
    }
    for (size_t n : {1, 2}) {
        real_layouts<double>(n, n / 2 + 1, [&](const Layout &a, const Layout &b) { real_tiny_case<double>(n, a, b); });
        real_layouts<float>(n, n / 2 + 1, [&](const Layout &a, const Layout &b) { real_tiny_case<float>(n, a, b); });
    }
    {  // more than one 256-thread workgroup of transforms for the one-thread-per-transform kernel
        const Layout sig{258, 3, 1}, spec{258, 3, 0};
        real_tiny_case<float>(2, sig, spec);
    }
    return report();
}
#endif

// ============================================================================================================ dct.hip
#if SWEEP_PART == 3
namespace {

// the scale of the twiddle sweeps, stated again: type II 2 f, type III N f; f = 1, 1 / sqrt(2N), 1 / (2N); ortho bin 0: II / sqrt 2, III * sqrt 2
ld scale_ref(int type, int norm, size_t n, bool bin0) {
    const ld f = norm == kDctForward ? 1.0L / (2.0L * n) : norm == kDctOrtho ? 1.0L / sqrtl(2.0L * n) : 1.0L;
    ld s = (type == 2 ? 2.0L : (ld)n) * f;
    if (bin0 && norm == kDctOrtho) s = type == 2 ? s / sqrtl(2.0L) : s * sqrtl(2.0L);
    return s;
}

// one chunk as DctPlanner::run_chunk launches its four sweeps
template <typename T> void dct_case(size_t n, bool dst, const Layout &lay) {
    constexpr size_t L = Fp<T>::V;
    const size_t c = lay.batch, dist = lay.dist, half = n / 2, e_ = (n + 1) / 2, h = n / 2;
    const size_t vd = round_up(n, L), cd = round_up(half + 1, L);
    const unsigned gpt_perm = (unsigned)((e_ + L - 1) / L), gpt_half = (unsigned)((half + 1 + L - 1) / L);
    Buf<T> probe(span(c, dist, n), lay.off);
    const bool planner_vec = al16(probe.p) && (c == 1 || dist % L == 0);
    const ld sgn = dst ? -1.0L : 1.0L;
    for (int vec = planner_vec ? 1 : 0; vec >= 0; --vec) {
        char tag[160];
        std::snprintf(tag, sizeof tag, "%s %s N=%zu batch=%zu dist=%zu off=%zu vec=%d", Fp<T>::name(), dst ? "dst" : "dct", n, c, dist,
                      lay.off, vec);
        {  // II-pre: v[i] = x[2i] (i < e), v[N-1-i] = +-x[2i+1] (i < h); the row's padding beyond N is not written
            set_case("%s", tag);
            Stat &s = stat_of(dst ? (vec ? "dct2_pre_kernel<DST,VEC>" : "dct2_pre_kernel<DST>") : (vec ? "dct2_pre_kernel<VEC>" : "dct2_pre_kernel"));
            Buf<T> x(span(c, dist, n), lay.off), v(c * vd);
            x.random(83 * n + c);
            v.sentinel();
            Expect<T> ex(v, "v");
            DctArgs a{};
            a.n = n;
            a.in = x.p;
            a.in_dist = dist;
            a.out = v.p;
            a.out_dist = vd;
            a.gpt = gpt_perm;
            a.groups = c * a.gpt;
            launched(s, launch_dct<T>(kDct2Pre, dst, vec != 0, a, nullptr));
            for (size_t b = 0; b < c; ++b) {
                for (size_t i = 0; i < e_; ++i) ex.exact(b * vd + i, x.at(b * dist + 2 * i));
                for (size_t i = 0; i < h; ++i) ex.exact(b * vd + n - 1 - i, sgn * x.at(b * dist + 2 * i + 1));
            }
            ex.verify(s);
        }
        {  // III-post: x[2i] = v[i] (i < e), x[2i+1] = +-v[N-1-i] (i < h)
            set_case("%s", tag);
            Stat &s = stat_of(dst ? (vec ? "dct3_post_kernel<DST,VEC>" : "dct3_post_kernel<DST>") : (vec ? "dct3_post_kernel<VEC>" : "dct3_post_kernel"));
            Buf<T> v(c * vd), x(span(c, dist, n), lay.off);
            v.random(89 * n + c);
            x.sentinel();
            Expect<T> ex(x, "x");
            DctArgs a{};
            a.n = n;
            a.in = v.p;
            a.in_dist = vd;
            a.out = x.p;
            a.out_dist = dist;
            a.gpt = gpt_perm;
            a.groups = c * a.gpt;
            launched(s, launch_dct<T>(kDct3Post, dst, vec != 0, a, nullptr));
            for (size_t b = 0; b < c; ++b) {
                for (size_t i = 0; i < e_; ++i) ex.exact(b * dist + 2 * i, v.at(b * vd + i));
                for (size_t i = 0; i < h; ++i) ex.exact(b * dist + 2 * i + 1, sgn * v.at(b * vd + n - 1 - i));
            }
            ex.verify(s);
        }
        for (int norm = kDctBackward; norm <= kDctForward; ++norm) {
            {  // II-post: z = e^{-i pi k/(2N)} V[k]; DCT y[k] = s Re z (k <= h), y[N-k] = -s Im z (1 <= k < e); DST y[N-1-k], y[k-1]
                set_case("%s norm=%d", tag, norm);
                Stat &s = stat_of(dst ? (vec ? "dct2_post_kernel<DST,VEC>" : "dct2_post_kernel<DST>") : (vec ? "dct2_post_kernel<VEC>" : "dct2_post_kernel"));
                Buf<T> fr(c * cd), fi(c * cd), y(span(c, dist, n), lay.off);
                fr.random(97 * n + c);
                fi.random(101 * n + c);
                y.sentinel();
                Expect<T> ey(y, "y");
                DctArgs a{};
                a.n = n;
                a.scale = dct_scale(2, norm, n);
                a.scale0 = dct_scale0(2, norm, n);
                a.in = fr.p;
                a.in_im = fi.p;
                a.in_dist = cd;
                a.out = y.p;
                a.out_dist = dist;
                a.gpt = gpt_half;
                a.groups = c * a.gpt;
                if (fabsl(a.scale - scale_ref(2, norm, n, false)) > 4 * kUD * a.scale || fabsl(a.scale0 - scale_ref(2, norm, n, true)) > 4 * kUD * a.scale0)
                    fail(s, "dct_scale(2, %d, %zu) is not the contract's", norm, n);
                launched(s, launch_dct<T>(kDct2Post, dst, vec != 0, a, nullptr));
                // roundings: the angle 1 (below pi / 4: no magnification), cos / sin 2, two products 2, their sum 1, the scale 1; the conversion
                const ld g = gate_k<T>(1, 7);
                for (size_t b = 0; b < c; ++b)
                    for (size_t k = 0; k <= h; ++k) {
                        const ld t = kPi * (ld)k / (ld)(2 * n), sc = k == 0 ? a.scale0 : a.scale;
                        const cld V_(fr.at(b * cd + k), fi.at(b * cd + k)), z = cld(cosl(t), -sinl(t)) * V_;
                        ey.name(b * dist + (dst ? n - 1 - k : k), sc * z.real(), g * sc * mag(V_));
                        if (k >= 1 && k < e_) ey.name(b * dist + (dst ? k - 1 : n - k), -sc * z.imag(), g * sc * mag(V_));
                    }
                ey.verify(s);
            }
            {  // III-pre: V[k] = s e^{i pi k/(2N)} (A - i B), A = X'[k], B = X'[N-k] (0 for k = 0); DST: X' = X reversed.
               // Im V[0], Im V[N/2] (even N) and the row's padding beyond h: exact zeros
                set_case("%s norm=%d", tag, norm);
                Stat &s = stat_of(dst ? (vec ? "dct3_pre_kernel<DST,VEC>" : "dct3_pre_kernel<DST>") : (vec ? "dct3_pre_kernel<VEC>" : "dct3_pre_kernel"));
                Buf<T> X(span(c, dist, n), lay.off), vr(c * cd), vi(c * cd);
                X.random(103 * n + c);
                vr.sentinel();
                vi.sentinel();
                Expect<T> er(vr, "V.re"), ei(vi, "V.im");
                DctArgs a{};
                a.n = n;
                a.scale = dct_scale(3, norm, n);
                a.scale0 = dct_scale0(3, norm, n);
                a.in = X.p;
                a.in_dist = dist;
                a.out = vr.p;
                a.out_im = vi.p;
                a.out_dist = cd;
                a.gpt = gpt_half;
                a.groups = c * a.gpt;
                if (fabsl(a.scale - scale_ref(3, norm, n, false)) > 4 * kUD * a.scale || fabsl(a.scale0 - scale_ref(3, norm, n, true)) > 4 * kUD * a.scale0)
                    fail(s, "dct_scale(3, %d, %zu) is not the contract's", norm, n);
                launched(s, launch_dct<T>(kDct3Pre, dst, vec != 0, a, nullptr));
                const ld g = gate_k<T>(1, 7);  // as II-post
                for (size_t b = 0; b < c; ++b)
                    for (size_t k = 0; k < cd; ++k) {
                        if (k > h) {
                            er.exact(b * cd + k, 0);
                            ei.exact(b * cd + k, 0);
                            continue;
                        }
                        auto Xp = [&](size_t j) { return X.at(b * dist + (dst ? n - 1 - j : j)); };
                        const ld A = Xp(k), B = k >= 1 ? Xp(n - k) : 0.0L, t = kPi * (ld)k / (ld)(2 * n), sc = k == 0 ? a.scale0 : a.scale;
                        const cld v = sc * cld(cosl(t), sinl(t)) * cld(A, -B);
                        er.name(b * cd + k, v.real(), g * sc * (fabsl(A) + fabsl(B)));
                        if (k == 0 || 2 * k == n) ei.exact(b * cd + k, 0);
                        else ei.name(b * cd + k, v.imag(), g * sc * (fabsl(A) + fabsl(B)));
                    }
                er.verify(s);
                ei.verify(s);
            }
        }
    }
}

}  // namespace

int sweep_dct() {
    for (size_t n : {1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 33, 1030})
        for (int dst = 0; dst < 2; ++dst) {
            for (const Layout &lay : layouts(n, 2)) dct_case<double>(n, dst != 0, lay);
            for (const Layout &lay : layouts(n, 4)) dct_case<float>(n, dst != 0, lay);
        }
    return report();
}
#endif

// ============================================================================================================ stft.hip
#if SWEEP_PART == 4
namespace {

struct StftShape {
    size_t len, f, h;
};

// StftPlanner::stft_dev / istft_dev: the frame sweep in chunks of `rows` workspace rows, the overlap-add sweep over whole signals
template <typename T> void stft_case(const StftShape &sh, int center, int pad, const Layout &lay, size_t rows) {
    constexpr size_t V = Fp<T>::V;
    const size_t len = sh.len, f = sh.f, h = sh.h, p = center ? f / 2 : 0, batch = lay.batch, sd = lay.dist;
    if (stft_bad_args(len, f, h, center, pad)) {  // every shape of the table is legal: a case must not skip itself
        set_case("L=%zu F=%zu H=%zu center=%d pad=%d", len, f, h, center, pad);
        fail(stat_of("stft_frame_kernel"), "stft_bad_args rejects a shape of the table");
        return;
    }
    const size_t frames = 1 + (len + 2 * p - f) / h, fd = round_up(f, V);
    if (frames != (size_t)stft_frames(len, f, h, p)) fail(stat_of("stft_frame_kernel"), "stft_frames");
    Buf<T> win(fd);  // the window, then zeros up to fd
    for (size_t j = 0; j < fd; ++j) win[j] = j < f ? (T)(0.25L + 0.75L * fabsl(rnd(107 * f, j))) : T(0);
    auto args = [&] {
        StftArgs a{};
        a.win = win.p;
        a.len = len;
        a.f = f;
        a.h = h;
        a.p = p;
        a.frames = frames;
        a.fd = fd;
        a.pad = pad;
        return a;
    };
    {  // frame: row r = w[j] x~[f H - p + j] (j < F) of flattened (signal, frame) q0 + r; zeros in the row's padding up to fd
        Stat &s = stat_of("stft_frame_kernel");
        Buf<T> x(span(batch, sd, len), lay.off);
        x.random(109 * len + f);
        const size_t total = batch * frames;
        for (size_t q0 = 0; q0 < total; q0 += rows) {
            const size_t c = total - q0 < rows ? total - q0 : rows;
            set_case("%s L=%zu F=%zu H=%zu center=%d pad=%d batch=%zu dist=%zu off=%zu rows q0=%zu..%zu", Fp<T>::name(), len, f, h, center,
                     pad, batch, sd, lay.off, q0, q0 + c);
            Buf<T> w(c * fd);
            w.sentinel();
            Expect<T> e(w, "rows");
            StftArgs a = args();
            a.in = x.p;
            a.sig_dist = sd;
            a.out = w.p;
            a.q0 = q0;
            a.gpt = (unsigned)(fd / V);
            a.groups = c * a.gpt;
            launched(s, launch_stft<T>(kStftFrame, a, nullptr));
            const ld g = gate_k<T>(1, 0);  // one product in T
            for (size_t r = 0; r < c; ++r) {
                const size_t b = (q0 + r) / frames, fr = (q0 + r) % frames;
                for (size_t j = 0; j < fd; ++j) {
                    if (j >= f) {
                        e.exact(r * fd + j, 0);
                        continue;
                    }
                    const long long i = (long long)(fr * h + j) - (long long)p, n = (long long)len;
                    ld v = 0;
                    if (i >= 0 && i < n) v = x.at(b * sd + i);
                    else if (pad == kStftReflect) v = x.at(b * sd + (size_t)(i < 0 ? -i : 2 * (n - 1) - i));
                    const ld y = win.at(j) * v;
                    if (y == 0) e.exact(r * fd + j, 0);
                    else e.name(r * fd + j, y, g * fabsl(y));
                }
            }
            e.verify(s);
        }
    }
    if (rows >= batch * frames) {  // overlap-add: out[t] = sum_f w[u - f H] y[f][u - f H] / sum_f w^2[u - f H], u = t + p; 0 without a frame
        Stat &s = stat_of("stft_ola_kernel");
        set_case("%s L=%zu F=%zu H=%zu center=%d batch=%zu dist=%zu off=%zu", Fp<T>::name(), len, f, h, center, batch, sd, lay.off);
        Buf<T> y(batch * frames * fd), out(span(batch, sd, len), lay.off);
        y.random(113 * len + f);
        out.sentinel();
        Expect<T> e(out, "signal");
        StftArgs a = args();
        a.in = y.p;
        a.out = out.p;
        a.sig_dist = sd;
        a.gpt = (unsigned)((len + V - 1) / V);
        a.groups = batch * a.gpt;
        launched(s, launch_stft<T>(kStftOla, a, nullptr));
        for (size_t b = 0; b < batch; ++b)
            for (size_t t = 0; t < len; ++t) {
                const size_t u = t + p;
                ld num = 0, den = 0, sum = 0;
                int taps = 0;
                for (size_t fr = 0; fr < frames; ++fr)
                    if (fr * h <= u && u < fr * h + f) {
                        const ld wv = win.at(u - fr * h), yv = y.at((b * frames + fr) * fd + u - fr * h);
                        num += wv * yv;
                        den += wv * wv;
                        sum += fabsl(wv * yv);
                        ++taps;
                    }
                if (!taps) e.exact(b * sd + t, 0);
                else e.name(b * sd + t, num / den, (ld)(taps + 2) * Fp<T>::u * sum / den);  // taps + 2, over den
            }
        e.verify(s);
    }
}

}  // namespace

int sweep_stft() {
    const StftShape shapes[] = {{10, 4, 1}, {9, 8, 8}, {23, 8, 3}, {17, 5, 2}, {12, 5, 3}, {9, 1, 1}, {7, 7, 7}, {300, 33, 7}};
    for (const StftShape &sh : shapes)
        for (int center = 0; center < 2; ++center)
            for (int pad = kStftReflect; pad <= kStftZero; ++pad) {
                if (!center && pad == kStftZero) continue;  // without centring nothing is padded
                for (size_t rows : {(size_t)1 << 20, (size_t)3}) {
                    for (const Layout &lay : layouts(sh.len, 2)) stft_case<double>(sh, center, pad, lay, rows);
                    for (const Layout &lay : layouts(sh.len, 4)) stft_case<float>(sh, center, pad, lay, rows);
                }
            }
    return report();
}
#endif

// ============================================================================================================ conv.hip
#if SWEEP_PART == 5
namespace {

struct ConvShape {
    size_t len, k, b;
    int mode;
};

// ConvPlanner::dev: per chunk of `rows` segments the segment, spectrum and save sweeps
template <typename T> void conv_case(const ConvShape &sh, const Layout &sig, size_t out_dist_extra, size_t rows) {
    constexpr size_t V = Fp<T>::V;
    const size_t len = sh.len, k = sh.k, bl = sh.b, batch = sig.batch, sd = sig.dist;
    if (conv_bad_args(len, k, sh.mode, 0, bl, V)) {  // every shape of the table is legal: a case must not skip itself
        set_case("L=%zu K=%zu B=%zu mode=%d", len, k, bl, sh.mode);
        fail(stat_of("conv_segment_kernel"), "conv_bad_args rejects a shape of the table");
        return;
    }
    const size_t hop = bl - k + 1, t0 = sh.mode == kConvFull ? 0 : sh.mode == kConvSame ? (k - 1) / 2 : k - 1;
    const size_t out_len = sh.mode == kConvFull ? len + k - 1 : sh.mode == kConvSame ? len : len - k + 1;
    const size_t segs = (out_len + hop - 1) / hop, bins = bl / 2 + 1, fd = round_up(bl, V), bd = round_up(bins, V);
    const size_t od = batch == 1 ? out_len : out_len + out_dist_extra, total = batch * segs;
    Stat &s_seg = stat_of("conv_segment_kernel"), &s_spec = stat_of("conv_spectrum_kernel"), &s_save = stat_of("conv_save_kernel");
    if (t0 != (size_t)conv_t0(k, sh.mode) || out_len != (size_t)conv_out_len(len, k, sh.mode) || segs != (size_t)conv_segments(out_len, k, bl))
        fail(s_seg, "the geometry of conv.hpp is not the contract's");
    Buf<T> x(span(batch, sd, len), sig.off), hh(2 * bd);
    x.random(127 * len + k);
    for (size_t j = 0; j < 2 * bd; ++j) hh[j] = j % bd < bins ? (T)rnd(131 * k, j) : T(0);  // H^: zeros beyond the bins
    const size_t out_groups = (out_len + V - 1) / V;
    for (size_t q0 = 0; q0 < total; q0 += rows) {
        const size_t c = total - q0 < rows ? total - q0 : rows;
        set_case("%s L=%zu K=%zu B=%zu mode=%d batch=%zu dist=%zu/%zu off=%zu segments q0=%zu..%zu of %zu per signal", Fp<T>::name(), len, k, bl,
                 sh.mode, batch, sd, od, sig.off, q0, q0 + c, segs);
        ConvArgs a{};
        a.h_re = hh.p;
        a.h_im = hh.p + bd;
        a.sig_dist = sd;
        a.out_dist = od;
        a.len = len;
        a.k = k;
        a.b = bl;
        a.s = hop;
        a.t0 = t0;
        a.out_len = out_len;
        a.segs = segs;
        a.fd = fd;
        a.bd = bd;
        a.q0 = q0;
        a.q1 = q0 + c;
        {  // segment: row r = x~[t0 + s S - (K - 1) + j] (j < B) of flattened (signal, segment) q0 + r; zeros up to fd.  Bit-equal
            Buf<T> row(c * fd);
            row.sentinel();
            Expect<T> e(row, "rows");
            a.in = x.p;
            a.out = row.p;
            a.gpt = (unsigned)(fd / V);
            a.groups = c * a.gpt;
            launched(s_seg, launch_conv<T>(kConvSegment, a, nullptr));
            for (size_t r = 0; r < c; ++r) {
                const size_t b = (q0 + r) / segs, sg = (q0 + r) % segs;
                for (size_t j = 0; j < fd; ++j) {
                    const long long i = (long long)(t0 + sg * hop + j) - (long long)(k - 1);
                    e.exact(r * fd + j, j < bl && i >= 0 && i < (long long)len ? x.at(b * sd + i) : 0.0L);
                }
            }
            e.verify(s_seg);
        }
        {  // spectrum: (re, im)[r][j] *= H^[j], j < bd
            Buf<T> re(c * bd), im(c * bd);
            re.random(137 * len + q0);
            im.random(139 * len + q0);
            Expect<T> er(re, "re"), ei(im, "im");
            const ld g = gate_k<T>(3, 0);  // two products and their difference / sum, in T
            for (size_t r = 0; r < c; ++r)
                for (size_t j = 0; j < bd; ++j) {
                    const ld xr = re.at(r * bd + j), xi = im.at(r * bd + j), hr = hh.at(j), hi = hh.at(bd + j);
                    if (j >= bins) {
                        er.exact(r * bd + j, 0);
                        ei.exact(r * bd + j, 0);
                        continue;
                    }
                    er.name(r * bd + j, xr * hr - xi * hi, g * (fabsl(xr * hr) + fabsl(xi * hi)));
                    ei.name(r * bd + j, xr * hi + xi * hr, g * (fabsl(xr * hi) + fabsl(xi * hr)));
                }
            a.re = re.p;
            a.im = im.p;
            a.gpt = (unsigned)(bd / V);
            a.groups = c * a.gpt;
            launched(s_spec, launch_conv<T>(kConvSpectrum, a, nullptr));
            er.verify(s_spec);
            ei.verify(s_spec);
        }
        {  // save: out[i] = y[s][K - 1 + i - s S], s = i / S, for the samples whose segment is in this chunk.  Bit-equal
            Buf<T> y(c * fd), out(span(batch, od, out_len), sig.off);
            y.random(149 * len + q0);
            out.sentinel();
            Expect<T> e(out, "out");
            const size_t b_lo = q0 / segs, s_lo = q0 % segs, b_hi = (q0 + c - 1) / segs, s_hi = (q0 + c - 1) % segs;
            const size_t i_end = ((s_hi + 1) * hop < out_len ? (s_hi + 1) * hop : out_len) - 1;
            a.in = y.p;
            a.out = out.p;
            a.gpt = (unsigned)out_groups;
            a.first = b_lo * out_groups + s_lo * hop / V;
            a.groups = b_hi * out_groups + i_end / V - a.first + 1;
            launched(s_save, launch_conv<T>(kConvSave, a, nullptr));
            for (size_t b = 0; b < batch; ++b)
                for (size_t i = 0; i < out_len; ++i) {
                    const size_t sg = i / hop, q = b * segs + sg;
                    if (q >= q0 && q < q0 + c) e.exact(b * od + i, y.at((q - q0) * fd + k - 1 + i - sg * hop));
                }
            e.verify(s_save);
        }
    }
}

}  // namespace

int sweep_conv() {
    // K = 1; K - 1 >= S (a sample in three segments); K - 1 and out_len no multiples of V; t0 > 0 (same, valid); one large
    const ConvShape shapes[] = {{10, 1, 4, kConvFull},  {10, 1, 1, kConvSame},  {13, 5, 6, kConvFull},   {13, 5, 6, kConvSame},
                                {13, 5, 6, kConvValid}, {11, 4, 6, kConvFull},  {11, 4, 6, kConvSame},   {11, 4, 7, kConvValid},
                                {9, 3, 16, kConvFull},  {7, 7, 8, kConvValid},  {600, 4, 16, kConvFull}, {600, 6, 11, kConvSame}};
    for (const ConvShape &sh : shapes)
        for (size_t rows : {(size_t)1 << 20, (size_t)3, (size_t)1}) {
            if (sh.len > 100 && rows == 1) continue;
            for (const Layout &lay : layouts(sh.len, 2)) conv_case<double>(sh, lay, lay.dist - sh.len, rows);
            for (const Layout &lay : layouts(sh.len, 4)) conv_case<float>(sh, lay, lay.dist - sh.len, rows);
        }
    return report();
}
#endif

// ============================================================================================================ czt.hip
#if SWEEP_PART == 6
namespace {

// (n v / 2^down) mod 1 of a double v, exactly: v = +-mant 2^(e - 53), so n v / 2^down = n mant / 2^q with q = 53 - e + down; the
// product fits 128 bits and its low q bits are the fraction (q <= 64 for the |v| >= 2^-10 used here)
ld frac_turns(unsigned long long n, double v, int down) {
    int e = 0;
    const double fr = std::frexp(std::fabs(v), &e);
    const unsigned long long mant = (unsigned long long)std::ldexp(fr, 53);
    const int q = 53 - e + down;
    if (mant == 0) return 0;
    if (q < 1 || q > 64) std::abort();  // outside what this test's steps and starts need
    const unsigned __int128 prod = (unsigned __int128)n * mant;
    const unsigned long long low = q == 64 ? (unsigned long long)prod : (unsigned long long)prod & ((1ull << q) - 1);
    const ld f = (ld)low * ldexpl(1.0L, -q);
    return v < 0 ? -f : f;
}
// exp(-2 pi i (k start + k^2 step / 2))
cld czt_unit_ref(unsigned long long k, double step, double start) {
    ld t = frac_turns(k * k, step, 1) + frac_turns(k, start, 0);
    t -= floorl(t);
    return cld(cosl(2 * kPi * t), -sinl(2 * kPi * t));
}

struct CztShape {
    size_t n, m;
    double step, start;
};

// one chunk as CztPlanner::run_chunk launches it
template <typename T> void czt_case(const CztShape &sh, const Layout &in, const Layout &out, bool real) {
    constexpr size_t V = Fp<T>::V;
    const size_t n = sh.n, bins = sh.m, c = in.batch;
    size_t l = 8;
    while (l < n + bins - 1) l <<= 1;
    if (l != (size_t)czt_conv_len(n, bins)) fail(stat_of("czt_pre_kernel"), "czt_conv_len");
    const unsigned log_l = ilog2_of(l);
    const CztFrac half_step = czt_frac(sh.step, 1), start_frac = czt_frac(sh.start, 0);
    // roundings: the phase's conversion and the doubling of the angle (2 pi 2^-55: below 2), cos / sin 2, two products 2, their sum 1;
    // the conversion
    const ld g = gate_k<T>(1, 7);
    {  // pre: a[b L + k] = x[b dist + k] exp(-2 pi i (k start + k^2 step / 2)) (k < N), 0 up to L; REAL: no imaginary plane
        Buf<T> xr(span(c, in.dist, n), in.off), xi(real ? 0 : span(c, in.dist, n), real ? 0 : in.off);
        xr.random(151 * n + c);
        xi.random(157 * n + c);
        const T *x_im = real ? nullptr : xi.p;
        const bool planner_vec = al16(xr.p) && al16(x_im) && in.dist % V == 0;
        for (int vec = planner_vec ? 1 : 0; vec >= 0; --vec) {
            set_case("%s N=%zu M=%zu L=%zu step=%g start=%g batch=%zu dist=%zu off=%zu real=%d vec=%d", Fp<T>::name(), n, bins, l, sh.step,
                     sh.start, c, in.dist, in.off, (int)real, vec);
            Stat &s = stat_of(real ? (vec ? "czt_pre_kernel<VEC,REAL>" : "czt_pre_kernel<REAL>") : (vec ? "czt_pre_kernel<VEC>" : "czt_pre_kernel"));
            Buf<T> w(2 * c * l);
            w.sentinel();
            Expect<T> e(w, "workspace");
            CztSweepArgs a{};
            a.log_l = log_l;
            a.in_dist = in.dist;
            a.out_dist = out.dist;
            a.half_step = half_step;
            a.start = start_frac;
            a.n = n;
            a.in_re = xr.p;
            a.in_im = x_im;
            a.out_re = w.p;
            a.out_im = w.p + c * l;
            a.groups = c * (l / V);
            launched(s, launch_czt_sweep<T>(0, vec != 0, a, nullptr));
            for (size_t b = 0; b < c; ++b)
                for (size_t k = 0; k < l; ++k) {
                    if (k >= n) {
                        e.exact(b * l + k, 0);
                        e.exact(c * l + b * l + k, 0);
                        continue;
                    }
                    const cld x(xr.at(b * in.dist + k), real ? 0.0L : xi.at(b * in.dist + k)), y = x * czt_unit_ref(k, sh.step, sh.start);
                    e.name(b * l + k, y.real(), g * mag(x));
                    e.name(c * l + b * l + k, y.imag(), g * mag(x));
                }
            e.verify(s);
        }
    }
    if (!real) {  // post: X[b dist + k] = exp(-2 pi i k^2 step / 2) w[b L + k], k < M
        Buf<T> w(2 * c * l);
        w.random(163 * n + c);
        Buf<T> probe_r(span(c, out.dist, bins), out.off), probe_i(span(c, out.dist, bins), out.off);
        const bool planner_vec = al16(probe_r.p) && al16(probe_i.p) && out.dist % V == 0;
        for (int vec = planner_vec ? 1 : 0; vec >= 0; --vec) {
            set_case("%s N=%zu M=%zu L=%zu step=%g batch=%zu dist=%zu off=%zu vec=%d", Fp<T>::name(), n, bins, l, sh.step, c, out.dist, out.off, vec);
            Stat &s = stat_of(vec ? "czt_post_kernel<VEC>" : "czt_post_kernel");
            Buf<T> outr(span(c, out.dist, bins), out.off), outi(span(c, out.dist, bins), out.off);
            outr.sentinel();
            outi.sentinel();
            Expect<T> er(outr, "re"), ei(outi, "im");
            CztSweepArgs a{};
            a.log_l = log_l;
            a.in_dist = in.dist;
            a.out_dist = out.dist;
            a.half_step = half_step;
            a.start = start_frac;
            a.n = bins;
            a.in_re = w.p;
            a.in_im = w.p + c * l;
            a.out_re = outr.p;
            a.out_im = outi.p;
            a.gpt = (unsigned)((bins + V - 1) / V);
            a.groups = c * a.gpt;
            launched(s, launch_czt_sweep<T>(2, vec != 0, a, nullptr));
            for (size_t b = 0; b < c; ++b)
                for (size_t k = 0; k < bins; ++k) {
                    const cld v(w.at(b * l + k), w.at(c * l + b * l + k)), y = v * czt_unit_ref(k, sh.step, 0.0);
                    er.name(b * out.dist + k, y.real(), g * mag(v));
                    ei.name(b * out.dist + k, y.imag(), g * mag(v));
                }
            er.verify(s);
            ei.verify(s);
        }
    }
}

void czt_chirp_b_case(const CztShape &sh) {  // b[j] = conj(c[j]) (j < M), b[L - j] = conj(c[j]) (0 < j < N), 0 elsewhere: CztPlanner::init
    const size_t l = (size_t)czt_conv_len(sh.n, sh.m);
    set_case("f64 N=%zu M=%zu L=%zu step=%g", sh.n, sh.m, l, sh.step);
    Stat &s = stat_of("czt_chirp_b_kernel");
    Buf<double> re(l), im(l);
    re.sentinel();
    im.sentinel();
    Expect<double> er(re, "re"), ei(im, "im");
    launched(s, launch_czt_chirp_b(re.p, im.p, sh.n, sh.m, ilog2_of(l), czt_frac(sh.step, 1), nullptr));
    const ld g = gate_k<double>(0, 3);  // the phase 2, the cosine or the sine 1
    for (size_t i = 0; i < l; ++i) {
        if (i >= sh.m && l - i >= sh.n) {
            er.exact(i, 0);
            ei.exact(i, 0);
            continue;
        }
        const cld b = std::conj(czt_unit_ref(i < sh.m ? i : l - i, sh.step, 0.0));
        er.name(i, b.real(), g);
        ei.name(i, b.imag(), g);
    }
    er.verify(s);
    ei.verify(s);
}

}  // namespace

int sweep_czt() {
    // N != M both ways, M < V (1 and 3), N = 1, a negative step and start, one shape with a second workgroup
    const CztShape shapes[] = {{5, 9, 0.013, 0.37},  {9, 5, 0.11, -0.2}, {7, 1, 0.25, 0.125},   {1, 7, -0.03, 0.4},    {3, 3, 0.4, 0.0},
                               {33, 17, 0.0071, 0.3}, {17, 33, 1.0 / 17, 0.0}, {15, 3, 0.21, -0.45}, {258, 300, 0.0019, 0.05}, {1030, 8, 0.003, -0.3},
                               {2, 4, 0.3, 0.1},      {4, 2, -0.17, 0.2},      {8, 16, 0.031, -0.07}, {16, 8, 1.0 / 16, 0.0}};
    for (const CztShape &sh : shapes) {
        for (int real = 0; real < 2; ++real) {
            const std::vector<Layout> li2 = layouts(sh.n, 2), lo2 = layouts(sh.m, 2), li4 = layouts(sh.n, 4), lo4 = layouts(sh.m, 4);
            for (size_t i = 0; i < li2.size(); ++i) czt_case<double>(sh, li2[i], lo2[i], real != 0);
            for (size_t i = 0; i < li4.size(); ++i) czt_case<float>(sh, li4[i], lo4[i], real != 0);
        }
        czt_chirp_b_case(sh);
    }
    return report();
}
#endif

// ============================================================================================================ complex_nums.hip
#if SWEEP_PART == 7
namespace {

// phast_deinterleave_*_dev / phast_combine_re_im_*_dev (c_abi.hip): `scalars` interleaved values, pairs = scalars / 2; nothing
// is launched for fewer than two.  Bit-equal both ways
template <typename T> void cn_case(size_t scalars, size_t off_in, size_t off_a, size_t off_b) {
    const size_t pairs = scalars / 2;
    if (scalars < 2) return;
    set_case("%s scalars=%zu offsets in=%zu a=%zu b=%zu", Fp<T>::name(), scalars, off_in, off_a, off_b);
    const bool vec = off_in == 0 && off_a == 0 && off_b == 0 && pairs >= Fp<T>::V;
    Buf<T> in(2 * pairs, off_in), a(pairs, off_a), b(pairs, off_b);
    in.random(167 * scalars + off_in);
    {
        Stat &s = stat_of(vec ? "deinterleave_vec+scalar_kernel" : "deinterleave_scalar_kernel");
        a.sentinel();
        b.sentinel();
        Expect<T> ea(a, "a"), eb(b, "b");
        for (size_t i = 0; i < pairs; ++i) {
            ea.exact(i, in.at(2 * i));
            eb.exact(i, in.at(2 * i + 1));
        }
        launched(s, launch_deinterleave<T>(in.p, a.p, b.p, pairs, nullptr));
        ea.verify(s);
        eb.verify(s);
    }
    {
        Stat &s = stat_of(vec ? "combine_vec+scalar_kernel" : "combine_scalar_kernel");
        Buf<T> out(2 * pairs, off_in);
        out.sentinel();
        Expect<T> e(out, "out");
        for (size_t i = 0; i < pairs; ++i) {
            e.exact(2 * i, a.at(i));
            e.exact(2 * i + 1, b.at(i));
        }
        launched(s, launch_combine<T>(a.p, b.p, out.p, pairs, nullptr));
        e.verify(s);
    }
}

}  // namespace

int sweep_complex_nums() {
    for (size_t scalars : {0, 1, 2, 3, 15, 16, 17, 127, 128, 129, 130, 131, 135, 1030, 4200}) {
        const size_t offs[5][3] = {{0, 0, 0}, {1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {1, 1, 1}};
        for (const auto &o : offs) {
            cn_case<double>(scalars, o[0], o[1], o[2]);
            cn_case<float>(scalars, o[0], o[1], o[2]);
        }
    }
    return report();
}
#endif

// ============================================================================================================ r2c.hip
#if SWEEP_PART == 8
namespace {

// roundings in T, along the twiddled term, which has the longer chain: the twiddle is a product of three table entries of unit
// modulus (each entry rounded once: 3; a complex product of unit-modulus factors adds u for its two products together, their
// magnitudes summing to at most 1, and u for their sum: 2 + 2) 7, the difference 1, the two products with it 1 and their sum 1,
// the last sum 1.  Every term of that last sum carries the factor 1/2 (exact), so the magnitude of the terms is half the data's
template <typename T> ld r2c_gate() { return gate_k<T>(11, 0); }

// R2cPlanner (planner_r2c.hpp): in place on planes of half + 1 points at `dist`, W_N tables as host_tw3 builds them.
// X[k] = (Z[k] + conj Z[H-k]) / 2 - i W^k (Z[k] - conj Z[H-k]) / 2, k <= H, Z[H] = Z[0]; Im X[0] = Im X[H] = 0 exactly
template <typename T> void untangle_case(size_t half, size_t batch, size_t dist, size_t off) {
    const size_t n = 2 * half;
    set_case("%s half=%zu batch=%zu dist=%zu off=%zu", Fp<T>::name(), half, batch, dist, off);
    Stat &s = stat_of("untangle_kernel");
    const unsigned tw_bits = tw3_bits_for(ilog2_of(n));
    const std::vector<cx_t<T>> tab = host_tw3<T>(ilog2_of(n), tw_bits);
    Buf<T> re(span(batch, dist, half + 1), off), im(span(batch, dist, half + 1), off);
    re.random(173 * half + batch);
    im.random(179 * half + batch);
    Expect<T> er(re, "re"), ei(im, "im");
    for (size_t b = 0; b < batch; ++b)
        for (size_t k = 0; k <= half; ++k) {
            const size_t k1 = k % half, k2 = (half - k1) % half;
            const cld z1(re.at(b * dist + k1), im.at(b * dist + k1)), z2 = std::conj(cld(re.at(b * dist + k2), im.at(b * dist + k2)));
            const cld x = (z1 + z2) * 0.5L - cld(0, 1) * root_ref(k, n) * (z1 - z2) * 0.5L;
            er.name(b * dist + k, x.real(), r2c_gate<T>() * 0.5L * (mag(z1) + mag(z2)));
            if (k == 0 || k == half) ei.exact(b * dist + k, 0);
            else ei.name(b * dist + k, x.imag(), r2c_gate<T>() * 0.5L * (mag(z1) + mag(z2)));
        }
    UntangleArgs ua{};
    ua.re = re.p;
    ua.im = im.p;
    ua.tw3 = tab.data();
    ua.dist = dist;
    ua.half = (unsigned)half;
    ua.tw_bits = tw_bits;
    ua.batch = (unsigned)batch;
    launched(s, launch_untangle<T>(ua, nullptr, nullptr, nullptr));
    er.verify(s);
    ei.verify(s);
}

// z[k] = (A + conj B) / 2 + i conj(W^k) (A - conj B) / 2, A = X[k], B = X[H - k], k < H; z planes at distance half
template <typename T> void c2r_pre_case(size_t half, size_t batch, size_t dist, size_t off) {
    const size_t n = 2 * half;
    set_case("%s half=%zu batch=%zu dist=%zu off=%zu", Fp<T>::name(), half, batch, dist, off);
    Stat &s = stat_of("c2r_preprocess_kernel");
    const unsigned tw_bits = tw3_bits_for(ilog2_of(n));
    const std::vector<cx_t<T>> tab = host_tw3<T>(ilog2_of(n), tw_bits);
    Buf<T> xr(span(batch, dist, half + 1), off), xi(span(batch, dist, half + 1), off), zr(batch * half), zi(batch * half);
    xr.random(181 * half + batch);
    xi.random(191 * half + batch);
    zr.sentinel();
    zi.sentinel();
    Expect<T> er(zr, "z.re"), ei(zi, "z.im");
    C2rPreArgs pa{};
    pa.in_re = xr.p;
    pa.in_im = xi.p;
    pa.z_re = zr.p;
    pa.z_im = zi.p;
    pa.tw3 = tab.data();
    pa.in_dist = dist;
    pa.z_dist = half;
    pa.half = (unsigned)half;
    pa.tw_bits = tw_bits;
    pa.batch = (unsigned)batch;
    launched(s, launch_c2r_preprocess<T>(pa, nullptr, nullptr, nullptr));
    for (size_t b = 0; b < batch; ++b)
        for (size_t k = 0; k < half; ++k) {
            const cld A(xr.at(b * dist + k), xi.at(b * dist + k)), B(xr.at(b * dist + half - k), xi.at(b * dist + half - k));
            const cld z = (A + std::conj(B)) * 0.5L + cld(0, 1) * std::conj(root_ref(k, n)) * (A - std::conj(B)) * 0.5L;
            er.name(b * half + k, z.real(), r2c_gate<T>() * 0.5L * (mag(A) + mag(B)));
            ei.name(b * half + k, z.imag(), r2c_gate<T>() * 0.5L * (mag(A) + mag(B)));
        }
    er.verify(s);
    ei.verify(s);
}

}  // namespace

int sweep_r2c() {
    for (size_t half : {2, 4, 8, 64, 1024})
        for (size_t batch : {1, 3})
            for (size_t dist : {half + 1, (half + 2) | 1})
                for (size_t off = 0; off < 2; ++off) {
                    if (batch == 1 && dist != half + 1) continue;
                    untangle_case<double>(half, batch, dist, off);
                    untangle_case<float>(half, batch, dist, off);
                    c2r_pre_case<double>(half, batch, dist, off);
                    c2r_pre_case<float>(half, batch, dist, off);
                }
    return report();
}
#endif

#endif  // SWEEP_PART != 0
