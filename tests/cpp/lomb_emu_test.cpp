// lomb_emu_test.cpp -- the sweeps of the Lomb-Scargle periodogram (csrc/lomb.hip, #included as it stands), run on the host
// under AddressSanitizer and UndefinedBehaviorSanitizer (tests/test_lomb_emulator.py builds and runs it; tests/emu/block_shim.hpp
// runs a workgroup as fibers that meet at __syncthreads(): the slab sweeps reduce through LDS).  A stand-alone program: no
// GPU, no HIP runtime.
//
// All kernels are driven through launch_lomb with arguments built as LombPlanner::run builds them, per chunk: whole
// (workspace_len(batch)) and in chunks of one signal (workspace_min()), aligned and one element off, on heap blocks of
// exactly the contract's elements (one element too far is an AddressSanitizer report).  Two kinds of data:
//     wide    y_j = n 2^-(j mod 60) with small integers n and y_0 = 0, weights k / 16: every product is exact, the sums are
//             not -- they round, so their bits depend on the order of the additions.  The first pass (partial) and, without
//             the floating mean, the strengths and the partials of YY are compared bit for bit with the same sums formed
//             here in the documented order: thread t adds its groups t, t + 256, ... ascending, then the tree of halving
//             strides; in both fiber orders.
//     exact   small integers and weights k / 16 with a final scale of 1: the mean difference, the residuals, the strengths
//             and every sum are exact in double and in float, so the floating-mean path is compared bit for bit with plain
//             sums in any order.
//     final   against the partials the workspace holds, in ascending slab order, times the scale
//     post    A1 planes of small integers and tables of dyadic values (which need not be a rotation: the formulas do not care):
//             every operation is exact, compared with the definition in long double
// so that a wrong kernel is blamed alone.  The type-3 transform between the strengths and A1 is the engine's own
// (tests/test_nufft_t3_emulator.py): here integer planes stand in for its output, with NaN in the planes' padding, which must
// not reach an output.  Outputs and the workspace start as a NaN bit pattern: an element the contract names must have lost
// it, every other one (lead-ins, gaps, the stand-in for the type-3 workspace) must have kept its bits.
#include <hip/hip_runtime.h>

#include "block_shim.hpp"

#include <cmath>
// any_len.hpp's chirp() (on lomb.hpp's include path, never called by these kernels) names the device's sincospi: a host
// overload so that the header compiles here
inline void sincospi(double t, double *s, double *c) {
    *s = std::sin(3.141592653589793238462643383279502884 * t);
    *c = std::cos(3.141592653589793238462643383279502884 * t);
}

#include "lomb.hip"

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
constexpr u64 kDoubleSentinel = 0x7ff8dead5eed0002ull;

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
    if (++counts[i] > 6) return;  // six lines per sweep: one sweep's failures do not hide another's
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
bool is_double_sentinel(const double *p) {
    u64 b;
    std::memcpy(&b, p, 8);
    return b == kDoubleSentinel;
}

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

// the geometry of LombPlanner<T> for (M, K); `nf4` elements per signal stand in for the type-3 workspace
template <typename T> struct Plan {
    static constexpr size_t V = Fp<T>::V, D = sizeof(double) / sizeof(T);
    size_t m, k, md, kd, q, slabs, nf4;
    Plan(size_t m_, size_t k_)
        : m(m_), k(k_), md((m_ + V - 1) / V * V), kd((k_ + V - 1) / V * V), q((size_t)lomb_slab_len(m_)),
          slabs((size_t)lomb_slabs(m_, q)), nf4(4 * V) {}
    size_t need(size_t c) const { return c * (md + 2 * kd) + c * nf4 + c * (2 + 2 * slabs) * D + (V - 1); }
    size_t chunk_of(T *d_work, size_t work_len, size_t batch, T **w) const {
        const size_t skip = ((16 - (reinterpret_cast<uintptr_t>(d_work) & 15u)) & 15u) / sizeof(T);
        *w = d_work + skip;
        const size_t avail = work_len - skip + (V - 1);
        size_t lo = 1, hi = batch;
        while (lo < hi) {
            const size_t mid = lo + (hi - lo + 1) / 2;
            if (need(mid) <= avail) lo = mid;
            else hi = mid - 1;
        }
        return lo;
    }
};

// the documented order of a slab's sum: thread t adds term(j) over its groups t, t + 256, ... (L elements each, ascending),
// then the tree of strides 128, 64, ... 1
template <typename F> double slab_sum(size_t lo, size_t hi, size_t L, F term) {
    double part[256];
    for (size_t t = 0; t < 256; ++t) {
        double s = 0;
        for (size_t j0 = lo + t * L; j0 < hi; j0 += 256 * L)
            for (size_t j = 0; j < L; ++j) s += term(j0 + j);
        part[t] = s;
    }
    for (size_t step = 128; step; step >>= 1)
        for (size_t t = 0; t < step; ++t) part[t] += part[t + step];
    return part[0];
}

struct Opt {
    size_t batch, off;
    bool chunked, wide, floating;
    int norm;
};

template <typename T> void run_case(size_t m, size_t k, const Opt &o) {
    constexpr size_t V = Fp<T>::V;
    set_case("%s M=%zu K=%zu batch=%zu off=%zu %s %s floating=%d norm=%d", Fp<T>::name(), m, k, o.batch, o.off,
             o.chunked ? "chunks of 1" : "whole", o.wide ? "wide" : "exact", (int)o.floating, o.norm);
    const Plan<T> pl(m, k);
    const size_t md = pl.md, kd = pl.kd, slabs = pl.slabs;
    const bool amp = o.norm == kLombAmplitude;
    // the weights k / 16, zeros beyond M
    Buf<T> wt(md);
    for (size_t j = 0; j < md; ++j) wt.p[j] = j < m ? (T)((1 + mix(3 * m + 1, j) % 15) / 16.0) : T(0);
    const size_t sd = o.batch == 1 ? m : m + 3, od = o.batch == 1 ? k : k + 5;
    Buf<T> y((o.batch - 1) * sd + m, o.off);
    auto yv = [&](size_t b, size_t j) -> T {
        const int n = small_int(7 * m + b, j, 8);
        if (!o.wide) return (T)n;
        return j == 0 ? T(0) : (T)std::ldexp((double)n, -(int)(j % 60));
    };
    for (size_t b = 0; b < o.batch; ++b)
        for (size_t j = 0; j < m; ++j) y.p[b * sd + j] = yv(b, j);
    // the tables: dyadic values, NaN-free padding as the planner's
    Buf<T> tab(4 * kd);
    for (size_t i = 0; i < 4 * kd; ++i) tab.p[i] = T(1);
    for (size_t i = 0; i < k; ++i) {
        tab.p[i] = (T)(0.5 * small_int(11, i, 3));
        tab.p[kd + i] = (T)(0.25 * small_int(13, i, 3));
        tab.p[2 * kd + i] = (T)std::ldexp(1.0, (int)(mix(17, i) % 5) - 2);
        tab.p[3 * kd + i] = (T)std::ldexp(1.0, (int)(mix(19, i) % 5) - 2);
    }
    Buf<T> out_re((o.batch - 1) * od + k, o.off), out_im((o.batch - 1) * od + k, o.off);
    const size_t want_chunk = o.chunked ? 1 : o.batch;
    const size_t work_len = pl.need(want_chunk);
    Buf<T> work(work_len, o.off);
    T *w = nullptr;
    const size_t chunk = pl.chunk_of(work.p, work_len, o.batch, &w);
    if (chunk != want_chunk) fail("chunk_of", "a chunk of %zu signals in a workspace of %zu elements", chunk, work_len);
    const double inv_wsum = 1.0;  // (the planner's is 1 / sum w; any scale shows that the final sweep applies it)
    auto zr = [&](size_t b, size_t i) { return (double)small_int(23 * k, b * k + i, 6); };
    auto zi = [&](size_t b, size_t i) { return (double)small_int(29 * k, b * k + i, 6); };

    for (size_t b0 = 0; b0 < o.batch; b0 += chunk) {
        const size_t c = o.batch - b0 < chunk ? o.batch - b0 : chunk;
        T *strength = w, *re = strength + c * md, *im = re + c * kd, *tw = im + c * kd;
        double *stat = reinterpret_cast<double *>(tw + c * pl.nf4), *part = stat + 2 * c;
        for (size_t i = 0; i < c * (2 + 2 * slabs); ++i) std::memcpy(stat + i, &kDoubleSentinel, 8);
        LombArgs a{};  // LombPlanner::run
        a.y = y.p + b0 * sd;
        a.w = wt.p;
        a.stat = stat;
        a.strength = strength;
        a.re = re;
        a.im = im;
        for (int i = 0; i < 4; ++i) a.tab[i] = tab.p + i * kd;
        a.out_re = out_re.p + b0 * od;
        a.out_im = amp ? out_im.p + b0 * od : nullptr;
        a.sig_dist = sd;
        a.out_dist = od;
        a.m = m;
        a.k = k;
        a.md = md;
        a.kd = kd;
        a.q = pl.q;
        a.slabs = slabs;
        a.floating_mean = o.floating;
        a.norm = o.norm;
        auto ys = [&](size_t b) { return y.p + (b0 + b) * sd; };
        auto slab_hi = [&](size_t s) { return (s + 1) * pl.q < m ? (s + 1) * pl.q : m; };
        if (o.floating) {
            a.part = part;
            a.groups = c * slabs * 256;
            for (int order = 0; order < 2; ++order) {
                block_shim::order = order ? block_shim::kDescending : block_shim::kAscending;
                for (size_t i = 0; i < c * slabs; ++i) std::memcpy(part + i, &kDoubleSentinel, 8);
                if (launch_lomb<T>(kLombPartial, false, a, nullptr) != hipSuccess) fail("lomb_partial", "the launcher failed");
                for (size_t b = 0; b < c; ++b)
                    for (size_t s = 0; s < slabs; ++s) {
                        const T *yy = ys(b);
                        const double want = slab_sum(s * pl.q, slab_hi(s), V, [&](size_t j) {
                            return j < m ? (double)wt.p[j] * ((double)yy[j] - (double)yy[0]) : 0.0;
                        });
                        ++g_compared;
                        if (!same_bits(part[b * slabs + s], want))
                            fail("lomb_partial", "partial of signal %zu slab %zu = %.17g, must be exactly %.17g (thread order %d)", b0 + b, s,
                                 part[b * slabs + s], want, order);
                    }
            }
            block_shim::order = block_shim::kAscending;
            a.which = 0;
            a.scale = inv_wsum;
            a.groups = c * 256;
            if (launch_lomb<T>(kLombFinal, false, a, nullptr) != hipSuccess) fail("lomb_final", "the launcher failed");
            for (size_t b = 0; b < c; ++b) {
                double s = 0;
                for (size_t i = 0; i < slabs; ++i) s += part[b * slabs + i];
                ++g_compared;
                if (!same_bits(stat[2 * b], s * inv_wsum)) fail("lomb_final", "mean difference of signal %zu = %.17g, must be exactly %.17g", b0 + b, stat[2 * b], s * inv_wsum);
                if (!is_double_sentinel(stat + 2 * b + 1)) fail("lomb_final", "the first final sweep wrote YY of signal %zu", b0 + b);
            }
        }
        double *part2 = part + c * slabs;
        a.part = part2;
        a.groups = c * slabs * 256;
        if (launch_lomb<T>(kLombStrength, false, a, nullptr) != hipSuccess) fail("lomb_strength", "the launcher failed");
        for (size_t b = 0; b < c; ++b) {
            const T *yy = ys(b);
            const double y0 = o.floating ? (double)yy[0] : 0.0, d = o.floating ? stat[2 * b] : 0.0;
            auto res = [&](size_t j) { return ((double)yy[j] - y0) - d; };
            for (size_t j = 0; j < md; ++j) {
                const T got = strength[b * md + j], want = j < m ? (T)((double)wt.p[j] * res(j)) : T(0);
                ++g_compared;
                if (!same_bits(got, want)) fail("lomb_strength", "strength %zu of signal %zu = %.9Lg, must be exactly %.9Lg", j, b0 + b, (ld)got, (ld)want);
            }
            for (size_t s = 0; s < slabs; ++s) {
                const double want = slab_sum(s * pl.q, slab_hi(s), V, [&](size_t j) { return j < m ? (double)wt.p[j] * res(j) * res(j) : 0.0; });
                ++g_compared;
                if (!same_bits(part2[b * slabs + s], want))
                    fail("lomb_strength", "partial of YY of signal %zu slab %zu = %.17g, must be exactly %.17g", b0 + b, s, part2[b * slabs + s], want);
            }
        }
        a.which = 1;
        a.scale = 0.5;  // any scale: the planner's is 1 / sum w
        a.groups = c * 256;
        const std::vector<double> stat0(stat, stat + 2 * c);
        if (launch_lomb<T>(kLombFinal, false, a, nullptr) != hipSuccess) fail("lomb_final", "the launcher failed");
        for (size_t b = 0; b < c; ++b) {
            double s = 0;
            for (size_t i = 0; i < slabs; ++i) s += part2[b * slabs + i];
            ++g_compared;
            if (!same_bits(stat[2 * b + 1], s * 0.5)) fail("lomb_final", "YY of signal %zu = %.17g, must be exactly %.17g", b0 + b, stat[2 * b + 1], s * 0.5);
            if (!same_bits(stat[2 * b], stat0[2 * b])) fail("lomb_final", "the second final sweep wrote the mean of signal %zu", b0 + b);
        }
        // A1: small integers, NaN in the padding of every plane; YY a power of two so that normalize is exact
        for (size_t b = 0; b < c; ++b) {
            for (size_t i = 0; i < kd; ++i) {
                if (i < k) {
                    re[b * kd + i] = (T)zr(b0 + b, i);
                    im[b * kd + i] = (T)zi(b0 + b, i);
                } else {
                    std::memcpy(re + b * kd + i, &Fp<T>::sentinel, sizeof(T));
                    std::memcpy(im + b * kd + i, &Fp<T>::sentinel, sizeof(T));
                }
            }
            stat[2 * b + 1] = std::ldexp(1.0, (int)((b0 + b) % 3) + 1);
        }
        a.scale = (double)m / 4;
        a.gpt = (unsigned)(kd / V);
        a.groups = c * a.gpt;
        auto al = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; };
        const bool vec = al(a.out_re) && (!amp || al(a.out_im)) && (c == 1 || od % V == 0);
        if (launch_lomb<T>(kLombPost, vec, a, nullptr) != hipSuccess) fail("lomb_post", "the launcher failed");
        for (size_t b = 0; b < c; ++b)
            for (size_t i = 0; i < k; ++i) {
                const ld ar = zr(b0 + b, i), ai = zi(b0 + b, i), ct = tab.p[i], st = tab.p[kd + i], icc = tab.p[2 * kd + i], iss = tab.p[3 * kd + i];
                const ld yc = ar * ct + ai * st, ysn = ai * ct - ar * st, ca = yc * icc, cb = ysn * iss, p = 2 * (ca * yc + cb * ysn);
                const T got_re = out_re.p[(b0 + b) * od + i];
                T want_re, want_im = T(0);
                if (amp) {
                    want_re = (T)(double)(ca * ct - cb * st);
                    want_im = (T)(double)(ca * st + cb * ct);
                } else {
                    want_re = (T)(double)(o.norm == kLombNormalize ? p * (ld)(0.5 / stat[2 * b + 1]) : p * (ld)((double)m / 4));
                }
                ++g_compared;
                if (!same_bits(got_re, want_re)) fail("lomb_post", "output %zu of signal %zu = %.9Lg, must be exactly %.9Lg", i, b0 + b, (ld)got_re, (ld)want_re);
                if (amp && !same_bits(out_im.p[(b0 + b) * od + i], want_im))
                    fail("lomb_post", "imaginary output %zu of signal %zu = %.9Lg, must be exactly %.9Lg", i, b0 + b, (ld)out_im.p[(b0 + b) * od + i], (ld)want_im);
            }
        // the stand-in for the type-3 workspace has kept its bits
        for (size_t e = 0; e < c * pl.nf4; ++e)
            if (!work.is_sentinel((long long)(tw - work.p + e))) {
                fail("lomb", "the type-3 part of the workspace was written at element %zu", e);
                break;
            }
    }
    // what the contract names has been written, nothing else has
    for (size_t b = 0; b < o.batch; ++b) {
        for (size_t i = 0; i < (b + 1 < o.batch ? od : k); ++i) {
            const bool named = i < k;
            if (out_re.is_sentinel((long long)(b * od + i)) == named) fail("lomb_post", "element %zu of output row %zu was %s", i, b, named ? "not written" : "written");
            if (out_im.is_sentinel((long long)(b * od + i)) == (named && amp))
                fail("lomb_post", "element %zu of imaginary output row %zu was %s", i, b, named && amp ? "not written" : "written");
        }
        for (size_t j = 0; j < m; ++j)
            if (!same_bits(y.p[b * sd + j], yv(b, j))) {
                fail("lomb", "value %zu of signal %zu was written", j, b);
                break;
            }
    }
    for (size_t e = 1; e <= o.off; ++e) {
        if (!out_re.is_sentinel(-(long long)e) || !out_im.is_sentinel(-(long long)e)) fail("lomb_post", "the element in front of an output was written");
        if (!work.is_sentinel(-(long long)e)) fail("lomb", "the element in front of the workspace was written");
    }
}

}  // namespace

int main() {
    struct Shape {
        size_t m, k;
        bool big;
    };
    // one point; below, at and above one group; one slab less one, exactly one, one more; three slabs with a ragged tail
    const Shape shapes[] = {{1, 1, false}, {3, 2, false}, {4, 5, false}, {37, 4, false}, {300, 257, false}, {2047, 3, true}, {2048, 8, true},
                            {2049, 7, true}, {5000, 9, true}};
    for (const Shape &s : shapes)
        for (size_t batch = 1; batch <= 3; batch += 2)
            for (size_t off = 0; off < 2; ++off)
                for (int chunked = 0; chunked < 2; ++chunked)
                    for (int mode = 0; mode < 3; ++mode) {  // (wide, floating): (1, 1), (1, 0), (0, 1)
                        if (s.big && (batch != 1 + 2 * off || chunked != (int)off)) continue;
                        const Opt o{batch, off, chunked != 0, mode != 2, mode != 1, (int)((s.m + batch + off + mode) % 3)};
                        run_case<double>(s.m, s.k, o);
                        run_case<float>(s.m, s.k, o);
                    }
    std::printf("lomb: ");
    block_shim::print_counters();
    std::printf("lomb: elements %llu checked\n", g_compared);
    std::printf("lomb: %s (%d failures)\n", g_fails ? "FAILED" : "ok", g_fails);
    phast_test_exit(g_fails ? 1 : 0);
}
