// mdct_emu_test.cpp -- the four sweeps of the MDCT and its inverse (csrc/mdct.hip, #included as it stands), run on the host
// under AddressSanitizer and UndefinedBehaviorSanitizer (tests/test_mdct_emulator.py builds and runs it;
// tests/emu/sweep_shim.hpp turns a launch into a serial loop).  A stand-alone program: no GPU, no HIP runtime.
//
// All four kernels are driven through launch_mdct with arguments built as MdctPlanner builds them, per chunk.  Signals,
// coefficients and spectra hold small integers and the window is all ones, so the fold, the de-interleave, the unfold and the
// overlap-add are exact in float and in double.  Every sweep with a twiddle runs twice:
//     with the identity table (cos = 1, sin = 0)   what it moves, bit for bit against the definition's own index formulas;
//     with the planner's table                      what it multiplies, against the same expression on the host (to 4 ulp of
//                                                   the operands: the compiler may contract either side into an fma).
// Padding elements of the z planes must be exact zeros.  Buffers are heap allocations of exactly the bytes the contract covers
// (one element too far is an AddressSanitizer report); an "unaligned" buffer is one element longer and used from element 1.
// Outputs and workspaces start as a NaN bit pattern: an element the contract names must have lost it, every other one (the
// lead-in, the gaps between the signals of a batch, the padding of the rows v) must have kept its exact bits.  The complex
// transform between the sweeps is the engine's own: tests/cpp/pass_emu_test.cpp and tests/cpp/sweep_emu_test.cpp have it.
#include <hip/hip_runtime.h>

#include "sweep_shim.hpp"

#include "mdct.hip"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
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

template <typename T> bool near(T got, ld want, ld scale) {
    const ld d = (ld)got - want;
    return (d < 0 ? -d : d) <= 4 * (ld)std::numeric_limits<T>::epsilon() * scale;
}

// the geometry and the device table of MdctPlanner<T> for (L, N, padded), the window all ones
template <typename T> struct Plan {
    static constexpr size_t V = Fp<T>::V;
    size_t len, n, h, frames, hd, nd, wd;
    int padded;
    Buf<T> tab, ident;  // w[wd], pre cos, pre sin, post cos, post sin (hd each); `ident`: cos = 1, sin = 0
    Plan(size_t len_, size_t n_, int padded_)
        : len(len_), n(n_), h(n_ / 2), frames((size_t)mdct_frames(len_, n_, padded_)), hd((n_ / 2 + V - 1) / V * V),
          nd((n_ + V - 1) / V * V), wd((2 * n_ + V - 1) / V * V), padded(padded_), tab(wd + 4 * hd), ident(wd + 4 * hd) {
        for (size_t i = 0; i < wd + 4 * hd; ++i) tab.p[i] = ident.p[i] = T(0);
        for (size_t j = 0; j < 2 * n; ++j) tab.p[j] = ident.p[j] = T(1);
        for (size_t m = 0; m < h; ++m) {
            ld c, s;
            dct4_twiddle(dct4_pre_num(m), 4 * n, &c, &s);
            tab.p[wd + m] = (T)c;
            tab.p[wd + hd + m] = (T)s;
            dct4_twiddle(dct4_post_num(m), 4 * n, &c, &s);
            tab.p[wd + 2 * hd + m] = (T)c;
            tab.p[wd + 3 * hd + m] = (T)s;
            ident.p[wd + m] = ident.p[wd + 2 * hd + m] = T(1);
        }
    }
    MdctArgs args(bool post, bool identity) const {  // MdctPlanner::args
        const T *t = identity ? ident.p : tab.p;
        MdctArgs a{};
        a.win = t;
        a.tw_c = t + wd + (post ? 2 * hd : 0);
        a.tw_s = t + wd + (post ? 3 * hd : hd);
        a.len = len;
        a.n = n;
        a.frames = frames;
        a.padded = padded;
        a.scale = 1.0;
        a.gpt = (unsigned)(hd / V);
        return a;
    }
};

// the fold of the definition: u[j] of the frame that starts at sample s0 of x (zero outside [0, L)), window all ones
template <typename T> ld fold_of(const T *x, long long s0, long long len, size_t j, size_t h) {
    auto xw = [&](size_t i) -> ld {
        const long long s = s0 + (long long)i;
        return s >= 0 && s < len ? (ld)x[s] : 0;
    };
    return j < h ? -xw(3 * h - 1 - j) - xw(3 * h + j) : xw(j - h) - xw(3 * h - 1 - j);
}

// one pre sweep (kMdctPre of signal rows or kDct4Pre of coefficient rows) into fresh z planes, with either table
template <typename T, typename Src>
void check_pre(const char *kernel, int kind, const Plan<T> &pl, MdctArgs a, size_t c, bool identity, Src &&u_of) {
    const size_t hd = pl.hd, h = pl.h;
    Buf<T> z(2 * c * hd);
    a.out = z.p;
    a.out_im = z.p + c * hd;
    a.out_dist = hd;
    a.groups = c * a.gpt;
    if (launch_mdct<T>(kind, false, a, nullptr) != hipSuccess) fail(kernel, "the launcher failed");
    const T *tc = (const T *)a.tw_c, *ts = (const T *)a.tw_s;
    for (size_t r = 0; r < c; ++r)
        for (size_t m = 0; m < hd; ++m)
            for (int part = 0; part < 2; ++part) {
                const long long at = (long long)((part ? c * hd : 0) + r * hd + m);
                const T got = z.p[at];
                ++g_compared;
                if (z.is_sentinel(at)) {
                    fail(kernel, "row %zu element %zu (%s) was not written", r, m, part ? "im" : "re");
                } else if (m >= h) {
                    if (!(got == T(0)) || std::signbit(got)) fail(kernel, "row %zu padding element %zu = %.9Lg, must be exactly 0", r, m, (ld)got);
                } else {
                    const T re = (T)u_of(r, 2 * m), im = (T)u_of(r, pl.n - 1 - 2 * m);
                    if (identity) {
                        const T want = part ? im : re;
                        if (!(got == want)) fail(kernel, "row %zu element %zu (%s) = %.9Lg, must be exactly %.9Lg", r, m, part ? "im" : "re", (ld)got, (ld)want);
                    } else {
                        const T want = part ? im * tc[m] - re * ts[m] : re * tc[m] + im * ts[m];
                        if (!near(got, (ld)want, std::fabs((ld)re) + std::fabs((ld)im)))
                            fail(kernel, "row %zu element %zu (%s) = %.17Lg, the host's expression gives %.17Lg", r, m, part ? "im" : "re", (ld)got, (ld)want);
                    }
                }
            }
}

template <typename T> void run_case(size_t n, size_t len, int padded, size_t batch, size_t off, bool chunked) {
    constexpr size_t V = Fp<T>::V;
    set_case("%s N=%zu L=%zu padded=%d batch=%zu off=%zu %s", Fp<T>::name(), n, len, padded, batch, off, chunked ? "chunked" : "whole");
    if (mdct_bad_args(len, n, padded)) {
        fail("mdct_bad_args", "rejects a shape of the table");
        return;
    }
    const Plan<T> pl(len, n, padded);
    const size_t h = pl.h, hd = pl.hd, nd = pl.nd, frames = pl.frames, total = batch * frames;
    const size_t sd = batch == 1 ? len : len + 3;
    Buf<T> x((batch - 1) * sd + len, off);
    for (size_t b = 0; b < batch; ++b)
        for (size_t i = 0; i < len; ++i) x.p[b * sd + i] = (T)small_int(7 * n + b, i, 8);

    // ---- forward: the fold-and-pre sweep per chunk of frames, then the post sweep into the caller's coefficients ----
    Buf<T> X(total * n, off);
    const size_t rows = chunked ? 1 : total;
    for (int identity = 1; identity >= 0; --identity)
        for (size_t q0 = 0; q0 < total; q0 += rows) {
            const size_t c = total - q0 < rows ? total - q0 : rows;
            MdctArgs a = pl.args(false, identity != 0);
            a.in = x.p;
            a.in_dist = sd;
            a.q0 = q0;
            check_pre<T>("mdct_pre_kernel<signal>", kMdctPre, pl, a, c, identity != 0, [&](size_t r, size_t j) {
                const size_t b = (q0 + r) / frames, t = (q0 + r) % frames;
                return fold_of(x.p + b * sd, ((long long)t - padded) * (long long)n, (long long)len, j, h);
            });
        }
    // Z planes of small integers stand in for the transform's output; the padding is poison the post sweep must not use
    std::vector<int> zr(total * h), zi(total * h);
    for (size_t i = 0; i < total * h; ++i) {
        zr[i] = small_int(11 * n, i, 6);
        zi[i] = small_int(13 * n, i, 6);
    }
    for (size_t q0 = 0; q0 < total; q0 += rows) {  // identity table, into the caller's coefficients: exact
        const size_t c = total - q0 < rows ? total - q0 : rows;
        Buf<T> z(2 * c * hd);
        for (size_t r = 0; r < c; ++r)
            for (size_t k = 0; k < h; ++k) {
                z.p[r * hd + k] = (T)zr[(q0 + r) * h + k];
                z.p[c * hd + r * hd + k] = (T)zi[(q0 + r) * h + k];
            }
        MdctArgs a = pl.args(true, true);
        a.in = z.p;
        a.in_im = z.p + c * hd;
        a.in_dist = hd;
        a.out = X.p + q0 * n;
        a.out_dist = n;
        a.groups = c * a.gpt;
        if (launch_mdct<T>(kDct4Post, true, a, nullptr) != hipSuccess) fail("dct4_post_kernel", "the launcher failed");
    }
    for (size_t q = 0; q < total; ++q)
        for (size_t j = 0; j < n; ++j) {
            const T want = j % 2 == 0 ? (T)zr[q * h + j / 2] : (T)-zi[q * h + (n - 1 - j) / 2];  // X[2k] = Re c, X[N-1-2k] = -Im c
            ++g_compared;
            if (X.is_sentinel((long long)(q * n + j))) fail("dct4_post_kernel", "coefficient %zu of frame %zu was not written", j, q);
            else if (!(X.p[q * n + j] == want))
                fail("dct4_post_kernel", "coefficient %zu of frame %zu = %.9Lg, must be exactly %.9Lg", j, q, (ld)X.p[q * n + j], (ld)want);
        }
    for (size_t i = 1; i <= off; ++i)
        if (!X.is_sentinel(-(long long)i)) fail("dct4_post_kernel", "the element in front of the coefficients was written");

    // ---- inverse, per chunk of whole signals: pre sweep of the coefficients, post sweep into v, overlap-add ----
    for (size_t q = 0; q < total; ++q)
        for (size_t j = 0; j < n; ++j) X.p[q * n + j] = (T)small_int(17 * n, q * n + j, 8);
    Buf<T> out((batch - 1) * sd + len, off);
    const size_t sigs = chunked ? 1 : batch;
    for (size_t b0 = 0; b0 < batch; b0 += sigs) {
        const size_t cb = batch - b0 < sigs ? batch - b0 : sigs, c = cb * frames;
        for (int identity = 1; identity >= 0 && c; --identity) {
            MdctArgs a = pl.args(false, identity != 0);
            a.in = X.p + b0 * frames * n;
            a.in_dist = n;
            check_pre<T>("mdct_pre_kernel<row>", kDct4Pre, pl, a, c, identity != 0,
                         [&](size_t r, size_t j) { return (ld)X.p[(b0 * frames + r) * n + j]; });
        }
        // the post sweep with the planner's table and 2 / N into the rows v: every element against the host's expression, the
        // rows' padding untouched
        Buf<T> z(2 * c * hd), v(c * nd);
        for (size_t r = 0; r < c; ++r)
            for (size_t k = 0; k < h; ++k) {
                z.p[r * hd + k] = (T)zr[(b0 * frames + r) * h + k];
                z.p[c * hd + r * hd + k] = (T)zi[(b0 * frames + r) * h + k];
            }
        MdctArgs a = pl.args(true, false);
        a.in = z.p;
        a.in_im = z.p + c * hd;
        a.in_dist = hd;
        a.out = v.p;
        a.out_dist = nd;
        a.scale = 2.0 / (double)n;
        a.groups = c * a.gpt;
        if (c && launch_mdct<T>(kDct4Post, false, a, nullptr) != hipSuccess) fail("dct4_post_kernel", "the launcher failed");
        const T *pc = (const T *)a.tw_c, *ps = (const T *)a.tw_s, sc = (T)a.scale;
        for (size_t r = 0; r < c; ++r)
            for (size_t j = 0; j < nd; ++j) {
                const long long at = (long long)(r * nd + j);
                ++g_compared;
                if (j >= n) {
                    if (!v.is_sentinel(at)) fail("dct4_post_kernel", "the padding of row %zu of v was written", r);
                    continue;
                }
                const size_t k = j % 2 == 0 ? j / 2 : (n - 1 - j) / 2;
                const T fr = z.p[r * hd + k], fi = z.p[c * hd + r * hd + k];
                const T want = j % 2 == 0 ? sc * (fr * pc[k] + fi * ps[k]) : sc * (fr * ps[k] - fi * pc[k]);
                if (v.is_sentinel(at)) fail("dct4_post_kernel", "element %zu of row %zu of v was not written", j, r);
                else if (!near(v.p[at], (ld)want, (ld)sc * (std::fabs((ld)fr) + std::fabs((ld)fi))))
                    fail("dct4_post_kernel", "element %zu of row %zu of v = %.17Lg, the host's expression gives %.17Lg", j, r, (ld)v.p[at], (ld)want);
            }
        // rows v of small integers for the overlap-add; their padding stays poison
        for (size_t r = 0; r < c; ++r)
            for (size_t j = 0; j < n; ++j) v.p[r * nd + j] = (T)small_int(19 * n, (b0 * frames + r) * n + j, 8);
        a = pl.args(false, true);
        a.in = v.p;
        a.in_dist = nd;
        a.out = out.p + b0 * sd;
        a.out_dist = sd;
        a.gpt = (unsigned)((len + V - 1) / V);
        a.groups = cb * a.gpt;
        if (launch_mdct<T>(kMdctOla, false, a, nullptr) != hipSuccess) fail("imdct_ola_kernel", "the launcher failed");
    }
    for (size_t b = 0; b < batch; ++b) {
        for (size_t s = 0; s < len; ++s) {
            ld want = 0;  // the definition: the sum over the frames that hold s of the unfolded v, window all ones
            for (size_t t = 0; t < frames; ++t) {
                const long long j = (long long)s - ((long long)t - padded) * (long long)n;
                if (j < 0 || j >= 2 * (long long)n) continue;
                const size_t q = b * frames + t, jj = (size_t)j;
                auto vv = [&](size_t i) { return (ld)small_int(19 * n, q * n + i, 8); };
                want += jj < h ? vv(jj + h) : jj < 3 * h ? -vv(3 * h - 1 - jj) : -vv(jj - 3 * h);
            }
            ++g_compared;
            if (out.is_sentinel((long long)(b * sd + s))) fail("imdct_ola_kernel", "sample %zu of signal %zu was not written", s, b);
            else if (!((ld)out.p[b * sd + s] == want))
                fail("imdct_ola_kernel", "sample %zu of signal %zu = %.9Lg, must be exactly %.9Lg", s, b, (ld)out.p[b * sd + s], want);
        }
        if (b + 1 < batch)
            for (size_t i = len; i < sd; ++i)
                if (!out.is_sentinel((long long)(b * sd + i))) fail("imdct_ola_kernel", "the gap behind signal %zu was written", b);
    }
    for (size_t i = 1; i <= off; ++i)
        if (!out.is_sentinel(-(long long)i)) fail("imdct_ola_kernel", "the element in front of the signals was written");
}

}  // namespace

int main() {
    for (size_t n : {2, 4, 6, 30, 34, 40})  // h = 1, 2, 3, 15, 17, 20 (the last: whole groups and 16-byte rows in f32 too)
        for (size_t len : {(size_t)1, n + 1, 3 * n + 5})
            for (int padded = 1; padded >= 0; --padded) {
                if (!padded && len < 2 * n) continue;
                for (size_t batch = 1; batch <= 2; ++batch)
                    for (size_t off = 0; off < 2; ++off)
                        for (int chunked = 0; chunked < 2; ++chunked) {
                            run_case<double>(n, len, padded, batch, off, chunked != 0);
                            run_case<float>(n, len, padded, batch, off, chunked != 0);
                        }
            }
    std::printf("mdct: launches %llu threads %llu elements %llu checked\n", sweep_shim::launches, sweep_shim::threads_run, g_compared);
    std::printf("mdct: %s (%d failures)\n", g_fails ? "FAILED" : "ok", g_fails);
    phast_test_exit(g_fails ? 1 : 0);
}
