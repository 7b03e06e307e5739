// dwt_emu_test.cpp -- the kernels of the discrete wavelet transform (csrc/dwt.hip, #included as it stands), run on the host under
// AddressSanitizer and UndefinedBehaviorSanitizer (tests/test_dwt_emulator.py builds and runs it; tests/emu/block_shim.hpp runs a
// workgroup as fibers that meet at __syncthreads(): both kernels stage their run through LDS).  A stand-alone program: no GPU, no
// HIP runtime.
//
// Both kernels are driven through their launchers, level by level, with arguments built as DwtPlanner::dev builds them: aligned
// and one element off, for batches of 1 and 3 (whole, and in chunks of one signal), on heap blocks of exactly the contract's
// elements (one element too far is an AddressSanitizer report), in both fiber orders.  Taps, samples and coefficients are
// m 2^-e with small integers m (never 0) and e in 0 .. 40: the products are exact, the sums round, so their bits depend on the
// order -- compared bit for bit with the documented one, written here from the definitions with an extension map of this
// file's own:
//     analysis   acc = fma(dec[j], ext(x, 2i + 1 - j), acc), j = 0 .. F - 1 ascending from 0, one chain per band
//     synthesis  k' ascending (tap t = r + s - 2k' descending); per tap acc = fma(rec_lo[t], cA, acc), acc = fma(rec_hi[t], cD, acc)
// Outputs and the workspace start as a NaN bit pattern: an element the contract names must have lost it, every other one must
// have kept it.  The waverec side runs on random coefficients, not on the analysis' own.
#include <hip/hip_runtime.h>

#include "block_shim.hpp"

#include <cmath>
// any_len.hpp's chirp() (on dwt.hpp's include path, never called by these kernels) names the device's sincospi: a host overload
// so that the header compiles here
inline void sincospi(double t, double *s, double *c) {
    *s = std::sin(3.141592653589793238462643383279502884 * t);
    *c = std::cos(3.141592653589793238462643383279502884 * t);
}

#include "dwt.hip"

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
using i64 = long long;

template <typename T> struct Fp;
template <> struct Fp<double> {
    using bits = unsigned long long;
    static constexpr bits sentinel = 0x7ff8dead5eed0001ull;  // a quiet NaN no kernel produces
    static const char *name() { return "f64"; }
};
template <> struct Fp<float> {
    using bits = unsigned;
    static constexpr bits sentinel = 0x7fc5eed1u;
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

const char *mode_name(int mode) {
    static const char *names[] = {"zero", "constant", "symmetric", "reflect", "periodic", "periodization"};
    return names[mode];
}
i64 floor_mod(i64 a, i64 b) {
    const i64 r = a % b;
    return r < 0 ? r + b : r;
}
// this file's own extension map, from the definitions: the index of ext(x, t), -1 for a zero
i64 ref_ext(int mode, i64 n, i64 t) {
    switch (mode) {
    case kDwtZero: return t >= 0 && t < n ? t : -1;
    case kDwtConstant: return t < 0 ? 0 : t >= n ? n - 1 : t;
    case kDwtPeriodic: return floor_mod(t, n);
    case kDwtSymmetric: {
        const i64 u = floor_mod(t, 2 * n);
        return u < n ? u : 2 * n - 1 - u;
    }
    case kDwtReflect: {
        if (n == 1) return 0;
        const i64 u = floor_mod(t, 2 * n - 2);
        return u < n ? u : 2 * n - 2 - u;
    }
    default: {  // periodization: x[n] := x[n - 1] for odd n
        const i64 u = floor_mod(t, n + n % 2);
        return u < n ? u : n - 1;
    }
    }
}

template <typename T> struct Bank {
    std::vector<T> dec_lo, dec_hi, rec_lo, rec_hi;
    Buf<T> table;  // DwtPlanner::init
    Bank(size_t f, u64 seed) : dec_lo(f), dec_hi(f), rec_lo(f), rec_hi(f), table(4 * f) {
        for (size_t j = 0; j < f; ++j) {
            dec_lo[j] = wide<T>(seed, j);
            dec_hi[j] = wide<T>(seed + 2, j);
            rec_lo[j] = wide<T>(seed + 4, j);
            rec_hi[j] = wide<T>(seed + 6, j);
        }
        const size_t h = f / 2;
        for (size_t p = 0; p < h; ++p) {
            table.p[4 * p + 0] = dec_lo[2 * p];
            table.p[4 * p + 1] = dec_hi[2 * p];
            table.p[4 * p + 2] = dec_lo[2 * p + 1];
            table.p[4 * p + 3] = dec_hi[2 * p + 1];
        }
        for (size_t i = 0; i < h; ++i) {
            const size_t d = h - 1 - i;
            table.p[2 * f + 4 * i + 0] = rec_lo[2 * d];
            table.p[2 * f + 4 * i + 1] = rec_hi[2 * d];
            table.p[2 * f + 4 * i + 2] = rec_lo[2 * d + 1];
            table.p[2 * f + 4 * i + 3] = rec_hi[2 * d + 1];
        }
    }
};

// one analysis level in the documented order
template <typename T> void ref_analysis(const std::vector<T> &x, const Bank<T> &bk, int mode, std::vector<T> &ca, std::vector<T> &cd) {
    const i64 n = (i64)x.size(), f = (i64)bk.dec_lo.size();
    const i64 m = mode == kDwtPeriodization ? (n + n % 2) / 2 : (n + f - 1) / 2, shift = mode == kDwtPeriodization ? f / 2 : 1;
    ca.assign((size_t)m, T(0));
    cd.assign((size_t)m, T(0));
    for (i64 i = 0; i < m; ++i) {
        T lo = T(0), hi = T(0);
        for (i64 j = 0; j < f; ++j) {
            const i64 s = ref_ext(mode, n, 2 * i + shift - j);
            const T v = s >= 0 ? x[(size_t)s] : T(0);
            lo = std::fma(bk.dec_lo[(size_t)j], v, lo);
            hi = std::fma(bk.dec_hi[(size_t)j], v, hi);
        }
        ca[(size_t)i] = lo;
        cd[(size_t)i] = hi;
    }
}
// one synthesis level in the documented order, the first `keep` samples
template <typename T>
void ref_synthesis(const std::vector<T> &ca, const std::vector<T> &cd, const Bank<T> &bk, int mode, size_t keep, std::vector<T> &y) {
    const i64 m = (i64)ca.size(), f = (i64)bk.rec_lo.size(), s = mode == kDwtPeriodization ? f / 2 - 1 : f - 2;
    y.assign(keep, T(0));
    for (i64 r = 0; r < (i64)keep; ++r) {
        T acc = T(0);
        // t = r + s - 2k' in [0, F): k' from ceil((r + s - F + 1) / 2) up to floor((r + s) / 2), ascending
        i64 k_lo = r + s - f + 1;
        k_lo = k_lo >= 0 ? (k_lo + 1) / 2 : -((-k_lo) / 2);
        const i64 k_hi = (r + s) / 2;  // r + s >= 0
        for (i64 k = k_lo; k <= k_hi; ++k) {
            const i64 t = r + s - 2 * k;
            i64 idx = k;
            if (mode == kDwtPeriodization) idx = floor_mod(k, m);
            else if (k < 0 || k >= m) continue;
            acc = std::fma(bk.rec_lo[(size_t)t], ca[(size_t)idx], acc);
            acc = std::fma(bk.rec_hi[(size_t)t], cd[(size_t)idx], acc);
        }
        y[(size_t)r] = acc;
    }
}

struct Shape {
    size_t len, f, levels;
};

// DwtPlanner::dev for one direction; the chunks are `chunk` signals
template <typename T>
void run_dev(bool inverse, const DwtGeom &g, const Shape &s, int mode, const Bank<T> &bk, T *sig, T *coeffs, size_t batch, size_t sd,
             size_t cdist, T *work, size_t chunk) {
    for (size_t b0 = 0; b0 < batch; b0 += chunk) {
        const size_t c = batch - b0 < chunk ? batch - b0 : chunk;
        T *x = sig + b0 * sd, *packed = coeffs + b0 * cdist;
        auto row = [&](size_t l, size_t *dist) {
            *dist = (size_t)(l % 2 ? g.row_a : g.row_b);
            return l % 2 ? work : work + c * (size_t)g.row_a;
        };
        for (size_t step = 1; step <= s.levels; ++step) {
            const size_t l = inverse ? s.levels + 1 - step : step;
            size_t fine_dist = sd, coarse_dist = cdist;
            T *fine = l == 1 ? x : row(l - 1, &fine_dist);
            T *coarse = l == s.levels ? packed : row(l, &coarse_dist);
            DwtArgs a{};
            a.taps = bk.table.p;
            a.f = (unsigned)s.f;
            a.mode = mode;
            if (!inverse) {
                a.in_lo = fine;
                a.in_lo_dist = fine_dist;
                a.out_lo = coarse;
                a.out_lo_dist = coarse_dist;
                a.out_hi = packed + g.off[l];
                a.out_hi_dist = cdist;
                a.n_in = g.n[l - 1];
                a.n_out = a.items = g.n[l];
            } else {
                a.in_lo = coarse;
                a.in_lo_dist = coarse_dist;
                a.in_hi = packed + g.off[l];
                a.in_hi_dist = cdist;
                a.out_lo = fine;
                a.out_lo_dist = fine_dist;
                a.n_in = g.n[l];
                a.n_out = g.n[l - 1];
                dwt_synth_pairs(a.n_out, a.f, mode, &a.q_first, &a.items);
            }
            a.tiles = (a.items + g.tile - 1) / g.tile;
            a.groups = c * a.tiles * 256;
            const hipError_t e = inverse ? launch_dwt_synthesis<T>(a, nullptr) : launch_dwt_analysis<T>(a, nullptr);
            if (e != hipSuccess) fail(inverse ? "synthesis" : "analysis", "the launcher failed");
        }
    }
}

template <typename T> void run_case(const Shape &s, int mode, size_t batch, bool chunked, size_t off) {
    set_case("%s L=%zu F=%zu J=%zu %s batch=%zu %s off=%zu", Fp<T>::name(), s.len, s.f, s.levels, mode_name(mode), batch,
             chunked ? "chunks of 1" : "whole", off);
    if (dwt_bad_args(s.len, s.f, s.levels, mode)) {
        fail("analysis", "the shape is refused");
        return;
    }
    const DwtGeom g = dwt_geom(s.len, (unsigned)s.f, (unsigned)s.levels, mode);
    const Bank<T> bk(s.f, 11 * s.f + s.len);
    const size_t nc = (size_t)g.coeff_len, per = (size_t)(g.row_a + g.row_b), chunk = chunked ? 1 : batch;
    const size_t sd = batch == 1 ? s.len : s.len + 3, cdist = batch == 1 ? nc : nc + 5;
    for (int inverse = 0; inverse < 2; ++inverse) {
        const char *kernel = inverse ? "synthesis" : "analysis";
        // the input: signals, or random coefficients
        Buf<T> sig((batch - 1) * sd + s.len, off), co((batch - 1) * cdist + nc, off);
        Buf<T> &in = inverse ? co : sig;
        const size_t in_len = inverse ? nc : s.len, in_dist = inverse ? cdist : sd;
        for (size_t b = 0; b < batch; ++b)
            for (size_t j = 0; j < in_len; ++j) in.p[b * in_dist + j] = wide<T>(7 * s.len + 13 * inverse + b, j);
        const std::vector<T> in0(in.base, in.base + in.n + in.off);
        // the reference cascade of every signal
        std::vector<std::vector<T>> want(batch);
        for (size_t b = 0; b < batch; ++b) {
            if (!inverse) {
                std::vector<T> a(sig.p + b * sd, sig.p + b * sd + s.len), ca, cd;
                want[b].assign(nc, T(0));
                for (size_t l = 1; l <= s.levels; ++l) {
                    ref_analysis(a, bk, mode, ca, cd);
                    if (ca.size() != g.n[l]) fail(kernel, "level %zu has %zu coefficients by the definition, %llu by dwt_geom", l, ca.size(), g.n[l]);
                    std::copy(cd.begin(), cd.end(), want[b].begin() + (size_t)g.off[l]);
                    a = ca;
                }
                std::copy(a.begin(), a.end(), want[b].begin());
            } else {
                const T *row = co.p + b * cdist;
                std::vector<T> a(row, row + g.n[s.levels]), y;
                for (size_t l = s.levels; l >= 1; --l) {
                    const std::vector<T> d(row + g.off[l], row + g.off[l] + g.n[l]);
                    ref_synthesis(a, d, bk, mode, (size_t)g.n[l - 1], y);
                    a = y;
                }
                want[b] = a;
            }
        }
        const size_t out_len = inverse ? s.len : nc, out_dist = inverse ? sd : cdist;
        for (int order = 0; order < 2; ++order) {
            block_shim::order = order ? block_shim::kDescending : block_shim::kAscending;
            Buf<T> out_buf((batch - 1) * out_dist + out_len, off), work(chunk * per, off);
            T *sig_p = inverse ? out_buf.p : sig.p, *co_p = inverse ? co.p : out_buf.p;
            run_dev<T>(inverse != 0, g, s, mode, bk, sig_p, co_p, batch, sd, cdist, work.p, chunk);
            for (size_t b = 0; b < batch; ++b) {
                for (size_t i = 0; i < out_len; ++i) {
                    ++g_compared;
                    const T got = out_buf.p[b * out_dist + i], ref = want[b][i];
                    if (!same_bits(got, ref))
                        fail(kernel, "element %zu of signal %zu = %.17Lg, must be exactly %.17Lg (thread order %d)", i, b, (ld)got, (ld)ref, order);
                }
                if (b + 1 < batch)
                    for (size_t i = out_len; i < out_dist; ++i)
                        if (!out_buf.is_sentinel((long long)(b * out_dist + i))) fail(kernel, "element %zu of output row %zu was written", i, b);
            }
            for (size_t e = 1; e <= off; ++e)
                if (!out_buf.is_sentinel(-(long long)e) || !work.is_sentinel(-(long long)e)) fail(kernel, "an element in front of a buffer was written");
        }
        block_shim::order = block_shim::kAscending;
        if (std::memcmp(in0.data(), in.base, in0.size() * sizeof(T))) fail(kernel, "the input was written");
    }
}

}  // namespace

int main() {
    // tests/test_gpu_dwt.py's cases (the long ones shorter), and first levels of tile - 1, tile, tile + 1 and 2 tile + 3
    // coefficients with F = 6: n_1 = (L + 5) div 2
    const Shape shapes[] = {{1, 2, 1},  {2, 2, 1},    {3, 4, 1},    {5, 8, 1},    {17, 4, 3},   {9, 4, 4},  {40, 6, 2},  {1, 8, 3},
                            {2041, 6, 1}, {2043, 6, 2}, {2045, 6, 1}, {4097, 6, 3}, {4100, 20, 5}, {300, 256, 2}, {2100, 2, 2}};
    for (const Shape &s : shapes)
        for (int mode = 0; mode < kDwtModes; ++mode)
            for (size_t batch = 1; batch <= 3; batch += 2)
                for (int chunked = 0; chunked < (batch > 1 && s.levels > 1 ? 2 : 1); ++chunked) {
                    const size_t off = (batch + chunked + (size_t)mode) % 2;  // both alignments for every shape, not for every combination
                    if (s.len > 1000 && batch == 3 && chunked) continue;
                    run_case<double>(s, mode, batch, chunked != 0, off);
                    run_case<float>(s, mode, batch, chunked != 0, 1 - off);
                }
    std::printf("dwt: ");
    block_shim::print_counters();
    std::printf("dwt: elements %llu checked\n", g_compared);
    std::printf("dwt: %s (%d failures)\n", g_fails ? "FAILED" : "ok", g_fails);
    phast_test_exit(g_fails ? 1 : 0);
}
