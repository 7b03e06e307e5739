// nufft_emu_test.cpp -- the four kernels of the non-uniform FFT (csrc/nufft.hip), run on the host under AddressSanitizer and
// UndefinedBehaviorSanitizer: the first kernels of the tree that index through tables (tests/test_nufft_emulator.py builds and
// runs it; tests/emu/sweep_shim.hpp turns a launch into a serial loop).  One translation unit with its own main, linked
// without the HIP runtime.  nufft.hip is #included as it stands and every kernel is driven through launch_nufft with
// arguments built as planner_nufft.hpp builds them, from tables made by nufft.hpp's own nufft_bin.
//
// Buffers: every plane, table and workspace is a heap allocation of exactly the bytes the contract covers; an "unaligned"
// buffer is one element longer and used from element 1.  Workspaces written by a kernel start as NaN, caller outputs as a
// NaN sentinel: an element the contract names must have lost it, every other element must have kept its exact bits.
//
// Every element is compared with a long double statement of its stage, written here a second time:
//     spread       g[l]  = sum_j phi(2 d(l, p_j) / w) c_j,  d the signed distance round the ring of n_g cells, p_j = n_g x_j
//     interpolate  c_j   = sum_l phi(2 d(l, p_j) / w) g[l]
//     pre          g^[s] = F[m] p[m] at s = slot(m), exactly 0 in every other slot
//     deconvolve   F[m]  = g^[slot(m)] p[m]
// The gate is derived: pre and deconvolve are one product rounded to T, 3 u_T |product|.  A kernel value phi is formed from z^2
// rounded to R (T's arithmetic): with s = sqrt(1 - z^2), |d phi| <= phi beta u_R / (2 s) + 4 u_R phi, and s >= sqrt(u_R) wherever
// z^2 < 1 in R, so |d phi| <= (beta e^{-beta (1 - s)} / (2 s) + 4) u_R <= (beta 2^11 e^{-beta} + beta + 4) u_R at worst, which is
// below (100 + 2 beta) u_R for every w >= 2.  A sum of n terms adds n + 2 roundings.  phi jumps from e^{-beta} to 0 at |z| = 1,
// so a term within 8 u_R of the edge may fall on either side: it is allowed e^{-beta} |value| more.
#include <hip/hip_runtime.h>

#include "sweep_shim.hpp"

#include "nufft.hip"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sanitizer_exit.hpp"

namespace {

using ld = long double;
using namespace phast;

template <typename T> struct Fp;
template <> struct Fp<double> {
    static constexpr ld u = 0x1p-53L;
    static constexpr unsigned long long sentinel = 0x7ff8dead5eed0001ull;
    static constexpr size_t V = 2;
    static const char *name() { return "f64"; }
};
template <> struct Fp<float> {
    static constexpr ld u = 0x1p-24L;
    static constexpr unsigned sentinel = 0x7fc5eed1u;
    static constexpr size_t V = 4;
    static const char *name() { return "f32"; }
};

int g_fails = 0;
unsigned long long g_compared = 0;
double g_worst[4] = {0, 0, 0, 0};
const char *const kKernel[4] = {"nufft_spread_kernel", "nufft_interp_kernel", "nufft_pre_kernel", "nufft_deconv_kernel"};
char g_case[256] = "";

void fail(int kind, const char *fmt, ...) {
    if (++g_fails > 12) return;
    std::printf("FAIL %s [%s]: ", kKernel[kind], g_case);
    va_list ap;
    va_start(ap, fmt);
    std::vprintf(fmt, ap);
    va_end(ap);
    std::printf("\n");
}

ld rnd(unsigned long long seed, unsigned long long i) {  // uniform in [-1, 1), exact in float
    unsigned long long x = seed * 0x9E3779B97F4A7C15ull + i * 0xD1B54A32D192ED03ull + 0x2545F4914F6CDD1Dull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    x ^= x >> 31;
    return (ld)(long long)(x >> 43) * 0x1p-20L - 1.0L;
}

// exactly n elements of E behind `off` elements of lead-in
template <typename E> struct Buf {
    E *base = nullptr, *p = nullptr;
    size_t n;
    explicit Buf(size_t n_, size_t off = 0) : n(n_) {
        void *q = nullptr;
        const size_t bytes = (n + off) * sizeof(E);
        if (posix_memalign(&q, 16, bytes ? bytes : 1)) std::abort();
        base = (E *)q;
        p = base + off;
        std::memset(base, 0xA5, bytes);
    }
    ~Buf() { std::free(base); }
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    E &operator[](size_t i) { return p[i]; }
};
template <typename T> void fill_sentinel(Buf<T> &b) {
    for (size_t i = 0; i < b.n; ++i) std::memcpy(b.p + i, &Fp<T>::sentinel, sizeof(T));
}
template <typename T> bool is_sentinel(const T *p) { return !std::memcmp(p, &Fp<T>::sentinel, sizeof(T)); }
template <typename T> void fill_random(Buf<T> &b, unsigned long long seed) {
    for (size_t i = 0; i < b.n; ++i) b.p[i] = (T)rnd(seed, i);
}

// the points of the binning test (tests/test_nufft_cpu.py): the specials first -- the support wraps both ends of the grid --
// then a clump inside one cell among uniform points
std::vector<double> make_points(size_t m, size_t grid) {
    const double specials[] = {0.0, 1 - 0x1p-53, -0.25, 7.5, 1e-300};
    std::vector<double> x(m);
    for (size_t j = 0; j < m; ++j) {
        if (j < 5)
            x[j] = specials[j];
        else if (j % 3)
            x[j] = (0.7 * (double)grid + 0.5 + 0.25 * (double)rnd(7, j)) / (double)grid - 3.0;  // one cell, a turn away
        else
            x[j] = 2.0 * (double)rnd(9, j);
    }
    return x;
}

struct Tables {
    size_t n, m, grid;
    unsigned log_g;
    int w;
    Buf<double> xs;
    Buf<uint32_t> perm, cell;
    Tables(size_t n_, size_t m_, int w_)
        : n(n_), m(m_), grid((size_t)nufft_grid(n_, w_)), log_g(0), w(w_), xs(m_), perm(m_), cell(grid + 1) {
        while (((size_t)1 << log_g) < grid) ++log_g;
        const std::vector<double> x = make_points(m, grid);
        nufft_bin(x.data(), m, log_g, xs.p, perm.p, cell.p);
    }
};

ld phi_ld(ld z, ld beta) { return z * z < 1 ? expl(beta * (sqrtl(1 - z * z) - 1)) : 0; }
// the signed distance from sorted point i to grid point l round the ring
ld ring(const Tables &t, size_t l, size_t i) {
    ld d = (ld)l - (ld)t.xs.p[i] * (ld)t.grid;
    if (d >= (ld)t.grid / 2) d -= (ld)t.grid;
    if (d < -(ld)t.grid / 2) d += (ld)t.grid;
    return d;
}

template <typename T> void compare(int kind, const char *what, size_t idx, const T *got, ld want, ld gate) {
    ++g_compared;
    if (is_sentinel(got)) return fail(kind, "%s[%zu] was not written", what, idx);
    const ld err = fabsl((ld)*got - want);
    if (gate > 0 && (double)(err / gate) > g_worst[kind]) g_worst[kind] = (double)(err / gate);
    if (!(err <= gate)) fail(kind, "%s[%zu] = %.17Lg, want %.17Lg: error %.3Lg > gate %.3Lg", what, idx, (ld)*got, want, err, gate);
}

template <typename T> NufftArgs args_of(const Tables &t, const T *inv) {
    NufftArgs a{};
    a.xs = t.xs.p;
    a.perm = t.perm.p;
    a.cell_start = t.cell.p;
    a.inv_hat = inv;
    a.n = t.n;
    a.m = t.m;
    a.log_g = t.log_g;
    a.w = t.w;
    return a;
}
bool al(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// one (type, batch, alignment) case: both kernels of the type, each on its own buffers
template <typename T> void run_case(const Tables &t, size_t batch, size_t plane_off, size_t wk_off, bool real) {
    constexpr size_t V = Fp<T>::V;
    const ld u = Fp<T>::u, beta = 2.30L * t.w, jump = expl(-beta);
    const size_t grid = t.grid, n = t.n, m = t.m;
    const size_t pd = batch > 1 ? m + 3 : m, fd = batch > 1 ? n + 5 : n;  // distances above the row: gaps keep their sentinel
    Buf<T> inv(n);
    for (size_t i = 0; i < n; ++i) inv[i] = (T)(1.5L + 0.5L * rnd(3, i));
    std::snprintf(g_case, sizeof g_case, "%s N=%zu M=%zu w=%d n_g=%zu batch=%zu planes+%zu work+%zu%s", Fp<T>::name(), n, m, t.w,
                  grid, batch, plane_off, wk_off, real ? " real" : "");
    auto term_gate = [&](ld z, ld value) {  // what one kernel value may be off by, times |value|
        ld g = (100 + 2 * beta) * u * fabsl(value);
        if (fabsl(1 - z * z) < 8 * u) g += jump * (1 + beta) * fabsl(value);
        return g;
    };
    // ---- spread: caller's point planes -> workspace
    {
        Buf<T> cr((batch - 1) * pd + m, plane_off), ci(real ? 0 : (batch - 1) * pd + m, plane_off), wk(2 * batch * grid, wk_off);
        fill_random(cr, 11);
        fill_random(ci, 12);
        fill_sentinel(wk);
        NufftArgs a = args_of<T>(t, inv.p);
        a.in_re = cr.p;
        a.in_im = real ? nullptr : ci.p;
        a.out_re = wk.p;
        a.out_im = wk.p + batch * grid;
        a.in_dist = pd;
        a.groups = batch * grid;
        if (launch_nufft<T>(0, false, a, nullptr) != hipSuccess) fail(0, "the launcher failed");
        for (size_t b = 0; b < batch; ++b)
            for (size_t l = 0; l < grid; ++l) {
                ld sr = 0, si = 0, gr = 0, gi = 0;
                size_t terms = 0;
                for (size_t i = 0; i < m; ++i) {
                    const ld z = 2 * ring(t, l, i) / t.w, k = phi_ld(z, beta);
                    if (!(fabsl(z) < 1 + 16 * u)) continue;
                    const ld vr = cr[b * pd + t.perm.p[i]], vi = real ? 0 : (ld)ci[b * pd + t.perm.p[i]];
                    sr += k * vr;
                    si += k * vi;
                    gr += term_gate(z, vr) + u * k * fabsl(vr) * 2;
                    gi += term_gate(z, vi) + u * k * fabsl(vi) * 2;
                    ++terms;
                }
                compare(0, "g.re", b * grid + l, wk.p + b * grid + l, sr, gr * (1 + terms * u) + terms * u * fabsl(sr));
                compare(0, "g.im", b * grid + l, wk.p + (batch + b) * grid + l, si, gi * (1 + terms * u) + terms * u * fabsl(si));
            }
    }
    // ---- interpolate: workspace -> caller's point planes
    if (!real) {
        Buf<T> wk(2 * batch * grid, wk_off), orr((batch - 1) * pd + m, plane_off), oi((batch - 1) * pd + m, plane_off);
        fill_random(wk, 21);
        fill_sentinel(orr);
        fill_sentinel(oi);
        NufftArgs a = args_of<T>(t, inv.p);
        a.in_re = wk.p;
        a.in_im = wk.p + batch * grid;
        a.out_re = orr.p;
        a.out_im = oi.p;
        a.out_dist = pd;
        a.groups = batch * m;
        if (launch_nufft<T>(1, false, a, nullptr) != hipSuccess) fail(1, "the launcher failed");
        std::vector<char> named(orr.n, 0);
        for (size_t b = 0; b < batch; ++b)
            for (size_t i = 0; i < m; ++i) {
                ld sr = 0, si = 0, gr = 0, gi = 0;
                size_t terms = 0;
                for (size_t l = 0; l < grid; ++l) {
                    const ld z = 2 * ring(t, l, i) / t.w, k = phi_ld(z, beta);
                    if (!(fabsl(z) < 1 + 16 * u)) continue;
                    const ld vr = wk[b * grid + l], vi = wk[(batch + b) * grid + l];
                    sr += k * vr;
                    si += k * vi;
                    gr += term_gate(z, vr) + u * k * fabsl(vr) * 2;
                    gi += term_gate(z, vi) + u * k * fabsl(vi) * 2;
                    ++terms;
                }
                const size_t o = b * pd + t.perm.p[i];
                named[o] = 1;
                compare(1, "c.re", o, orr.p + o, sr, gr * (1 + terms * u) + terms * u * fabsl(sr));
                compare(1, "c.im", o, oi.p + o, si, gi * (1 + terms * u) + terms * u * fabsl(si));
            }
        for (size_t o = 0; o < orr.n; ++o)
            if (!named[o] && !(is_sentinel(orr.p + o) && is_sentinel(oi.p + o))) fail(1, "out[%zu] lies between two rows and was written", o);
    }
    // ---- pre: caller's mode planes -> workspace
    {
        Buf<T> fr((batch - 1) * fd + n, plane_off), fi(real ? 0 : (batch - 1) * fd + n, plane_off), wk(2 * batch * grid, wk_off);
        fill_random(fr, 31);
        fill_random(fi, 32);
        fill_sentinel(wk);
        NufftArgs a = args_of<T>(t, inv.p);
        a.in_re = fr.p;
        a.in_im = real ? nullptr : fi.p;
        a.out_re = wk.p;
        a.out_im = wk.p + batch * grid;
        a.in_dist = fd;
        a.groups = batch * (grid / V);
        const bool vec = al(fr.p) && (real || al(fi.p)) && al(wk.p) && fd % V == 0;
        if (launch_nufft<T>(2, vec, a, nullptr) != hipSuccess) fail(2, "the launcher failed");
        for (size_t b = 0; b < batch; ++b) {
            std::vector<char> named(grid, 0);
            for (size_t i = 0; i < n; ++i) {
                const size_t s = (size_t)nufft_slot(i, n, grid);
                named[s] = 1;
                const ld wr = (ld)fr[b * fd + i] * (ld)inv[i], wi = real ? 0 : (ld)fi[b * fd + i] * (ld)inv[i];
                compare(2, "g^.re", b * grid + s, wk.p + b * grid + s, wr, 3 * u * fabsl(wr));
                compare(2, "g^.im", b * grid + s, wk.p + (batch + b) * grid + s, wi, 3 * u * fabsl(wi));
            }
            for (size_t s = 0; s < grid; ++s)
                if (!named[s]) {
                    const T zr = wk[b * grid + s], zi = wk[(batch + b) * grid + s];
                    ++g_compared;
                    if (!(zr == 0 && zi == 0)) fail(2, "workspace[%zu] = (%g, %g) must be exactly 0", b * grid + s, (double)zr, (double)zi);
                }
        }
    }
    // ---- deconvolve: workspace -> caller's mode planes
    if (!real) {
        Buf<T> wk(2 * batch * grid, wk_off), orr((batch - 1) * fd + n, plane_off), oi((batch - 1) * fd + n, plane_off);
        fill_random(wk, 41);
        fill_sentinel(orr);
        fill_sentinel(oi);
        NufftArgs a = args_of<T>(t, inv.p);
        a.in_re = wk.p;
        a.in_im = wk.p + batch * grid;
        a.out_re = orr.p;
        a.out_im = oi.p;
        a.out_dist = fd;
        a.gpt = (unsigned)((n + V - 1) / V);
        a.groups = batch * a.gpt;
        const bool vec = al(orr.p) && al(oi.p) && al(wk.p) && fd % V == 0;
        if (launch_nufft<T>(3, vec, a, nullptr) != hipSuccess) fail(3, "the launcher failed");
        for (size_t b = 0; b < batch; ++b)
            for (size_t i = 0; i < n; ++i) {
                const size_t s = (size_t)nufft_slot(i, n, grid);
                const ld wr = (ld)wk[b * grid + s] * (ld)inv[i], wi = (ld)wk[(batch + b) * grid + s] * (ld)inv[i];
                compare(3, "F.re", b * fd + i, orr.p + b * fd + i, wr, 3 * u * fabsl(wr));
                compare(3, "F.im", b * fd + i, oi.p + b * fd + i, wi, 3 * u * fabsl(wi));
            }
        for (size_t b = 0; b + 1 < batch; ++b)
            for (size_t o = b * fd + n; o < (b + 1) * fd; ++o)
                if (!(is_sentinel(orr.p + o) && is_sentinel(oi.p + o))) fail(3, "out[%zu] lies between two rows and was written", o);
    }
}

template <typename T> void run_all() {
    const size_t shapes[][3] = {{1, 1, 2}, {2, 5, 3}, {7, 3, 16}, {16, 100, 4}, {101, 1000, 13}};
    for (const auto &s : shapes) {
        const Tables t(s[0], s[1], (int)s[2]);
        for (size_t batch : {(size_t)1, (size_t)3}) {
            run_case<T>(t, batch, 0, 0, false);
            run_case<T>(t, batch, 1, 0, false);  // caller planes at element alignment (buf[1:])
            run_case<T>(t, batch, 0, 1, false);  // the workspace at element alignment
            run_case<T>(t, batch, 0, 0, true);   // no imaginary input plane
            run_case<T>(t, batch, 1, 0, true);
        }
    }
}

}  // namespace

int main() {
    run_all<double>();
    run_all<float>();
    for (int k = 0; k < 4; ++k) std::printf("  %-22s worst error / gate %.3f\n", kKernel[k], g_worst[k]);
    std::printf("launches %llu threads %llu elements %llu\n", sweep_shim::launches, sweep_shim::threads_run, g_compared);
    std::printf("nufft: %s (%d failures)\n", g_fails ? "FAILED" : "ok", g_fails);
    phast_test_exit(g_fails ? 1 : 0);
}
