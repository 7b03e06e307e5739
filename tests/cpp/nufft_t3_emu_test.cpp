// nufft_t3_emu_test.cpp -- the two kernels of the type-3 non-uniform FFT (csrc/nufft_t3.hip), run on the host under
// AddressSanitizer and UndefinedBehaviorSanitizer (tests/test_nufft_t3_emulator.py builds and runs it; tests/emu/sweep_shim.hpp
// turns a launch into a serial loop).  One translation unit with its own main, linked without the HIP runtime.  nufft_t3.hip is
// #included as it stands and both kernels are driven through launch_nufft_t3 with arguments built as planner_nufft_t3.hpp
// builds them, from tables made by nufft_t3.hpp's own builders and nufft_bin.
//
// Buffers: every plane, table and workspace is a heap allocation of exactly the bytes the contract covers; an "unaligned"
// buffer is one element longer and used from element 1.  The workspace starts as a NaN sentinel, and so do the gaps between the
// rows of the caller's output planes: an element the contract names must have lost it, every other element must have kept it.
//
// Every element is compared with a long double statement of its stage, written here a second time:
//     spread   w[s] = p[m] sum_i phi(2 (l - n_f xs_i) / w) c[perm_i] (pre_c[i] -+ i pre_s[i]) in the slot s of mode
//              k = l - n_f / 2 (m its fftfreq index), exactly 0 in every other slot of the n_g = 2 n_f
//     post     f[k] = f[k] (D_re[k] +- i D_im[k]), in place, k < K
// The gates are those of tests/cpp/nufft_emu_test.cpp: a kernel value within (100 + 2 beta) u_R of phi, e^{-beta} more for a
// term on the edge of the support, n + 2 roundings for a sum of n terms; here each term carries a complex product (3 more
// roundings) and the sum one more product.  post is one complex product: 4 u_T of the sum of its terms' magnitudes.
#include <hip/hip_runtime.h>

#include "sweep_shim.hpp"

#include "nufft_t3.hip"

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
double g_worst[2] = {0, 0};
const char *const kKernel[2] = {"nufft_t3_spread_kernel", "nufft_t3_post_kernel"};
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

// the plan of a case, built as NufftT3Planner::init builds it: centres off zero, both ends of each range taken, a clump of
// sources inside one cell among uniform ones
template <typename T> struct Tables {
    size_t m, k;
    std::vector<double> x, s;   // before g: plan() fills them
    NufftT3Grid g;
    std::vector<double> t;
    Buf<double> xs;
    Buf<uint32_t> perm, cell;
    Buf<T> pre, inv, dre, dim;
    static NufftT3Grid plan(size_t m, size_t k, double X, double S, int w, std::vector<double> &x, std::vector<double> &s) {
        x.resize(m);
        s.resize(k);
        for (size_t j = 0; j < m; ++j) x[j] = 10.0 + X * (j == 0 ? -1.0 : j == 1 ? 1.0 : j % 3 ? 0.3 + 1e-3 * (double)rnd(7, j) : (double)rnd(9, j));
        for (size_t j = 0; j < k; ++j) s[j] = -7.0 + S * (j == 0 ? 1.0 : j == 1 ? -1.0 : (double)rnd(5, j));
        double eps = 1;
        for (int i = 1; i < w; ++i) eps /= 10;   // w = ceil(log10(1 / eps)) + 1
        return nufft_t3_grid(x.data(), m, s.data(), k, eps);
    }
    Tables(size_t m_, size_t k_, double X, double S, int w)
        : m(m_), k(k_), g(plan(m_, k_, X, S, w, x, s)), t(k_), xs(m_), perm(m_), cell((size_t)g.nf + 1), pre(2 * m_), inv((size_t)g.nf),
          dre(k_), dim(k_) {
        if (g.w != w || g.nf == 0) std::abort();
        std::vector<double> u(m);
        nufft_t3_positions(g, x.data(), m, u.data());
        nufft_t3_targets(g, s.data(), k, t.data());
        nufft_bin(u.data(), m, g.log_f, xs.p, perm.p, cell.p);
        nufft_t3_pre_table<T>(g, x.data(), perm.p, m, pre.p);
        nufft_t3_post_table<T>(g, s.data(), t.data(), k, dre.p, dim.p);
        for (size_t i = 0; i < inv.n; ++i) inv[i] = (T)(1.5L + 0.5L * rnd(3, i));
    }
};

ld phi_ld(ld z, ld beta) { return z * z < 1 ? expl(beta * (sqrtl(1 - z * z) - 1)) : 0; }

template <typename T> void compare(int kind, const char *what, size_t idx, const T *got, ld want, ld gate) {
    ++g_compared;
    if (is_sentinel(got)) return fail(kind, "%s[%zu] was not written", what, idx);
    const ld err = fabsl((ld)*got - want);
    if (gate > 0 && (double)(err / gate) > g_worst[kind]) g_worst[kind] = (double)(err / gate);
    if (!(err <= gate)) fail(kind, "%s[%zu] = %.17Lg, want %.17Lg: error %.3Lg > gate %.3Lg", what, idx, (ld)*got, want, err, gate);
}

template <typename T> NufftT3Args args_of(Tables<T> &t, bool reverse) {
    NufftT3Args a{};
    a.xs = t.xs.p;
    a.perm = t.perm.p;
    a.cell_start = t.cell.p;
    a.pre = t.pre.p;
    a.inv_hat = t.inv.p;
    a.d_re = t.dre.p;
    a.d_im = t.dim.p;
    a.k = t.k;
    a.log_f = t.g.log_f;
    a.w = t.g.w;
    a.reverse = reverse;
    return a;
}
bool al(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// one (batch, alignment, data, direction) case: both kernels, each on its own buffers
template <typename T> void run_case(Tables<T> &t, size_t batch, size_t plane_off, size_t wk_off, bool real, bool reverse) {
    constexpr size_t V = Fp<T>::V;
    const ld u = Fp<T>::u, beta = 2.30L * t.g.w, jump = expl(-beta), sg = reverse ? 1 : -1;
    const size_t nf = (size_t)t.g.nf, ng = 2 * nf, m = t.m, k = t.k;
    const size_t pd = batch > 1 ? m + 3 : m;  // distances above the row: gaps are never read
    // post: rows a multiple of the 16-byte group apart where the planes are aligned (the 16-byte variant with a tail), odd otherwise
    const size_t od = batch > 1 ? (plane_off ? k + 5 : (k + V - 1) / V * V + V) : k;
    std::snprintf(g_case, sizeof g_case, "%s M=%zu K=%zu w=%d n_f=%zu batch=%zu planes+%zu work+%zu%s%s", Fp<T>::name(), m, k, t.g.w, nf,
                  batch, plane_off, wk_off, real ? " real" : "", reverse ? " reverse" : "");
    auto term_gate = [&](ld z, ld value) {  // what one kernel value may be off by, times |value|
        ld g = (100 + 2 * beta) * u * fabsl(value);
        if (fabsl(1 - z * z) < 8 * u) g += jump * (1 + beta) * fabsl(value);
        return g;
    };
    // ---- spread: caller's source planes -> workspace
    {
        Buf<T> cr((batch - 1) * pd + m, plane_off), ci(real ? 0 : (batch - 1) * pd + m, plane_off), wk(2 * batch * ng, wk_off);
        fill_random(cr, 11);
        fill_random(ci, 12);
        fill_sentinel(wk);
        NufftT3Args a = args_of<T>(t, reverse);
        a.in_re = cr.p;
        a.in_im = real ? nullptr : ci.p;
        a.out_re = wk.p;
        a.out_im = wk.p + batch * ng;
        a.in_dist = pd;
        a.groups = batch * ng;
        if (launch_nufft_t3<T>(0, false, a, nullptr) != hipSuccess) fail(0, "the launcher failed");
        for (size_t b = 0; b < batch; ++b)
            for (size_t s = 0; s < ng; ++s) {
                const T *gr = wk.p + b * ng + s, *gi = wk.p + (batch + b) * ng + s;
                const bool low = s < nf / 2, high = s >= ng - nf / 2;
                if (!low && !high) {
                    ++g_compared;
                    if (is_sentinel(gr) || is_sentinel(gi) || !(*gr == 0 && *gi == 0))
                        fail(0, "workspace[%zu] = (%g, %g) must be exactly 0", b * ng + s, (double)*gr, (double)*gi);
                    continue;
                }
                const size_t l = low ? s + nf / 2 : s - (ng - nf / 2), mode = low ? s : s - nf;
                ld sr = 0, si = 0, gate_r = 0, gate_i = 0;
                size_t terms = 0;
                for (size_t i = 0; i < m; ++i) {
                    const ld z = 2 * ((ld)l - (ld)t.xs.p[i] * (ld)nf) / t.g.w, kv = phi_ld(z, beta);
                    if (!(fabsl(z) < 1 + 16 * u)) continue;
                    const ld vr = cr[b * pd + t.perm.p[i]], vi = real ? 0 : (ld)ci[b * pd + t.perm.p[i]];
                    const ld pc = t.pre.p[2 * i], ps = sg * (ld)t.pre.p[2 * i + 1];
                    const ld tr = vr * pc - vi * ps, ti = vi * pc + vr * ps, mag = fabsl(vr) + fabsl(vi);
                    sr += kv * tr;
                    si += kv * ti;
                    gate_r += term_gate(z, mag) + 5 * u * kv * mag;
                    gate_i += term_gate(z, mag) + 5 * u * kv * mag;
                    ++terms;
                }
                const ld p = t.inv.p[mode];
                compare(0, "w.re", b * ng + s, gr, p * sr, fabsl(p) * (gate_r * (1 + terms * u) + (terms + 3) * u * fabsl(sr)));
                compare(0, "w.im", b * ng + s, gi, p * si, fabsl(p) * (gate_i * (1 + terms * u) + (terms + 3) * u * fabsl(si)));
            }
    }
    // ---- post: the caller's target planes, in place
    if (!real) {
        Buf<T> orr((batch - 1) * od + k, plane_off), oi((batch - 1) * od + k, plane_off);
        fill_sentinel(orr);
        fill_sentinel(oi);
        std::vector<ld> vr(batch * k), vi(batch * k);
        for (size_t b = 0; b < batch; ++b)
            for (size_t i = 0; i < k; ++i) {
                orr[b * od + i] = (T)rnd(21, b * k + i);
                oi[b * od + i] = (T)rnd(22, b * k + i);
                vr[b * k + i] = orr[b * od + i];
                vi[b * k + i] = oi[b * od + i];
            }
        NufftT3Args a = args_of<T>(t, reverse);
        a.out_re = orr.p;
        a.out_im = oi.p;
        a.out_dist = od;
        a.gpt = (unsigned)((k + V - 1) / V);
        a.groups = batch * a.gpt;
        const bool vec = al(orr.p) && al(oi.p) && od % V == 0;
        if (launch_nufft_t3<T>(1, vec, a, nullptr) != hipSuccess) fail(1, "the launcher failed");
        for (size_t b = 0; b < batch; ++b)
            for (size_t i = 0; i < k; ++i) {
                const ld dr = t.dre.p[i], di = -sg * (ld)t.dim.p[i];   // Forward as stored, Reverse conjugated
                const ld xr = vr[b * k + i], xi = vi[b * k + i];
                const ld mag = (fabsl(xr) + fabsl(xi)) * (fabsl(dr) + fabsl(di));
                compare(1, "f.re", b * od + i, orr.p + b * od + i, xr * dr - xi * di, 4 * u * mag);
                compare(1, "f.im", b * od + i, oi.p + b * od + i, xr * di + xi * dr, 4 * u * mag);
            }
        for (size_t b = 0; b + 1 < batch; ++b)
            for (size_t o = b * od + k; o < (b + 1) * od; ++o)
                if (!(is_sentinel(orr.p + o) && is_sentinel(oi.p + o))) fail(1, "out[%zu] lies between two rows and was written", o);
    }
}

template <typename T> void run_all() {
    // (M, K, w) and half-widths that keep the grids small: n_f = 16, 32, 64, 256, 256
    const struct {
        size_t m, k;
        int w;
        double X, S;
    } shapes[] = {{1, 1, 2, 1, 1}, {5, 3, 3, 0.7, 3}, {40, 7, 16, 1, 2}, {300, 64, 4, 2, 8}, {1000, 257, 13, 0.5, 30}};
    for (const auto &s : shapes) {
        Tables<T> t(s.m, s.k, s.X, s.S, s.w);
        for (size_t batch : {(size_t)1, (size_t)3})
            for (bool reverse : {false, true}) {
                run_case<T>(t, batch, 0, 0, false, reverse);
                run_case<T>(t, batch, 1, 0, false, reverse);  // caller planes at element alignment (buf[1:])
                run_case<T>(t, batch, 0, 1, false, reverse);  // the workspace at element alignment
                run_case<T>(t, batch, 0, 0, true, reverse);   // no imaginary input plane
                run_case<T>(t, batch, 1, 1, true, reverse);
            }
    }
}

}  // namespace

int main() {
    run_all<double>();
    run_all<float>();
    for (int k = 0; k < 2; ++k) std::printf("  %-24s worst error / gate %.3f\n", kKernel[k], g_worst[k]);
    std::printf("launches %llu threads %llu elements %llu\n", sweep_shim::launches, sweep_shim::threads_run, g_compared);
    std::printf("nufft_t3: %s (%d failures)\n", g_fails ? "FAILED" : "ok", g_fails);
    phast_test_exit(g_fails ? 1 : 0);
}
