// nufft2d_emu_test.cpp -- the four kernels of the two-dimensional non-uniform FFT (csrc/nufft_nd.hip at D = 2), run on the host
// under AddressSanitizer and UndefinedBehaviorSanitizer (tests/test_nufft2d_emulator.py builds and runs it).  The unit also holds
// the tiled spread of three dimensions (__shared__, __syncthreads), so the program stands on tests/emu/block_shim.hpp, where a
// workgroup's threads are fibers, and every case runs in BOTH thread orders, ascending and descending.  One translation unit with
// its own main, linked without the HIP runtime.  nufft_nd.hip is #included as it stands and every kernel is driven through
// launch_nufft_nd<T, 2> with arguments built as planner_nufft_nd.hpp builds them, from tables made by nufft_nd.hpp's own
// nufft_nd_bin.
//
// Buffers: every plane, table and workspace is a heap allocation of exactly the bytes the contract covers; an "unaligned"
// buffer is one element longer and used from element 1.  Workspaces written by a kernel start as NaN, caller outputs as a
// NaN sentinel: an element the contract names must have lost it, every other element must have kept its exact bits.
//
// Every element is compared with a long double statement of its stage, written here a second time (d_i: the signed distance
// round the ring of g_i cells from the point's position g_i x to the grid index):
//     spread       g[l1, l2]  = sum_j phi(2 d1 / w) phi(2 d2 / w) c_j
//     interpolate  c_j        = sum_{l1, l2} phi(2 d1 / w) phi(2 d2 / w) g[l1, l2]
//     pre          g^[s1, s2] = F[m1, m2] p1[m1] p2[m2] at s_i = slot(m_i), exactly 0 in every other slot of the grid
//     deconvolve   F[m1, m2]  = g^[slot(m1), slot(m2)] p1[m1] p2[m2]
// The gate is derived as tests/cpp/nufft_emu_test.cpp derives its own: pre and deconvolve are two products rounded to T,
// 3 u_T |product|.  One kernel value is off by at most e = (100 + 2 beta) u_R (phi <= 1), the product of two by 2 e + u_R; a
// sum of n terms adds n + 2 roundings.  phi jumps from e^{-beta} to 0 at |z| = 1, so a term with either factor within 8 u_R of
// the edge may fall on either side: it is allowed e^{-beta} (1 + beta) |value| more.
#include <hip/hip_runtime.h>

#include "block_shim.hpp"

#include <cmath>
// any_len.hpp's chirp() (on nufft_nd.hip's include path, never called by its kernels) names the device's sincospi: a host
// overload so that the header compiles here
inline void sincospi(double t, double *s, double *c) {
    *s = std::sin(3.141592653589793238462643383279502884 * t);
    *c = std::cos(3.141592653589793238462643383279502884 * t);
}

#include "nufft_nd.hip"

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
const char *const kKernel[4] = {"nufft_nd_spread_kernel", "nufft_nd_interp_kernel", "nufft_nd_pre_kernel", "nufft_nd_deconv_kernel"};
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

// one coordinate of the points: the specials first (x) or last-first (y) -- the support wraps both ends of both axes -- then a
// clump inside one cell, a turn or three away, among uniform points
std::vector<double> make_coordinate(size_t m, size_t grid, int axis) {
    const double specials[] = {0.0, 1 - 0x1p-53, -0.25, 7.5, 1e-300};
    std::vector<double> x(m);
    for (size_t j = 0; j < m; ++j) {
        if (j < 5)
            x[j] = specials[axis ? 4 - j : j];
        else if (j % 3)
            x[j] = ((axis ? 0.2 : 0.7) * (double)grid + 0.5 + 0.25 * (double)rnd(7 + axis, j)) / (double)grid - 3.0 + 4.0 * axis;
        else
            x[j] = 2.0 * (double)rnd(9 + axis, j);
    }
    return x;
}

struct Tables {
    size_t n1, n2, m, g1, g2, cells;
    unsigned log_g1 = 0, log_g2 = 0;
    int w;
    Buf<double> xs, ys;
    Buf<uint32_t> perm, cell;
    Tables(size_t n1_, size_t n2_, size_t m_, int w_)
        : n1(n1_), n2(n2_), m(m_), g1((size_t)nufft_grid(n1_, w_)), g2((size_t)nufft_grid(n2_, w_)), cells(g1 * g2), w(w_), xs(m_),
          ys(m_), perm(m_), cell(g1 * g2 + 1) {
        while (((size_t)1 << log_g1) < g1) ++log_g1;
        while (((size_t)1 << log_g2) < g2) ++log_g2;
        const std::vector<double> x = make_coordinate(m, g1, 0), y = make_coordinate(m, g2, 1);
        const double *const in[2] = {x.data(), y.data()};
        const unsigned log_g[2] = {log_g1, log_g2};
        double *const sorted[2] = {xs.p, ys.p};
        nufft_nd_bin<2>(in, m, log_g, sorted, perm.p, cell.p);
    }
};

ld phi_ld(ld z, ld beta) { return z * z < 1 ? expl(beta * (sqrtl(1 - z * z) - 1)) : 0; }
// the signed distance from a position p (turns) to grid point l round a ring of `grid` cells
ld ring(ld p, size_t l, size_t grid) {
    ld d = (ld)l - p * (ld)grid;
    if (d >= (ld)grid / 2) d -= (ld)grid;
    if (d < -(ld)grid / 2) d += (ld)grid;
    return d;
}

template <typename T> void compare(int kind, const char *what, size_t idx, const T *got, ld want, ld gate) {
    ++g_compared;
    if (is_sentinel(got)) return fail(kind, "%s[%zu] was not written", what, idx);
    const ld err = fabsl((ld)*got - want);
    if (gate > 0 && (double)(err / gate) > g_worst[kind]) g_worst[kind] = (double)(err / gate);
    if (!(err <= gate)) fail(kind, "%s[%zu] = %.17Lg, want %.17Lg: error %.3Lg > gate %.3Lg", what, idx, (ld)*got, want, err, gate);
}

template <typename T> NufftNdArgs<2> args_of(const Tables &t, const T *inv1, const T *inv2) {
    NufftNdArgs<2> a{};
    const double *const xs[2] = {t.xs.p, t.ys.p};
    const T *const inv[2] = {inv1, inv2};
    const size_t n[2] = {t.n1, t.n2};
    const unsigned log_g[2] = {t.log_g1, t.log_g2};
    for (size_t i = 0; i < 2; ++i) {
        a.xs[i] = xs[i];
        a.inv[i] = inv[i];
        a.n[i] = n[i];
        a.log_g[i] = log_g[i];
    }
    a.perm = t.perm.p;
    a.cell_start = t.cell.p;
    a.m = t.m;
    a.w = t.w;
    return a;
}
bool al(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// the kernel values of every (grid index, sorted point) pair of one axis inside the support, with what each may be off by
struct Weights {
    struct Term {
        uint32_t l, i;
        ld k, e;  // the value, and the error it is allowed per unit of data (the edge allowance included)
    };
    std::vector<Term> terms;
    Weights(const double *pos, size_t m, size_t grid, int w, ld u) {
        const ld beta = 2.30L * w, jump = expl(-beta);
        for (size_t l = 0; l < grid; ++l)
            for (size_t i = 0; i < m; ++i) {
                const ld z = 2 * ring((ld)pos[i], l, grid) / w;
                if (!(fabsl(z) < 1 + 16 * u)) continue;
                ld e = (100 + 2 * beta) * u;
                if (fabsl(1 - z * z) < 8 * u) e += jump * (1 + beta);
                terms.push_back({(uint32_t)l, (uint32_t)i, phi_ld(z, beta), e});
            }
    }
};

// one (batch, alignment, real) case: all four kernels, each on its own buffers
template <typename T> void run_case(const Tables &t, const Weights &w1, const Weights &w2, size_t batch, size_t plane_off, size_t wk_off, bool real,
                                    bool group_dist = false) {
    constexpr size_t V = Fp<T>::V;
    const ld u = Fp<T>::u;
    const size_t G = t.cells, g2 = t.g2, n = t.n1 * t.n2, m = t.m;
    // distances above the row: gaps keep their sentinel.  group_dist: multiples of the 16-byte group, so that a batch takes
    // the vector variants of pre and deconvolve at b * dist
    auto up = [](size_t k) { return (k + 4) & ~(size_t)3; };
    const size_t pd = batch == 1 ? m : group_dist ? up(m) : m + 3, fd = batch == 1 ? n : group_dist ? up(n) : n + 5;
    Buf<T> inv1(t.n1), inv2(t.n2);
    for (size_t i = 0; i < t.n1; ++i) inv1[i] = (T)(1.5L + 0.5L * rnd(3, i));
    for (size_t i = 0; i < t.n2; ++i) inv2[i] = (T)(1.25L + 0.25L * rnd(4, i));
    std::snprintf(g_case, sizeof g_case, "%s %s N=%zux%zu M=%zu w=%d grid=%zux%zu batch=%zu dist %zu/%zu planes+%zu work+%zu%s", Fp<T>::name(),
                  block_shim::order == block_shim::kAscending ? "ascending" : "descending", t.n1, t.n2, m, t.w, t.g1, g2, batch, pd, fd, plane_off, wk_off, real ? " real" : "");
    // the pairs (l1, l2, i) of the support, grouped by point: per point the axis-1 and axis-2 terms
    std::vector<std::vector<const Weights::Term *>> by1(m), by2(m);
    for (const auto &a : w1.terms) by1[a.i].push_back(&a);
    for (const auto &a : w2.terms) by2[a.i].push_back(&a);
    // ---- spread: caller's point planes -> workspace
    {
        Buf<T> cr((batch - 1) * pd + m, plane_off), ci(real ? 0 : (batch - 1) * pd + m, plane_off), wk(2 * batch * G, wk_off);
        fill_random(cr, 11);
        fill_random(ci, 12);
        fill_sentinel(wk);
        NufftNdArgs<2> a = args_of<T>(t, inv1.p, inv2.p);
        a.in_re = cr.p;
        a.in_im = real ? nullptr : ci.p;
        a.out_re = wk.p;
        a.out_im = wk.p + batch * G;
        a.in_dist = pd;
        a.groups = batch * G;
        if (launch_nufft_nd<T, 2>(0, false, a, nullptr) != hipSuccess) fail(0, "the launcher failed");
        for (size_t b = 0; b < batch; ++b) {
            std::vector<ld> sr(G, 0), si(G, 0), gr(G, 0), gi(G, 0);
            std::vector<size_t> terms(G, 0);
            for (size_t i = 0; i < m; ++i) {
                const ld vr = cr[b * pd + t.perm.p[i]], vi = real ? 0 : (ld)ci[b * pd + t.perm.p[i]];
                for (const auto *a1 : by1[i])
                    for (const auto *a2 : by2[i]) {
                        const size_t l = (size_t)a1->l * g2 + a2->l;
                        const ld k = a1->k * a2->k, e = a1->e + a2->e + 3 * u;
                        sr[l] += k * vr;
                        si[l] += k * vi;
                        gr[l] += e * fabsl(vr);
                        gi[l] += e * fabsl(vi);
                        ++terms[l];
                    }
            }
            for (size_t l = 0; l < G; ++l) {
                compare(0, "g.re", b * G + l, wk.p + b * G + l, sr[l], gr[l] * (1 + terms[l] * u) + terms[l] * u * fabsl(sr[l]));
                compare(0, "g.im", b * G + l, wk.p + (batch + b) * G + l, si[l], gi[l] * (1 + terms[l] * u) + terms[l] * u * fabsl(si[l]));
            }
        }
    }
    // ---- interpolate: workspace -> caller's point planes
    if (!real) {
        Buf<T> wk(2 * batch * G, wk_off), orr((batch - 1) * pd + m, plane_off), oi((batch - 1) * pd + m, plane_off);
        fill_random(wk, 21);
        fill_sentinel(orr);
        fill_sentinel(oi);
        NufftNdArgs<2> a = args_of<T>(t, inv1.p, inv2.p);
        a.in_re = wk.p;
        a.in_im = wk.p + batch * G;
        a.out_re = orr.p;
        a.out_im = oi.p;
        a.out_dist = pd;
        a.groups = batch * m;
        if (launch_nufft_nd<T, 2>(1, false, a, nullptr) != hipSuccess) fail(1, "the launcher failed");
        std::vector<char> named(orr.n, 0);
        for (size_t b = 0; b < batch; ++b)
            for (size_t i = 0; i < m; ++i) {
                ld sr = 0, si = 0, gr = 0, gi = 0;
                size_t terms = 0;
                for (const auto *a1 : by1[i])
                    for (const auto *a2 : by2[i]) {
                        const size_t l = (size_t)a1->l * g2 + a2->l;
                        const ld k = a1->k * a2->k, e = a1->e + a2->e + 3 * u;
                        const ld vr = wk[b * G + l], vi = wk[(batch + b) * G + l];
                        sr += k * vr;
                        si += k * vi;
                        gr += e * fabsl(vr);
                        gi += e * fabsl(vi);
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
        Buf<T> fr((batch - 1) * fd + n, plane_off), fi(real ? 0 : (batch - 1) * fd + n, plane_off), wk(2 * batch * G, wk_off);
        fill_random(fr, 31);
        fill_random(fi, 32);
        fill_sentinel(wk);
        NufftNdArgs<2> a = args_of<T>(t, inv1.p, inv2.p);
        a.in_re = fr.p;
        a.in_im = real ? nullptr : fi.p;
        a.out_re = wk.p;
        a.out_im = wk.p + batch * G;
        a.in_dist = fd;
        a.groups = batch * (G / V);
        const bool vec = al(fr.p) && (real || al(fi.p)) && al(wk.p) && fd % V == 0;
        if (launch_nufft_nd<T, 2>(2, vec, a, nullptr) != hipSuccess) fail(2, "the launcher failed");
        for (size_t b = 0; b < batch; ++b) {
            std::vector<char> named(G, 0);
            for (size_t i1 = 0; i1 < t.n1; ++i1)
                for (size_t i2 = 0; i2 < t.n2; ++i2) {
                    const size_t s = (size_t)nufft_slot(i1, t.n1, t.g1) * g2 + (size_t)nufft_slot(i2, t.n2, g2), i = i1 * t.n2 + i2;
                    named[s] = 1;
                    const ld p = (ld)inv1[i1] * (ld)inv2[i2];
                    const ld wr = (ld)fr[b * fd + i] * p, wi = real ? 0 : (ld)fi[b * fd + i] * p;
                    compare(2, "g^.re", b * G + s, wk.p + b * G + s, wr, 3 * u * fabsl(wr));
                    compare(2, "g^.im", b * G + s, wk.p + (batch + b) * G + s, wi, 3 * u * fabsl(wi));
                }
            for (size_t s = 0; s < G; ++s)
                if (!named[s]) {
                    const T zr = wk[b * G + s], zi = wk[(batch + b) * G + s];
                    ++g_compared;
                    if (!(zr == 0 && zi == 0)) fail(2, "workspace[%zu] = (%g, %g) must be exactly 0", b * G + s, (double)zr, (double)zi);
                }
        }
    }
    // ---- deconvolve: workspace -> caller's mode planes
    if (!real) {
        Buf<T> wk(2 * batch * G, wk_off), orr((batch - 1) * fd + n, plane_off), oi((batch - 1) * fd + n, plane_off);
        fill_random(wk, 41);
        fill_sentinel(orr);
        fill_sentinel(oi);
        NufftNdArgs<2> a = args_of<T>(t, inv1.p, inv2.p);
        a.in_re = wk.p;
        a.in_im = wk.p + batch * G;
        a.out_re = orr.p;
        a.out_im = oi.p;
        a.out_dist = fd;
        a.gpt = (unsigned)(t.n1 * ((t.n2 + V - 1) / V));
        a.groups = batch * a.gpt;
        const bool vec = al(orr.p) && al(oi.p) && al(wk.p) && fd % V == 0;
        if (launch_nufft_nd<T, 2>(3, vec, a, nullptr) != hipSuccess) fail(3, "the launcher failed");
        for (size_t b = 0; b < batch; ++b)
            for (size_t i1 = 0; i1 < t.n1; ++i1)
                for (size_t i2 = 0; i2 < t.n2; ++i2) {
                    const size_t s = (size_t)nufft_slot(i1, t.n1, t.g1) * g2 + (size_t)nufft_slot(i2, t.n2, g2), i = i1 * t.n2 + i2;
                    const ld p = (ld)inv1[i1] * (ld)inv2[i2];
                    const ld wr = (ld)wk[b * G + s] * p, wi = (ld)wk[(batch + b) * G + s] * p;
                    compare(3, "F.re", b * fd + i, orr.p + b * fd + i, wr, 3 * u * fabsl(wr));
                    compare(3, "F.im", b * fd + i, oi.p + b * fd + i, wi, 3 * u * fabsl(wi));
                }
        for (size_t b = 0; b + 1 < batch; ++b)
            for (size_t o = b * fd + n; o < (b + 1) * fd; ++o)
                if (!(is_sentinel(orr.p + o) && is_sentinel(oi.p + o))) fail(3, "out[%zu] lies between two rows and was written", o);
    }
}

template <typename T> void run_all() {
    const size_t shapes[][4] = {{1, 1, 1, 2}, {2, 3, 5, 3}, {7, 5, 40, 16}, {16, 12, 300, 4}, {33, 20, 1000, 13}};
    for (const auto &s : shapes) {
        const Tables t(s[0], s[1], s[2], (int)s[3]);
        const Weights w1(t.xs.p, t.m, t.g1, t.w, Fp<T>::u), w2(t.ys.p, t.m, t.g2, t.w, Fp<T>::u);
        for (block_shim::Order order : {block_shim::kAscending, block_shim::kDescending}) {
            block_shim::order = order;
            for (size_t batch : {(size_t)1, (size_t)3}) {
                run_case<T>(t, w1, w2, batch, 0, 0, false);
                run_case<T>(t, w1, w2, batch, 1, 0, false);  // caller planes at element alignment (buf[1:])
                run_case<T>(t, w1, w2, batch, 0, 1, false);  // the workspace at element alignment
                run_case<T>(t, w1, w2, batch, 0, 0, true);   // no imaginary input plane
                run_case<T>(t, w1, w2, batch, 1, 0, true);
                if (batch > 1) {  // distances that are multiples of the group: the vector variants of the sweeps in a batch
                    run_case<T>(t, w1, w2, batch, 0, 0, false, true);
                    run_case<T>(t, w1, w2, batch, 0, 0, true, true);
                }
            }
        }
        block_shim::order = block_shim::kAscending;
    }
}

}  // namespace

int main() {
    run_all<double>();
    run_all<float>();
    for (int k = 0; k < 4; ++k) std::printf("  %-23s worst error / gate %.3f\n", kKernel[k], g_worst[k]);
    std::printf("launches %llu threads %llu elements %llu\n", block_shim::launches, block_shim::threads_run, g_compared);
    std::printf("nufft2d: %s (%d failures)\n", g_fails ? "FAILED" : "ok", g_fails);
    phast_test_exit(g_fails ? 1 : 0);
}
