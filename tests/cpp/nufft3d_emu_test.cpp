// nufft3d_emu_test.cpp -- the four kernels of the three-dimensional non-uniform FFT (csrc/nufft_nd.hip at D = 3), run on the host under
// AddressSanitizer and UndefinedBehaviorSanitizer (tests/test_nufft3d_emulator.py builds and runs it).  The spread kernel stages
// points through LDS between barriers, so the program stands on tests/emu/block_shim.hpp: a workgroup's threads are fibers that
// run from one __syncthreads() to the next in ascending or in descending order, and every case runs in BOTH orders -- a thread
// that reads LDS another has not yet written, or overwrites LDS another has not yet read, gets wrong bits in one of them.  One
// translation unit with its own main, linked without the HIP runtime.  nufft_nd.hip is #included as it stands and every kernel is
// driven through launch_nufft_nd<T, 3> with arguments built as planner_nufft_nd.hpp builds them, from tables made by
// nufft_nd.hpp's own nufft_nd_bin.
//
// Buffers: every plane, table and workspace is a heap allocation of exactly the bytes the contract covers; an "unaligned"
// buffer is one element longer and used from element 1.  Workspaces written by a kernel start as NaN, caller outputs as a
// NaN sentinel: an element the contract names must have lost it, every other element must have kept its exact bits.
//
// Every element is compared with a long double statement of its stage, written here a second time (d_i: the signed distance
// round the ring of g_i cells from the point's position g_i x to the grid index):
//     spread       g[l1, l2, l3]  = sum_j phi(2 d1 / w) phi(2 d2 / w) phi(2 d3 / w) c_j
//     interpolate  c_j            = sum_l phi(2 d1 / w) phi(2 d2 / w) phi(2 d3 / w) g[l1, l2, l3]
//     pre          g^[s1, s2, s3] = F[m1, m2, m3] p1[m1] p2[m2] p3[m3] at s_i = slot(m_i), exactly 0 in every other slot
//     deconvolve   F[m1, m2, m3]  = g^[slot(m1), slot(m2), slot(m3)] p1[m1] p2[m2] p3[m3]
// The gate is derived as tests/cpp/nufft2d_emu_test.cpp derives its own: pre and deconvolve are three products rounded to T,
// 4 u_T |product|.  One kernel value is off by at most e = (100 + 2 beta) u_R (phi <= 1), the product of three by 3 e + 2 u_R; a
// sum of n terms adds n + 2 roundings.  phi jumps from e^{-beta} to 0 at |z| = 1, so a term with a factor within 8 u_R of the
// edge may fall on either side: it is allowed e^{-beta} (1 + beta) |value| more.
//
// The clump cases put exactly kNufft3dChunk points, and then one more, into a single cell: one full pass through LDS, and a
// full pass followed by a pass of one point.
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
char g_case[320] = "";

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

// one coordinate of the points: the specials first (x), last-first (y) or rotated by two (z) -- the support wraps both ends of
// every axis -- then a clump inside one cell, a turn or three away, among uniform points.  clump: every point inside ONE cell
std::vector<double> make_coordinate(size_t m, size_t grid, int axis, bool clump) {
    const double specials[] = {0.0, 1 - 0x1p-53, -0.25, 7.5, 1e-300};
    const double spot[] = {0.7, 0.2, 0.45};
    std::vector<double> x(m);
    for (size_t j = 0; j < m; ++j) {
        const double in_cell = ((double)(size_t)(spot[axis] * (double)grid) + 0.5 + 0.25 * (double)rnd(7 + axis, j)) / (double)grid;
        if (clump)
            x[j] = in_cell;
        else if (j < 5)
            x[j] = specials[axis == 0 ? j : axis == 1 ? 4 - j : (j + 2) % 5];
        else if (j % 3)
            x[j] = in_cell - 3.0 + 2.0 * axis;
        else
            x[j] = 2.0 * (double)rnd(9 + axis, j);
    }
    return x;
}

struct Tables {
    size_t n[3], m, g[3], cells;
    unsigned log_g[3] = {0, 0, 0};
    int w;
    Buf<double> xs, ys, zs;
    Buf<uint32_t> perm, cell;
    Tables(size_t n1, size_t n2, size_t n3, size_t m_, int w_, bool clump = false)
        : n{n1, n2, n3}, m(m_), g{(size_t)nufft_grid(n1, w_), (size_t)nufft_grid(n2, w_), (size_t)nufft_grid(n3, w_)},
          cells(g[0] * g[1] * g[2]), w(w_), xs(m_), ys(m_), zs(m_), perm(m_), cell(g[0] * g[1] * g[2] + 1) {
        for (int i = 0; i < 3; ++i)
            while (((size_t)1 << log_g[i]) < g[i]) ++log_g[i];
        const std::vector<double> x = make_coordinate(m, g[0], 0, clump), y = make_coordinate(m, g[1], 1, clump),
                                  z = make_coordinate(m, g[2], 2, clump);
        const double *const in[3] = {x.data(), y.data(), z.data()};
        double *const sorted[3] = {xs.p, ys.p, zs.p};
        nufft_nd_bin<3>(in, m, log_g, sorted, perm.p, cell.p);
        if (clump) {  // the case is what it says: one cell holds every point
            size_t most = 0;
            for (size_t q = 0; q < cells; ++q) most = std::max<size_t>(most, cell.p[q + 1] - cell.p[q]);
            if (most != m) std::abort();
            std::printf("clump: %zu points in one cell\n", most);
        }
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

template <typename T> NufftNdArgs<3> args_of(const Tables &t, const T *inv1, const T *inv2, const T *inv3) {
    NufftNdArgs<3> a{};
    const double *const xs[3] = {t.xs.p, t.ys.p, t.zs.p};
    const T *const inv[3] = {inv1, inv2, inv3};
    for (size_t i = 0; i < 3; ++i) {
        a.xs[i] = xs[i];
        a.inv[i] = inv[i];
        a.n[i] = t.n[i];
        a.log_g[i] = t.log_g[i];
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
    std::vector<std::vector<Term>> by;  // per sorted point
    Weights(const double *pos, size_t m, size_t grid, int w, ld u) : by(m) {
        const ld beta = 2.30L * w, jump = expl(-beta);
        for (size_t i = 0; i < m; ++i)
            for (size_t l = 0; l < grid; ++l) {
                const ld z = 2 * ring((ld)pos[i], l, grid) / w;
                if (!(fabsl(z) < 1 + 16 * u)) continue;
                ld e = (100 + 2 * beta) * u;
                if (fabsl(1 - z * z) < 8 * u) e += jump * (1 + beta);
                by[i].push_back({(uint32_t)l, (uint32_t)i, phi_ld(z, beta), e});
            }
    }
};

// one (batch, alignment, real) case: all four kernels, each on its own buffers
template <typename T>
void run_case(const Tables &t, const Weights &w1, const Weights &w2, const Weights &w3, size_t batch, size_t plane_off, size_t wk_off, bool real,
              bool group_dist = false) {
    constexpr size_t V = Fp<T>::V;
    const ld u = Fp<T>::u;
    const size_t G = t.cells, g2 = t.g[1], g3 = t.g[2], n = t.n[0] * t.n[1] * t.n[2], m = t.m;
    // distances above the row: gaps keep their sentinel.  group_dist: multiples of the 16-byte group, so that a batch takes
    // the vector variants of pre and deconvolve at b * dist
    auto up = [](size_t k) { return (k + 4) & ~(size_t)3; };
    const size_t pd = batch == 1 ? m : group_dist ? up(m) : m + 3, fd = batch == 1 ? n : group_dist ? up(n) : n + 5;
    Buf<T> inv1(t.n[0]), inv2(t.n[1]), inv3(t.n[2]);
    for (size_t i = 0; i < t.n[0]; ++i) inv1[i] = (T)(1.5L + 0.5L * rnd(3, i));
    for (size_t i = 0; i < t.n[1]; ++i) inv2[i] = (T)(1.25L + 0.25L * rnd(4, i));
    for (size_t i = 0; i < t.n[2]; ++i) inv3[i] = (T)(1.125L + 0.125L * rnd(5, i));
    std::snprintf(g_case, sizeof g_case, "%s %s N=%zux%zux%zu M=%zu w=%d grid=%zux%zux%zu batch=%zu dist %zu/%zu planes+%zu work+%zu%s", Fp<T>::name(),
                  block_shim::order == block_shim::kAscending ? "ascending" : "descending", t.n[0], t.n[1], t.n[2], m, t.w, t.g[0], g2, g3, batch, pd,
                  fd, plane_off, wk_off, real ? " real" : "");
    auto slot_of = [&](size_t i1, size_t i2, size_t i3) {
        return ((size_t)nufft_slot(i1, t.n[0], t.g[0]) * g2 + (size_t)nufft_slot(i2, t.n[1], g2)) * g3 + (size_t)nufft_slot(i3, t.n[2], g3);
    };
    // ---- spread: caller's point planes -> workspace
    {
        Buf<T> cr((batch - 1) * pd + m, plane_off), ci(real ? 0 : (batch - 1) * pd + m, plane_off), wk(2 * batch * G, wk_off);
        fill_random(cr, 11);
        fill_random(ci, 12);
        fill_sentinel(wk);
        NufftNdArgs<3> a = args_of<T>(t, inv1.p, inv2.p, inv3.p);
        a.in_re = cr.p;
        a.in_im = real ? nullptr : ci.p;
        a.out_re = wk.p;
        a.out_im = wk.p + batch * G;
        a.in_dist = pd;
        a.groups = batch * G;
        if (launch_nufft_nd<T, 3>(0, false, a, nullptr) != hipSuccess) fail(0, "the launcher failed");
        for (size_t b = 0; b < batch; ++b) {
            std::vector<ld> sr(G, 0), si(G, 0), gr(G, 0), gi(G, 0);
            std::vector<size_t> terms(G, 0);
            for (size_t i = 0; i < m; ++i) {
                const ld vr = cr[b * pd + t.perm.p[i]], vi = real ? 0 : (ld)ci[b * pd + t.perm.p[i]];
                for (const auto &a1 : w1.by[i])
                    for (const auto &a2 : w2.by[i])
                        for (const auto &a3 : w3.by[i]) {
                            const size_t l = ((size_t)a1.l * g2 + a2.l) * g3 + a3.l;
                            const ld k = a1.k * a2.k * a3.k, e = a1.e + a2.e + a3.e + 4 * u;
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
        NufftNdArgs<3> a = args_of<T>(t, inv1.p, inv2.p, inv3.p);
        a.in_re = wk.p;
        a.in_im = wk.p + batch * G;
        a.out_re = orr.p;
        a.out_im = oi.p;
        a.out_dist = pd;
        a.groups = batch * m;
        if (launch_nufft_nd<T, 3>(1, false, a, nullptr) != hipSuccess) fail(1, "the launcher failed");
        std::vector<char> named(orr.n, 0);
        for (size_t b = 0; b < batch; ++b)
            for (size_t i = 0; i < m; ++i) {
                ld sr = 0, si = 0, gr = 0, gi = 0;
                size_t terms = 0;
                for (const auto &a1 : w1.by[i])
                    for (const auto &a2 : w2.by[i])
                        for (const auto &a3 : w3.by[i]) {
                            const size_t l = ((size_t)a1.l * g2 + a2.l) * g3 + a3.l;
                            const ld k = a1.k * a2.k * a3.k, e = a1.e + a2.e + a3.e + 4 * u;
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
        NufftNdArgs<3> a = args_of<T>(t, inv1.p, inv2.p, inv3.p);
        a.in_re = fr.p;
        a.in_im = real ? nullptr : fi.p;
        a.out_re = wk.p;
        a.out_im = wk.p + batch * G;
        a.in_dist = fd;
        a.groups = batch * (G / V);
        const bool vec = al(fr.p) && (real || al(fi.p)) && al(wk.p) && (batch == 1 || fd % V == 0);
        if (launch_nufft_nd<T, 3>(2, vec, a, nullptr) != hipSuccess) fail(2, "the launcher failed");
        for (size_t b = 0; b < batch; ++b) {
            std::vector<char> named(G, 0);
            for (size_t i1 = 0; i1 < t.n[0]; ++i1)
                for (size_t i2 = 0; i2 < t.n[1]; ++i2)
                    for (size_t i3 = 0; i3 < t.n[2]; ++i3) {
                        const size_t s = slot_of(i1, i2, i3), i = (i1 * t.n[1] + i2) * t.n[2] + i3;
                        named[s] = 1;
                        const ld p = (ld)inv1[i1] * (ld)inv2[i2] * (ld)inv3[i3];
                        const ld wr = (ld)fr[b * fd + i] * p, wi = real ? 0 : (ld)fi[b * fd + i] * p;
                        compare(2, "g^.re", b * G + s, wk.p + b * G + s, wr, 4 * u * fabsl(wr));
                        compare(2, "g^.im", b * G + s, wk.p + (batch + b) * G + s, wi, 4 * u * fabsl(wi));
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
        NufftNdArgs<3> a = args_of<T>(t, inv1.p, inv2.p, inv3.p);
        a.in_re = wk.p;
        a.in_im = wk.p + batch * G;
        a.out_re = orr.p;
        a.out_im = oi.p;
        a.out_dist = fd;
        a.gpt = (unsigned)(t.n[0] * t.n[1] * ((t.n[2] + V - 1) / V));
        a.groups = batch * a.gpt;
        const bool vec = al(orr.p) && al(oi.p) && al(wk.p) && (batch == 1 || fd % V == 0);
        if (launch_nufft_nd<T, 3>(3, vec, a, nullptr) != hipSuccess) fail(3, "the launcher failed");
        for (size_t b = 0; b < batch; ++b)
            for (size_t i1 = 0; i1 < t.n[0]; ++i1)
                for (size_t i2 = 0; i2 < t.n[1]; ++i2)
                    for (size_t i3 = 0; i3 < t.n[2]; ++i3) {
                        const size_t s = slot_of(i1, i2, i3), i = (i1 * t.n[1] + i2) * t.n[2] + i3;
                        const ld p = (ld)inv1[i1] * (ld)inv2[i2] * (ld)inv3[i3];
                        const ld wr = (ld)wk[b * G + s] * p, wi = (ld)wk[(batch + b) * G + s] * p;
                        compare(3, "F.re", b * fd + i, orr.p + b * fd + i, wr, 4 * u * fabsl(wr));
                        compare(3, "F.im", b * fd + i, oi.p + b * fd + i, wi, 4 * u * fabsl(wi));
                    }
        for (size_t b = 0; b + 1 < batch; ++b)
            for (size_t o = b * fd + n; o < (b + 1) * fd; ++o)
                if (!(is_sentinel(orr.p + o) && is_sentinel(oi.p + o))) fail(3, "out[%zu] lies between two rows and was written", o);
    }
}

template <typename T> void run_shape(const Tables &t, bool every_variant) {
    const Weights w1(t.xs.p, t.m, t.g[0], t.w, Fp<T>::u), w2(t.ys.p, t.m, t.g[1], t.w, Fp<T>::u), w3(t.zs.p, t.m, t.g[2], t.w, Fp<T>::u);
    for (block_shim::Order order : {block_shim::kAscending, block_shim::kDescending}) {
        block_shim::order = order;
        for (size_t batch : {(size_t)1, (size_t)3}) {
            run_case<T>(t, w1, w2, w3, batch, 0, 0, false);
            run_case<T>(t, w1, w2, w3, batch, 0, 0, true);  // no imaginary input plane
            // alignment moves the sweeps, which hold no barrier: one thread order says all there is to say about them
            if (!every_variant || order == block_shim::kDescending) continue;
            run_case<T>(t, w1, w2, w3, batch, 1, 0, false);  // caller planes at element alignment (buf[1:])
            run_case<T>(t, w1, w2, w3, batch, 0, 1, false);  // the workspace at element alignment
            run_case<T>(t, w1, w2, w3, batch, 1, 0, true);
            if (batch > 1) {  // distances that are multiples of the group: the vector variants of the sweeps in a batch
                run_case<T>(t, w1, w2, w3, batch, 0, 0, false, true);
                run_case<T>(t, w1, w2, w3, batch, 0, 0, true, true);
            }
        }
    }
    block_shim::order = block_shim::kAscending;
}

template <typename T> void run_all() {
    const size_t shapes[][5] = {{1, 1, 1, 1, 2}, {2, 3, 4, 5, 3}, {5, 7, 3, 40, 16}, {12, 10, 9, 300, 4}, {33, 20, 7, 1000, 13}};
    for (const auto &s : shapes) {
        const Tables t(s[0], s[1], s[2], s[3], (int)s[4]);
        run_shape<T>(t, true);
    }
    // one cell holds exactly the LDS chunk, then one point more (the alignment variants add nothing to what the chunking does)
    for (size_t m : {(size_t)kNufft3dChunk, (size_t)kNufft3dChunk + 1}) {
        const Tables t(2, 3, 4, m, 3, true);
        run_shape<T>(t, false);
    }
}

}  // namespace

// no argument: both types; "f64" or "f32": that type alone (the test runs the two side by side)
int main(int argc, char **argv) {
    const bool f64 = argc < 2 || !std::strcmp(argv[1], "f64"), f32 = argc < 2 || !std::strcmp(argv[1], "f32");
    if (!f64 && !f32) {
        std::printf("usage: %s [f64|f32]\n", argv[0]);
        return 2;
    }
    if (f64) run_all<double>();
    if (f32) run_all<float>();
    for (int k = 0; k < 4; ++k) std::printf("  %-23s worst error / gate %.3f\n", kKernel[k], g_worst[k]);
    std::printf("chunk %u ", kNufft3dChunk);
    std::printf("launches %llu threads %llu barriers %llu elements %llu\n", block_shim::launches, block_shim::threads_run, block_shim::barriers, g_compared);
    std::printf("nufft3d: %s (%d failures)\n", g_fails ? "FAILED" : "ok", g_fails);
    phast_test_exit(g_fails ? 1 : 0);
}
