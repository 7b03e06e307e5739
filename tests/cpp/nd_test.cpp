// nd_test.cpp -- the C++ host side (include/phastft.hpp) of the multi-dimensional transforms: PlannerNd64/32,
// PlannerR2cNd64/32 and the free functions.  Built and run by tests/test_nd_cpu.py (no GPU: shape panics, compute fails
// loudly) and tests/test_gpu_nd.py (with "gpu": against a long-double 2-D DFT, round trips, planner vs no planner bits).
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "phastft.hpp"

using namespace phastft;

static int failures = 0;
#define EXPECT(cond)                                                            \
    do {                                                                        \
        if (!(cond)) {                                                          \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);         \
            ++failures;                                                         \
        }                                                                       \
    } while (0)

template <typename F> static int code_of(F &&f) {
    try {
        f();
    } catch (const Panic &p) {
        return p.code;
    } catch (const HipError &e) {
        return e.code;
    }
    return PHAST_OK;
}

static void fill(std::vector<double> &v, unsigned long long seed) {
    unsigned long long s = seed * 0x9e3779b97f4a7c15ull + 1;
    for (double &x : v) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        x = (double)(s >> 11) / 9007199254740992.0 * 2 - 1;
    }
}

// O(N^2) long-double 2-D DFT [r][c], exact phases (j k mod n)
static double dft2_rel_err(size_t r, size_t c, const std::vector<double> &xr, const std::vector<double> &xi,
                           const std::vector<double> &gr, const std::vector<double> &gi) {
    const long double tau = 6.283185307179586476925286766559005768L;
    long double num = 0, den = 0;
    for (size_t k0 = 0; k0 < r; ++k0)
        for (size_t k1 = 0; k1 < c; ++k1) {
            long double sr = 0, si = 0;
            for (size_t j0 = 0; j0 < r; ++j0)
                for (size_t j1 = 0; j1 < c; ++j1) {
                    const long double a = -tau * ((long double)((j0 * k0) % r) / r + (long double)((j1 * k1) % c) / c);
                    const long double cr = cosl(a), ci = sinl(a);
                    sr += xr[j0 * c + j1] * cr - xi[j0 * c + j1] * ci;
                    si += xr[j0 * c + j1] * ci + xi[j0 * c + j1] * cr;
                }
            const size_t k = k0 * c + k1;
            num += (gr[k] - sr) * (gr[k] - sr) + (gi[k] - si) * (gi[k] - si);
            den += sr * sr + si * si;
        }
    return (double)sqrtl(num / den);
}

static void no_gpu() {
    EXPECT(code_of([] { PlannerNd64 p(std::vector<size_t>{}); }) == PHAST_ERR_INVALID_ARG);
    EXPECT(code_of([] { PlannerNd32 p({4, 0}); }) == PHAST_ERR_INVALID_ARG);
    EXPECT(code_of([] { PlannerR2cNd64 p({1u << 16, 1u << 15}); }) == PHAST_ERR_INVALID_ARG);
    EXPECT(code_of([] { PlannerR2cNd32 p(std::vector<size_t>(9, 2)); }) == PHAST_ERR_INVALID_ARG);
    EXPECT(code_of([] { PlannerNd64 p({30, 40}); }) == PHAST_ERR_NO_DEVICE);
    std::vector<double> a(12), b(11), c(12);
    EXPECT(code_of([&] { fft_64_nd(a, b, {3, 4}, Direction::Forward); }) == PHAST_ERR_LEN_MISMATCH);
    EXPECT(code_of([&] { fft_64_nd(a, c, {3, 5}, Direction::Forward); }) == PHAST_ERR_PLANNER_SIZE);
    EXPECT(code_of([&] { fft_64_nd(a, c, {3, 4}, Direction::Forward); }) == PHAST_ERR_NO_DEVICE);
    std::vector<double> h(9);
    EXPECT(code_of([&] { r2c_fft_f64_nd(a, h, h, {3, 4}); }) == PHAST_ERR_NO_DEVICE);
    EXPECT(code_of([&] { r2c_fft_f64_nd(a, b, h, {3, 4}); }) == PHAST_ERR_R2C_OUT_RE_LEN);
    EXPECT(code_of([&] { c2r_fft_f64_nd(h, h, b, {3, 4}); }) == PHAST_ERR_C2R_OUTPUT_LEN);
}

static void gpu() {
    for (auto rc : {std::vector<size_t>{3, 5}, std::vector<size_t>{16, 9}, std::vector<size_t>{7, 8}}) {
        const size_t r = rc[0], c = rc[1], n = r * c;
        std::vector<double> xr(n), xi(n);
        fill(xr, n);
        fill(xi, n + 1);
        std::vector<double> gr = xr, gi = xi, hr = xr, hi = xi;
        PlannerNd64 p(rc);
        fft_64_nd_with_planner(gr, gi, Direction::Forward, p);
        const double e = dft2_rel_err(r, c, xr, xi, gr, gi);
        std::printf("nd %zux%zu f64 rel %.3g\n", r, c, e);
        EXPECT(e < 1e-14);
        fft_64_nd(hr, hi, rc, Direction::Forward);
        EXPECT(hr == gr && hi == gi);
        fft_64_nd_with_planner(gr, gi, Direction::Reverse, p);
        double back = 0;
        for (size_t k = 0; k < n; ++k) back = std::fmax(back, std::fmax(std::fabs(gr[k] - xr[k]), std::fabs(gi[k] - xi[k])));
        EXPECT(back < 1e-13);
        std::vector<float> fr(xr.begin(), xr.end()), fi(xi.begin(), xi.end());
        PlannerNd32 p32(rc);
        fft_32_nd_with_planner(fr, fi, Direction::Forward, p32);
        std::vector<double> dr(fr.begin(), fr.end()), di(fi.begin(), fi.end());
        EXPECT(dft2_rel_err(r, c, xr, xi, dr, di) < 1e-5);
        // real: R2C -> C2R round trip
        std::vector<double> sr((n / c) * (c / 2 + 1)), si(sr.size()), out(n);
        PlannerR2cNd64 q(rc);
        r2c_fft_f64_nd_with_planner(xr, sr, si, q);
        c2r_fft_f64_nd_with_planner(sr, si, out, q);
        double rt = 0;
        for (size_t k = 0; k < n; ++k) rt = std::fmax(rt, std::fabs(out[k] - xr[k]));
        EXPECT(rt < 1e-13);
        EXPECT(q.workspace_len(1) >= 4 * sr.size());
        EXPECT(q.describe().find("real nd") != std::string::npos);
    }
}

int main(int argc, char **argv) {
    const bool on_gpu = argc > 1 && std::string(argv[1]) == "gpu";
    if (on_gpu)
        gpu();
    else
        no_gpu();
    if (failures) {
        std::printf("nd: %d failures\n", failures);
        return 1;
    }
    std::printf("nd: ok\n");
    return 0;
}
