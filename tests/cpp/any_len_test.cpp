// any_len_test.cpp -- the C++ host side (include/phastft.hpp) of the arbitrary-length transforms: PlannerAny64/32,
// fft_64/32_any[_with_planner].  Built and run by tests/test_any_len_cpu.py (no GPU: argument panics, compute fails loudly)
// and tests/test_gpu_any_len.py (with "gpu": against a long-double DFT, round trips, the power-of-two path's bits).
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

// O(N^2) long-double DFT with the exact phase (k j mod N)
static double dft_rel_err(const std::vector<double> &xr, const std::vector<double> &xi, const std::vector<double> &gr,
                          const std::vector<double> &gi) {
    const size_t n = xr.size();
    const long double tau = 6.283185307179586476925286766559005768L;
    long double num = 0, den = 0;
    for (size_t k = 0; k < n; ++k) {
        long double sr = 0, si = 0;
        for (size_t j = 0; j < n; ++j) {
            const long double a = -tau * (long double)((k * j) % n) / (long double)n;
            sr += xr[j] * cosl(a) - xi[j] * sinl(a);
            si += xr[j] * sinl(a) + xi[j] * cosl(a);
        }
        num += (gr[k] - sr) * (gr[k] - sr) + (gi[k] - si) * (gi[k] - si);
        den += sr * sr + si * si;
    }
    return (double)std::sqrt(num / den);
}

static void fill(std::vector<double> &re, std::vector<double> &im, size_t n, unsigned seed) {
    re.resize(n);
    im.resize(n);
    unsigned long long s = 0x9E3779B97F4A7C15ull * (seed + 1);
    for (size_t i = 0; i < n; ++i) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        re[i] = (double)(s >> 11) / 9007199254740992.0 * 2 - 1;
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        im[i] = (double)(s >> 11) / 9007199254740992.0 * 2 - 1;
    }
}

static void no_gpu() {
    EXPECT(code_of([] { PlannerAny64 p(0); }) == PHAST_ERR_INVALID_ARG);
    EXPECT(code_of([] { PlannerAny32 p((1u << 29) + 1); }) == PHAST_ERR_INVALID_ARG);
    EXPECT(code_of([] { PlannerAny64 p(1000); }) == PHAST_ERR_NO_DEVICE);
    std::vector<double> a(10), b(9);
    EXPECT(code_of([&] { fft_64_any(a, b, Direction::Forward); }) == PHAST_ERR_LEN_MISMATCH);
    std::vector<double> c(10);
    EXPECT(code_of([&] { fft_64_any(a, c, Direction::Forward); }) == PHAST_ERR_NO_DEVICE);
}

static void gpu() {
    for (size_t n : {1u, 2u, 3u, 5u, 7u, 12u, 100u, 127u, 1000u, 1009u}) {
        std::vector<double> xr, xi;
        fill(xr, xi, n, (unsigned)n);
        std::vector<double> gr = xr, gi = xi;
        PlannerAny64 p(n);
        EXPECT(p.workspace_len(3) == ((n & (n - 1)) == 0 ? 0 : 3 * 2 * p.workspace_len(1) / 2));
        fft_64_any_with_planner(gr, gi, Direction::Forward, p);
        const double e = dft_rel_err(xr, xi, gr, gi);
        if (!(e < 1e-14)) std::printf("n=%zu rel-L2 %.3e\n", n, e);
        EXPECT(e < 1e-14);
        fft_64_any_with_planner(gr, gi, Direction::Reverse, p);
        double worst = 0;
        for (size_t i = 0; i < n; ++i) worst = std::fmax(worst, std::fmax(std::fabs(gr[i] - xr[i]), std::fabs(gi[i] - xi[i])));
        EXPECT(worst < 1e-13);
        // the planner-less form: the same bits
        std::vector<double> hr = xr, hi = xi, kr = xr, ki = xi;
        fft_64_any(hr, hi, Direction::Forward);
        fft_64_any_with_planner(kr, ki, Direction::Forward, p);
        EXPECT(hr == kr && hi == ki);
        // f32
        std::vector<float> fr(xr.begin(), xr.end()), fi(xi.begin(), xi.end());
        PlannerAny32 q(n);
        fft_32_any_with_planner(fr, fi, Direction::Forward, q);
        std::vector<double> dr(fr.begin(), fr.end()), di(fi.begin(), fi.end());
        std::vector<double> xr32(n), xi32(n);
        for (size_t i = 0; i < n; ++i) {
            xr32[i] = (float)xr[i];
            xi32[i] = (float)xi[i];
        }
        EXPECT(dft_rel_err(xr32, xi32, dr, di) < 5e-6);
        EXPECT(q.device_bytes() > 0 && !q.describe().empty());
    }
    // a power of two: the PlannerDit64 path's bits
    const size_t n = 4096;
    std::vector<double> xr, xi;
    fill(xr, xi, n, 7);
    std::vector<double> ar = xr, ai = xi, br = xr, bi = xi;
    PlannerAny64 pa(n);
    PlannerDit64 pd(n);
    fft_64_any_with_planner(ar, ai, Direction::Forward, pa);
    fft_64_dit_with_planner(br, bi, Direction::Forward, pd);
    EXPECT(ar == br && ai == bi);
    EXPECT(pa.workspace_len(5) == 0);
    std::vector<double> s(999), t(999);
    EXPECT(code_of([&] { fft_64_any_with_planner(s, t, Direction::Forward, pa); }) == PHAST_ERR_PLANNER_SIZE);
}

int main(int argc, char **argv) {
    const bool on_gpu = argc > 1 && std::string(argv[1]) == "gpu";
    if (on_gpu)
        gpu();
    else
        no_gpu();
    if (failures) {
        std::printf("any_len: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("any_len: ok\n");
    return 0;
}
