// any_real_test.cpp -- the C++ host side (include/phastft.hpp) of the arbitrary-length real transforms: PlannerR2cAny64/32,
// r2c_fft_f64/f32_any[_with_planner], c2r_fft_f64/f32_any[_with_planner].  Built and run by tests/test_any_real_cpu.py (no
// GPU: argument panics, compute fails loudly) and tests/test_gpu_any_real.py (with "gpu": against a long-double DFT, round
// trips, the power-of-two path's bits).
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

// O(N^2) long-double real DFT (half spectrum) with the exact phase (k j mod N): rel-L2 of (gr, gi) against it
static double rdft_rel_err(const std::vector<double> &x, const std::vector<double> &gr, const std::vector<double> &gi) {
    const size_t n = x.size();
    const long double tau = 6.283185307179586476925286766559005768L;
    long double num = 0, den = 0;
    for (size_t k = 0; k <= n / 2; ++k) {
        long double sr = 0, si = 0;
        for (size_t j = 0; j < n; ++j) {
            const long double a = -tau * (long double)((k * j) % n) / (long double)n;
            sr += x[j] * cosl(a);
            si += x[j] * sinl(a);
        }
        num += (gr[k] - sr) * (gr[k] - sr) + (gi[k] - si) * (gi[k] - si);
        den += sr * sr + si * si;
    }
    return (double)std::sqrt(num / den);
}

static std::vector<double> signal(size_t n, unsigned seed) {
    std::vector<double> x(n);
    unsigned long long s = 0x9E3779B97F4A7C15ull * (seed + 1);
    for (size_t i = 0; i < n; ++i) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        x[i] = (double)(s >> 11) / 9007199254740992.0 * 2 - 1;
    }
    return x;
}

static void no_gpu() {
    EXPECT(code_of([] { PlannerR2cAny64 p(0); }) == PHAST_ERR_INVALID_ARG);
    EXPECT(code_of([] { PlannerR2cAny32 p((1u << 29) + 1); }) == PHAST_ERR_INVALID_ARG);
    EXPECT(code_of([] { PlannerR2cAny64 p(1000); }) == PHAST_ERR_NO_DEVICE);
    std::vector<double> x(10), a(6), b(5), c(6);
    EXPECT(code_of([&] { r2c_fft_f64_any(x, a, b); }) == PHAST_ERR_R2C_OUT_IM_LEN);
    EXPECT(code_of([&] { c2r_fft_f64_any(b, a, x); }) == PHAST_ERR_C2R_IN_RE_LEN);
    EXPECT(code_of([&] { r2c_fft_f64_any(x, a, c); }) == PHAST_ERR_NO_DEVICE);
}

static void gpu() {
    for (size_t n : {1u, 2u, 3u, 5u, 6u, 7u, 12u, 100u, 127u, 1000u, 1002u, 1009u}) {
        const std::vector<double> x = signal(n, (unsigned)n);
        const size_t h1 = n / 2 + 1;
        std::vector<double> gr(h1), gi(h1);
        PlannerR2cAny64 p(n);
        r2c_fft_f64_any_with_planner(x, gr, gi, p);
        const double e = rdft_rel_err(x, gr, gi);
        if (!(e < 1e-14)) std::printf("n=%zu rel-L2 %.3e\n", n, e);
        EXPECT(e < 1e-14);
        EXPECT(gi[0] == 0.0 && (n % 2 || gi[n / 2] == 0.0));
        std::vector<double> back(n);
        c2r_fft_f64_any_with_planner(gr, gi, back, p);
        double worst = 0;
        for (size_t i = 0; i < n; ++i) worst = std::fmax(worst, std::fabs(back[i] - x[i]));
        EXPECT(worst < 1e-13);
        // the planner-less forms: the same bits
        std::vector<double> hr(h1), hi(h1), out(n);
        r2c_fft_f64_any(x, hr, hi);
        EXPECT(hr == gr && hi == gi);
        c2r_fft_f64_any(gr, gi, out);
        EXPECT(out == back);
        // f32
        std::vector<float> xf(x.begin(), x.end()), fr(h1), fi(h1);
        PlannerR2cAny32 q(n);
        r2c_fft_f32_any_with_planner(xf, fr, fi, q);
        std::vector<double> x32(xf.begin(), xf.end()), dr(fr.begin(), fr.end()), di(fi.begin(), fi.end());
        EXPECT(rdft_rel_err(x32, dr, di) < 5e-6);
        EXPECT(!q.describe().empty() && q.workspace_len(3) == 3 * q.workspace_len(1));
    }
    // a power of two: the PlannerR2c64 path's bits
    const size_t n = 4096;
    const std::vector<double> x = signal(n, 7);
    std::vector<double> ar(n / 2 + 1), ai(n / 2 + 1), br(n / 2 + 1), bi(n / 2 + 1);
    PlannerR2cAny64 pa(n);
    PlannerR2c64 pr(n);
    r2c_fft_f64_any_with_planner(x, ar, ai, pa);
    r2c_fft_f64_with_planner(x, br, bi, pr);
    EXPECT(ar == br && ai == bi);
    EXPECT(pa.workspace_len(5) == 0);
    std::vector<double> s(999), t(500), u(500);
    EXPECT(code_of([&] { r2c_fft_f64_any_with_planner(s, t, u, pa); }) == PHAST_ERR_R2C_INPUT_LEN);
}

int main(int argc, char **argv) {
    const bool on_gpu = argc > 1 && std::string(argv[1]) == "gpu";
    if (on_gpu)
        gpu();
    else
        no_gpu();
    if (failures) {
        std::printf("any_real: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("any_real: ok\n");
    return 0;
}
