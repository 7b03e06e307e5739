// dct_test.cpp -- the C++ host side (include/phastft.hpp) of the DCT / DST of types II and III: PlannerDct64/32,
// dct_f64/f32[_with_planner], dst_f64/f32[_with_planner].  Built and run by tests/test_dct_cpu.py (no GPU: argument codes,
// compute fails loudly) and tests/test_gpu_dct.py (with "gpu": against a long-double O(N^2) sum, round trips, the
// planner-less forms' bits).
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

// the backward definitions of include/phastft_hip.h in long double, the angle reduced exactly (mod 4N)
static std::vector<long double> direct(bool dst, int type, const std::vector<double> &x) {
    const size_t n = x.size();
    const long double pi = 3.141592653589793238462643383279502884L;
    std::vector<long double> y(n);
    for (size_t k = 0; k < n; ++k) {
        long double s = 0;
        for (size_t j = 0; j < n; ++j) {
            const size_t a = type == 2 ? j : k, b = type == 2 ? k : j;  // II: x[j] at (k, j); III: x[j] at (j, k)
            const size_t p = dst ? ((b + 1) * (2 * a + 1)) % (4 * n) : (b * (2 * a + 1)) % (4 * n);
            const long double ang = pi * (long double)p / (long double)(2 * n);
            long double w = 2 * (dst ? sinl(ang) : cosl(ang));
            if (type == 3 && !dst && j == 0) w = 1;
            if (type == 3 && dst && j == n - 1) w = (k & 1) ? -1 : 1;
            s += x[j] * w;
        }
        y[k] = s;
    }
    return y;
}

static double rel_err(const std::vector<double> &got, const std::vector<long double> &want) {
    long double num = 0, den = 0;
    for (size_t i = 0; i < got.size(); ++i) {
        num += (got[i] - want[i]) * (got[i] - want[i]);
        den += want[i] * want[i];
    }
    return den > 0 ? (double)std::sqrt(num / den) : (double)std::sqrt(num);
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
    EXPECT(code_of([] { PlannerDct64 p(0); }) == PHAST_ERR_INVALID_ARG);
    EXPECT(code_of([] { PlannerDct32 p((1u << 29) + 1); }) == PHAST_ERR_INVALID_ARG);
    EXPECT(code_of([] { PlannerDct64 p(1000); }) == PHAST_ERR_NO_DEVICE);
    std::vector<double> x(10), y(9), z(10);
    EXPECT(code_of([&] { dct_f64(x, y); }) == PHAST_ERR_LEN_MISMATCH);
    EXPECT(code_of([&] { dst_f64(x, z, 4); }) == PHAST_ERR_INVALID_ARG);
    EXPECT(code_of([&] { dct_f64(x, z, 2, static_cast<Norm>(3)); }) == PHAST_ERR_INVALID_ARG);
    EXPECT(code_of([&] { dct_f64(x, z); }) == PHAST_ERR_NO_DEVICE);
}

static void gpu() {
    for (size_t n : {1u, 2u, 3u, 4u, 5u, 7u, 8u, 16u, 17u, 100u, 101u, 1000u, 1001u}) {
        const std::vector<double> x = signal(n, (unsigned)n);
        PlannerDct64 p(n);
        PlannerDct32 q(n);
        for (int dst = 0; dst < 2; ++dst)
            for (int type = 2; type <= 3; ++type) {
                std::vector<double> y(n), back(n), free_form(n);
                if (dst) dst_f64_with_planner(x, y, p, type);
                else dct_f64_with_planner(x, y, p, type);
                const double e = rel_err(y, direct(dst, type, x));
                if (!(e < 1e-14)) std::printf("n=%zu dst=%d type=%d rel-L2 %.3e\n", n, dst, type, e);
                EXPECT(e < 1e-14);
                if (dst) dst_f64(x, free_form, type);
                else dct_f64(x, free_form, type);
                EXPECT(free_form == y);  // the planner-less form: the same bits
                // the inverse: type 5 - t, norm forward; ortho is its own inverse pair
                if (dst) dst_f64_with_planner(y, back, p, 5 - type, Norm::Forward);
                else dct_f64_with_planner(y, back, p, 5 - type, Norm::Forward);
                double worst = 0;
                for (size_t i = 0; i < n; ++i) worst = std::fmax(worst, std::fabs(back[i] - x[i]));
                EXPECT(worst < 1e-13);
                std::vector<float> xf(x.begin(), x.end()), yf(n);
                if (dst) dst_f32_with_planner(xf, yf, q, type, Norm::Ortho);
                else dct_f32_with_planner(xf, yf, q, type, Norm::Ortho);
                std::vector<double> x32(xf.begin(), xf.end()), y32(yf.begin(), yf.end());
                std::vector<long double> want = direct(dst, type, x32);
                // ortho of the backward sum: the bin-0 fix (II after, III before -- III's x[0] term is linear in it)
                const long double f = 1.0L / std::sqrt((long double)(2 * n)), r2 = std::sqrt(2.0L);
                if (type == 3) {
                    const size_t j = dst ? n - 1 : 0;
                    std::vector<double> x2 = x32;
                    x2[j] *= (double)r2;
                    want = direct(dst, type, x2);
                }
                for (auto &w : want) w *= f;
                if (type == 2) want[dst ? n - 1 : 0] /= r2;
                EXPECT(rel_err(y32, want) < 5e-6);
            }
        EXPECT(!p.describe().empty() && p.workspace_len(3) > p.workspace_len(1));
    }
    PlannerDct64 pa(4096);
    std::vector<double> s(999), t(999);
    EXPECT(code_of([&] { dct_f64_with_planner(s, t, pa); }) == PHAST_ERR_PLANNER_SIZE);
}

int main(int argc, char **argv) {
    const bool on_gpu = argc > 1 && std::string(argv[1]) == "gpu";
    if (on_gpu)
        gpu();
    else
        no_gpu();
    if (failures) {
        std::printf("dct: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("dct: ok\n");
    return 0;
}
