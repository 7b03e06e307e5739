// czt_test.cpp -- the C++ host side (include/phastft.hpp) of the chirp-Z transform: PlannerCzt64/32, czt_64/32[_with_planner].
// Built and run by tests/test_czt_cpu.py (no GPU: argument codes, compute fails loudly) and tests/test_gpu_czt.py (with "gpu":
// the host forms against the direct sum in long double, complex and real signals, M > N and M < N; the length codes).
#include <cmath>
#include <cstdio>
#include <limits>
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

template <typename T> static std::vector<T> uniform(size_t n, unsigned seed) {
    std::vector<T> x(n);
    unsigned long long s = 0x9E3779B97F4A7C15ull * (seed + 1);
    for (size_t i = 0; i < n; ++i) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        x[i] = (T)((double)(s >> 11) / 9007199254740992.0 * 2 - 1);
    }
    return x;
}

// the definition of include/phastft_hip.h in long double; the phase n (start + k step) is reduced mod 1 before the product
// with 2 pi (n k < 2^20 here and step and start have few bits, so the products are exact in long double)
template <typename T>
static double rel_err(const std::vector<T> &xr, const std::vector<T> *xi, const std::vector<T> &got_re, const std::vector<T> &got_im,
                      double step, double start) {
    const long double two_pi = 8 * std::atan((long double)1);
    long double num = 0, den = 0;
    for (size_t k = 0; k < got_re.size(); ++k) {
        long double re = 0, im = 0;
        for (size_t n = 0; n < xr.size(); ++n) {
            long double t = (long double)n * (long double)start + (long double)(n * k) * (long double)step;
            t -= std::floor(t);
            const long double c = std::cos(two_pi * t), s = -std::sin(two_pi * t);
            const long double a = xr[n], b = xi ? (long double)(*xi)[n] : 0;
            re += a * c - b * s;
            im += a * s + b * c;
        }
        num += (got_re[k] - re) * (got_re[k] - re) + (got_im[k] - im) * (got_im[k] - im);
        den += re * re + im * im;
    }
    return den > 0 ? (double)std::sqrt(num / den) : (double)std::sqrt(num);
}

static void no_gpu() {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    EXPECT(code_of([&] { PlannerCzt64 p(0, 8, 0.01); }) == PHAST_ERR_INVALID_ARG);
    EXPECT(code_of([&] { PlannerCzt64 p(8, 0, 0.01); }) == PHAST_ERR_INVALID_ARG);
    EXPECT(code_of([&] { PlannerCzt32 p((size_t)1 << 30, 2, 0.01); }) == PHAST_ERR_INVALID_ARG);  // N + M - 1 > 2^30
    EXPECT(code_of([&] { PlannerCzt64 p(8, 8, nan); }) == PHAST_ERR_INVALID_ARG);
    EXPECT(code_of([&] { PlannerCzt32 p(8, 8, 0.01, -inf); }) == PHAST_ERR_INVALID_ARG);
    EXPECT(code_of([&] { PlannerCzt64 p(100, 29, 0.0037, 0.25); }) == PHAST_ERR_NO_DEVICE);
    EXPECT(code_of([&] { PlannerCzt32 p(1, 1, -0.5); }) == PHAST_ERR_NO_DEVICE);
    std::vector<double> x(16), y(15), o_re(8), o_im(8), few(7);
    EXPECT(code_of([&] { czt_64(x, y, o_re, o_im, 0.01); }) == PHAST_ERR_LEN_MISMATCH);
    EXPECT(code_of([&] { czt_64(x, Slice<const double>(nullptr, 0), o_re, few, 0.01); }) == PHAST_ERR_LEN_MISMATCH);
    EXPECT(code_of([&] { czt_64(x, Slice<const double>(nullptr, 0), o_re, o_im, nan); }) == PHAST_ERR_INVALID_ARG);
    EXPECT(code_of([&] { czt_64(x, Slice<const double>(nullptr, 0), o_re, o_im, 0.01); }) == PHAST_ERR_NO_DEVICE);
}

static void gpu() {
    struct Case {
        size_t n, m;
        double step, start;
    };
    const double eighth = 0.125;
    for (const Case &c : {Case{1, 1, 0.25, 0.5}, Case{1, 5, 0.125, 0.25}, Case{5, 1, 0.125, 0.25}, Case{37, 101, 1.0 / 4096, eighth},
                          Case{101, 37, 3.0 / 1024, -0.375}, Case{100, 29, -5.0 / 2048, 0.0}, Case{100, 30, 1.0 / 128, 0.75},
                          Case{64, 64, 1.0 / 64, 0.0}, Case{700, 300, 7.0 / 8192, 0.3125}})
        for (int real = 0; real < 2; ++real) {
            const std::vector<double> xr = uniform<double>(c.n, (unsigned)(c.n + c.m)), xi = uniform<double>(c.n, (unsigned)(c.n * 3 + 1));
            const Slice<const double> none(nullptr, 0);
            PlannerCzt64 p(c.n, c.m, c.step, c.start);
            EXPECT(p.input_len() == c.n && p.output_len() == c.m && p.conv_len() >= c.n + c.m - 1 && p.conv_len() >= 8 &&
                   (p.conv_len() & (p.conv_len() - 1)) == 0 && p.workspace_len(3) == 6 * p.conv_len());
            EXPECT(!p.describe().empty() && p.device_bytes() > 0);
            std::vector<double> o_re(c.m, 5.0), o_im(c.m, 5.0), q_re(c.m, 6.0), q_im(c.m, 6.0);
            if (real) {
                czt_64_with_planner(xr, none, o_re, o_im, p);
                czt_64(xr, none, q_re, q_im, c.step, c.start);
            } else {
                czt_64_with_planner(xr, xi, o_re, o_im, p);
                czt_64(xr, xi, q_re, q_im, c.step, c.start);
            }
            EXPECT(o_re == q_re && o_im == q_im);  // the one-shot form builds the same planner
            const double e = rel_err(xr, real ? nullptr : &xi, o_re, o_im, c.step, c.start);
            if (!(e < 1e-14)) std::printf("N=%zu M=%zu real=%d rel-L2 %.3e\n", c.n, c.m, real, e);
            EXPECT(e < 1e-14);
            const std::vector<float> fr(xr.begin(), xr.end()), fi(xi.begin(), xi.end());
            PlannerCzt32 q(c.n, c.m, c.step, c.start);
            std::vector<float> f_re(c.m, 5.0f), f_im(c.m, 5.0f);
            if (real)
                czt_32_with_planner(fr, Slice<const float>(nullptr, 0), f_re, f_im, q);
            else
                czt_32_with_planner(fr, fi, f_re, f_im, q);
            const double ef = rel_err(fr, real ? nullptr : &fi, f_re, f_im, c.step, c.start);
            if (!(ef < 5e-6)) std::printf("N=%zu M=%zu real=%d f32 rel-L2 %.3e\n", c.n, c.m, real, ef);
            EXPECT(ef < 5e-6);
        }
    PlannerCzt64 p(400, 50, 0.001, 0.1);
    const std::vector<double> x = uniform<double>(400, 7), shorter(399);
    std::vector<double> o_re(50), o_im(50), more(51), more2(51);
    EXPECT(code_of([&] { czt_64_with_planner(shorter, shorter, o_re, o_im, p); }) == PHAST_ERR_PLANNER_SIZE);
    EXPECT(code_of([&] { czt_64_with_planner(x, x, more, more2, p); }) == PHAST_ERR_PLANNER_SIZE);
    EXPECT(code_of([&] { czt_64_with_planner(x, x, o_re, more, p); }) == PHAST_ERR_LEN_MISMATCH);
    EXPECT(code_of([&] { czt_64_with_planner(x, x, Slice<double>(nullptr, 50), o_im, p); }) == PHAST_ERR_INVALID_ARG);
}

int main(int argc, char **argv) {
    const bool on_gpu = argc > 1 && std::string(argv[1]) == "gpu";
    if (on_gpu)
        gpu();
    else
        no_gpu();
    if (failures) {
        std::printf("czt: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("czt: ok\n");
    return 0;
}
