// conv_test.cpp -- the C++ host side (include/phastft.hpp) of overlap-save convolution: PlannerConv64/32,
// conv_f64/f32_with_planner.  Built and run by tests/test_conv_cpu.py (no GPU: argument codes, compute fails loudly) and
// tests/test_gpu_conv.py (with "gpu": the host forms against the direct sum in long double for every mode, convolution and
// correlation, power-of-two, Bluestein and automatic blocks; the length codes).
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

static std::vector<double> uniform(size_t n, unsigned seed) {
    std::vector<double> x(n);
    unsigned long long s = 0x9E3779B97F4A7C15ull * (seed + 1);
    for (size_t i = 0; i < n; ++i) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        x[i] = (double)(s >> 11) / 9007199254740992.0 * 2 - 1;
    }
    return x;
}

// the definition of include/phastft_hip.h in long double
template <typename T>
static std::vector<long double> direct(const std::vector<T> &x, const std::vector<T> &h, ConvMode mode, bool flip) {
    const long long len = (long long)x.size(), k = (long long)h.size();
    const long long t0 = mode == ConvMode::Full ? 0 : mode == ConvMode::Same ? (k - 1) / 2 : k - 1;
    const long long n = mode == ConvMode::Full ? len + k - 1 : mode == ConvMode::Same ? len : len - k + 1;
    std::vector<long double> out((size_t)n, 0);
    for (long long i = 0; i < n; ++i)
        for (long long j = 0; j < k; ++j) {
            const long long t = t0 + i - j;
            if (t >= 0 && t < len) out[(size_t)i] += (long double)h[(size_t)(flip ? k - 1 - j : j)] * (long double)x[(size_t)t];
        }
    return out;
}

template <typename T> static double rel_err(const std::vector<T> &got, const std::vector<long double> &want) {
    long double num = 0, den = 0;
    for (size_t i = 0; i < got.size(); ++i) {
        num += (got[i] - want[i]) * (got[i] - want[i]);
        den += want[i] * want[i];
    }
    return den > 0 ? (double)std::sqrt(num / den) : (double)std::sqrt(num);
}

static void no_gpu() {
    const std::vector<double> h(16, 0.25);
    EXPECT(code_of([&] { PlannerConv64 p(15, h, ConvMode::Valid); }) == PHAST_ERR_INVALID_ARG);  // valid with L < K
    EXPECT(code_of([&] { PlannerConv64 p(100, h, ConvMode::Full, false, 15); }) == PHAST_ERR_INVALID_ARG);  // B < K
    EXPECT(code_of([&] { PlannerConv64 p(100, std::vector<double>()); }) == PHAST_ERR_INVALID_ARG);  // no taps
    EXPECT(code_of([&] { PlannerConv64 p(0, h); }) == PHAST_ERR_INVALID_ARG);
    EXPECT(code_of([&] { PlannerConv64 p((1u << 29) + 1, h, ConvMode::Same); }) == PHAST_ERR_INVALID_ARG);
    EXPECT(code_of([&] { PlannerConv64 p(1u << 29, h, ConvMode::Full, false, 1u << 20); }) == PHAST_ERR_INVALID_ARG);  // out_len > 2^29
    EXPECT(code_of([&] { PlannerConv64 p(1u << 29, h, ConvMode::Same, false, 16); }) == PHAST_ERR_INVALID_ARG);  // segments * B > 2^30
    EXPECT(code_of([&] { PlannerConv32 p(100, std::vector<float>(16, 1.f), static_cast<ConvMode>(3)); }) == PHAST_ERR_INVALID_ARG);
    EXPECT(code_of([&] { PlannerConv64 p(100, h); }) == PHAST_ERR_NO_DEVICE);
    EXPECT(code_of([&] { PlannerConv32 p(15, std::vector<float>(16, 1.f), ConvMode::Same, true, 17); }) == PHAST_ERR_NO_DEVICE);
}

static void gpu() {
    struct Case {
        size_t len, k, block;
    };
    for (const Case &c : {Case{1, 1, 1}, Case{37, 1, 8}, Case{64, 5, 8}, Case{100, 17, 17}, Case{101, 7, 16}, Case{10, 30, 64},
                          Case{300, 33, 100}, Case{700, 64, 256}, Case{700, 40, 0}})
        for (ConvMode mode : {ConvMode::Full, ConvMode::Same, ConvMode::Valid})
            for (int flip = 0; flip < 2; ++flip) {
                if (mode == ConvMode::Valid && c.len < c.k) {
                    EXPECT(code_of([&] { PlannerConv64 p(c.len, uniform(c.k, 1), mode); }) == PHAST_ERR_INVALID_ARG);
                    continue;
                }
                const std::vector<double> x = uniform(c.len, (unsigned)(c.len + c.k)), h = uniform(c.k, (unsigned)c.k);
                PlannerConv64 p(c.len, h, mode, flip != 0, c.block);
                const std::vector<long double> want = direct(x, h, mode, flip != 0);
                EXPECT(p.out_len() == want.size() && p.block() >= c.k && (c.block == 0 || p.block() == c.block));
                EXPECT(p.segments() == (p.out_len() + p.block() - c.k) / (p.block() - c.k + 1));
                std::vector<double> out(want.size(), 5.0);
                conv_f64_with_planner(x, out, p);
                const double e = rel_err(out, want);
                if (!(e < 1e-14)) std::printf("L=%zu K=%zu B=%zu mode=%d flip=%d rel-L2 %.3e\n", c.len, c.k, p.block(), (int)mode, flip, e);
                EXPECT(e < 1e-14);
                const std::vector<float> xf(x.begin(), x.end()), hf(h.begin(), h.end());
                PlannerConv32 q(c.len, hf, mode, flip != 0, c.block);
                std::vector<float> of(want.size(), 5.0f);
                conv_f32_with_planner(xf, of, q);
                EXPECT(rel_err(of, direct(xf, hf, mode, flip != 0)) < 5e-6);
                EXPECT(!p.describe().empty() && p.device_bytes() > 0 && p.workspace_len(3) > p.workspace_len(1) &&
                       p.workspace_len(1) >= p.workspace_min());
            }
    const std::vector<double> h = uniform(16, 3), x = uniform(400, 7), shorter(399);
    PlannerConv64 p(400, h, ConvMode::Same);
    std::vector<double> out(400), few(399);
    EXPECT(code_of([&] { conv_f64_with_planner(shorter, out, p); }) == PHAST_ERR_PLANNER_SIZE);
    EXPECT(code_of([&] { conv_f64_with_planner(x, few, p); }) == PHAST_ERR_LEN_MISMATCH);
    EXPECT(code_of([&] { conv_f64_with_planner(x, Slice<double>(nullptr, 400), p); }) == PHAST_ERR_INVALID_ARG);
}

int main(int argc, char **argv) {
    const bool on_gpu = argc > 1 && std::string(argv[1]) == "gpu";
    if (on_gpu)
        gpu();
    else
        no_gpu();
    if (failures) {
        std::printf("conv: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("conv: ok\n");
    return 0;
}
