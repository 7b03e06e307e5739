// convnd_test.cpp -- the C++ host side (include/phastft.hpp) of N-d overlap-save convolution: PlannerConvNd64/32,
// convnd_f64/f32_with_planner.  Built and run by tests/test_convnd_cpu.py (no GPU: argument codes, compute fails loudly) and
// tests/test_gpu_convnd.py (with "gpu": the host forms against the direct sum in long double for every mode, convolution and
// correlation, at rank 1, 2 and 3; the length codes).
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "phastft.hpp"

using namespace phastft;
using Shape = std::vector<size_t>;

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

static size_t prod(const Shape &s) {
    size_t p = 1;
    for (size_t v : s) p *= v;
    return p;
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

// the shapes padded in front to rank 3
static void pad3(const Shape &s, long long *d) {
    for (int i = 0; i < 3; ++i) d[i] = 1;
    for (size_t i = 0; i < s.size(); ++i) d[3 - s.size() + i] = (long long)s[i];
}

// the definition of include/phastft_hip.h in long double
template <typename T>
static std::vector<long double> direct(const std::vector<T> &x, const Shape &ls, const std::vector<T> &h, const Shape &ks, ConvMode mode,
                                       bool flip, Shape *out_shape) {
    long long L[3], K[3], t0[3], n[3];
    pad3(ls, L);
    pad3(ks, K);
    for (int i = 0; i < 3; ++i) {
        t0[i] = mode == ConvMode::Full ? 0 : mode == ConvMode::Same ? (K[i] - 1) / 2 : K[i] - 1;
        n[i] = mode == ConvMode::Full ? L[i] + K[i] - 1 : mode == ConvMode::Same ? L[i] : L[i] - K[i] + 1;
    }
    out_shape->clear();
    for (size_t i = 3 - ls.size(); i < 3; ++i) out_shape->push_back((size_t)n[i]);
    std::vector<long double> out((size_t)(n[0] * n[1] * n[2]), 0);
    for (long long i0 = 0; i0 < n[0]; ++i0)
        for (long long i1 = 0; i1 < n[1]; ++i1)
            for (long long i2 = 0; i2 < n[2]; ++i2) {
                long double acc = 0;
                for (long long j0 = 0; j0 < K[0]; ++j0)
                    for (long long j1 = 0; j1 < K[1]; ++j1)
                        for (long long j2 = 0; j2 < K[2]; ++j2) {
                            const long long a = t0[0] + i0 - j0, b = t0[1] + i1 - j1, c = t0[2] + i2 - j2;
                            if (a < 0 || a >= L[0] || b < 0 || b >= L[1] || c < 0 || c >= L[2]) continue;
                            const long long g = flip ? ((K[0] - 1 - j0) * K[1] + (K[1] - 1 - j1)) * K[2] + (K[2] - 1 - j2)
                                                     : (j0 * K[1] + j1) * K[2] + j2;
                            acc += (long double)h[(size_t)g] * (long double)x[(size_t)((a * L[1] + b) * L[2] + c)];
                        }
                out[(size_t)((i0 * n[1] + i1) * n[2] + i2)] = acc;
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
    const std::vector<double> h(12, 0.25);
    const Shape k{3, 4};
    EXPECT(code_of([&] { PlannerConvNd64 p({9, 3}, k, h, ConvMode::Valid); }) == PHAST_ERR_INVALID_ARG);  // valid with L_1 < K_1 only
    EXPECT(code_of([&] { PlannerConvNd64 p({9, 7}, k, h, ConvMode::Full, false, {4, 3}); }) == PHAST_ERR_INVALID_ARG);  // B_1 < K_1
    EXPECT(code_of([&] { PlannerConvNd64 p({9, 7}, k, h, ConvMode::Full, false, {4}); }) == PHAST_ERR_INVALID_ARG);     // one block for two axes
    EXPECT(code_of([&] { PlannerConvNd64 p({9, 7}, {3}, h); }) == PHAST_ERR_INVALID_ARG);                               // ranks differ
    EXPECT(code_of([&] { PlannerConvNd64 p({9, 7}, k, std::vector<double>(11)); }) == PHAST_ERR_INVALID_ARG);           // 11 taps for 3 x 4
    EXPECT(code_of([&] { PlannerConvNd64 p({}, {}, h); }) == PHAST_ERR_INVALID_ARG);                                    // rank 0
    EXPECT(code_of([&] { PlannerConvNd64 p({2, 2, 2, 2}, {1, 1, 3, 4}, h); }) == PHAST_ERR_INVALID_ARG);                // rank 4
    EXPECT(code_of([&] { PlannerConvNd64 p({9, 0}, k, h); }) == PHAST_ERR_INVALID_ARG);                                 // a zero dimension
    EXPECT(code_of([&] { PlannerConvNd64 p({9, 7}, k, h, ConvMode::Same, false, {1u << 15, 1u << 14}); }) == PHAST_ERR_INVALID_ARG);  // prod B > 2^28
    EXPECT(code_of([&] { PlannerConvNd32 p({9, 7}, k, std::vector<float>(12, 1.f), static_cast<ConvMode>(3)); }) == PHAST_ERR_INVALID_ARG);
    EXPECT(code_of([&] { PlannerConvNd64 p({9, 7}, k, h); }) == PHAST_ERR_NO_DEVICE);
    EXPECT(code_of([&] { PlannerConvNd32 p({5, 6}, {7, 9}, std::vector<float>(63, 1.f), ConvMode::Same, true, {8, 16}); }) == PHAST_ERR_NO_DEVICE);
}

static void gpu() {
    struct Case {
        Shape len, k, block;
    };
    for (const Case &c : {Case{{1, 1}, {1, 1}, {}}, Case{{9, 7}, {3, 4}, {4, 4}}, Case{{12, 10}, {1, 4}, {1, 8}}, Case{{5, 6}, {7, 9}, {8, 16}},
                          Case{{10, 11}, {4, 5}, {6, 17}}, Case{{40, 50}, {9, 9}, {0, 0}}, Case{{6, 5, 7}, {2, 3, 2}, {4, 4, 4}},
                          Case{{200}, {33}, {100}}})
        for (ConvMode mode : {ConvMode::Full, ConvMode::Same, ConvMode::Valid})
            for (int flip = 0; flip < 2; ++flip) {
                bool has = true;
                for (size_t i = 0; i < c.len.size(); ++i) has = has && (mode != ConvMode::Valid || c.len[i] >= c.k[i]);
                const std::vector<double> x = uniform(prod(c.len), (unsigned)prod(c.len)), h = uniform(prod(c.k), (unsigned)prod(c.k));
                if (!has) {
                    EXPECT(code_of([&] { PlannerConvNd64 p(c.len, c.k, h, mode); }) == PHAST_ERR_INVALID_ARG);
                    continue;
                }
                PlannerConvNd64 p(c.len, c.k, h, mode, flip != 0, c.block);
                Shape want_shape;
                const std::vector<long double> want = direct(x, c.len, h, c.k, mode, flip != 0, &want_shape);
                EXPECT(p.out_len() == want.size() && p.out_shape() == want_shape && p.tiles() >= 1);
                const Shape b = p.block();
                for (size_t i = 0; i < b.size(); ++i) EXPECT(b[i] >= c.k[i] && (c.block.empty() || c.block[i] == 0 || b[i] == c.block[i]));
                std::vector<double> out(want.size(), 5.0);
                convnd_f64_with_planner(x, out, p);
                const double e = rel_err(out, want);
                if (!(e < 1e-14)) std::printf("%s: rel-L2 %.3e\n", p.describe().c_str(), e);
                EXPECT(e < 1e-14);
                const std::vector<float> xf(x.begin(), x.end()), hf(h.begin(), h.end());
                PlannerConvNd32 q(c.len, c.k, hf, mode, flip != 0, c.block);
                std::vector<float> of(want.size(), 5.0f);
                convnd_f32_with_planner(xf, of, q);
                Shape s32;
                EXPECT(rel_err(of, direct(xf, c.len, hf, c.k, mode, flip != 0, &s32)) < 5e-6);
                EXPECT(!p.describe().empty() && p.device_bytes() > 0 && p.workspace_len(3) > p.workspace_len(1) &&
                       p.workspace_len(1) >= p.workspace_min());
            }
    const std::vector<double> h = uniform(12, 3), x = uniform(20 * 13, 7), shorter(20 * 13 - 1);
    PlannerConvNd64 p({20, 13}, {3, 4}, h, ConvMode::Same);
    std::vector<double> out(20 * 13), few(20 * 13 - 1);
    EXPECT(code_of([&] { convnd_f64_with_planner(shorter, out, p); }) == PHAST_ERR_PLANNER_SIZE);
    EXPECT(code_of([&] { convnd_f64_with_planner(x, few, p); }) == PHAST_ERR_LEN_MISMATCH);
    EXPECT(code_of([&] { convnd_f64_with_planner(x, Slice<double>(nullptr, 20 * 13), p); }) == PHAST_ERR_INVALID_ARG);
}

int main(int argc, char **argv) {
    const bool on_gpu = argc > 1 && std::string(argv[1]) == "gpu";
    if (on_gpu)
        gpu();
    else
        no_gpu();
    if (failures) {
        std::printf("convnd: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("convnd: ok\n");
    return 0;
}
