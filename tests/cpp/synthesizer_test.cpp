// synthesizer_test.cpp -- the C++ host side (include/phastft.hpp) of the polyphase synthesis bank: PlannerSynthesizer64/32,
// synthesize_f64/f32_with_planner.  Built and run by tests/test_synthesizer_cpp_host.py: without a GPU the argument codes and a
// loud failure of the rest; with "gpu" the host forms against the definition of include/phastft_hip.h in long double, and the
// length codes.
#include <cmath>
#include <complex>
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

using ld = long double;
using cld = std::complex<ld>;
static const ld kTwoPi = 6.283185307179586476925286766559005768L;

template <typename T> static std::vector<T> uniform(size_t n, unsigned seed) {
    std::vector<T> x(n);
    unsigned long long s = 0x9E3779B97F4A7C15ull * (seed + 1);
    for (size_t i = 0; i < n; ++i) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        x[i] = (T)(float)(-1.0 + 2.0 * ((double)(s >> 11) / 9007199254740992.0));
    }
    return x;
}

// bin_gate: tests/tolerances.py's worst-bin gate at log2 <= 4 (64 eps 4, 2e-6 4), relative to the rms of a row of v.  Per
// output: (t + 3) u sum |tab v| + bin_gate sum_m |tab[n - m D]| rms(v[m]), as tests/synthesizer_reference.py
template <typename T, typename P, typename Call> static void on_gpu(const char *name, Call call, ld u, ld bin_gate) {
    const size_t F = 9, K = 21, M = 6, D = 4, first = 2, extra = 3;
    const std::vector<T> g = uniform<T>(K, 1);
    const size_t full = (F - 1) * D + K;
    for (int cplx = 0; cplx < 2; ++cplx) {
        const size_t bins = cplx ? M : M / 2 + 1;
        const std::vector<T> yr = uniform<T>(F * bins, 2), yi = uniform<T>(F * bins, 3);
        P whole(F, Slice<const T>(g.data(), K), M, D, 0, 0, cplx != 0), part(F, Slice<const T>(g.data(), K), M, D, first, full - first + extra, cplx != 0);
        EXPECT(whole.out_len() == full && whole.full_len() == full && part.out_len() == full - first + extra && whole.bins() == bins);
        EXPECT(whole.tile_samples() == 1024 && whole.per_thread() == 4 && whole.max_terms() == (K + D - 1) / D);
        EXPECT(whole.workspace_min() > 0 && whole.workspace_len(2) >= 2 * (whole.workspace_min() - 3) && whole.device_bytes() > K * sizeof(T));
        EXPECT(whole.describe().rfind(std::string("synthesizer ") + (cplx ? "complex" : "real") + " F=9 K=21 M=6 D=4 first=0", 0) == 0);
        std::vector<T> ar(full, T(7)), ai(ar), br(part.out_len(), T(7)), bi(br);
        const Slice<const T> sr(yr.data(), yr.size()), si(yi.data(), yi.size());
        call(sr, si, Slice<T>(ar.data(), full), Slice<T>(cplx ? ai.data() : nullptr, cplx ? full : 0), whole);
        call(sr, si, Slice<T>(br.data(), br.size()), Slice<T>(cplx ? bi.data() : nullptr, cplx ? bi.size() : 0), part);
        // v[m][p] = (1 / M) sum_k Y[m][k] exp(2 pi i k p / M), the real case by irfft's rules
        std::vector<cld> v(F * M);
        std::vector<ld> rms(F, 0);
        for (size_t m = 0; m < F; ++m)
            for (size_t p = 0; p < M; ++p) {
                cld sum = 0;
                for (size_t k = 0; k < M; ++k) {
                    cld y;
                    if (cplx) y = cld((ld)yr[m * bins + k], (ld)yi[m * bins + k]);
                    else {
                        const size_t kk = k <= M / 2 ? k : M - k;
                        const bool edge = kk == 0 || 2 * kk == M;
                        y = cld((ld)yr[m * bins + kk], edge ? (ld)0 : (k <= M / 2 ? (ld)yi[m * bins + kk] : -(ld)yi[m * bins + kk]));
                    }
                    const ld ph = kTwoPi * (ld)((k * p) % M) / (ld)M;
                    sum += y * cld(std::cos(ph), std::sin(ph));
                }
                v[m * M + p] = sum / (ld)M;
                rms[m] += std::norm(v[m * M + p]) / (ld)M;
            }
        ld worst = 0;
        for (size_t n = 0; n < full; ++n) {
            cld want = 0;
            ld a = 0, b = 0;
            size_t t = 0;
            for (size_t m = 0; m < F; ++m) {
                const long long j = (long long)n - (long long)(m * D);
                if (j < 0 || j >= (long long)K) continue;
                const ld tab = (ld)(T)((double)g[j] * (double)M);
                want += tab * v[m * M + n % M];
                a += std::fabs(tab) * std::abs(v[m * M + n % M]);
                b += std::fabs(tab) * std::sqrt(rms[m]);
                ++t;
            }
            const ld gate = (ld)(t + 3) * u * a + bin_gate * b;
            const ld err = std::max(std::fabs((ld)ar[n] - want.real()), cplx ? std::fabs((ld)ai[n] - want.imag()) : (ld)0);
            EXPECT(err <= gate);
            if (gate > 0) worst = std::max(worst, err / gate);
            if (n >= first) EXPECT(br[n - first] == ar[n] && (!cplx || bi[n - first] == ai[n]));  // the same bits through the window
        }
        for (size_t e = full - first; e < br.size(); ++e) EXPECT(br[e] == T(0) && (!cplx || bi[e] == T(0)));  // zeros beyond full_len
        std::printf("%s synthesize %s: worst output %.3Lf of its gate\n", name, cplx ? "complex" : "real", worst);
        std::vector<T> shorter(full - 1), fewer(F * bins - 1);
        const Slice<T> oi(cplx ? ai.data() : nullptr, cplx ? full : 0);
        EXPECT(code_of([&] { call(Slice<const T>(fewer.data(), fewer.size()), Slice<const T>(fewer.data(), fewer.size()), Slice<T>(ar.data(), full), oi,
                                  whole); }) == PHAST_ERR_PLANNER_SIZE);
        EXPECT(code_of([&] { call(sr, si, Slice<T>(shorter.data(), shorter.size()), Slice<T>(cplx ? ai.data() : nullptr, cplx ? shorter.size() : 0),
                                  whole); }) == PHAST_ERR_LEN_MISMATCH);
        EXPECT(code_of([&] { call(sr, si, Slice<T>(ar.data(), full), Slice<T>(cplx ? nullptr : ai.data(), cplx ? 0 : full), whole); }) ==
               PHAST_ERR_INVALID_ARG);  // the wrong planes
    }
}

template <typename T, typename P> static void argument_codes() {
    const std::vector<T> g = {T(1), T(2), T(3)};
    auto make = [&](size_t frames, size_t k, size_t m, size_t d, size_t first, size_t out_len) {
        return code_of([&] { P pl(frames, Slice<const T>(g.data(), k), m, d, first, out_len); });
    };
    EXPECT(make(0, 3, 4, 4, 0, 0) == PHAST_ERR_INVALID_ARG);
    EXPECT(make(10, 0, 4, 4, 0, 0) == PHAST_ERR_INVALID_ARG);
    EXPECT(make(10, 3, (1u << 29) + 1, 4, 0, 0) == PHAST_ERR_INVALID_ARG);
    EXPECT(make(10, 3, 4, (1u << 29) + 1, 0, 0) == PHAST_ERR_INVALID_ARG);
    EXPECT(make(10, 3, 4, 4, 40, 1) == PHAST_ERR_INVALID_ARG);  // full_len is 39
    EXPECT(make(10, 3, 4, 4, 39, 0) == PHAST_ERR_INVALID_ARG);  // nothing left
    EXPECT(make(2048, 3, 1u << 20, 4, 0, 0) == PHAST_ERR_INVALID_ARG);  // frames x channels > 2^30
    EXPECT(make(10, 3, 4, 4, 0, (1u << 30) + 1) == PHAST_ERR_INVALID_ARG);
    EXPECT(code_of([&] { P pl(10, Slice<const T>(nullptr, 3), 4); }) == PHAST_ERR_INVALID_ARG);
}

int main(int argc, char **argv) {
    const bool gpu = argc > 1 && std::string(argv[1]) == "gpu";
    argument_codes<double, PlannerSynthesizer64>();
    argument_codes<float, PlannerSynthesizer32>();
    if (gpu) {
        on_gpu<double, PlannerSynthesizer64>("f64", [](const auto &...a) { synthesize_f64_with_planner(a...); }, std::ldexp((ld)1, -53), 5.7e-14L);
        on_gpu<float, PlannerSynthesizer32>("f32", [](const auto &...a) { synthesize_f32_with_planner(a...); }, std::ldexp((ld)1, -24), 8e-6L);
    } else {
        const std::vector<double> g = {1.0, 2.0, 3.0};
        const std::vector<float> gf = {1.0f, 2.0f, 3.0f};
        // a good call gets past the checks and fails loudly
        EXPECT(code_of([&] { PlannerSynthesizer64 pl(10, Slice<const double>(g.data(), 3), 4); }) == PHAST_ERR_NO_DEVICE);
        EXPECT(code_of([&] { PlannerSynthesizer32 pl(10, Slice<const float>(gf.data(), 3), 4, 2, 0, 0, true); }) == PHAST_ERR_NO_DEVICE);
    }
    std::printf("synthesizer: %s (%d failures)\n", failures ? "FAILED" : "ok", failures);
    return failures ? 1 : 0;
}
