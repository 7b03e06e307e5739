// channelizer_test.cpp -- the C++ host side (include/phastft.hpp) of the polyphase channelizer: PlannerChannelizer64/32,
// channelize_f64/f32_with_planner.  Built and run by tests/test_channelizer_cpp_host.py: without a GPU the argument codes and a
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

// y[m][k] = sum_n h[m D - n] x[n] exp(-2 pi i k n / M) and sum |h x| over the frame, in long double
template <typename T>
static std::complex<ld> chan_def(const std::vector<T> &h, const std::vector<T> &xr, const std::vector<T> &xi, size_t M, size_t D, size_t m,
                                 size_t k, ld *scale) {
    std::complex<ld> sum = 0;
    *scale = 0;
    for (size_t n = 0; n < xr.size(); ++n) {
        const long long i = (long long)(m * D) - (long long)n;
        if (i < 0 || i >= (long long)h.size()) continue;
        const std::complex<ld> t = (ld)h[i] * std::complex<ld>((ld)xr[n], xi.empty() ? (ld)0 : (ld)xi[n]);
        const ld ph = -kTwoPi * (ld)((k * n) % M) / (ld)M;
        sum += t * std::complex<ld>(std::cos(ph), std::sin(ph));
        *scale += std::abs(t);
    }
    return sum;
}

// bin_gate: tests/tolerances.py's worst-bin gate at log2 M <= 4 (64 eps 4, 2e-6 4), relative to the rms bin
template <typename T, typename P, typename Call> static void on_gpu(const char *name, Call call, ld u, ld bin_gate) {
    const size_t L = 50, K = 21, M = 6, D = 4, first = 2, extra = 3, t = (K + M - 1) / M;
    const std::vector<T> h = uniform<T>(K, 1), xr = uniform<T>(L, 2), xi = uniform<T>(L, 3), none;
    const size_t full = (L + K - 2) / D + 1;
    for (int cplx = 0; cplx < 2; ++cplx) {
        const size_t bins = cplx ? M : M / 2 + 1;
        P whole(L, Slice<const T>(h.data(), K), M, D, 0, 0, cplx != 0), part(L, Slice<const T>(h.data(), K), M, D, first, full - first + extra, cplx != 0);
        EXPECT(whole.out_frames() == full && whole.full_frames() == full && part.out_frames() == full - first + extra && whole.bins() == bins);
        EXPECT(whole.tile_cols() == M && whole.tile_frames() == 168 && whole.chunk() == t && whole.periods() == 117);
        EXPECT(whole.workspace_min() > 0 && whole.workspace_len(2) >= whole.workspace_min() && whole.device_bytes() > t * M * sizeof(T));
        EXPECT(whole.describe().rfind(std::string("channelizer ") + (cplx ? "complex" : "real") + " L=50 K=21 M=6 D=4 first=0", 0) == 0);
        std::vector<T> ar(full * bins, T(7)), ai(ar), br(part.out_frames() * bins, T(7)), bi(br);
        const Slice<const T> sr(xr.data(), L), si(cplx ? xi.data() : nullptr, cplx ? L : 0);
        call(sr, si, Slice<T>(ar.data(), ar.size()), Slice<T>(ai.data(), ai.size()), whole);
        call(sr, si, Slice<T>(br.data(), br.size()), Slice<T>(bi.data(), bi.size()), part);
        ld worst = 0, rms = 0, fold = 0;
        std::vector<std::complex<ld>> want(full * bins);
        for (size_t m = 0; m < full; ++m)
            for (size_t k = 0; k < bins; ++k) {
                ld scale;
                want[m * bins + k] = chan_def(h, xr, cplx ? xi : none, M, D, m, k, &scale);
                rms += std::norm(want[m * bins + k]);
                fold = std::max(fold, scale);  // sum_p A[m][p]: every product of the frame
            }
        rms = std::sqrt(rms / (ld)(full * bins));
        for (size_t e = 0; e < full * bins; ++e) {
            worst = std::max(worst, std::max(std::fabs((ld)ar[e] - want[e].real()), std::fabs((ld)ai[e] - want[e].imag())));
            if (e >= first * bins) EXPECT(br[e - first * bins] == ar[e] && bi[e - first * bins] == ai[e]);  // the same bits through the window
        }
        for (size_t e = (full - first) * bins; e < br.size(); ++e) EXPECT(br[e] == T(0) && bi[e] == T(0));  // zeros beyond full_frames
        const ld gate = bin_gate + (ld)(t + 2) * u * fold / rms;
        std::printf("%s channelize %s: %.3Le of the rms, gate %.3Le\n", name, cplx ? "complex" : "real", worst / rms, gate);
        EXPECT(worst <= gate * rms);
        std::vector<T> shorter(full * bins - 1), fewer(L - 1);
        EXPECT(code_of([&] { call(Slice<const T>(fewer.data(), L - 1), Slice<const T>(cplx ? fewer.data() : nullptr, cplx ? L - 1 : 0),
                                  Slice<T>(ar.data(), ar.size()), Slice<T>(ai.data(), ai.size()), whole); }) == PHAST_ERR_PLANNER_SIZE);
        EXPECT(code_of([&] { call(sr, si, Slice<T>(shorter.data(), shorter.size()), Slice<T>(ai.data(), shorter.size()), whole); }) == PHAST_ERR_LEN_MISMATCH);
        EXPECT(code_of([&] { call(sr, Slice<const T>(cplx ? nullptr : xi.data(), cplx ? 0 : L), Slice<T>(ar.data(), ar.size()),
                                  Slice<T>(ai.data(), ai.size()), whole); }) == PHAST_ERR_INVALID_ARG);  // the wrong planes
    }
}

template <typename T, typename P> static void argument_codes() {
    const std::vector<T> h = {T(1), T(2), T(3)};
    auto make = [&](size_t len, size_t k, size_t m, size_t d, size_t first, size_t out_frames) {
        return code_of([&] { P pl(len, Slice<const T>(h.data(), k), m, d, first, out_frames); });
    };
    EXPECT(make(0, 3, 4, 4, 0, 0) == PHAST_ERR_INVALID_ARG);
    EXPECT(make(10, 0, 4, 4, 0, 0) == PHAST_ERR_INVALID_ARG);
    EXPECT(make(10, 3, 0, 4, 0, 0) == PHAST_ERR_INVALID_ARG);
    EXPECT(make(10, 3, (1u << 29) + 1, 4, 0, 0) == PHAST_ERR_INVALID_ARG);
    EXPECT(make(10, 3, 4, (1u << 29) + 1, 0, 0) == PHAST_ERR_INVALID_ARG);
    EXPECT(make(10, 3, 4, 4, 4, 1) == PHAST_ERR_INVALID_ARG);  // full_frames is 3
    EXPECT(make(10, 3, 4, 4, 3, 0) == PHAST_ERR_INVALID_ARG);  // nothing left
    EXPECT(make(10, 3, 1u << 20, 4, 0, 1025) == PHAST_ERR_INVALID_ARG);
    EXPECT(code_of([&] { P pl(10, Slice<const T>(nullptr, 3), 4); }) == PHAST_ERR_INVALID_ARG);
}

int main(int argc, char **argv) {
    const bool gpu = argc > 1 && std::string(argv[1]) == "gpu";
    argument_codes<double, PlannerChannelizer64>();
    argument_codes<float, PlannerChannelizer32>();
    if (gpu) {
        on_gpu<double, PlannerChannelizer64>("f64", [](const auto &...a) { channelize_f64_with_planner(a...); }, std::ldexp((ld)1, -53), 5.7e-14L);
        on_gpu<float, PlannerChannelizer32>("f32", [](const auto &...a) { channelize_f32_with_planner(a...); }, std::ldexp((ld)1, -24), 8e-6L);
    } else {
        const std::vector<double> h = {1.0, 2.0, 3.0};
        const std::vector<float> hf = {1.0f, 2.0f, 3.0f};
        // a good call gets past the checks and fails loudly
        EXPECT(code_of([&] { PlannerChannelizer64 pl(10, Slice<const double>(h.data(), 3), 4); }) == PHAST_ERR_NO_DEVICE);
        EXPECT(code_of([&] { PlannerChannelizer32 pl(10, Slice<const float>(hf.data(), 3), 4, 2, 0, 0, true); }) == PHAST_ERR_NO_DEVICE);
    }
    std::printf("channelizer: %s (%d failures)\n", failures ? "FAILED" : "ok", failures);
    return failures ? 1 : 0;
}
