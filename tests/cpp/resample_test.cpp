// resample_test.cpp -- the C++ host side (include/phastft.hpp) of sample-rate conversion: PlannerUpfirdn64/32,
// PlannerResample64/32, upfirdn_f64/f32_with_planner, resample_f64/f32_with_planner.  Built and run by
// tests/test_resample_cpp_host.py: without a GPU the argument codes and a loud failure of the rest; with "gpu" the host forms
// against the definitions of include/phastft_hip.h in long double, and the length codes.
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

// full[m] = sum_n h[m down - n up] x[n] and sum |h x|, in long double
template <typename T>
static void upfirdn_def(const std::vector<T> &h, const std::vector<T> &x, size_t up, size_t down, size_t m, ld *sum, ld *scale) {
    *sum = *scale = 0;
    for (size_t n = 0; n < x.size(); ++n) {
        const long long i = (long long)(m * down) - (long long)(n * up);
        if (i < 0 || i >= (long long)h.size()) continue;
        const ld t = (ld)h[i] * (ld)x[n];
        *sum += t;
        *scale += std::fabs(t);
    }
}

template <typename T, typename P, typename Call> static void upfirdn_on_gpu(const char *name, Call call, ld u) {
    const size_t L = 50, K = 33, up = 3, down = 2, first = 2, extra = 4;
    const std::vector<T> h = uniform<T>(K, 1), x = uniform<T>(L, 2);
    const size_t full = ((L - 1) * up + K - 1) / down + 1, kp = (K + up - 1) / up;
    P whole(L, Slice<const T>(h.data(), K), up, down), part(L, Slice<const T>(h.data(), K), up, down, first, full - first + extra);
    EXPECT(whole.out_len() == full && whole.full_len() == full && part.out_len() == full - first + extra && whole.workspace_len(3) == 0);
    EXPECT(whole.tile() == 1024 && whole.chunk() == kp && whole.device_bytes() == up * (kp | 1) * sizeof(T));
    EXPECT(whole.describe().rfind("upfirdn L=50 K=33 up=3 down=2 first=0", 0) == 0);
    std::vector<T> a(whole.out_len(), T(7)), b(part.out_len(), T(7));
    call(Slice<const T>(x.data(), L), Slice<T>(a.data(), a.size()), whole);
    call(Slice<const T>(x.data(), L), Slice<T>(b.data(), b.size()), part);
    ld worst = 0;
    for (size_t m = 0; m < full; ++m) {
        ld want, scale;
        upfirdn_def(h, x, up, down, m, &want, &scale);
        const ld gate = (ld)(kp + 2) * u * scale;  // a sum of Kp products in any order
        EXPECT(std::fabs((ld)a[m] - want) <= gate);
        if (scale > 0) worst = std::max(worst, std::fabs((ld)a[m] - want) / gate);
        if (m >= first) EXPECT(b[m - first] == a[m]);  // the same bits through the window
    }
    for (size_t i = full - first; i < b.size(); ++i) EXPECT(b[i] == T(0));  // zeros beyond full_len
    std::printf("%s upfirdn: %.3Lf of the gate\n", name, worst);
    std::vector<T> shorter(full - 1), fewer(L - 1);
    EXPECT(code_of([&] { call(Slice<const T>(fewer.data(), L - 1), Slice<T>(a.data(), full), whole); }) == PHAST_ERR_PLANNER_SIZE);
    EXPECT(code_of([&] { call(Slice<const T>(x.data(), L), Slice<T>(shorter.data(), full - 1), whole); }) == PHAST_ERR_LEN_MISMATCH);
}

template <typename T, typename P, typename Call> static void resample_on_gpu(const char *name, Call call, ld gate) {
    const size_t pairs[][2] = {{8, 12}, {8, 6}, {9, 14}, {100, 44}, {44, 100}, {64, 64}};
    for (const auto &pr : pairs) {
        const size_t L = pr[0], num = pr[1], N = L < num ? L : num;
        const std::vector<T> x = uniform<T>(L, (unsigned)(L + num));
        P pl(L, num);
        EXPECT(pl.out_len() == num && pl.workspace_min() == pl.workspace_len(1) && pl.workspace_len(2) >= pl.workspace_len(1));
        EXPECT(pl.describe().rfind("resample L=" + std::to_string(L) + " num=" + std::to_string(num), 0) == 0);
        std::vector<T> y(num, T(7));
        call(Slice<const T>(x.data(), L), Slice<T>(y.data(), num), pl);
        // the definition: X by a direct sum, Y, and the inverse real sum
        std::vector<std::complex<ld>> Y(num / 2 + 1);
        for (size_t k = 0; k <= N / 2; ++k) {
            std::complex<ld> s = 0;
            for (size_t n = 0; n < L; ++n) {
                const ld ph = -kTwoPi * (ld)((k * n) % L) / (ld)L;
                s += (ld)x[n] * std::complex<ld>(std::cos(ph), std::sin(ph));
            }
            Y[k] = s;
        }
        if (N % 2 == 0 && num < L) Y[N / 2] *= 2;
        if (N % 2 == 0 && num > L) Y[N / 2] *= (ld)0.5;
        ld worst = 0, rms = 0;
        std::vector<ld> want(num);
        for (size_t n = 0; n < num; ++n) {
            ld s = Y[0].real();
            for (size_t k = 1; k <= num / 2; ++k) {
                const ld ph = kTwoPi * (ld)((k * n) % num) / (ld)num;
                const bool nyq = num % 2 == 0 && k == num / 2;
                s += nyq ? Y[k].real() * std::cos(ph) : 2 * (Y[k].real() * std::cos(ph) - Y[k].imag() * std::sin(ph));
            }
            want[n] = s / (ld)L;
            rms += want[n] * want[n];
        }
        rms = std::sqrt(rms / (ld)num);
        for (size_t n = 0; n < num; ++n) worst = std::max(worst, std::fabs((ld)y[n] - want[n]));
        std::printf("%s resample %zu -> %zu: %.3Le of the rms\n", name, L, num, worst / rms);
        EXPECT(worst <= gate * rms);
        std::vector<T> shorter(num - 1), fewer(L - 1);
        EXPECT(code_of([&] { call(Slice<const T>(fewer.data(), L - 1), Slice<T>(y.data(), num), pl); }) == PHAST_ERR_PLANNER_SIZE);
        EXPECT(code_of([&] { call(Slice<const T>(x.data(), L), Slice<T>(shorter.data(), num - 1), pl); }) == PHAST_ERR_LEN_MISMATCH);
    }
}

template <typename T, typename PU, typename PR> static void argument_codes() {
    const std::vector<T> h = {T(1), T(2), T(3)};
    auto make = [&](size_t len, size_t k, size_t up, size_t down, size_t first, size_t out_len) {
        return code_of([&] { PU pl(len, Slice<const T>(h.data(), k), up, down, first, out_len); });
    };
    EXPECT(make(0, 3, 1, 1, 0, 0) == PHAST_ERR_INVALID_ARG);
    EXPECT(make(10, 0, 1, 1, 0, 0) == PHAST_ERR_INVALID_ARG);
    EXPECT(make(10, 3, 0, 1, 0, 0) == PHAST_ERR_INVALID_ARG);
    EXPECT(make(10, 3, 1, 0, 0, 0) == PHAST_ERR_INVALID_ARG);
    EXPECT(make(10, 3, (1u << 20) + 1, 1, 0, 0) == PHAST_ERR_INVALID_ARG);
    EXPECT(make(10, 3, 1, 1, 13, 1) == PHAST_ERR_INVALID_ARG);  // full_len is 12
    EXPECT(make(10, 3, 1, 1, 12, 0) == PHAST_ERR_INVALID_ARG);  // nothing left
    EXPECT(make(10, 3, 1, 1, 0, (1u << 29) + 1) == PHAST_ERR_INVALID_ARG);
    EXPECT(code_of([&] { PU pl(10, Slice<const T>(nullptr, 3)); }) == PHAST_ERR_INVALID_ARG);
    EXPECT(code_of([] { PR pl(0, 5); }) == PHAST_ERR_INVALID_ARG);
    EXPECT(code_of([] { PR pl(5, 0); }) == PHAST_ERR_INVALID_ARG);
    EXPECT(code_of([] { PR pl((1u << 29) + 1, 5); }) == PHAST_ERR_INVALID_ARG);
}

int main(int argc, char **argv) {
    const bool gpu = argc > 1 && std::string(argv[1]) == "gpu";
    argument_codes<double, PlannerUpfirdn64, PlannerResample64>();
    argument_codes<float, PlannerUpfirdn32, PlannerResample32>();
    if (gpu) {
        upfirdn_on_gpu<double, PlannerUpfirdn64>("f64", [](const auto &...a) { upfirdn_f64_with_planner(a...); }, std::ldexp((ld)1, -53));
        upfirdn_on_gpu<float, PlannerUpfirdn32>("f32", [](const auto &...a) { upfirdn_f32_with_planner(a...); }, std::ldexp((ld)1, -24));
        // the bounds: tests/tolerances.py's worst-sample gates at log2 = 8 (the inner transform of 100 and 44 is 256 points at
        // most): 64 eps 8 = 1.1e-13 and 2e-6 8 = 1.6e-5
        resample_on_gpu<double, PlannerResample64>("f64", [](const auto &...a) { resample_f64_with_planner(a...); }, 1.1e-13L);
        resample_on_gpu<float, PlannerResample32>("f32", [](const auto &...a) { resample_f32_with_planner(a...); }, 1.6e-5L);
    } else {
        const std::vector<double> h = {1.0, 2.0, 3.0};
        EXPECT(code_of([&] { PlannerUpfirdn64 pl(10, Slice<const double>(h.data(), 3), 2, 3); }) == PHAST_ERR_NO_DEVICE);
        EXPECT(code_of([] { PlannerResample32 pl(8, 12); }) == PHAST_ERR_NO_DEVICE);  // a good call gets past the checks and fails loudly
    }
    std::printf("resample: %s (%d failures)\n", failures ? "FAILED" : "ok", failures);
    return failures ? 1 : 0;
}
