// cwt_test.cpp -- the C++ host side (include/phastft.hpp) of the continuous wavelet transform: PlannerCwt64/32,
// cwt_64/32_with_planner.  Built and run by tests/test_cwt_cpp_host.py: without an argument the argument codes, and a good
// constructor that either works or fails loudly for want of a device; with "gpu" the host forms against the definition of
// include/phastft_hip.h in long double, and the length codes.
#include <cmath>
#include <complex>
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

using ld = long double;
using cld = std::complex<ld>;
static const ld kPi = 3.141592653589793238462643383279502884L;

template <typename T> static std::vector<T> uniform(size_t n, unsigned seed) {
    std::vector<T> x(n);
    unsigned long long s = 0x9E3779B97F4A7C15ull * (seed + 1);
    for (size_t i = 0; i < n; ++i) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        x[i] = (T)(float)(-1.0 + 2.0 * ((double)(s >> 11) / 9007199254740992.0));
    }
    return x;
}

// conj(c psi0^(x)) of the definition: Morlet (w0), DOG (m), L2 norm
static cld filter(CwtFamily f, double param, ld s, ld w) {
    const ld x = s * w, c = std::sqrt(2 * kPi * s);
    if (f == CwtFamily::Morlet) return x > 0 ? cld(c * std::pow(kPi, -0.25L) * std::exp(-(x - (ld)param) * (x - (ld)param) / 2), 0) : cld(0, 0);
    const int m = (int)param;
    ld gam = std::sqrt(kPi);
    for (int i = 0; i < m; ++i) gam *= i + 0.5L;
    const cld unit = -std::pow(cld(0, 1), m);
    return std::conj(unit * (c / std::sqrt(gam) * std::pow(x, (ld)m) * std::exp(-x * x / 2)));
}

// rel_gate: tests/tolerances.py's rel-L2 gate at log2 = 6 (the inner transform of P = 24 has 64 points), per row
template <typename T, typename P, typename Call> static void on_gpu(const char *name, Call call, ld rel_gate) {
    const size_t L = 20, Pn = 24, S = 3;
    const std::vector<double> scales = {0.7, 2.0, 5.0};
    for (int cplx = 0; cplx < 2; ++cplx) {
        const CwtFamily fam = cplx ? CwtFamily::Dog : CwtFamily::Morlet;
        const double param = cplx ? 1.0 : 6.0;
        P pl(L, Slice<const double>(scales.data(), S), fam, param, CwtNorm::L2, Pn, cplx == 0);
        EXPECT(pl.signal_len() == L && pl.pad_len() == Pn && pl.num_scales() == S && pl.scale_group() == 8 && pl.tile_bins() == 4096 / sizeof(T));
        EXPECT(pl.workspace_min() > 0 && pl.workspace_len(2) > pl.workspace_min() && pl.device_bytes() >= 2 * S * sizeof(double));
        EXPECT(pl.describe().rfind(std::string("cwt ") + (cplx ? "dog(m=1) l2 complex" : "morlet(w0=6.000000) l2 real") + " L=20 P=24 S=3", 0) == 0);
        const std::vector<T> xr = uniform<T>(L, 2), xi = uniform<T>(L, 3);
        std::vector<T> wr(S * L, T(7)), wi(wr);
        const Slice<const T> sr(xr.data(), L), si(cplx ? xi.data() : nullptr, cplx ? L : 0);
        call(sr, si, Slice<T>(wr.data(), wr.size()), Slice<T>(wi.data(), wi.size()), pl);
        std::vector<cld> X(Pn);
        for (size_t k = 0; k < Pn; ++k) {
            cld sum = 0;
            for (size_t n = 0; n < L; ++n) {
                const ld ph = -2 * kPi * (ld)((k * n) % Pn) / (ld)Pn;
                sum += cld((ld)xr[n], cplx ? (ld)xi[n] : 0) * cld(std::cos(ph), std::sin(ph));
            }
            X[k] = sum;
        }
        ld worst = 0;
        for (size_t j = 0; j < S; ++j) {
            ld num = 0, den = 0;
            for (size_t n = 0; n < L; ++n) {
                cld sum = 0;
                for (size_t k = 0; k < Pn; ++k) {
                    const ld w = 2 * kPi * (k <= Pn / 2 ? (ld)k : (ld)k - (ld)Pn) / (ld)Pn;
                    const ld ph = 2 * kPi * (ld)((k * n) % Pn) / (ld)Pn;
                    sum += X[k] * filter(fam, param, (ld)scales[j], w) * cld(std::cos(ph), std::sin(ph));
                }
                const cld want = sum / (ld)Pn;
                num += std::norm(cld((ld)wr[j * L + n], (ld)wi[j * L + n]) - want);
                den += std::norm(want);
            }
            EXPECT(den > 0 && std::sqrt(num / den) <= rel_gate);
            worst = std::max(worst, std::sqrt(num / den) / rel_gate);
        }
        std::printf("%s cwt %s: worst row %.3Lf of its gate\n", name, cplx ? "dog complex" : "morlet real", worst);
        std::vector<T> shorter(S * L - 1), fewer(L - 1);
        EXPECT(code_of([&] { call(Slice<const T>(fewer.data(), L - 1), Slice<const T>(cplx ? fewer.data() : nullptr, cplx ? L - 1 : 0),
                                  Slice<T>(wr.data(), wr.size()), Slice<T>(wi.data(), wi.size()), pl); }) == PHAST_ERR_PLANNER_SIZE);
        EXPECT(code_of([&] { call(sr, si, Slice<T>(shorter.data(), shorter.size()), Slice<T>(wi.data(), shorter.size()), pl); }) == PHAST_ERR_LEN_MISMATCH);
        EXPECT(code_of([&] { call(sr, Slice<const T>(cplx ? nullptr : xi.data(), cplx ? 0 : L), Slice<T>(wr.data(), wr.size()),
                                  Slice<T>(wi.data(), wi.size()), pl); }) == PHAST_ERR_INVALID_ARG);  // the wrong planes
    }
}

template <typename P> static void argument_codes() {
    const std::vector<double> sc = {1.0, 2.0, 4.0};
    auto make = [&](size_t l, size_t s, CwtFamily f, double param, size_t pad) {
        return code_of([&] { P pl(l, Slice<const double>(sc.data(), s), f, param, CwtNorm::L2, pad); });
    };
    EXPECT(make(0, 3, CwtFamily::Morlet, 6.0, 0) == PHAST_ERR_INVALID_ARG);
    EXPECT(make(8, 0, CwtFamily::Morlet, 6.0, 0) == PHAST_ERR_INVALID_ARG);
    EXPECT(make(8, 3, CwtFamily::Morlet, 0.0, 0) == PHAST_ERR_INVALID_ARG);
    EXPECT(make(8, 3, CwtFamily::Paul, 2.5, 0) == PHAST_ERR_INVALID_ARG);
    EXPECT(make(8, 3, CwtFamily::Paul, 86.0, 0) == PHAST_ERR_INVALID_ARG);
    EXPECT(make(8, 3, CwtFamily::Dog, 171.0, 0) == PHAST_ERR_INVALID_ARG);
    EXPECT(make(8, 3, static_cast<CwtFamily>(9), 6.0, 0) == PHAST_ERR_INVALID_ARG);
    EXPECT(make(8, 3, CwtFamily::Morlet, 6.0, 7) == PHAST_ERR_INVALID_ARG);
    EXPECT(make(8, 3, CwtFamily::Morlet, 6.0, (1u << 29) + 1) == PHAST_ERR_INVALID_ARG);
    const std::vector<double> bad = {1.0, std::numeric_limits<double>::quiet_NaN()};
    EXPECT(code_of([&] { P pl(8, Slice<const double>(bad.data(), 2)); }) == PHAST_ERR_INVALID_ARG);
    EXPECT(code_of([&] { P pl(8, Slice<const double>(nullptr, 3)); }) == PHAST_ERR_INVALID_ARG);
    EXPECT(code_of([&] { P pl(8, Slice<const double>(sc.data(), 3), CwtFamily::Morlet, 6.0, static_cast<CwtNorm>(5)); }) == PHAST_ERR_INVALID_ARG);
}

int main(int argc, char **argv) {
    const bool gpu = argc > 1 && std::string(argv[1]) == "gpu";
    argument_codes<PlannerCwt64>();
    argument_codes<PlannerCwt32>();
    if (gpu) {
        on_gpu<double, PlannerCwt64>("f64", [](const auto &...a) { cwt_64_with_planner(a...); }, 8e-16L * 6);
        on_gpu<float, PlannerCwt32>("f32", [](const auto &...a) { cwt_32_with_planner(a...); }, 1.5e-7L * 6);
    } else {
        // a good call gets past the checks: it works, or fails loudly where there is no device
        const std::vector<double> sc = {1.0, 2.0, 4.0};
        const int a = code_of([&] { PlannerCwt64 pl(10, Slice<const double>(sc.data(), 3)); });
        const int b = code_of([&] { PlannerCwt32 pl(10, Slice<const double>(sc.data(), 3), CwtFamily::Step, 0.0, CwtNorm::Peak, 16, false); });
        EXPECT(a == PHAST_OK || a == PHAST_ERR_NO_DEVICE);
        EXPECT(b == a);
    }
    std::printf("cwt: %s (%d failures)\n", failures ? "FAILED" : "ok", failures);
    return failures ? 1 : 0;
}
