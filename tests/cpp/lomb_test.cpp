// lomb_test.cpp -- the C++ host side (include/phastft.hpp) of the Lomb-Scargle periodogram: PlannerLomb64/32,
// lombscargle_f64/f32_with_planner.  Built and run by tests/test_lomb_cpp_host.py: without a GPU the argument codes and a
// loud failure of the rest; with "gpu" the host forms against the definition of include/phastft_hip.h by an O(M K) sum in
// long double, and the length codes.
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

static std::vector<double> uniform(size_t n, unsigned seed, double lo, double hi) {
    std::vector<double> x(n);
    unsigned long long s = 0x9E3779B97F4A7C15ull * (seed + 1);
    for (size_t i = 0; i < n; ++i) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        x[i] = lo + (hi - lo) * ((double)(s >> 11) / 9007199254740992.0);
    }
    return x;
}

// the definition (times of a few hundred turns at most: the phase is good to a long double)
static std::vector<std::complex<ld>> definition(const std::vector<double> &t, const std::vector<double> &y, const std::vector<double> &f,
                                                const std::vector<double> &w_in, bool fm, LombNorm norm, ld epsneg) {
    const size_t m = t.size(), k = f.size();
    std::vector<ld> w(m);
    ld ws = 0;
    for (size_t j = 0; j < m; ++j) ws += w[j] = w_in.empty() ? 1 : w_in[j];
    for (ld &v : w) v /= ws;
    ld mean = 0, yy = 0;
    if (fm)
        for (size_t j = 0; j < m; ++j) mean += w[j] * y[j];
    for (size_t j = 0; j < m; ++j) yy += w[j] * (y[j] - mean) * (y[j] - mean);
    std::vector<std::complex<ld>> out(k);
    for (size_t i = 0; i < k; ++i) {
        std::complex<ld> a0 = 0, a1 = 0, a2 = 0;
        for (size_t j = 0; j < m; ++j) {
            const ld ph = kTwoPi * (ld)f[i] * (ld)t[j];
            const std::complex<ld> e(std::cos(ph), std::sin(ph));
            a0 += w[j] * e;
            a1 += w[j] * (y[j] - mean) * e;
            a2 += w[j] * e * e;
        }
        const ld c = a0.real(), s = a0.imag(), c2 = a2.real(), s2 = a2.imag();
        ld cc = (1 + c2) / 2, ss = (1 - c2) / 2, cs = s2 / 2;
        if (fm) cc -= c * c, ss -= s * s, cs -= c * s;
        const ld tau = std::atan2(2 * cs, cc - ss) / 2, ct = std::cos(tau), st = std::sin(tau);
        ld cct = (1 + c2 * std::cos(2 * tau) + s2 * std::sin(2 * tau)) / 2, sst = 1 - cct;
        if (fm) {
            cct -= (c * ct + s * st) * (c * ct + s * st);
            sst -= (s * ct - c * st) * (s * ct - c * st);
        }
        cct = cct < epsneg ? epsneg : cct;
        sst = sst < epsneg ? epsneg : sst;
        const ld yc = a1.real() * ct + a1.imag() * st, ys = a1.imag() * ct - a1.real() * st, a = yc / cct, b = ys / sst;
        const ld p = 2 * (a * yc + b * ys);
        if (norm == LombNorm::Power) out[i] = p * (ld)m / 4;
        else if (norm == LombNorm::Normalize) out[i] = p / (2 * yy);
        else out[i] = std::complex<ld>(a, b) * std::complex<ld>(ct, st);
    }
    return out;
}

template <typename T, typename P, typename Call> static void on_gpu(const char *name, Call call, ld gate, ld epsneg) {
    const size_t m = 200, k = 41;
    const std::vector<double> t = uniform(m, 1, 0.0, 50.0), f = uniform(k, 2, 0.05, 2.0), w = uniform(m, 3, 0.5, 1.5);
    std::vector<double> y = uniform(m, 4, -1.0, 1.0);
    for (size_t j = 0; j < m; ++j) y[j] = (double)(float)(y[j] + std::sin(6.283185307179586 * f[7] * t[j]));
    const std::vector<T> yt(y.begin(), y.end());
    const double eps = sizeof(T) == 4 ? 1e-6 : 1e-12;
    for (int weighted = 0; weighted < 2; ++weighted)
        for (int fm = 0; fm < 2; ++fm) {
            const std::vector<double> ww = weighted ? w : std::vector<double>();
            P pl(Slice<const double>(t.data(), m), Slice<const double>(f.data(), k), Slice<const double>(ww.data(), ww.size()), fm != 0, eps);
            EXPECT(pl.points() == m && pl.freqs() == k && pl.slab() == 2048 && pl.workspace_min() == pl.workspace_len(1));
            EXPECT(pl.describe().rfind("lomb M=200 K=41", 0) == 0 && pl.device_bytes() > 0 && pl.grid_len() >= 8);
            for (LombNorm norm : {LombNorm::Power, LombNorm::Normalize, LombNorm::Amplitude}) {
                std::vector<T> re(k, T(7)), im(k, T(7));
                const bool amp = norm == LombNorm::Amplitude;
                call(Slice<const T>(yt.data(), m), Slice<T>(re.data(), k), pl, norm, amp ? Slice<T>(im.data(), k) : Slice<T>(nullptr, 0));
                const auto want = definition(t, y, f, ww, fm != 0, norm, epsneg);
                ld top = 0, worst = 0;
                for (size_t i = 0; i < k; ++i) {
                    top = std::max(top, std::abs(want[i]));
                    worst = std::max(worst, std::abs(std::complex<ld>(re[i], amp ? (ld)im[i] : 0) - want[i]));
                }
                if (!amp)
                    for (size_t i = 0; i < k; ++i) EXPECT(im[i] == T(7));  // not written
                std::printf("%s weighted %d floating_mean %d norm %d: %.3Le of the peak\n", name, weighted, fm, (int)norm, worst / top);
                EXPECT(worst <= gate * top);
            }
            std::vector<T> out(k), shorter(k - 1), fewer(m - 1);
            EXPECT(code_of([&] { call(Slice<const T>(fewer.data(), m - 1), Slice<T>(out.data(), k), pl, LombNorm::Power, Slice<T>(nullptr, 0)); }) ==
                   PHAST_ERR_PLANNER_SIZE);
            EXPECT(code_of([&] { call(Slice<const T>(yt.data(), m), Slice<T>(shorter.data(), k - 1), pl, LombNorm::Power, Slice<T>(nullptr, 0)); }) ==
                   PHAST_ERR_LEN_MISMATCH);
            EXPECT(code_of([&] { call(Slice<const T>(yt.data(), m), Slice<T>(out.data(), k), pl, LombNorm::Amplitude, Slice<T>(nullptr, 0)); }) ==
                   PHAST_ERR_INVALID_ARG);  // amplitude needs the imaginary plane
        }
}

template <typename P> static void argument_codes(double low_eps) {
    const std::vector<double> t = {0.0, 1.0, 2.5}, f = {0.1, 0.2}, w = {1.0, 0.5, 2.0}, neg = {1.0, -0.5, 2.0}, two = {1.0, 1.0};
    const double nan = std::nan("");
    const std::vector<double> bad_t = {0.0, nan, 2.5};
    auto make = [](const std::vector<double> &t_, const std::vector<double> &f_, const std::vector<double> &w_, double eps) {
        return code_of([&] { P pl(Slice<const double>(t_.data(), t_.size()), Slice<const double>(f_.data(), f_.size()), Slice<const double>(w_.data(), w_.size()), true, eps); });
    };
    EXPECT(make(bad_t, f, w, 1e-6) == PHAST_ERR_INVALID_ARG);
    EXPECT(make(t, f, neg, 1e-6) == PHAST_ERR_INVALID_ARG);
    EXPECT(make(t, f, two, 1e-6) == PHAST_ERR_INVALID_ARG);     // two weights for three times
    EXPECT(make(t, {}, w, 1e-6) == PHAST_ERR_INVALID_ARG);
    EXPECT(make(t, f, w, 0.5) == PHAST_ERR_INVALID_ARG);
    EXPECT(make(t, f, w, low_eps) == PHAST_ERR_INVALID_ARG);
}

int main(int argc, char **argv) {
    const bool gpu = argc > 1 && std::string(argv[1]) == "gpu";
    argument_codes<PlannerLomb64>(0.9e-14);
    argument_codes<PlannerLomb32>(0.9e-6);
    if (gpu) {
        // the bounds: tests/test_lomb_cpu.py's lomb_gate for this case -- eps 1e-12 / 1e-6, Q = 2 pi 2 25 = 314, n_g <= 2^11, d of
        // a few tenths for 200 uniform times -- is 2e-11 (f64) and 1e-5 (f32) for the power; these are those, rounded down
        on_gpu<double, PlannerLomb64>("f64", [](const auto &...a) { lombscargle_f64_with_planner(a...); }, 1e-11L, 1.1102230246251565e-16L);
        on_gpu<float, PlannerLomb32>("f32", [](const auto &...a) { lombscargle_f32_with_planner(a...); }, 1e-5L, 5.9604644775390625e-08L);
    } else {
        const std::vector<double> t = {0.0, 1.0, 2.5}, f = {0.1, 0.2};
        const int rc = code_of([&] { PlannerLomb64 pl(Slice<const double>(t.data(), 3), Slice<const double>(f.data(), 2)); });
        EXPECT(rc == PHAST_ERR_NO_DEVICE);  // a good call gets past the checks and fails loudly
    }
    std::printf("lomb: %s (%d failures)\n", failures ? "FAILED" : "ok", failures);
    return failures ? 1 : 0;
}
