// mdct_test.cpp -- the C++ host side (include/phastft.hpp) of the MDCT and its inverse: PlannerMdct64/32,
// mdct_f64/f32_with_planner, imdct_f64/f32_with_planner.  Built and run by tests/test_mdct_cpp_host.py: without a GPU the
// argument codes and a loud failure of the rest; with "gpu" the host forms against the long-double O(N^2) definition, the
// round trip through the sine window in both framings, the TDAC defect and the length codes.
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

static const long double kPi = 3.141592653589793238462643383279502884L;

static std::vector<double> signal(size_t n, unsigned seed) {
    std::vector<double> x(n);
    unsigned long long s = 0x9E3779B97F4A7C15ull * (seed + 1);
    for (size_t i = 0; i < n; ++i) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        x[i] = (double)(s >> 11) / 9007199254740992.0 * 2 - 1;
    }
    return x;
}

static std::vector<double> sine(size_t n) {
    std::vector<double> w(2 * n);
    for (size_t j = 0; j < 2 * n; ++j) w[j] = (double)sinl(kPi * ((long double)j + 0.5L) / (long double)(2 * n));
    return w;
}

static size_t frames_of(size_t len, size_t n, bool padded) { return padded ? (len + n - 1) / n + 1 : len / n - 1; }

// the definition of include/phastft_hip.h in long double: frames * n coefficients
static std::vector<long double> direct(const std::vector<double> &x, const std::vector<double> &w, size_t n, bool padded) {
    const long long len = (long long)x.size();
    const size_t frames = frames_of(x.size(), n, padded);
    std::vector<long double> out(frames * n, 0);
    for (size_t t = 0; t < frames; ++t)
        for (size_t k = 0; k < n; ++k) {
            long double acc = 0;
            for (size_t j = 0; j < 2 * n; ++j) {
                const long long i = ((long long)t - (padded ? 1 : 0)) * (long long)n + (long long)j;
                if (i < 0 || i >= len) continue;
                acc += (long double)w[j] * x[(size_t)i] * cosl(kPi / (long double)n * ((long double)j + 0.5L + (long double)n / 2) * ((long double)k + 0.5L));
            }
            out[t * n + k] = acc;
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
    EXPECT(code_of([&] { PlannerMdct64 p(100, 7); }) == PHAST_ERR_INVALID_ARG);  // odd N
    EXPECT(code_of([&] { PlannerMdct64 p(100, 0); }) == PHAST_ERR_INVALID_ARG);
    EXPECT(code_of([&] { PlannerMdct32 p(100, (1u << 29) + 2); }) == PHAST_ERR_INVALID_ARG);
    EXPECT(code_of([&] { PlannerMdct64 p(0, 8); }) == PHAST_ERR_INVALID_ARG);
    EXPECT(code_of([&] { PlannerMdct64 p(15, 8, {nullptr, 0}, false); }) == PHAST_ERR_INVALID_ARG);  // L < 2N without padding
    EXPECT(code_of([&] { PlannerMdct64 p(100, 8, sine(4)); }) == PHAST_ERR_INVALID_ARG);             // a window of N values
    EXPECT(code_of([&] { PlannerMdct64 p(100, 8, sine(8)); }) == PHAST_ERR_NO_DEVICE);
    EXPECT(code_of([&] { PlannerMdct32 p(16, 8, {nullptr, 0}, false); }) == PHAST_ERR_NO_DEVICE);
}

static void gpu() {
    struct Case {
        size_t n, len;
    };
    for (const Case &c : {Case{2, 1}, Case{2, 11}, Case{4, 5}, Case{6, 23}, Case{30, 95}, Case{34, 107}, Case{64, 200}})
        for (int padded = 1; padded >= 0; --padded) {
            if (!padded && c.len < 2 * c.n) continue;
            const std::vector<double> x = signal(c.len, (unsigned)(c.len + c.n)), w = sine(c.n);
            PlannerMdct64 p(c.len, c.n, w, padded != 0);
            const std::vector<long double> want = direct(x, w, c.n, padded != 0);
            EXPECT(p.frames() == frames_of(c.len, c.n, padded != 0) && p.frames() * c.n == want.size());
            EXPECT(p.tdac_defect() < 1e-15);
            std::vector<double> X(want.size()), back(c.len, 5.0);
            mdct_f64_with_planner(x, X, p);
            const double e = rel_err(X, want);
            if (!(e < 1e-14)) std::printf("N=%zu L=%zu padded=%d rel-L2 %.3e\n", c.n, c.len, padded, e);
            EXPECT(e < 1e-14);
            imdct_f64_with_planner(X, back, p);
            const size_t lo = padded ? 0 : c.n, hi = padded ? c.len : p.frames() * c.n;
            double worst = 0;
            for (size_t t = lo; t < hi; ++t) worst = std::fmax(worst, std::fabs(back[t] - x[t]));
            for (size_t t = (p.frames() + 1) * c.n; !padded && t < c.len; ++t) EXPECT(back[t] == 0.0);  // no frame holds the tail
            if (!(worst < 1e-13)) std::printf("N=%zu L=%zu padded=%d round trip %.3e\n", c.n, c.len, padded, worst);
            EXPECT(worst < 1e-13);
            std::vector<float> xf(x.begin(), x.end()), wf(w.begin(), w.end()), Xf(want.size()), bf(c.len);
            PlannerMdct32 q(c.len, c.n, wf, padded != 0);
            mdct_f32_with_planner(xf, Xf, q);
            const std::vector<double> x32(xf.begin(), xf.end()), w32(wf.begin(), wf.end());
            EXPECT(rel_err(Xf, direct(x32, w32, c.n, padded != 0)) < 5e-6);
            imdct_f32_with_planner(Xf, bf, q);
            float worst32 = 0;
            for (size_t t = lo; t < hi; ++t) worst32 = std::fmax(worst32, std::fabs(bf[t] - xf[t]));
            EXPECT(worst32 < 2e-5f);
            EXPECT(!p.describe().empty() && p.workspace_len(3) > p.workspace_len(1) && p.workspace_min(true) >= p.workspace_min());
            EXPECT(p.device_bytes() >= 4 * c.n * sizeof(double));
        }
    PlannerMdct64 rect(400, 16, std::vector<double>(32, 0.5));
    EXPECT(std::fabs(rect.tdac_defect() - 0.5) < 1e-15);  // reported, never refused
    PlannerMdct64 po(400, 16);  // the sine window
    EXPECT(po.tdac_defect() < 1e-15);
    std::vector<double> x = signal(400, 7), X(po.frames() * 16), back(400), shorter(399), few(X.size() - 1);
    mdct_f64_with_planner(x, X, po);
    imdct_f64_with_planner(X, back, po);
    EXPECT(code_of([&] { mdct_f64_with_planner(shorter, X, po); }) == PHAST_ERR_PLANNER_SIZE);
    EXPECT(code_of([&] { mdct_f64_with_planner(x, few, po); }) == PHAST_ERR_LEN_MISMATCH);
    EXPECT(code_of([&] { imdct_f64_with_planner(few, back, po); }) == PHAST_ERR_LEN_MISMATCH);
    EXPECT(code_of([&] { imdct_f64_with_planner(X, shorter, po); }) == PHAST_ERR_PLANNER_SIZE);
}

int main(int argc, char **argv) {
    const bool on_gpu = argc > 1 && std::string(argv[1]) == "gpu";
    if (on_gpu)
        gpu();
    else
        no_gpu();
    if (failures) {
        std::printf("mdct: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("mdct: ok\n");
    return 0;
}
