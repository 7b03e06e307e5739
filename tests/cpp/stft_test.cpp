// stft_test.cpp -- the C++ host side (include/phastft.hpp) of the STFT and its inverse: PlannerStft64/32,
// stft_f64/f32_with_planner, istft_f64/f32_with_planner.  Built and run by tests/test_stft_cpu.py (no GPU: argument codes,
// compute fails loudly) and tests/test_gpu_stft.py (with "gpu": the host forms against a long-double O(F^2) sum per frame,
// the round trip, the refusal of a window that does not overlap-add to nonzero, the length codes).
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

static std::vector<double> hann(size_t f) {
    std::vector<double> w(f, 1.0);
    for (size_t j = 0; f > 1 && j < f; ++j) w[j] = (double)(0.5L - 0.5L * cosl(2 * kPi * (long double)j / (long double)f));
    return w;
}

// the definition of include/phastft_hip.h in long double: (re, im) planes of frames * bins
static void direct(const std::vector<double> &x, const std::vector<double> &w, size_t f, size_t h, bool center, bool reflect,
                   std::vector<long double> &re, std::vector<long double> &im) {
    const long long len = (long long)x.size(), p = center ? (long long)(f / 2) : 0;
    const size_t frames = 1 + (size_t)(len + 2 * p - (long long)f) / h, bins = f / 2 + 1;
    re.assign(frames * bins, 0);
    im.assign(frames * bins, 0);
    for (size_t k = 0; k < frames; ++k)
        for (size_t b = 0; b < bins; ++b) {
            long double sr = 0, si = 0;
            for (size_t j = 0; j < f; ++j) {
                long long i = (long long)(k * h) - p + (long long)j;
                long double v = 0;
                if (i >= 0 && i < len) v = x[(size_t)i];
                else if (reflect) v = x[(size_t)(i < 0 ? -i : 2 * (len - 1) - i)];
                const long double ang = -2 * kPi * (long double)((b * j) % f) / (long double)f;
                sr += w[j] * v * cosl(ang);
                si += w[j] * v * sinl(ang);
            }
            re[k * bins + b] = sr;
            im[k * bins + b] = si;
        }
}

static double rel_err(const std::vector<double> &gr, const std::vector<double> &gi, const std::vector<long double> &wr,
                      const std::vector<long double> &wi) {
    long double num = 0, den = 0;
    for (size_t i = 0; i < gr.size(); ++i) {
        num += (gr[i] - wr[i]) * (gr[i] - wr[i]) + (gi[i] - wi[i]) * (gi[i] - wi[i]);
        den += wr[i] * wr[i] + wi[i] * wi[i];
    }
    return den > 0 ? (double)std::sqrt(num / den) : (double)std::sqrt(num);
}

static void no_gpu() {
    const std::vector<double> w = hann(16);
    EXPECT(code_of([&] { PlannerStft64 p(100, 16, 17, w); }) == PHAST_ERR_INVALID_ARG);  // H > F
    EXPECT(code_of([&] { PlannerStft64 p(100, 16, 0, w); }) == PHAST_ERR_INVALID_ARG);
    EXPECT(code_of([&] { PlannerStft64 p(8, 16, 4, w); }) == PHAST_ERR_INVALID_ARG);  // p >= L with reflect
    EXPECT(code_of([&] { PlannerStft32 p(15, 16, 4, {nullptr, 0}, false); }) == PHAST_ERR_INVALID_ARG);  // L < F without center
    EXPECT(code_of([&] { PlannerStft64 p(100, 16, 4, hann(15)); }) == PHAST_ERR_INVALID_ARG);  // a window that is not F long
    EXPECT(code_of([&] { PlannerStft64 p(0, 16, 4); }) == PHAST_ERR_INVALID_ARG);
    EXPECT(code_of([&] { PlannerStft64 p((1u << 29) + 1, 16, 4); }) == PHAST_ERR_INVALID_ARG);
    EXPECT(code_of([&] { PlannerStft64 p(1u << 20, 1024, 1); }) == PHAST_ERR_INVALID_ARG);  // frames * F > 2^30
    EXPECT(code_of([&] { PlannerStft64 p(100, 16, 4, w); }) == PHAST_ERR_NO_DEVICE);
    EXPECT(code_of([&] { PlannerStft32 p(8, 16, 4, {nullptr, 0}, true, PadMode::Zero); }) == PHAST_ERR_NO_DEVICE);
}

static void gpu() {
    struct Case {
        size_t len, f, h;
    };
    for (const Case &c : {Case{37, 1, 1}, Case{64, 2, 1}, Case{101, 7, 3}, Case{200, 16, 16}, Case{300, 30, 23}, Case{500, 64, 16}})
        for (int center = 0; center < 2; ++center)
            for (int zero = 0; zero < 2; ++zero) {
                const std::vector<double> x = signal(c.len, (unsigned)(c.len + c.f)), ones(c.f, 1.0);
                const std::vector<double> w = center && c.h < c.f ? hann(c.f) : ones;  // windows the inverse accepts
                PlannerStft64 p(c.len, c.f, c.h, w, center != 0, zero ? PadMode::Zero : PadMode::Reflect);
                std::vector<long double> wr, wi;
                direct(x, w, c.f, c.h, center != 0, !zero, wr, wi);
                EXPECT(p.frames() * p.bins() == wr.size() && p.bins() == c.f / 2 + 1);
                std::vector<double> re(wr.size()), im(wr.size()), back(c.len, 5.0);
                stft_f64_with_planner(x, re, im, p);
                const double e = rel_err(re, im, wr, wi);
                if (!(e < 1e-14)) std::printf("L=%zu F=%zu H=%zu center=%d zero=%d rel-L2 %.3e\n", c.len, c.f, c.h, center, zero, e);
                EXPECT(e < 1e-14);
                EXPECT(p.envelope_min() > 1e-11);
                istft_f64_with_planner(re, im, back, p);
                const size_t pad = center ? c.f / 2 : 0, covered = (p.frames() - 1) * c.h + c.f;  // positions the frames hold
                double worst = 0;
                for (size_t t = 0; t < c.len; ++t) worst = std::fmax(worst, std::fabs(back[t] - (t + pad < covered ? x[t] : 0.0)));
                if (!(worst < 1e-13)) std::printf("L=%zu F=%zu H=%zu center=%d zero=%d round trip %.3e\n", c.len, c.f, c.h, center, zero, worst);
                EXPECT(worst < 1e-13);
                std::vector<float> xf(x.begin(), x.end()), wf(w.begin(), w.end()), ref(wr.size()), imf(wr.size()), bf(c.len);
                PlannerStft32 q(c.len, c.f, c.h, wf, center != 0, zero ? PadMode::Zero : PadMode::Reflect);
                stft_f32_with_planner(xf, ref, imf, q);
                const std::vector<double> x32(xf.begin(), xf.end()), w32(wf.begin(), wf.end());
                direct(x32, w32, c.f, c.h, center != 0, !zero, wr, wi);
                EXPECT(rel_err(std::vector<double>(ref.begin(), ref.end()), std::vector<double>(imf.begin(), imf.end()), wr, wi) < 5e-6);
                istft_f32_with_planner(ref, imf, bf, q);
                float worst32 = 0;
                for (size_t t = 0; t < c.len; ++t) worst32 = std::fmax(worst32, std::fabs(bf[t] - (t + pad < covered ? xf[t] : 0.0f)));
                EXPECT(worst32 < 2e-5f);
                EXPECT(!p.describe().empty() && p.workspace_len(3) > p.workspace_len(1) && p.workspace_min(true) >= p.workspace_min());
            }
    // Hann without center: w[0] = 0 is sample 0's only tap -- the forward runs, the inverse refuses
    PlannerStft64 pz(400, 16, 4, hann(16), false);
    EXPECT(pz.envelope_min() == 0.0);
    std::vector<double> x = signal(400, 7), re(pz.frames() * pz.bins()), im(re.size()), back(400), shorter(399);
    stft_f64_with_planner(x, re, im, pz);
    EXPECT(code_of([&] { istft_f64_with_planner(re, im, back, pz); }) == PHAST_ERR_INVALID_ARG);
    EXPECT(code_of([&] { stft_f64_with_planner(shorter, re, im, pz); }) == PHAST_ERR_PLANNER_SIZE);
    PlannerStft64 po(400, 16, 4);
    std::vector<double> few(re.size() - 1);
    EXPECT(code_of([&] { stft_f64_with_planner(x, few, im, po); }) == PHAST_ERR_LEN_MISMATCH);
    EXPECT(code_of([&] { istft_f64_with_planner(re, few, back, po); }) == PHAST_ERR_LEN_MISMATCH);
    EXPECT(code_of([&] { istft_f64_with_planner(re, im, shorter, po); }) == PHAST_ERR_PLANNER_SIZE);
}

int main(int argc, char **argv) {
    const bool on_gpu = argc > 1 && std::string(argv[1]) == "gpu";
    if (on_gpu)
        gpu();
    else
        no_gpu();
    if (failures) {
        std::printf("stft: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("stft: ok\n");
    return 0;
}
