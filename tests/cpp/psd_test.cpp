// psd_test.cpp -- the C++ host side (include/phastft.hpp) of Welch spectral estimation: PlannerPsd64/32,
// psd_f64/f32_with_planner, csd_f64/f32_with_planner.  Built and run by tests/test_psd_cpp_host.py: without a GPU the
// argument codes and a loud failure of the rest; with "gpu" the host forms against the definition of include/phastft_hip.h by
// an O(S P F) sum in long double, and the length codes.
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
static const ld kPi = 3.141592653589793238462643383279502884L;

static std::vector<double> signal(size_t n, unsigned seed) {
    std::vector<double> x(n);
    unsigned long long s = 0x9E3779B97F4A7C15ull * (seed + 1);
    for (size_t i = 0; i < n; ++i) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        x[i] = (double)(s >> 11) / 9007199254740992.0 * 2 - 1;
    }
    return x;
}

struct Shape {
    size_t len, p, h, f;
};
static size_t segments_of(const Shape &s) { return 1 + (s.len - s.p) / s.h; }

// X_f[k] of every segment by the definition: (S, bins)
static std::vector<std::complex<ld>> spectra(const std::vector<double> &x, const std::vector<double> &w, const Shape &s, bool detrend) {
    const size_t seg = segments_of(s), bins = s.f / 2 + 1;
    std::vector<std::complex<ld>> out(seg * bins);
    for (size_t t = 0; t < seg; ++t) {
        ld mean = 0;
        for (size_t j = 0; j < s.p; ++j) mean += x[t * s.h + j];
        mean = detrend ? mean / (ld)s.p : 0;
        for (size_t k = 0; k < bins; ++k) {
            std::complex<ld> acc = 0;
            for (size_t j = 0; j < s.p; ++j) {
                const ld ang = -2 * kPi * (ld)((k * j) % s.f) / (ld)s.f;
                acc += (ld)w[j] * ((ld)x[t * s.h + j] - mean) * std::complex<ld>(cosl(ang), sinl(ang));
            }
            out[t * bins + k] = acc;
        }
    }
    return out;
}

static ld scale_of(const std::vector<double> &w, PsdScaling sc, double fs) {
    ld s1 = 0, s2 = 0;
    for (double v : w) {
        s1 += v;
        s2 += (ld)v * v;
    }
    return sc == PsdScaling::Density ? 1 / ((ld)fs * s2) : 1 / (s1 * s1);
}

template <typename T> static double rel_err(const std::vector<T> &got, const std::vector<ld> &want, ld den = -1) {
    ld num = 0, d = 0;
    for (size_t i = 0; i < got.size(); ++i) {
        num += (got[i] - want[i]) * (got[i] - want[i]);
        d += want[i] * want[i];
    }
    if (den >= 0) d = den * den;
    return d > 0 ? (double)std::sqrt(num / d) : (double)std::sqrt(num);
}

static void no_gpu() {
    const std::vector<double> w8(8, 1.0), w7(7, 1.0), zero(8, 0.0);
    EXPECT(code_of([&] { PlannerPsd64 p(1000, 100, 0, 128); }) == PHAST_ERR_INVALID_ARG);    // hop 0
    EXPECT(code_of([&] { PlannerPsd64 p(1000, 100, 101, 128); }) == PHAST_ERR_INVALID_ARG);  // hop > nperseg
    EXPECT(code_of([&] { PlannerPsd32 p(1000, 100, 50, 99); }) == PHAST_ERR_INVALID_ARG);    // nfft < nperseg
    EXPECT(code_of([&] { PlannerPsd64 p(99, 100, 50, 128); }) == PHAST_ERR_INVALID_ARG);     // nperseg > L
    EXPECT(code_of([&] { PlannerPsd64 p(100, 8, 4, 8, w7); }) == PHAST_ERR_INVALID_ARG);     // a window of another length
    EXPECT(code_of([&] { PlannerPsd64 p(100, 8, 4, 8, zero); }) == PHAST_ERR_INVALID_ARG);   // sum w^2 = 0
    EXPECT(code_of([&] { PlannerPsd64 p(100, 8, 4, 8, w8, Detrend::Constant, PsdScaling::Density, 0.0); }) == PHAST_ERR_INVALID_ARG);
    EXPECT(code_of([&] { PlannerPsd64 p(100, 8, 4, 8, w8); }) == PHAST_ERR_NO_DEVICE);
    EXPECT(code_of([&] { PlannerPsd32 p(1000, 100, 63, 128); }) == PHAST_ERR_NO_DEVICE);
}

static void gpu() {
    // the gate of tests/test_gpu_psd.py at the largest inner length of these shapes (2^8): 4 x 8e-16 x 8 (f64), 4 x 1.5e-7 x 8 (f32)
    const double gate64 = 4 * 8e-16 * 8, gate32 = 4 * 1.5e-7 * 8;
    for (const Shape &s : {Shape{300, 100, 63, 128}, Shape{200, 50, 50, 50}, Shape{37, 37, 1, 37}, Shape{300, 7, 3, 9}, Shape{50, 2, 1, 2}})
        for (int variant = 0; variant < 2; ++variant) {
            const bool detrend = variant == 0;
            const PsdScaling sc = variant ? PsdScaling::Spectrum : PsdScaling::Density;
            const double fs = 2.5;
            const std::vector<double> x = signal(s.len, (unsigned)(s.len + s.p)), y = signal(s.len, (unsigned)(s.len + s.p + 1));
            std::vector<double> w = signal(s.p, 99);
            for (double &v : w) v = 0.55 + 0.45 * v;  // [0.1, 1)
            PlannerPsd64 p(s.len, s.p, s.h, s.f, w, detrend ? Detrend::Constant : Detrend::None, sc, fs);
            const size_t seg = segments_of(s), bins = s.f / 2 + 1;
            EXPECT(p.segments() == seg && p.bins() == bins && p.slab() == 16);
            const std::vector<std::complex<ld>> fx = spectra(x, w, s, detrend), fy = spectra(y, w, s, detrend);
            const ld sigma = scale_of(w, sc, fs);
            std::vector<ld> pxx(bins, 0), pyy(bins, 0), re(bins, 0), im(bins, 0), sxx(seg * bins);
            for (size_t t = 0; t < seg; ++t)
                for (size_t k = 0; k < bins; ++k) {
                    const ld c = sigma * ((k == 0 || 2 * k == s.f) ? 1 : 2);
                    const std::complex<ld> a = fx[t * bins + k], b = fy[t * bins + k], ab = std::conj(a) * b;
                    sxx[t * bins + k] = c * std::norm(a);
                    pxx[k] += c * std::norm(a) / (ld)seg;
                    pyy[k] += c * std::norm(b) / (ld)seg;
                    re[k] += c * ab.real() / (ld)seg;
                    im[k] += c * ab.imag() / (ld)seg;
                }
            ld den = 0;
            for (size_t k = 0; k < bins; ++k) den += pxx[k] * pyy[k];
            den = std::sqrt(den);
            std::vector<double> g(bins), gs(seg * bins), gre(bins), gim(bins), gxx(bins), gyy(bins);
            psd_f64_with_planner(x, g, p);
            psd_f64_with_planner(x, gs, p, false);
            csd_f64_with_planner(x, y, gre, gim, p, gxx, gyy);
            const double e[] = {rel_err(g, pxx), rel_err(gs, sxx), rel_err(gre, re, den), rel_err(gim, im, den), rel_err(gxx, pxx), rel_err(gyy, pyy)};
            for (double v : e) {
                if (!(v <= gate64)) std::printf("L=%zu P=%zu H=%zu F=%zu variant %d: rel-L2 %.3e\n", s.len, s.p, s.h, s.f, variant, v);
                EXPECT(v <= gate64);
            }
            std::vector<float> xf(x.begin(), x.end()), gf(bins);
            const std::vector<double> x32(xf.begin(), xf.end());
            PlannerPsd32 q(s.len, s.p, s.h, s.f, w, detrend ? Detrend::Constant : Detrend::None, sc, fs);
            psd_f32_with_planner(xf, gf, q);
            const std::vector<std::complex<ld>> f32x = spectra(x32, w, s, detrend);
            std::vector<ld> p32(bins, 0);
            for (size_t t = 0; t < seg; ++t)
                for (size_t k = 0; k < bins; ++k) p32[k] += sigma * ((k == 0 || 2 * k == s.f) ? 1 : 2) * std::norm(f32x[t * bins + k]) / (ld)seg;
            EXPECT(rel_err(gf, p32) <= gate32);
            EXPECT(!p.describe().empty() && p.workspace_len(3) > p.workspace_len(1) && p.workspace_len(1, true) > p.workspace_len(1));
            EXPECT(p.workspace_min(true) > p.workspace_min() && p.workspace_min() <= p.workspace_len(1));
            EXPECT(p.device_bytes() >= s.p * sizeof(double));
        }
    PlannerPsd64 hann(1000, 100, 50, 128);  // the Hann window the library builds
    std::vector<double> x = signal(1000, 7), out(hann.bins()), shorter(999), few(hann.bins() - 1), all(hann.segments() * hann.bins());
    psd_f64_with_planner(x, out, hann);
    psd_f64_with_planner(x, all, hann, false);
    for (size_t k = 0; k < out.size(); ++k) {  // the mean of the spectrogram over the segments is the Welch estimate
        ld m = 0;
        for (size_t t = 0; t < hann.segments(); ++t) m += all[t * hann.bins() + k];
        EXPECT(std::fabs((double)(m / (ld)hann.segments()) - out[k]) <= 4e-16 * out[k] * 8);
    }
    EXPECT(code_of([&] { psd_f64_with_planner(shorter, out, hann); }) == PHAST_ERR_PLANNER_SIZE);
    EXPECT(code_of([&] { psd_f64_with_planner(x, few, hann); }) == PHAST_ERR_LEN_MISMATCH);
    EXPECT(code_of([&] { psd_f64_with_planner(x, out, hann, false); }) == PHAST_ERR_LEN_MISMATCH);
    EXPECT(code_of([&] { csd_f64_with_planner(x, shorter, out, out, hann); }) == PHAST_ERR_PLANNER_SIZE);
}

int main(int argc, char **argv) {
    const bool on_gpu = argc > 1 && std::string(argv[1]) == "gpu";
    if (on_gpu)
        gpu();
    else
        no_gpu();
    if (failures) {
        std::printf("psd: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("psd: ok\n");
    return 0;
}
