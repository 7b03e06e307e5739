// dwt_test.cpp -- the C++ host side (include/phastft.hpp) of the discrete wavelet transform: PlannerDwt64/32, enum DwtMode,
// wavedec_f64/f32_with_planner, waverec_f64/f32_with_planner.  Built and run by tests/test_dwt_cpp_host.py: without a GPU the
// argument codes and a loud failure of the rest; with "gpu" the host forms against the definitions of include/phastft_hip.h in
// long double (db2 from its closed form, three levels, every mode), and the length codes.
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

using ld = long double;
using i64 = long long;

template <typename T> static std::vector<T> uniform(size_t n, unsigned seed) {
    std::vector<T> x(n);
    unsigned long long s = 0x9E3779B97F4A7C15ull * (seed + 1);
    for (size_t i = 0; i < n; ++i) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        x[i] = (T)(float)(-1.0 + 2.0 * ((double)(s >> 11) / 9007199254740992.0));
    }
    return x;
}

static i64 floor_mod(i64 a, i64 b) {
    const i64 r = a % b;
    return r < 0 ? r + b : r;
}
// the extension map of the header's comment: the index of ext(x, t), -1 for a zero
static i64 ext(DwtMode mode, i64 n, i64 t) {
    switch (mode) {
    case DwtMode::Zero: return t >= 0 && t < n ? t : -1;
    case DwtMode::Constant: return t < 0 ? 0 : t >= n ? n - 1 : t;
    case DwtMode::Periodic: return floor_mod(t, n);
    case DwtMode::Symmetric: {
        const i64 u = floor_mod(t, 2 * n);
        return u < n ? u : 2 * n - 1 - u;
    }
    case DwtMode::Reflect: {
        if (n == 1) return 0;
        const i64 u = floor_mod(t, 2 * n - 2);
        return u < n ? u : 2 * n - 2 - u;
    }
    default: {
        const i64 u = floor_mod(t, n + n % 2);
        return u < n ? u : n - 1;
    }
    }
}

struct Level {
    std::vector<ld> a, d, abs_a, abs_d;  // the bands and the same sums of absolute values
};
// one analysis level of the values v (and of their absolute cascade w) by the definition
template <typename T>
static Level analyse(const std::vector<ld> &v, const std::vector<ld> &w, const std::vector<T> &lo, const std::vector<T> &hi, DwtMode mode) {
    const i64 n = (i64)v.size(), f = (i64)lo.size(), per = mode == DwtMode::Periodization;
    const i64 m = per ? (n + n % 2) / 2 : (n + f - 1) / 2;
    Level out;
    for (i64 i = 0; i < m; ++i) {
        ld a = 0, d = 0, aa = 0, ad = 0;
        for (i64 j = 0; j < f; ++j) {
            const i64 s = ext(mode, n, 2 * i + (per ? f / 2 : 1) - j);
            if (s < 0) continue;
            a += (ld)lo[j] * v[s];
            d += (ld)hi[j] * v[s];
            aa += std::fabs((ld)lo[j]) * w[s];
            ad += std::fabs((ld)hi[j]) * w[s];
        }
        out.a.push_back(a);
        out.d.push_back(d);
        out.abs_a.push_back(aa);
        out.abs_d.push_back(ad);
    }
    return out;
}

template <typename T, typename P, typename Dec, typename Rec> static void on_gpu(const char *name, Dec dec, Rec rec, ld u) {
    const ld s3 = std::sqrt((ld)3), den = 4 * std::sqrt((ld)2);
    const std::vector<T> rec_lo = {(T)((1 + s3) / den), (T)((3 + s3) / den), (T)((3 - s3) / den), (T)((1 - s3) / den)};
    const std::vector<T> dec_lo(rec_lo.rbegin(), rec_lo.rend());
    const std::vector<T> rec_hi = {rec_lo[3], (T)-rec_lo[2], rec_lo[1], (T)-rec_lo[0]};
    const std::vector<T> dec_hi(rec_hi.rbegin(), rec_hi.rend());
    const size_t L = 17, J = 3, F = 4;
    const std::vector<T> x = uniform<T>(L, 3);
    const DwtMode modes[] = {DwtMode::Zero, DwtMode::Constant, DwtMode::Symmetric, DwtMode::Reflect, DwtMode::Periodic, DwtMode::Periodization};
    ld worst = 0, worst_back = 0;
    for (DwtMode mode : modes) {
        P pl(L, Slice<const T>(dec_lo.data(), F), Slice<const T>(dec_hi.data(), F), Slice<const T>(rec_lo.data(), F),
             Slice<const T>(rec_hi.data(), F), J, mode);
        // the cascade by the definition
        std::vector<Level> levels;
        std::vector<ld> v(x.begin(), x.end()), w(L);
        for (size_t i = 0; i < L; ++i) w[i] = std::fabs(v[i]);
        for (size_t l = 1; l <= J; ++l) {
            levels.push_back(analyse(v, w, dec_lo, dec_hi, mode));
            v = levels.back().a;
            w = levels.back().abs_a;
            EXPECT(pl.level_len(l) == v.size());
        }
        size_t total = levels[J - 1].a.size();
        for (const Level &lv : levels) total += lv.d.size();
        EXPECT(pl.coeff_len() == total && pl.level_len(0) == L && pl.tile() == 1024);
        EXPECT(pl.workspace_min() == levels[0].a.size() + levels[1].a.size() && pl.workspace_len(3) == 3 * pl.workspace_min());
        EXPECT(pl.device_bytes() == 4 * F * sizeof(T));
        EXPECT(pl.describe().rfind("dwt L=17 F=4 J=3 mode=", 0) == 0);
        std::vector<T> packed(total, T(7));
        dec(Slice<const T>(x.data(), L), Slice<T>(packed.data(), total), pl);
        auto compare = [&](const std::vector<ld> &want, const std::vector<ld> &scale, size_t at, size_t level) {
            for (size_t i = 0; i < want.size(); ++i) {
                const ld gate = (ld)level * (ld)(F + 2) * u * scale[i], err = std::fabs((ld)packed[at + i] - want[i]);
                EXPECT(err <= gate);
                if (gate > 0) worst = std::max(worst, err / gate);
            }
        };
        compare(levels[J - 1].a, levels[J - 1].abs_a, 0, J);
        for (size_t l = J; l >= 1; --l) {
            EXPECT(pl.level_offset(l) + pl.level_len(l) <= total);
            compare(levels[l - 1].d, levels[l - 1].abs_d, pl.level_offset(l), l);
        }
        // and back: an orthogonal bank, so the signal returns; the gate of tests/test_gpu_dwt.py's round trip with the absolute
        // cascade bounded by its largest value (sum |h| <= 2 per stage: 4^J max|x| ... formed here from the packed values)
        std::vector<T> back(L, T(7));
        rec(Slice<const T>(packed.data(), total), Slice<T>(back.data(), L), pl);
        ld top = 0;
        for (T c : packed) top = std::max(top, std::fabs((ld)c));
        const ld gate = 2 * (ld)J * (ld)(F + 2) * u * top * std::pow((ld)2, (ld)J) + 8 * std::ldexp((ld)1, sizeof(T) == 8 ? -53 : -24);
        for (size_t i = 0; i < L; ++i) {
            EXPECT(std::fabs((ld)back[i] - (ld)x[i]) <= gate);
            worst_back = std::max(worst_back, std::fabs((ld)back[i] - (ld)x[i]) / gate);
        }
        std::vector<T> shorter(total - 1), fewer(L - 1);
        EXPECT(code_of([&] { dec(Slice<const T>(fewer.data(), L - 1), Slice<T>(packed.data(), total), pl); }) == PHAST_ERR_PLANNER_SIZE);
        EXPECT(code_of([&] { dec(Slice<const T>(x.data(), L), Slice<T>(shorter.data(), total - 1), pl); }) == PHAST_ERR_LEN_MISMATCH);
        EXPECT(code_of([&] { rec(Slice<const T>(shorter.data(), total - 1), Slice<T>(back.data(), L), pl); }) == PHAST_ERR_LEN_MISMATCH);
        EXPECT(code_of([&] { rec(Slice<const T>(packed.data(), total), Slice<T>(fewer.data(), L - 1), pl); }) == PHAST_ERR_PLANNER_SIZE);
    }
    std::printf("%s wavedec: %.3Lf of the gate; round trip: %.3Lf of its bound\n", name, worst, worst_back);
}

template <typename T, typename P> static void argument_codes() {
    const std::vector<T> h(258, T(1));
    auto make = [&](size_t len, size_t f, size_t level, int mode) {
        return code_of([&] {
            const Slice<const T> s(h.data(), f);
            P pl(len, s, s, s, s, level, static_cast<DwtMode>(mode));
        });
    };
    EXPECT(make(0, 4, 1, 2) == PHAST_ERR_INVALID_ARG);
    EXPECT(make((1u << 29) + 1, 4, 1, 2) == PHAST_ERR_INVALID_ARG);
    EXPECT(make(16, 0, 1, 2) == PHAST_ERR_INVALID_ARG);
    EXPECT(make(16, 3, 1, 2) == PHAST_ERR_INVALID_ARG);    // an odd filter
    EXPECT(make(16, 258, 1, 2) == PHAST_ERR_INVALID_ARG);  // too long
    EXPECT(make(16, 4, 0, 2) == PHAST_ERR_INVALID_ARG);
    EXPECT(make(16, 4, 33, 2) == PHAST_ERR_INVALID_ARG);
    EXPECT(make(16, 4, 1, 6) == PHAST_ERR_INVALID_ARG);    // an unknown mode
    EXPECT(make(16, 4, 1, -1) == PHAST_ERR_INVALID_ARG);
    EXPECT(code_of([&] {
               const Slice<const T> s(h.data(), 4), other(h.data(), 6);
               P pl(16, s, s, other, s);
           }) == PHAST_ERR_INVALID_ARG);  // filters of unequal lengths
    EXPECT(code_of([&] {
               const Slice<const T> s(h.data(), 4), none(nullptr, 4);
               P pl(16, s, none, s, s);
           }) == PHAST_ERR_INVALID_ARG);
    EXPECT(static_cast<int>(DwtMode::Zero) == PHAST_DWT_ZERO && static_cast<int>(DwtMode::Constant) == PHAST_DWT_CONSTANT &&
           static_cast<int>(DwtMode::Symmetric) == PHAST_DWT_SYMMETRIC && static_cast<int>(DwtMode::Reflect) == PHAST_DWT_REFLECT &&
           static_cast<int>(DwtMode::Periodic) == PHAST_DWT_PERIODIC && static_cast<int>(DwtMode::Periodization) == PHAST_DWT_PERIODIZATION);
}

int main(int argc, char **argv) {
    const bool gpu = argc > 1 && std::string(argv[1]) == "gpu";
    argument_codes<double, PlannerDwt64>();
    argument_codes<float, PlannerDwt32>();
    if (gpu) {
        on_gpu<double, PlannerDwt64>("f64", [](const auto &...a) { wavedec_f64_with_planner(a...); }, [](const auto &...a) { waverec_f64_with_planner(a...); },
                                     std::ldexp((ld)1, -53));
        on_gpu<float, PlannerDwt32>("f32", [](const auto &...a) { wavedec_f32_with_planner(a...); }, [](const auto &...a) { waverec_f32_with_planner(a...); },
                                    std::ldexp((ld)1, -24));
    } else {
        const std::vector<double> h = {0.5, 0.5};
        const Slice<const double> s(h.data(), 2);
        EXPECT(code_of([&] { PlannerDwt64 pl(10, s, s, s, s, 2, DwtMode::Periodization); }) == PHAST_ERR_NO_DEVICE);  // a good call gets past the checks and fails loudly
    }
    std::printf("dwt: %s (%d failures)\n", failures ? "FAILED" : "ok", failures);
    return failures ? 1 : 0;
}
