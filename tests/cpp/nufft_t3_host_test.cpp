// nufft_t3_host_test.cpp -- the type-3 non-uniform FFT through the C++ mirror (include/phastft.hpp).
//     nufft_t3_host_test args     every argument error of the C ABI comes back as phastft::Panic with the C ABI's code, from the
//                                 planner's constructor and from the one-shot form; needs no device (the checks come first)
//     nufft_t3_host_test values   one transform through a planner and one through the one-shot form, in f64 and in f32, against
//                                 values tests/test_nufft_t3_cpp_host.py computed with tests/nufft_t3_reference.py and writes to
//                                 stdin: m k, then per dtype "eps gate_rel gate_bin", then x[m] s[k], c re[m] im[m], want re[k] im[k]
#include <cmath>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <limits>
#include <vector>

#include "phastft.hpp"

namespace {

int g_fails = 0;

void fail(const char *what) {
    ++g_fails;
    std::printf("FAIL %s\n", what);
}

// f() must throw Panic with `code`
template <typename F> void refused(const char *what, int code, F &&f) {
    try {
        f();
        fail(what);
    } catch (const phastft::Panic &p) {
        if (p.code != code) fail(what);
    } catch (const std::exception &) {
        fail(what);
    }
}

template <typename T, typename Planner, typename Shot> void args(const char *name, double eps_low, Shot one_shot) {
    using phastft::Slice;
    const std::vector<double> one{0.5}, two{-1.0, 1.0}, nan{0.5, std::numeric_limits<double>::quiet_NaN()},
        inf{std::numeric_limits<double>::infinity(), 0.5}, wide{-4e7, 4e7}, none;
    std::vector<T> c(2), o(2);
    const int inv = PHAST_ERR_INVALID_ARG;
    std::printf("%s\n", name);
    refused("no sources", inv, [&] { Planner p(none, one, 1e-3); });
    refused("no targets", inv, [&] { Planner p(one, none, 1e-3); });
    refused("null sources", inv, [&] { Planner p(Slice<const double>{nullptr, 1}, one, 1e-3); });
    refused("null targets", inv, [&] { Planner p(one, Slice<const double>{nullptr, 1}, 1e-3); });
    refused("too many sources", inv, [&] { Planner p(Slice<const double>{one.data(), (std::size_t(1) << 30) + 1}, one, 1e-3); });
    refused("too many targets", inv, [&] { Planner p(one, Slice<const double>{one.data(), (std::size_t(1) << 30) + 1}, 1e-3); });
    refused("eps above", inv, [&] { Planner p(one, one, 0.11); });
    refused("eps below", inv, [&] { Planner p(one, one, eps_low); });
    refused("a NaN source", inv, [&] { Planner p(nan, one, 1e-3); });
    refused("an infinite target", inv, [&] { Planner p(one, inf, 1e-3); });
    refused("a grid beyond 2^28", inv, [&] { Planner p(wide, two, 1e-3); });   // 8 S X = 3.2e8
    refused("one-shot: eps", inv, [&] { one_shot(two, two, c, c, o, o, 0.5); });
    refused("one-shot: a NaN source", inv, [&] { one_shot(nan, two, c, c, o, o, 1e-3); });
    refused("one-shot: sources and values differ", PHAST_ERR_LEN_MISMATCH, [&] { one_shot(one, two, c, c, o, o, 1e-3); });
    refused("one-shot: targets and outputs differ", PHAST_ERR_LEN_MISMATCH, [&] { one_shot(two, one, c, c, o, o, 1e-3); });
    std::vector<T> shorter(1);
    refused("one-shot: planes differ", PHAST_ERR_LEN_MISMATCH, [&] { one_shot(two, two, c, shorter, o, o, 1e-3); });
}

std::vector<double> read(std::size_t n) {
    std::vector<double> v(n);
    for (auto &e : v)
        if (!(std::cin >> e)) {
            std::printf("FAIL short input\n");
            std::exit(2);
        }
    return v;
}

template <typename T>
void gate(const std::string &what, const std::vector<T> &re, const std::vector<T> &im, const std::vector<double> &w_re,
          const std::vector<double> &w_im, double g_rel, double g_bin) {
    double err = 0, ref = 0, worst = 0;
    for (std::size_t i = 0; i < re.size(); ++i) {
        const double dr = (double)re[i] - w_re[i], di = (double)im[i] - w_im[i];
        err += dr * dr + di * di;
        ref += w_re[i] * w_re[i] + w_im[i] * w_im[i];
        worst = std::fmax(worst, std::fmax(std::fabs(dr), std::fabs(di)));
    }
    const double rel = std::sqrt(err / ref), bin = worst / std::sqrt(ref / (double)re.size());
    std::printf("%s: rel %.3e / %.3e, element %.3e / %.3e\n", what.c_str(), rel, g_rel, bin, g_bin);
    if (!(rel <= g_rel && bin <= g_bin)) fail(what.c_str());
}

template <typename T> std::vector<T> as(const std::vector<double> &v) { return std::vector<T>(v.begin(), v.end()); }

template <typename T, typename Planner, typename With, typename Shot>
void values(const std::string &name, double eps, double g_rel, double g_bin, const std::vector<double> &x, const std::vector<double> &s,
            const std::vector<double> *d, With with_planner, Shot one_shot) {
    const std::size_t m = x.size(), k = s.size();
    const Planner planner(x, s, eps);
    if (planner.num_points() != m || planner.num_targets() != k || planner.grid_len() < 8 || (planner.grid_len() & (planner.grid_len() - 1)) ||
        planner.workspace_len(3) != 12 * planner.grid_len() || planner.width() < 2 || planner.describe().rfind("nufft_t3 M=", 0) != 0 ||
        planner.device_bytes() == 0)
        fail((name + ": the planner's getters").c_str());
    const std::vector<T> c_re = as<T>(d[0]), c_im = as<T>(d[1]);
    std::vector<T> o_re(k), o_im(k), p_re(k), p_im(k);
    with_planner(c_re, c_im, o_re, o_im, planner);
    gate(name + " value with a planner", o_re, o_im, d[2], d[3], g_rel, g_bin);
    one_shot(x, s, c_re, c_im, p_re, p_im, eps);
    gate(name + " value one-shot", p_re, p_im, d[2], d[3], g_rel, g_bin);
    if (std::memcmp(o_re.data(), p_re.data(), k * sizeof(T)) || std::memcmp(o_im.data(), p_im.data(), k * sizeof(T)))
        fail((name + ": the two forms differ").c_str());
    refused((name + ": a short output").c_str(), PHAST_ERR_PLANNER_SIZE, [&] {
        std::vector<T> a(k - 1), b(k - 1);
        with_planner(c_re, c_im, a, b, planner);
    });
}

}  // namespace

int main(int argc, char **argv) {
    using namespace phastft;
    auto shot64 = [](const std::vector<double> &x, const std::vector<double> &s, const std::vector<double> &a, const std::vector<double> &b,
                     std::vector<double> &o, std::vector<double> &p, double e) { nufft3_64(x, s, a, b, o, p, e); };
    auto shot32 = [](const std::vector<double> &x, const std::vector<double> &s, const std::vector<float> &a, const std::vector<float> &b,
                     std::vector<float> &o, std::vector<float> &p, double e) { nufft3_32(x, s, a, b, o, p, e); };
    if (argc == 2 && !std::strcmp(argv[1], "args")) {
        args<double, PlannerNufftT3_64>("f64", 0.9e-14, shot64);
        args<float, PlannerNufftT3_32>("f32", 0.9e-6, shot32);
    } else if (argc == 2 && !std::strcmp(argv[1], "values")) {
        std::size_t m, k;
        if (!(std::cin >> m >> k)) return 2;
        double eps[2], g_rel[2], g_bin[2];
        for (int i = 0; i < 2; ++i) std::cin >> eps[i] >> g_rel[i] >> g_bin[i];
        const std::vector<double> x = read(m), s = read(k);
        const std::size_t lens[4] = {m, m, k, k};
        std::vector<double> d[4];
        for (int i = 0; i < 4; ++i) d[i] = read(lens[i]);
        values<double, PlannerNufftT3_64>(
            "f64", eps[0], g_rel[0], g_bin[0], x, s, d,
            [](const std::vector<double> &a, const std::vector<double> &b, std::vector<double> &o, std::vector<double> &p,
               const PlannerNufftT3_64 &pl) { nufft3_64_with_planner(a, b, o, p, pl); },
            shot64);
        values<float, PlannerNufftT3_32>(
            "f32", eps[1], g_rel[1], g_bin[1], x, s, d,
            [](const std::vector<float> &a, const std::vector<float> &b, std::vector<float> &o, std::vector<float> &p,
               const PlannerNufftT3_32 &pl) { nufft3_32_with_planner(a, b, o, p, pl); },
            shot32);
    } else {
        return 2;
    }
    std::printf("nufft_t3 host: %s (%d failures)\n", g_fails ? "FAILED" : "ok", g_fails);
    return g_fails ? 1 : 0;
}
