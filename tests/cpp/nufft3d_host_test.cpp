// nufft3d_host_test.cpp -- the three-dimensional non-uniform FFT through the C++ mirror (include/phastft.hpp): one type 1 through a
// planner and one type 2 through the one-shot form, in f64 and in f32, against values tests/test_nufft3d_cpp_host.py computed
// with tests/nufft3d_reference.py and writes to stdin:
//     n1 n2 n3 m, then per dtype "eps gate_rel gate_bin", then x[m] y[m] z[m], c re[m] im[m], want F re[n] im[n] (type 1 Forward),
//     F re[n] im[n], want c re[m] im[m] (type 2 Forward)
#include <cmath>
#include <cstdio>
#include <iostream>
#include <vector>

#include "phastft.hpp"

namespace {

int g_fails = 0;

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
void gate(const char *what, const std::vector<T> &re, const std::vector<T> &im, const std::vector<double> &w_re, const std::vector<double> &w_im,
          double g_rel, double g_bin) {
    double err = 0, ref = 0, worst = 0;
    for (std::size_t i = 0; i < re.size(); ++i) {
        const double dr = (double)re[i] - w_re[i], di = (double)im[i] - w_im[i];
        err += dr * dr + di * di;
        ref += w_re[i] * w_re[i] + w_im[i] * w_im[i];
        worst = std::fmax(worst, std::sqrt(dr * dr + di * di));
    }
    const double rel = std::sqrt(err / ref), bin = worst / std::sqrt(ref / (double)re.size());
    std::printf("%s: rel %.3e / %.3e, element %.3e / %.3e\n", what, rel, g_rel, bin, g_bin);
    if (!(rel <= g_rel && bin <= g_bin)) {
        ++g_fails;
        std::printf("FAIL %s\n", what);
    }
}

template <typename T> std::vector<T> as(const std::vector<double> &v) { return std::vector<T>(v.begin(), v.end()); }

template <typename T, typename Planner, typename With, typename Shot>
void run(const char *name, std::size_t n1, std::size_t n2, std::size_t n3, std::size_t m, double eps, double g_rel, double g_bin, const std::vector<double> &x,
         const std::vector<double> &y, const std::vector<double> &z, const std::vector<double> *d, With with_planner, Shot one_shot) {
    const std::size_t n = n1 * n2 * n3;
    const Planner planner(n1, n2, n3, x, y, z, eps);
    if (planner.num_modes_1() != n1 || planner.num_modes_2() != n2 || planner.num_modes_3() != n3 || planner.num_points() != m ||
        planner.grid_len() != planner.grid_dim(0) * planner.grid_dim(1) * planner.grid_dim(2) || planner.grid_dim(3) != 0 || planner.workspace_len(3) != 12 * planner.grid_len() ||
        planner.width() < 2 || planner.describe().rfind("nufft3d N=", 0) != 0 || planner.device_bytes() == 0) {
        ++g_fails;
        std::printf("FAIL %s: the planner's getters\n", name);
    }
    const std::vector<T> c_re = as<T>(d[0]), c_im = as<T>(d[1]), f_re = as<T>(d[4]), f_im = as<T>(d[5]);
    std::vector<T> o_re(n), o_im(n), p_re(m), p_im(m);
    with_planner(c_re, c_im, o_re, o_im, planner);
    gate((std::string(name) + " type 1 with a planner").c_str(), o_re, o_im, d[2], d[3], g_rel, g_bin);
    one_shot(x, y, z, f_re, f_im, p_re, p_im, n1, n2, n3, eps);
    gate((std::string(name) + " type 2 one-shot").c_str(), p_re, p_im, d[6], d[7], g_rel, g_bin);
    try {  // a wrong length is a panic, not a wrong answer
        std::vector<T> shorter(n - 1);
        with_planner(c_re, c_im, shorter, shorter, planner);
        ++g_fails;
        std::printf("FAIL %s: a short output was accepted\n", name);
    } catch (const std::exception &) {
    }
}

}  // namespace

int main() {
    std::size_t n1, n2, n3, m;
    if (!(std::cin >> n1 >> n2 >> n3 >> m)) return 2;
    double eps[2], g_rel[2], g_bin[2];
    for (int k = 0; k < 2; ++k) std::cin >> eps[k] >> g_rel[k] >> g_bin[k];
    const std::vector<double> x = read(m), y = read(m), z = read(m);
    const std::size_t n = n1 * n2 * n3, lens[8] = {m, m, n, n, n, n, m, m};
    std::vector<double> d[8];
    for (int k = 0; k < 8; ++k) d[k] = read(lens[k]);
    using namespace phastft;
    run<double, PlannerNufft3d64>(
        "f64", n1, n2, n3, m, eps[0], g_rel[0], g_bin[0], x, y, z, d,
        [](const std::vector<double> &a, const std::vector<double> &b, std::vector<double> &o, std::vector<double> &p, const PlannerNufft3d64 &pl) {
            nufft3d1_64_with_planner(a, b, o, p, pl);
        },
        [](const std::vector<double> &px, const std::vector<double> &py, const std::vector<double> &pz, const std::vector<double> &a,
           const std::vector<double> &b, std::vector<double> &o, std::vector<double> &p, std::size_t r, std::size_t c, std::size_t l, double e) {
            nufft3d2_64(px, py, pz, a, b, o, p, r, c, l, e);
        });
    run<float, PlannerNufft3d32>(
        "f32", n1, n2, n3, m, eps[1], g_rel[1], g_bin[1], x, y, z, d,
        [](const std::vector<float> &a, const std::vector<float> &b, std::vector<float> &o, std::vector<float> &p, const PlannerNufft3d32 &pl) {
            nufft3d1_32_with_planner(a, b, o, p, pl);
        },
        [](const std::vector<double> &px, const std::vector<double> &py, const std::vector<double> &pz, const std::vector<float> &a,
           const std::vector<float> &b, std::vector<float> &o, std::vector<float> &p, std::size_t r, std::size_t c, std::size_t l, double e) {
            nufft3d2_32(px, py, pz, a, b, o, p, r, c, l, e);
        });
    std::printf("nufft3d host: %s (%d failures)\n", g_fails ? "FAILED" : "ok", g_fails);
    return g_fails ? 1 : 0;
}
