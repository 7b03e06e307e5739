// nufft_dev_points_host_test.cpp -- NUFFT planners built from points in device memory and re-pointed in place, through the C++
// mirror (include/phastft.hpp) over the C ABI: from_device and set_points_dev of a 1-D and of a 3-D planner, f64 and f32.  Every
// output must EQUAL, bit for bit, that of a planner the host constructor built at the same points
// (tests/test_nufft_dev_points_cpp_host.py builds and runs it).  The program makes its own points and data: the comparison needs no
// reference values.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "phastft.hpp"

#define HIP_OK(x)                                                        \
    do {                                                                 \
        if ((x) != hipSuccess) {                                         \
            std::printf("FAIL %s\n", #x);                                \
            std::exit(2);                                                \
        }                                                                \
    } while (0)

namespace {

int g_fails = 0, g_compared = 0;

double rnd(unsigned long long seed, unsigned long long i) {  // uniform in [0, 1)
    unsigned long long x = seed * 0x9E3779B97F4A7C15ull + i * 0xD1B54A32D192ED03ull + 0x2545F4914F6CDD1Dull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    x ^= x >> 31;
    return (double)(x >> 11) * 0x1p-53;
}

// uniform in [-3, 3), every fourth point one of three values: cells with ties
std::vector<double> points(unsigned long long seed, std::size_t m) {
    const double tie[3] = {0.3, -0.7, 1.3};
    std::vector<double> x(m);
    for (std::size_t j = 0; j < m; ++j) x[j] = j % 4 == 3 ? tie[(j / 4) % 3] : 6.0 * rnd(seed, j) - 3.0;
    return x;
}

template <typename E> struct Dev {
    E *p = nullptr;
    std::size_t n;
    explicit Dev(std::size_t n_) : n(n_) { HIP_OK(hipMalloc((void **)&p, (n ? n : 1) * sizeof(E))); }
    explicit Dev(const std::vector<E> &h) : Dev(h.size()) { HIP_OK(hipMemcpy(p, h.data(), n * sizeof(E), hipMemcpyHostToDevice)); }
    ~Dev() { (void)hipFree(p); }
    Dev(const Dev &) = delete;
    std::vector<E> host() const {
        std::vector<E> h(n);
        HIP_OK(hipMemcpy(h.data(), p, n * sizeof(E), hipMemcpyDeviceToHost));
        return h;
    }
};

// both types, Forward, through `planner` on device data: the four output planes, concatenated
template <typename T, typename CT, typename Dev1, typename Dev2>
std::vector<T> outputs(const CT *planner, std::size_t modes, std::size_t m, std::size_t work_len, Dev1 type1, Dev2 type2) {
    std::vector<T> c_re(m), c_im(m), f_re(modes), f_im(modes);
    for (std::size_t j = 0; j < m; ++j) c_re[j] = (T)(2 * rnd(5, j) - 1), c_im[j] = (T)(2 * rnd(6, j) - 1);
    for (std::size_t k = 0; k < modes; ++k) f_re[k] = (T)(2 * rnd(7, k) - 1), f_im[k] = (T)(2 * rnd(8, k) - 1);
    Dev<T> d_c_re(c_re), d_c_im(c_im), d_f_re(f_re), d_f_im(f_im), o1_re(modes), o1_im(modes), o2_re(m), o2_im(m), work(work_len);
    phastft::check(type1(d_c_re.p, d_c_im.p, m, o1_re.p, o1_im.p, modes, 1, PHAST_FORWARD, planner, work.p, work_len, nullptr));
    phastft::check(type2(d_f_re.p, d_f_im.p, modes, o2_re.p, o2_im.p, m, 1, PHAST_FORWARD, planner, work.p, work_len, nullptr));
    HIP_OK(hipDeviceSynchronize());
    std::vector<T> all;
    for (const Dev<T> *d : {&o1_re, &o1_im, &o2_re, &o2_im}) {
        const std::vector<T> h = d->host();
        all.insert(all.end(), h.begin(), h.end());
    }
    return all;
}

template <typename T> void same(const char *what, const std::vector<T> &got, const std::vector<T> &want) {
    ++g_compared;
    const bool ok = got.size() == want.size() && std::memcmp(got.data(), want.data(), got.size() * sizeof(T)) == 0;
    std::printf("%s: %s\n", what, ok ? "equal" : "DIFFERENT");
    if (!ok) {
        ++g_fails;
        std::printf("FAIL %s\n", what);
    }
}

template <typename T, typename Planner, typename Dev1, typename Dev2> void one_d(const char *name, double eps, Dev1 type1, Dev2 type2) {
    const std::size_t n = 1000, m = 4099;
    const std::vector<double> a = points(1, m), b = points(2, m);
    Dev<double> d_a(a), d_b(b);
    char what[96];
    auto out = [&](const Planner &p) { return outputs<T>(p.get(), n, m, p.workspace_len(1), type1, type2); };
    const Planner host_a(n, a, eps), host_b(n, b, eps);
    Planner dev = Planner::from_device(n, d_a.p, m, eps);
    if (dev.num_modes() != n || dev.num_points() != m || dev.grid_len() != host_a.grid_len() || dev.device_bytes() != host_a.device_bytes()) {
        ++g_fails;
        std::printf("FAIL %s: the getters of the planner from device points\n", name);
    }
    std::snprintf(what, sizeof what, "%s 1-D from_device", name);
    same(what, out(dev), out(host_a));
    dev.set_points_dev(d_b.p, m);
    std::snprintf(what, sizeof what, "%s 1-D set_points_dev", name);
    same(what, out(dev), out(host_b));
    Planner built_on_host(n, a, eps);
    built_on_host.set_points_dev(d_b.p, m);
    std::snprintf(what, sizeof what, "%s 1-D set_points_dev of a host-built planner", name);
    same(what, out(built_on_host), out(host_b));
}

template <typename T, typename Planner, typename Dev1, typename Dev2> void three_d(const char *name, double eps, Dev1 type1, Dev2 type2) {
    const std::size_t n1 = 5, n2 = 7, n3 = 3, m = 4500;
    const std::vector<double> ax = points(11, m), ay = points(12, m), az = points(13, m), bx = points(14, m), by = points(15, m), bz = points(16, m);
    Dev<double> d_ax(ax), d_ay(ay), d_az(az), d_bx(bx), d_by(by), d_bz(bz);
    char what[96];
    auto out = [&](const Planner &p) { return outputs<T>(p.get(), n1 * n2 * n3, m, p.workspace_len(1), type1, type2); };
    const Planner host_a(n1, n2, n3, ax, ay, az, eps), host_b(n1, n2, n3, bx, by, bz, eps);
    Planner dev = Planner::from_device(n1, n2, n3, d_ax.p, d_ay.p, d_az.p, m, eps);
    if (dev.num_modes_3() != n3 || dev.num_points() != m || dev.grid_len() != host_a.grid_len() || dev.device_bytes() != host_a.device_bytes()) {
        ++g_fails;
        std::printf("FAIL %s: the getters of the planner from device points\n", name);
    }
    std::snprintf(what, sizeof what, "%s 3-D from_device", name);
    same(what, out(dev), out(host_a));
    dev.set_points_dev(d_bx.p, d_by.p, d_bz.p, m);
    std::snprintf(what, sizeof what, "%s 3-D set_points_dev", name);
    same(what, out(dev), out(host_b));
}

}  // namespace

int main() {
    using namespace phastft;
    try {
        one_d<double, PlannerNufft64>("f64", 1e-9, phast_nufft1_64_dev, phast_nufft2_64_dev);
        one_d<float, PlannerNufft32>("f32", 1e-5, phast_nufft1_32_dev, phast_nufft2_32_dev);
        three_d<double, PlannerNufft3d64>("f64", 1e-9, phast_nufft3d1_64_dev, phast_nufft3d2_64_dev);
        three_d<float, PlannerNufft3d32>("f32", 1e-5, phast_nufft3d1_32_dev, phast_nufft3d2_32_dev);
    } catch (const std::exception &e) {
        std::printf("FAIL exception: %s\n", e.what());
        ++g_fails;
    }
    std::printf("nufft dev points host: %s (%d failures, %d comparisons)\n", g_fails ? "FAILED" : "ok", g_fails, g_compared);
    return g_fails ? 1 : 0;
}
