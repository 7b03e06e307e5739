// planner_lomb.hpp -- LombPlanner<T>: the generalised Lomb-Scargle periodogram of M unevenly spaced samples at K frequencies
// (lomb.hpp).  It owns one NufftT3Planner<T>(t, f, eps), run Reverse (the + sign) on real strengths, the M
// weights and four tables of K values (cos tau, sin tau, 1 / CCt, 1 / SSt) on the device: immutable after init, no per-call
// state.  The tables depend on (t, f, w) alone.  init builds them in double for both types: temporary f64 type-3 planners
// transform the weights at f (A0, floating mean only) and at 2 f (A2) through their host-slice call and are freed before
// init returns; lomb_table then runs on the host and the values are rounded to T.
//
// The caller's workspace, from its first 16-byte boundary on, for a chunk of c signals:
//     strength  c md elements of T        md = M rounded up to 16 bytes
//     re, im    c kd each                 kd = K rounded up to 16 bytes: A1's planes
//     type 3    the inner planner's workspace_len(c)
//     doubles   c (2 + 2 slabs): Y - y_0 and YY of each signal, then the partials of the two passes
// workspace_len(batch) holds the batch in one chunk; any length >= workspace_min() (one signal) runs the largest chunk that
// fits.  A signal never straddles two chunks, so the result's bits do not depend on the chunking.
#pragma once

#include <vector>

#include "lomb.hpp"
#include "planner_nufft_t3.hpp"

namespace phast {

template <typename T> struct LombPlanner {
    static constexpr size_t V = 16 / sizeof(T), D = sizeof(double) / sizeof(T);
    size_t m = 0, k = 0, md = 0, kd = 0, q = 0, slabs = 0;
    int floating_mean = 0;
    double eps = 0, inv_wsum = 1;  // 1 / the sum of the weights as rounded to T
    T *d_w = nullptr, *d_tab = nullptr;  // md weights; 4 kd table values
    NufftT3Planner<T> t3;

    ~LombPlanner() {
        DeviceGuard on(t3.inner.device);
        if (d_w) hipFree(d_w);
        if (d_tab) hipFree(d_tab);
    }

    // A = sum_j w_j exp(+2 pi i s_k t_j) in double, through a temporary f64 planner's host-slice call
    static int table_sums(const double *t, size_t m, const double *s, size_t k, const double *w, double eps, double *re, double *im) {
        NufftT3Planner<double> tmp;
        int rc = tmp.init(t, m, s, k, eps);
        return rc ? rc : tmp.nufft_host(PHAST_REVERSE, w, nullptr, m, re, im, k);
    }

    // the arguments were checked by lomb_planner_new; `w`: the M normalised weights, `f2` = 2 f
    int init(const double *t, size_t m_, const double *f, const double *f2, size_t k_, const std::vector<double> &w, int floating,
             double eps_, double table_eps) {
        m = m_;
        k = k_;
        md = (m + V - 1) / V * V;
        kd = (k + V - 1) / V * V;
        q = (size_t)lomb_slab_len(m);
        slabs = (size_t)lomb_slabs(m, q);
        floating_mean = floating;
        eps = eps_;
        int rc = t3.init(t, m, f, k, eps);
        if (rc) return rc;
        std::vector<double> c(k, 0.0), s(k, 0.0), c2(k), s2(k);
        if (floating_mean && (rc = table_sums(t, m, f, k, w.data(), table_eps, c.data(), s.data()))) return rc;
        if ((rc = table_sums(t, m, f2, k, w.data(), table_eps, c2.data(), s2.data()))) return rc;
        std::vector<T> tab(4 * kd, T(1)), wt(md, T(0));  // (the padding of the tables is never stored from)
        const double epsneg = lomb_epsneg(sizeof(T) == 4);
        for (size_t i = 0; i < k; ++i) {
            double ct, st, cct, sst;
            lomb_table(c[i], s[i], c2[i], s2[i], floating_mean, epsneg, &ct, &st, &cct, &sst);
            tab[i] = (T)ct;
            tab[kd + i] = (T)st;
            tab[2 * kd + i] = (T)(1.0 / cct);
            tab[3 * kd + i] = (T)(1.0 / sst);
        }
        long double sum = 0;
        for (size_t j = 0; j < m; ++j) {
            wt[j] = (T)w[j];
            sum += (long double)wt[j];
        }
        if (!(sum > 0)) return PHAST_ERR_INVALID_ARG;  // every weight rounds to 0 in T
        inv_wsum = (double)(1.0L / sum);
        PHAST_ON_DEVICE(t3.inner.device);
        PHAST_HIP(hipMalloc(reinterpret_cast<void **>(&d_w), md * sizeof(T)));
        PHAST_HIP(hipMalloc(reinterpret_cast<void **>(&d_tab), 4 * kd * sizeof(T)));
        PHAST_HIP(hipMemcpy(d_w, wt.data(), md * sizeof(T), hipMemcpyHostToDevice));
        PHAST_HIP(hipMemcpy(d_tab, tab.data(), 4 * kd * sizeof(T), hipMemcpyHostToDevice));
        return PHAST_OK;
    }

    // elements of T of a chunk of c signals (and V - 1 more to align the caller's base)
    size_t need(size_t c) const { return c * (md + 2 * kd) + t3.workspace_len(c) + c * (2 + 2 * slabs) * D + (V - 1); }
    size_t workspace_len(size_t batch) const { return need(batch ? batch : 1); }
    size_t workspace_min() const { return need(1); }
    size_t device_bytes() const { return t3.device_bytes() + (md + 4 * kd) * sizeof(T); }
    std::string describe() const {
        return "lomb M=" + std::to_string(m) + " K=" + std::to_string(k) + (floating_mean ? " floating_mean" : " fixed_mean") +
               " slab=" + std::to_string(q) + " x " + std::to_string(slabs) + " around " + t3.describe();
    }

    // the checks of a _dev call, before the device is touched
    int check_dev(const T *y, const T *out_re, const T *out_im, size_t points, size_t batch, size_t sig_dist, size_t out_dist, int norm,
                  const T *d_work, size_t work_len) const {
        if (norm < kLombPower || norm > kLombAmplitude) return PHAST_ERR_INVALID_ARG;
        if (!y || !out_re || (norm == kLombAmplitude && !out_im)) return PHAST_ERR_INVALID_ARG;
        if (points != m) return PHAST_ERR_PLANNER_SIZE;
        if (batch > 1 && (sig_dist < m || out_dist < k)) return PHAST_ERR_INVALID_ARG;
        if (batch && (!d_work || (reinterpret_cast<uintptr_t>(d_work) % sizeof(T)) || work_len < workspace_min()))
            return PHAST_ERR_INVALID_ARG;
        return PHAST_OK;
    }

    // the caller's workspace from its first 16-byte boundary on; the signals of a chunk: the most that fit, at least one
    size_t chunk_of(T *d_work, size_t work_len, size_t batch, T **w) const {
        const size_t skip = ((16 - (reinterpret_cast<uintptr_t>(d_work) & 15u)) & 15u) / sizeof(T);
        *w = d_work + skip;
        const size_t avail = work_len - skip + (V - 1);
        size_t lo = 1, hi = batch;  // need() grows with c
        while (lo < hi) {
            const size_t mid = lo + (hi - lo + 1) / 2;
            if (need(mid) <= avail) lo = mid;
            else hi = mid - 1;
        }
        return lo;
    }

    // device pointers, asynchronous on `s`: signal b at d_y + b sig_dist, its K results at d_out_re + b out_dist (and, for
    // amplitude, d_out_im + b out_dist).  ev (time_stages): 4 events around the pre-sweeps, the type-3 call and the post
    // sweep of a call that fits one chunk
    int run(const T *d_y, T *d_out_re, T *d_out_im, size_t points, size_t batch, size_t sig_dist, size_t out_dist, int norm,
            T *d_work, size_t work_len, hipStream_t s, hipEvent_t *ev = nullptr) const {
        int rc = check_dev(d_y, d_out_re, d_out_im, points, batch, sig_dist, out_dist, norm, d_work, work_len);
        if (rc) return rc;
        if (batch == 0) return PHAST_OK;
        if (batch == 1) {
            sig_dist = m;
            out_dist = k;
        }
        PHAST_ON_DEVICE(t3.inner.device);
        T *w = nullptr;
        const size_t chunk = chunk_of(d_work, work_len, batch, &w);
        const bool amp = norm == kLombAmplitude;
        for (size_t b0 = 0; b0 < batch; b0 += chunk) {
            const size_t c = batch - b0 < chunk ? batch - b0 : chunk;
            T *strength = w, *re = strength + c * md, *im = re + c * kd, *tw = im + c * kd;
            const size_t tl = t3.workspace_len(c);
            double *stat = reinterpret_cast<double *>(tw + tl), *part = stat + 2 * c;
            LombArgs a{};
            a.y = d_y + b0 * sig_dist;
            a.w = d_w;
            a.stat = stat;
            a.strength = strength;
            a.re = re;
            a.im = im;
            for (int i = 0; i < 4; ++i) a.tab[i] = d_tab + i * kd;
            a.out_re = d_out_re + b0 * out_dist;
            a.out_im = amp ? d_out_im + b0 * out_dist : nullptr;
            a.sig_dist = sig_dist;
            a.out_dist = out_dist;
            a.m = m;
            a.k = k;
            a.md = md;
            a.kd = kd;
            a.q = q;
            a.slabs = slabs;
            a.floating_mean = floating_mean;
            a.norm = norm;
            if (ev) PHAST_HIP(hipEventRecord(ev[0], s));
            if (floating_mean) {
                a.part = part;
                a.groups = c * slabs * 256;
                PHAST_HIP(launch_lomb<T>(kLombPartial, false, a, s));
                a.which = 0;
                a.scale = inv_wsum;
                a.groups = c * 256;
                PHAST_HIP(launch_lomb<T>(kLombFinal, false, a, s));
            }
            a.part = part + c * slabs;
            a.groups = c * slabs * 256;
            PHAST_HIP(launch_lomb<T>(kLombStrength, false, a, s));
            a.which = 1;
            a.scale = inv_wsum;
            a.groups = c * 256;
            PHAST_HIP(launch_lomb<T>(kLombFinal, false, a, s));
            if (ev) PHAST_HIP(hipEventRecord(ev[1], s));
            rc = t3.nufft_dev(PHAST_REVERSE, strength, nullptr, md, re, im, kd, c, tw, tl, s);
            if (rc) return rc;
            if (ev) PHAST_HIP(hipEventRecord(ev[2], s));
            a.scale = (double)m / 4;
            a.gpt = (unsigned)(kd / V);
            a.groups = c * a.gpt;
            const bool vec = t3.inner.aligned(a.out_re) && (!amp || t3.inner.aligned(a.out_im)) && (c == 1 || out_dist % V == 0);
            PHAST_HIP(launch_lomb<T>(kLombPost, vec, a, s));
            if (ev) PHAST_HIP(hipEventRecord(ev[3], s));
        }
        return PHAST_OK;
    }

    // host slices: one signal through device buffers of the call's own on the null stream; blocking.  out_im and im_len are
    // read for amplitude only
    int host(const T *y, size_t points, T *out_re, size_t re_len, T *out_im, size_t im_len, int norm) const {
        if (norm < kLombPower || norm > kLombAmplitude) return PHAST_ERR_INVALID_ARG;
        const bool amp = norm == kLombAmplitude;
        if (!y || !out_re || (amp && !out_im)) return PHAST_ERR_INVALID_ARG;
        if (points != m) return PHAST_ERR_PLANNER_SIZE;
        if (re_len != k || (amp && im_len != k)) return PHAST_ERR_LEN_MISMATCH;
        PHAST_ON_DEVICE(t3.inner.device);
        const size_t nw = workspace_len(1);
        DevBuf buf;
        int rc = buf.alloc((md + 2 * kd + nw) * sizeof(T));
        if (rc) return rc;
        T *d_y = reinterpret_cast<T *>(buf.p), *d_re = d_y + md, *d_im = d_re + kd, *d_wk = d_im + kd;
        PHAST_HIP(hipMemcpy(d_y, y, m * sizeof(T), hipMemcpyHostToDevice));
        rc = run(d_y, d_re, amp ? d_im : nullptr, m, 1, m, k, norm, d_wk, nw, nullptr);
        if (rc) return rc;
        PHAST_HIP(hipMemcpy(out_re, d_re, k * sizeof(T), hipMemcpyDeviceToHost));
        if (amp) PHAST_HIP(hipMemcpy(out_im, d_im, k * sizeof(T), hipMemcpyDeviceToHost));
        return PHAST_OK;
    }

    // measurement hook: ms[0..2] = the pre-sweeps (partial, final, strength, final), the type-3 call and the post sweep,
    // average milliseconds over `reps` calls of `batch` signals at the natural distances in one chunk (work_len >=
    // workspace_len(batch)); blocks
    int time_stages(const T *d_y, T *d_out_re, T *d_out_im, size_t batch, int norm, T *d_work, size_t work_len, int reps, float *ms,
                    hipStream_t s) const {
        if (!ms || reps < 1 || batch == 0) return PHAST_ERR_INVALID_ARG;
        int rc = check_dev(d_y, d_out_re, d_out_im, m, batch, m, k, norm, d_work, work_len);
        if (rc) return rc;
        if (work_len < workspace_len(batch)) return PHAST_ERR_INVALID_ARG;
        PHAST_ON_DEVICE(t3.inner.device);
        struct Events {
            hipEvent_t e[4] = {};
            ~Events() {
                for (hipEvent_t x : e)
                    if (x) hipEventDestroy(x);
            }
        } ev;
        for (hipEvent_t &x : ev.e) PHAST_HIP(hipEventCreate(&x));
        double acc[3] = {0, 0, 0};
        for (int r = 0; r < reps; ++r) {
            rc = run(d_y, d_out_re, d_out_im, m, batch, m, k, norm, d_work, work_len, s, ev.e);
            if (rc) return rc;
            PHAST_HIP(hipStreamSynchronize(s));
            for (int i = 0; i < 3; ++i) {
                float t = 0;
                PHAST_HIP(hipEventElapsedTime(&t, ev.e[i], ev.e[i + 1]));
                acc[i] += t;
            }
        }
        for (int i = 0; i < 3; ++i) ms[i] = (float)(acc[i] / reps);
        return PHAST_OK;
    }
};

// every argument rule, before the device is touched: the counts, the values, eps, and both type-3 grids -- the one of 2 f,
// which only the tables need, included
template <typename T, typename P>
static int lomb_planner_new(const double *t, size_t m, const double *freqs, size_t k, const double *weights, int floating_mean,
                            double eps, P **out) {
    if (!out) return PHAST_ERR_INVALID_ARG;
    *out = nullptr;
    constexpr bool f32 = sizeof(T) == 4;
    if (lomb_bad_args(t, m, freqs, k, weights)) return PHAST_ERR_INVALID_ARG;
    if (floating_mean != 0 && floating_mean != 1) return PHAST_ERR_INVALID_ARG;
    std::vector<double> f2(k);
    for (size_t i = 0; i < k; ++i) f2[i] = 2 * freqs[i];
    const double table_eps = f32 ? 1e-10 : 1e-14;  // the tables are built in f64 for both types
    if (nufft_t3_bad_args(t, m, freqs, k, eps, f32) || nufft_t3_bad_args(t, m, freqs, k, table_eps, false) ||
        nufft_t3_bad_args(t, m, f2.data(), k, table_eps, false))
        return PHAST_ERR_INVALID_ARG;
    std::vector<double> w(m);
    lomb_weights(weights, m, w.data());
    auto *p = new (std::nothrow) P();
    if (!p) return PHAST_ERR_ALLOC;
    int rc = p->init(t, m, freqs, f2.data(), k, w, floating_mean, eps, table_eps);
    if (rc) {
        delete p;
        return rc;
    }
    *out = p;
    return PHAST_OK;
}

}  // namespace phast
