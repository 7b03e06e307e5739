// planner_czt.hpp -- CztPlanner<T>: the chirp-Z transform on the unit circle (czt.hpp), M bins of N points at start + k step
// turns, on the convolution core of the any-length planner (planner_any.hpp: ConvCore).  Immutable after init: the inner
// Planner<T>(L), the device table Bh = FFT_L(b) / L and the two fixed-point phases.  What a call mutates is the caller's
// workspace (_dev calls) or a workspace of the inner planner's pool (host-slice calls), so graph capture and concurrent
// streams and threads need nothing beyond what the engine already does.
#pragma once

#include "czt.hpp"
#include "planner_any.hpp"

namespace phast {

template <typename T> struct CztPlanner : ConvCore<T> {
    using ConvCore<T>::m;  // the convolution length L
    using ConvCore<T>::log_m;
    using ConvCore<T>::device;
    using ConvCore<T>::inner;
    using ConvCore<T>::engine;
    using ConvCore<T>::convolve;
    using ConvCore<T>::for_each_chunk;
    size_t n = 0, bins = 0;  // N input points, M output points
    double step = 0, start = 0;
    CztFrac half_step{0, 0}, start_frac{0, 0};

    int init(size_t num_points, size_t num_bins, double step_turns, double start_turns) {
        if (czt_bad_args(num_points, num_bins, step_turns, start_turns)) return PHAST_ERR_INVALID_ARG;
        n = num_points;
        bins = num_bins;
        step = step_turns;
        start = start_turns;
        half_step = czt_frac(step, 1);
        start_frac = czt_frac(start, 0);
        int rc = this->init_core((size_t)czt_conv_len(n, bins));
        if (rc) return rc;
        return this->make_table(
            [&](double *br, double *bi, hipStream_t s) { return launch_czt_chirp_b(br, bi, n, bins, log_m, half_step, s); });
    }

    size_t workspace_len(size_t batch) const { return 2 * m * batch; }
    size_t device_bytes() const { return 2 * m * sizeof(T) + (inner ? inner->device_bytes() : 0); }
    std::string describe() const {
        char f[96];
        std::snprintf(f, sizeof f, " step=%.17g start=%.17g", step, start);
        return "czt N=" + std::to_string(n) + " M=" + std::to_string(bins) + " L=" + std::to_string(m) + f + ": " + inner->describe();
    }

    // `c` transforms: x planes (re, im or null) at b * in_dist -> X planes at b * out_dist, through the workspace w (2 c L
    // elements).  ev: optional 6 events recorded around the five stages (time_stages)
    int run_chunk(const Planner<T> *pl, const typename Planner<T>::Lease &L, const typename Planner<T>::Choice &ch,
                  const T *x_re, const T *x_im, size_t in_dist, T *o_re, T *o_im, size_t out_dist, size_t c, T *w,
                  hipEvent_t *ev = nullptr) const {
        hipStream_t s = L.stream;
        constexpr unsigned V = 16 / sizeof(T);
        T *w_re = w, *w_im = w + c * m;
        auto al = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; };
        CztSweepArgs a{};
        a.log_l = log_m;
        a.in_dist = in_dist;
        a.out_dist = out_dist;
        a.half_step = half_step;
        a.start = start_frac;
        if (ev) PHAST_HIP(hipEventRecord(ev[0], s));
        a.n = n;
        a.in_re = x_re;
        a.in_im = x_im;
        a.out_re = w_re;
        a.out_im = w_im;
        a.groups = c * (m / V);
        PHAST_HIP(launch_czt_sweep<T>(0, al(x_re) && al(x_im) && in_dist % V == 0, a, s));
        int rc = convolve(pl, L, ch, w, c, ev);
        if (rc) return rc;
        a.n = bins;
        a.in_re = w_re;
        a.in_im = w_im;
        a.out_re = o_re;
        a.out_im = o_im;
        a.gpt = (unsigned)((bins + V - 1) / V);
        a.groups = c * a.gpt;
        PHAST_HIP(launch_czt_sweep<T>(2, al(o_re) && al(o_im) && out_dist % V == 0, a, s));
        if (ev) PHAST_HIP(hipEventRecord(ev[5], s));
        return PHAST_OK;
    }

    // the batch in chunks
    int run(const Planner<T> *pl, const typename Planner<T>::Lease &L, const T *x_re, const T *x_im, size_t in_dist, T *o_re,
            T *o_im, size_t out_dist, size_t batch, T *work, size_t work_len, hipEvent_t *ev = nullptr) const {
        const typename Planner<T>::Choice ch = pl->choose(kC2C, 1, 1);
        return for_each_chunk(batch, work_len, [&](size_t b0, size_t c) {
            return run_chunk(pl, L, ch, x_re + b0 * in_dist, x_im ? x_im + b0 * in_dist : nullptr, in_dist, o_re + b0 * out_dist,
                             o_im + b0 * out_dist, out_dist, c, work, ev);
        });
    }

    // [p, p + len) and [q, q + qlen) share an element
    static bool overlap(const T *p, size_t len, const T *q, size_t qlen) {
        const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
        return p && q && a < b + qlen * sizeof(T) && b < a + len * sizeof(T);
    }

    int check_dev(const T *d_in_re, const T *d_in_im, size_t num, size_t in_dist, const T *d_out_re, const T *d_out_im,
                  size_t num_bins, size_t out_dist, size_t batch, const T *d_work, size_t work_len) const {
        if (!d_in_re || !d_out_re || !d_out_im) return PHAST_ERR_INVALID_ARG;  // d_in_im may be null: a real signal
        if (num != n || num_bins != bins) return PHAST_ERR_PLANNER_SIZE;
        if (batch > 1 && (in_dist < n || out_dist < bins)) return PHAST_ERR_INVALID_ARG;
        if (batch && (!d_work || work_len < 2 * m)) return PHAST_ERR_INVALID_ARG;
        if (batch) {  // the output is written while later chunks still read the input and the workspace
            const size_t in_span = (batch - 1) * (batch > 1 ? in_dist : 0) + n, out_span = (batch - 1) * (batch > 1 ? out_dist : 0) + bins;
            for (const T *o : {d_out_re, d_out_im})
                if (overlap(o, out_span, d_in_re, in_span) || overlap(o, out_span, d_in_im, in_span) ||
                    overlap(o, out_span, d_work, work_len))
                    return PHAST_ERR_INVALID_ARG;
            if (overlap(d_out_re, out_span, d_out_im, out_span)) return PHAST_ERR_INVALID_ARG;
        }
        return PHAST_OK;
    }

    // device pointers, asynchronous on `s`
    int czt_dev(const T *d_in_re, const T *d_in_im, size_t num, size_t in_dist, T *d_out_re, T *d_out_im, size_t num_bins,
                size_t out_dist, size_t batch, T *d_work, size_t work_len, hipStream_t s) const {
        int rc = check_dev(d_in_re, d_in_im, num, in_dist, d_out_re, d_out_im, num_bins, out_dist, batch, d_work, work_len);
        if (rc || batch == 0) return rc;
        if (batch == 1) {
            in_dist = n;
            out_dist = bins;
        }
        const Planner<T> *pl = engine(s);
        PHAST_ON_DEVICE(device);
        typename Planner<T>::Lease L;
        rc = pl->lease(L, s);
        return rc ? rc : run(pl, L, d_in_re, d_in_im, in_dist, d_out_re, d_out_im, out_dist, batch, d_work, work_len);
    }

    // host slices: staged through the staging buffer of a workspace checked out of the inner planner's pool (x planes, X
    // planes, then the convolution workspace), on that workspace's own stream; blocking.  in_im may be null: a real signal
    int czt_host(const T *in_re, const T *in_im, size_t num, T *out_re, T *out_im, size_t num_bins) const {
        if (!in_re || !out_re || !out_im) return PHAST_ERR_INVALID_ARG;
        if (num != n || num_bins != bins) return PHAST_ERR_PLANNER_SIZE;
        const Planner<T> *pl = inner->route_small(1);
        PHAST_ON_DEVICE(device);
        typename Planner<T>::Lease L;
        int rc = pl->check_out(L, nullptr, 1);
        if (rc) return rc;
        const size_t x_len = (n + 1) & ~(size_t)1, o_len = (bins + 1) & ~(size_t)1;  // the workspace stays 16-byte aligned
        void *stage = nullptr;
        rc = pl->stage(L, (2 * x_len + 2 * o_len + 2 * m) * sizeof(T), &stage);
        if (rc) return rc;
        T *d_re = reinterpret_cast<T *>(stage), *d_im = d_re + x_len, *d_or = d_im + x_len, *d_oi = d_or + o_len, *d_w = d_oi + o_len;
        PHAST_HIP(hipMemcpyAsync(d_re, in_re, n * sizeof(T), hipMemcpyHostToDevice, L.stream));
        if (in_im) PHAST_HIP(hipMemcpyAsync(d_im, in_im, n * sizeof(T), hipMemcpyHostToDevice, L.stream));
        rc = run(pl, L, d_re, in_im ? d_im : nullptr, n, d_or, d_oi, bins, 1, d_w, 2 * m);
        if (rc) return rc;
        PHAST_HIP(hipMemcpyAsync(out_re, d_or, bins * sizeof(T), hipMemcpyDeviceToHost, L.stream));
        PHAST_HIP(hipMemcpyAsync(out_im, d_oi, bins * sizeof(T), hipMemcpyDeviceToHost, L.stream));
        PHAST_HIP(hipStreamSynchronize(L.stream));
        return PHAST_OK;
    }

    // measurement hook: average milliseconds of the five stages (pre, forward engine, spectrum, inverse engine, post) over
    // `reps` calls of one chunk (work_len / 2L >= batch) at distances N and M; blocks
    int time_stages(const T *d_in_re, const T *d_in_im, T *d_out_re, T *d_out_im, size_t batch, T *d_work, size_t work_len,
                    int reps, float *ms, hipStream_t s) const {
        if (!ms || reps < 1 || batch == 0) return PHAST_ERR_INVALID_ARG;
        int rc = check_dev(d_in_re, d_in_im, n, n, d_out_re, d_out_im, bins, bins, batch, d_work, work_len);
        if (rc) return rc;
        if (work_len < 2 * m * batch) return PHAST_ERR_INVALID_ARG;
        const Planner<T> *pl = engine(s);
        PHAST_ON_DEVICE(device);
        return time_stages_of(pl, reps, ms, s, [&](const auto &L, hipEvent_t *ev) {
            return run(pl, L, d_in_re, d_in_im, n, d_out_re, d_out_im, bins, batch, d_work, work_len, ev);
        });
    }
};

template <typename P> static int czt_planner_new(size_t n, size_t m, double step, double start, P **out) {
    if (!out) return PHAST_ERR_INVALID_ARG;
    *out = nullptr;
    if (czt_bad_args(n, m, step, start)) return PHAST_ERR_INVALID_ARG;  // before the device is touched
    auto *p = new (std::nothrow) P();
    if (!p) return PHAST_ERR_ALLOC;
    int rc = p->init(n, m, step, start);
    if (rc) {
        delete p;
        return rc;
    }
    *out = p;
    return PHAST_OK;
}

}  // namespace phast
