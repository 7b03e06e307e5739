// planner_any.hpp -- AnyPlanner<T>: complex transforms of any length N (Bluestein, any_len.hpp) on the power-of-two engine.
// Immutable after init: the inner Planner<T>(M) and the device table Bh = FFT_M(b) / M.  What a call mutates is the caller's
// workspace (_dev calls) or a workspace of the inner planner's pool (its staging buffer: host-slice calls), so graph capture
// and concurrent streams and threads need nothing beyond what the engine already does.  The convolution core (convolve),
// the chunk loop (for_each_chunk) and the table build live in ConvCore<T>, in terms of (m, log_m, d_bh): with the stage timer
// (time_stages_of) they serve the real planner too (planner_any_real.hpp), which runs its own pad and post sweeps around the
// core, and the chirp-Z planner (planner_czt.hpp), which derives from ConvCore with a table and sweeps of its own.
#pragma once

#include "any_len.hpp"
#include "entry.hpp"
#include "host_api.hpp"

namespace phast {

// measurement hook of the any-length planners: average milliseconds of the five stages (pad, forward engine, spectrum, inverse
// engine, post) over `reps` calls of run(lease, ev) on a lease of pl on `s`, which record the six events ev[0..5]; blocks
template <typename T, typename F> static int time_stages_of(const Planner<T> *pl, int reps, float *ms, hipStream_t s, F &&run) {
    struct Events {
        hipEvent_t e[6] = {};
        ~Events() {
            for (hipEvent_t x : e)
                if (x) hipEventDestroy(x);
        }
    } ev;
    for (hipEvent_t &x : ev.e) PHAST_HIP(hipEventCreate(&x));
    double acc[5] = {0, 0, 0, 0, 0};
    for (int r = 0; r < reps; ++r) {
        {
            typename Planner<T>::Lease L;  // checked in before the wait
            int rc = pl->lease(L, s);
            if (!rc) rc = run(L, ev.e);
            if (rc) return rc;
        }
        PHAST_HIP(hipStreamSynchronize(s));
        for (int i = 0; i < 5; ++i) {
            float t = 0;
            PHAST_HIP(hipEventElapsedTime(&t, ev.e[i], ev.e[i + 1]));
            acc[i] += t;
        }
    }
    for (int i = 0; i < 5; ++i) ms[i] = (float)(acc[i] / reps);
    return PHAST_OK;
}

// What every convolution on the engine shares (AnyPlanner below, CztPlanner in planner_czt.hpp): the inner Planner<T>(M), the
// device table Bh = FFT_M(b) / M, the engine plan, the convolution core and the chunk loop, all in terms of (m, log_m, d_bh)
template <typename T> struct ConvCore {
    size_t m = 0;  // the convolution length, a power of two
    unsigned log_m = 0;
    int device = -1;
    std::unique_ptr<Planner<T>> inner;  // Planner<T>(M)
    T *d_bh = nullptr;                  // [2][M]: Bh re plane, im plane (1/M folded in)

    ~ConvCore() {
        DeviceGuard on(device);
        if (d_bh) hipFree(d_bh);
    }

    // the device and the inner planner of `conv_len` points
    int init_core(size_t conv_len) {
        m = conv_len;
        log_m = ilog2(m);
        int rc = ensure_device(&device);
        if (rc) return rc;
        inner.reset(new (std::nothrow) Planner<T>());
        if (!inner) return PHAST_ERR_ALLOC;
        return inner->init(m);
    }

    // fill(re, im, stream) writes b as f64 planes [M] on the device; FFT_M in an f64 engine with 1/M on its last store (an exact
    // power of two); the f32 planner rounds the result, so its table carries no f32 transform error.  Synchronised on a stream
    // of its own before it returns.
    template <typename F> int make_table(F &&fill) {
        PHAST_ON_DEVICE(device);
        hipStream_t s = nullptr;
        PHAST_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        struct StreamGone {
            hipStream_t s;
            ~StreamGone() { hipStreamDestroy(s); }
        } gone{s};
        PHAST_HIP(hipMalloc((void **)&d_bh, 2 * m * sizeof(T)));
        // a planner of its own, not the inner one: nothing of the build stays in the inner planner's workspace pool
        std::unique_ptr<Planner<double>> eng(new (std::nothrow) Planner<double>());
        if (!eng) return PHAST_ERR_ALLOC;
        int rc = eng->init(m);
        if (rc) return rc;
        DevBuf b64;
        double *br = reinterpret_cast<double *>(d_bh);
        if constexpr (sizeof(T) == 4) {
            rc = b64.alloc(2 * m * sizeof(double));
            if (rc) return rc;
            br = reinterpret_cast<double *>(b64.p);
        }
        double *bi = br + m;
        PHAST_HIP(fill(br, bi, s));
        rc = eng->exec(br, bi, m, 0, br, bi, m, 0, 1, 1.0 / (double)m, s);
        if (rc) return rc;
        if constexpr (sizeof(T) == 4) PHAST_HIP(launch_any_round(br, reinterpret_cast<float *>(d_bh), 2 * m, s));
        PHAST_HIP(hipStreamSynchronize(s));
        return PHAST_OK;
    }

    // The engine runs ONE plan for every batch and chunk size -- the one of a single transform -- so the bits of a
    // transform do not depend on what it is batched with (a batch plan would round differently).
    const Planner<T> *engine(hipStream_t s) const {
        const Planner<T> *pl = inner->route_small(1);
        if (pl != inner.get() && Planner<T>::capturing(s) && !pl->capture_ready(s)) pl = inner.get();  // as Planner::exec
        return pl;
    }

    // The convolution core of `c` transforms on the chirp-padded workspace w (2 c M elements: c re planes, then c im planes),
    // in place: forward engine, spectrum sweep, inverse engine.  ev: the events ev[1..4] around the three steps (time_stages)
    int convolve(const Planner<T> *pl, const typename Planner<T>::Lease &L, const typename Planner<T>::Choice &ch, T *w,
                 size_t c, hipEvent_t *ev) const {
        hipStream_t s = L.stream;
        T *w_re = w, *w_im = w + c * m;
        if (ev) PHAST_HIP(hipEventRecord(ev[1], s));
        int rc = pl->exec_in(L, w_re, w_im, m, 0, w_re, w_im, m, 0, c, 1.0, nullptr, nullptr, nullptr, nullptr, &ch);
        if (rc) return rc;
        if (ev) PHAST_HIP(hipEventRecord(ev[2], s));
        AnySweepArgs a{};
        a.out_re = w_re;
        a.out_im = w_im;
        a.bh_re = d_bh;
        a.bh_im = d_bh + m;
        a.log_m = log_m;
        a.groups = c * (m / (16 / sizeof(T)));
        PHAST_HIP(launch_any_sweep<T>(1, true, a, s));
        if (ev) PHAST_HIP(hipEventRecord(ev[3], s));
        // the inverse by the swap trick: FFT of (im, re) = (im, re) of M IFFT -- its 1/M is in Bh
        rc = pl->exec_in(L, w_im, w_re, m, 0, w_im, w_re, m, 0, c, 1.0, nullptr, nullptr, nullptr, nullptr, &ch);
        if (rc) return rc;
        if (ev) PHAST_HIP(hipEventRecord(ev[4], s));
        return PHAST_OK;
    }

    // f(b0, c) for the batch in chunks of c <= floor(work_len / 2M) transforms from transform b0 on
    template <typename F> int for_each_chunk(size_t batch, size_t work_len, F &&f) const {
        size_t chunk = work_len / (2 * m);
        const size_t cap = ((size_t)1 << 39) / m;  // a launch's groups stay below 2^38
        if (chunk > cap) chunk = cap;
        for (size_t b0 = 0; b0 < batch; b0 += chunk) {
            int rc = f(b0, batch - b0 < chunk ? batch - b0 : chunk);
            if (rc) return rc;
        }
        return PHAST_OK;
    }
};

template <typename T> struct AnyPlanner : ConvCore<T> {
    using ConvCore<T>::m;
    using ConvCore<T>::log_m;
    using ConvCore<T>::device;
    using ConvCore<T>::inner;
    using ConvCore<T>::d_bh;
    using ConvCore<T>::engine;
    using ConvCore<T>::convolve;
    using ConvCore<T>::for_each_chunk;
    size_t n = 0;  // N; m == n: a power of two, the pow2 path (inner is Planner<T>(N), d_bh null)

    bool pow2() const { return d_bh == nullptr; }

    int init(size_t num_points) {
        if (num_points == 0 || num_points > kAnyMaxN) return PHAST_ERR_INVALID_ARG;
        n = num_points;
        int rc = this->init_core((size_t)any_conv_len(n));
        if (rc || is_pow2(n)) return rc;
        return this->make_table([&](double *br, double *bi, hipStream_t s) { return launch_any_chirp_b(br, bi, n, log_m, s); });
    }

    size_t workspace_len(size_t batch) const { return pow2() ? 0 : 2 * m * batch; }
    size_t device_bytes() const { return (pow2() ? 0 : 2 * m * sizeof(T)) + (inner ? inner->device_bytes() : 0); }
    std::string describe() const {
        if (pow2()) return "any N=" + std::to_string(n) + " (power of two): " + inner->describe();
        return "any N=" + std::to_string(n) + " M=" + std::to_string(m) + " (Bluestein): " + inner->describe();
    }

    // `c` transforms: x planes (re, im) at b * dist -> X planes at b * dist, through the workspace w (2 c M elements).
    // ev: optional 6 events recorded around the five stages (time_stages)
    int run_chunk(const Planner<T> *pl, const typename Planner<T>::Lease &L, const typename Planner<T>::Choice &ch,
                  const T *x_re, const T *x_im, T *o_re, T *o_im, size_t c, size_t dist, T *w, double scale,
                  hipEvent_t *ev = nullptr) const {
        hipStream_t s = L.stream;
        constexpr unsigned V = 16 / sizeof(T);
        T *w_re = w, *w_im = w + c * m;
        auto al = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; };
        AnySweepArgs a{};
        a.n = n;
        a.log_m = log_m;
        a.in_dist = a.out_dist = dist;
        if (ev) PHAST_HIP(hipEventRecord(ev[0], s));
        a.in_re = x_re;
        a.in_im = x_im;
        a.out_re = w_re;
        a.out_im = w_im;
        a.groups = c * (m / V);
        PHAST_HIP(launch_any_sweep<T>(0, al(x_re) && al(x_im) && dist % V == 0, a, s));
        int rc = convolve(pl, L, ch, w, c, ev);
        if (rc) return rc;
        a.in_re = w_re;
        a.in_im = w_im;
        a.out_re = o_re;
        a.out_im = o_im;
        a.gpt = (unsigned)((n + V - 1) / V);
        a.groups = c * a.gpt;
        a.scale = scale;
        PHAST_HIP(launch_any_sweep<T>(2, al(o_re) && al(o_im) && dist % V == 0, a, s));
        if (ev) PHAST_HIP(hipEventRecord(ev[5], s));
        return PHAST_OK;
    }

    // the batch in chunks, in place in (re, im); the inverse: the forward of (im, re) * 1/N
    int run(const Planner<T> *pl, const typename Planner<T>::Lease &L, T *re, T *im, size_t batch, size_t dist, int direction,
            T *work, size_t work_len, hipEvent_t *ev = nullptr) const {
        const typename Planner<T>::Choice ch = pl->choose(kC2C, 1, 1);
        const double scale = direction == PHAST_REVERSE ? 1.0 / (double)n : 1.0;
        if (direction == PHAST_REVERSE) std::swap(re, im);
        return for_each_chunk(batch, work_len, [&](size_t b0, size_t c) {
            T *r = re + b0 * dist, *i = im + b0 * dist;
            return run_chunk(pl, L, ch, r, i, r, i, c, dist, work, scale, ev);
        });
    }

    int check_dev(const T *d_re, const T *d_im, size_t num, size_t batch, size_t dist, int direction, const T *d_work,
                  size_t work_len) const {
        if (!d_re || !d_im) return PHAST_ERR_INVALID_ARG;
        if (direction != PHAST_FORWARD && direction != PHAST_REVERSE) return PHAST_ERR_INVALID_ARG;
        if (num != n) return PHAST_ERR_PLANNER_SIZE;
        if (batch > 1 && dist < n) return PHAST_ERR_INVALID_ARG;
        if (!pow2() && batch && (!d_work || work_len < 2 * m)) return PHAST_ERR_INVALID_ARG;
        return PHAST_OK;
    }

    // device pointers, asynchronous on `s`
    int fft_dev_any(T *d_re, T *d_im, size_t num, size_t batch, size_t dist, int direction, T *d_work, size_t work_len,
                    hipStream_t s) const {
        int rc = check_dev(d_re, d_im, num, batch, dist, direction, d_work, work_len);
        if (rc) return rc;
        if (pow2()) return fft_dev<T>(d_re, d_im, n, batch, dist, direction, inner.get(), s);
        if (batch == 0) return PHAST_OK;
        if (batch == 1) dist = n;
        const Planner<T> *pl = engine(s);
        PHAST_ON_DEVICE(device);
        typename Planner<T>::Lease L;
        rc = pl->lease(L, s);
        return rc ? rc : run(pl, L, d_re, d_im, batch, dist, direction, d_work, work_len);
    }

    // host slices: staged through the staging buffer of a workspace checked out of the inner planner's pool (x planes, then
    // the convolution workspace), on that workspace's own stream; blocking
    int fft_host_any(T *re, size_t re_len, T *im, size_t im_len, int direction) const {
        if ((!re && re_len) || (!im && im_len)) return PHAST_ERR_INVALID_ARG;
        if (direction != PHAST_FORWARD && direction != PHAST_REVERSE) return PHAST_ERR_INVALID_ARG;
        if (re_len != im_len) return PHAST_ERR_LEN_MISMATCH;
        if (re_len != n) return PHAST_ERR_PLANNER_SIZE;
        if (pow2()) return fft_host<T>(re, re_len, im, im_len, direction, inner.get());
        const Planner<T> *pl = inner->route_small(1);
        PHAST_ON_DEVICE(device);
        typename Planner<T>::Lease L;
        int rc = pl->check_out(L, nullptr, 1);
        if (rc) return rc;
        const size_t bytes = n * sizeof(T);
        const size_t x_len = (n + 1) & ~(size_t)1;  // the workspace behind the planes stays 16-byte aligned
        void *stage = nullptr;
        rc = pl->stage(L, (2 * x_len + 2 * m) * sizeof(T), &stage);
        if (rc) return rc;
        T *d_re = reinterpret_cast<T *>(stage), *d_im = d_re + x_len, *d_w = d_im + x_len;
        PHAST_HIP(hipMemcpyAsync(d_re, re, bytes, hipMemcpyHostToDevice, L.stream));
        PHAST_HIP(hipMemcpyAsync(d_im, im, bytes, hipMemcpyHostToDevice, L.stream));
        rc = run(pl, L, d_re, d_im, 1, n, direction, d_w, 2 * m);
        if (rc) return rc;
        PHAST_HIP(hipMemcpyAsync(re, d_re, bytes, hipMemcpyDeviceToHost, L.stream));
        PHAST_HIP(hipMemcpyAsync(im, d_im, bytes, hipMemcpyDeviceToHost, L.stream));
        PHAST_HIP(hipStreamSynchronize(L.stream));
        return PHAST_OK;
    }

    // measurement hook: average milliseconds of the five stages (pre, forward engine, spectrum, inverse engine, post) over
    // `reps` forward calls of one chunk (work_len / 2M >= batch); blocks
    int time_stages(T *d_re, T *d_im, size_t batch, size_t dist, T *d_work, size_t work_len, int reps, float *ms,
                    hipStream_t s) const {
        if (!ms || reps < 1 || batch == 0) return PHAST_ERR_INVALID_ARG;
        int rc = check_dev(d_re, d_im, n, batch, dist, PHAST_FORWARD, d_work, work_len);
        if (rc) return rc;
        if (pow2() || work_len < 2 * m * batch) return PHAST_ERR_INVALID_ARG;
        if (batch == 1) dist = n;
        const Planner<T> *pl = engine(s);
        PHAST_ON_DEVICE(device);
        return time_stages_of(pl, reps, ms, s, [&](const auto &L, hipEvent_t *ev) {
            return run(pl, L, d_re, d_im, batch, dist, PHAST_FORWARD, d_work, work_len, ev);
        });
    }
};

template <typename P> static int any_planner_new(size_t n, P **out) {
    if (!out) return PHAST_ERR_INVALID_ARG;
    *out = nullptr;
    if (n == 0 || n > kAnyMaxN) return PHAST_ERR_INVALID_ARG;  // before the device is touched
    auto *p = new (std::nothrow) P();
    if (!p) return PHAST_ERR_ALLOC;
    int rc = p->init(n);
    if (rc) {
        delete p;
        return rc;
    }
    *out = p;
    return PHAST_OK;
}

}  // namespace phast
