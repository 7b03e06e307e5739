// planner_nufft.hpp -- NufftPlanner<T>: non-uniform FFTs of types 1 and 2 (nufft.hpp) of M points and N modes on an inner
// Planner<T>(n_g).  Immutable after init but for set_points_dev: the inner planner, the point set sorted by grid cell (positions,
// permutation, cell starts) and the N reciprocals 1 / phi^(k) on the device.  The points come from host memory (init: sorted on
// the host) or from device memory (init_dev, set_points_dev: sorted on the device, nufft_sort.hpp, to the same bits).  What a
// transform mutates is the caller's workspace (_dev calls) or a
// workspace of the inner planner's pool (host-slice calls), so graph capture and concurrent streams and threads need nothing
// beyond what the engine already does.  Of ConvCore (planner_any.hpp) it uses the inner planner, the single-transform
// engine plan and the chunk loop; it has no convolution table.
#pragma once

#include "planner_any.hpp"
#include "planner_nufft_common.hpp"

namespace phast {

template <typename T> struct NufftPlanner : ConvCore<T> {
    using ConvCore<T>::m;  // the fine grid n_g
    using ConvCore<T>::log_m;
    using ConvCore<T>::device;
    using ConvCore<T>::inner;
    using ConvCore<T>::engine;
    using ConvCore<T>::for_each_chunk;
    size_t modes = 0, points = 0;  // N, M
    int w = 0;
    double eps = 0;
    double *d_xs = nullptr;
    uint32_t *d_perm = nullptr, *d_cell = nullptr;
    T *d_inv = nullptr;

    ~NufftPlanner() {
        DeviceGuard on(device);
        for (void *p : {(void *)d_xs, (void *)d_perm, (void *)d_cell, (void *)d_inv})
            if (p) hipFree(p);
    }

    // what does not depend on the points: the sizes, the inner planner, 1 / phi^ on the device, and room for the point tables
    int init_grid(size_t n_modes, size_t m_points, double eps_) {
        modes = n_modes;
        points = m_points;
        eps = eps_;
        w = nufft_width(eps);
        int rc = this->init_core((size_t)nufft_grid(modes, w));
        if (rc) return rc;
        const std::vector<T> inv = nufft_inv_table<T>(w, modes, m);
        PHAST_ON_DEVICE(device);
        PHAST_HIP(hipMalloc(reinterpret_cast<void **>(&d_xs), points * sizeof(double)));
        PHAST_HIP(hipMalloc(reinterpret_cast<void **>(&d_perm), points * sizeof(uint32_t)));
        PHAST_HIP(hipMalloc(reinterpret_cast<void **>(&d_cell), (m + 1) * sizeof(uint32_t)));
        PHAST_HIP(hipMalloc(reinterpret_cast<void **>(&d_inv), modes * sizeof(T)));
        PHAST_HIP(hipMemcpy(d_inv, inv.data(), modes * sizeof(T), hipMemcpyHostToDevice));
        return PHAST_OK;
    }

    // `x`: M host doubles in turns; the arguments were checked by nufft_bad_args
    int init(size_t n_modes, const double *x, size_t m_points, double eps_) {
        int rc = init_grid(n_modes, m_points, eps_);
        if (rc) return rc;
        std::vector<double> xs(points);
        std::vector<uint32_t> perm(points), cell(m + 1);
        nufft_bin(x, points, log_m, xs.data(), perm.data(), cell.data());
        PHAST_ON_DEVICE(device);
        PHAST_HIP(hipMemcpy(d_xs, xs.data(), points * sizeof(double), hipMemcpyHostToDevice));
        PHAST_HIP(hipMemcpy(d_perm, perm.data(), points * sizeof(uint32_t), hipMemcpyHostToDevice));
        PHAST_HIP(hipMemcpy(d_cell, cell.data(), (m + 1) * sizeof(uint32_t), hipMemcpyHostToDevice));
        return PHAST_OK;
    }

    // as init, with `d_x`: M doubles in device memory (nufft_sort.hpp), ordered after the earlier work of `s`; blocks.  The
    // arguments but the points' values were checked by nufft_bad_sizes; PHAST_ERR_INVALID_ARG for a point that is not finite
    int init_dev(size_t n_modes, const double *d_x, size_t m_points, double eps_, hipStream_t s) {
        int rc = init_grid(n_modes, m_points, eps_);
        if (rc) return rc;
        PHAST_ON_DEVICE(device);
        return nufft_sort_build(d_x, nullptr, nullptr, points, log_m, 0, 0, d_perm, d_cell, d_xs, nullptr, nullptr, s);
    }

    // New points for this planner, the same M of them (PHAST_ERR_PLANNER_SIZE otherwise), from device memory: the point tables
    // are rewritten IN PLACE, at the same addresses, so a HIP graph captured through the planner stays valid and, replayed,
    // transforms at the new points.  The grid, the width, 1 / phi^, the inner planner and the workspace length do not depend on
    // the points and are untouched.  The keys, the finiteness check and the sort run into temporaries first: a rejected point set
    // (PHAST_ERR_INVALID_ARG: a point that is not finite, a null pointer, a stream that is capturing) leaves the planner as it
    // was.  Blocks until done.  The call orders itself after the earlier work of `s` ONLY: as with free, the caller must have
    // finished the work on other streams that uses the planner.  ms: nufft_sort_build's
    int set_points_dev(const double *d_x, size_t m_points, hipStream_t s, float *ms = nullptr) {
        if (!d_x) return PHAST_ERR_INVALID_ARG;
        if (m_points != points) return PHAST_ERR_PLANNER_SIZE;
        PHAST_ON_DEVICE(device);
        if (nufft_sort_stream_busy(s)) return PHAST_ERR_INVALID_ARG;
        return nufft_sort_build(d_x, nullptr, nullptr, points, log_m, 0, 0, d_perm, d_cell, d_xs, nullptr, nullptr, s, ms);
    }

    size_t workspace_len(size_t batch) const { return 2 * m * batch; }
    size_t grid_len() const { return m; }
    size_t table_bytes() const { return points * (sizeof(double) + sizeof(uint32_t)) + (m + 1) * sizeof(uint32_t) + modes * sizeof(T); }
    size_t device_bytes() const { return table_bytes() + (inner ? inner->device_bytes() : 0); }
    std::string describe() const {
        char f[48];
        std::snprintf(f, sizeof f, " eps=%.3g w=%d", eps, w);
        return "nufft N=" + std::to_string(modes) + " M=" + std::to_string(points) + f + " n_g=" + std::to_string(m) + ": " +
               inner->describe();
    }
    size_t in_len(int type) const { return type == 1 ? points : modes; }
    size_t out_len(int type) const { return type == 1 ? modes : points; }

    // the arguments every launch of a chunk shares: the tables, the sizes and the caller's distances
    NufftArgs chunk_args(size_t in_dist, size_t out_dist) const {
        NufftArgs a{};
        a.xs = d_xs;
        a.perm = d_perm;
        a.cell_start = d_cell;
        a.inv_hat = d_inv;
        a.in_dist = in_dist;
        a.out_dist = out_dist;
        a.n = modes;
        a.m = points;
        a.log_g = log_m;
        a.w = w;
        return a;
    }
    static bool aligned(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

    // The three stages of a chunk of `c` transforms on the workspace wk (2 c n_g elements: c re planes, then c im planes), each
    // callable on its own: the type-3 planner (planner_nufft_t3.hpp) puts a stage of its own in front of `transform` and runs
    // `interpolate` as it stands.
    // stage a of type 2: the caller's modes (re, im or null) at b * a.in_dist over phi^ into the slots of the grid
    int pre(NufftArgs a, const T *x_re, const T *x_im, size_t c, T *wk, hipStream_t s) const {
        constexpr unsigned V = 16 / sizeof(T);
        a.in_re = x_re;
        a.in_im = x_im;
        a.out_re = wk;
        a.out_im = wk + c * m;
        a.groups = c * (m / V);
        PHAST_HIP(launch_nufft<T>(2, aligned(x_re) && aligned(x_im) && aligned(wk) && a.in_dist % V == 0, a, s));
        return PHAST_OK;
    }
    // stage b: the n_g-point transform of the c grids, in place.  Reverse by the swap trick: FFT of (im, re) = (im, re) of the
    // transform with the + sign
    int transform(const Planner<T> *pl, const typename Planner<T>::Lease &L, const typename Planner<T>::Choice &ch, int direction,
                  size_t c, T *wk) const {
        T *w_re = wk, *w_im = wk + c * m;
        T *e_re = direction == PHAST_REVERSE ? w_im : w_re, *e_im = direction == PHAST_REVERSE ? w_re : w_im;
        return pl->exec_in(L, e_re, e_im, m, 0, e_re, e_im, m, 0, c, 1.0, nullptr, nullptr, nullptr, nullptr, &ch);
    }
    // stage c of type 2: the grids at the sorted points, onto the caller's planes at b * a.out_dist
    int interpolate(NufftArgs a, size_t c, const T *wk, T *o_re, T *o_im, hipStream_t s) const {
        a.in_re = wk;
        a.in_im = wk + c * m;
        a.out_re = o_re;
        a.out_im = o_im;
        a.groups = c * points;
        PHAST_HIP(launch_nufft<T>(1, false, a, s));
        return PHAST_OK;
    }

    // `c` transforms of type 1 or 2: input planes (re, im or null) at b * in_dist -> output planes at b * out_dist, through
    // the workspace wk (2 c n_g elements: c re planes, then c im planes).  ev: optional 6 events; ev[0..3] bound the three stages
    int run_chunk(const Planner<T> *pl, const typename Planner<T>::Lease &L, const typename Planner<T>::Choice &ch, int type,
                  int direction, const T *x_re, const T *x_im, size_t in_dist, T *o_re, T *o_im, size_t out_dist, size_t c,
                  T *wk, hipEvent_t *ev = nullptr) const {
        hipStream_t s = L.stream;
        constexpr unsigned V = 16 / sizeof(T);
        T *w_re = wk, *w_im = wk + c * m;
        NufftArgs a = chunk_args(in_dist, out_dist);
        int rc;
        if (ev) PHAST_HIP(hipEventRecord(ev[0], s));
        if (type == 1) {
            a.in_re = x_re;
            a.in_im = x_im;
            a.out_re = w_re;
            a.out_im = w_im;
            a.groups = c * m;
            PHAST_HIP(launch_nufft<T>(0, false, a, s));
        } else if ((rc = pre(a, x_re, x_im, c, wk, s))) {
            return rc;
        }
        if (ev) PHAST_HIP(hipEventRecord(ev[1], s));
        if ((rc = transform(pl, L, ch, direction, c, wk))) return rc;
        if (ev) PHAST_HIP(hipEventRecord(ev[2], s));
        if (type == 1) {
            a.in_re = w_re;
            a.in_im = w_im;
            a.out_re = o_re;
            a.out_im = o_im;
            a.gpt = (unsigned)((modes + V - 1) / V);
            a.groups = c * a.gpt;
            PHAST_HIP(launch_nufft<T>(3, aligned(o_re) && aligned(o_im) && aligned(wk) && out_dist % V == 0, a, s));
        } else if ((rc = interpolate(a, c, wk, o_re, o_im, s))) {
            return rc;
        }
        if (ev)
            for (int i = 3; i < 6; ++i) PHAST_HIP(hipEventRecord(ev[i], s));
        return PHAST_OK;
    }

    // the batch in chunks
    int run(const Planner<T> *pl, const typename Planner<T>::Lease &L, int type, int direction, const T *x_re, const T *x_im,
            size_t in_dist, T *o_re, T *o_im, size_t out_dist, size_t batch, T *work, size_t work_len,
            hipEvent_t *ev = nullptr) const {
        const typename Planner<T>::Choice ch = pl->choose(kC2C, 1, 1);
        return for_each_chunk(batch, work_len, [&](size_t b0, size_t c) {
            return run_chunk(pl, L, ch, type, direction, x_re + b0 * in_dist, x_im ? x_im + b0 * in_dist : nullptr, in_dist,
                             o_re + b0 * out_dist, o_im + b0 * out_dist, out_dist, c, work, ev);
        });
    }

    int check_dev(int type, int direction, const T *d_in_re, const T *d_in_im, size_t in_dist, const T *d_out_re,
                  const T *d_out_im, size_t out_dist, size_t batch, const T *d_work, size_t work_len) const {
        return nufft_check_dev(direction, d_in_re, d_in_im, in_dist, in_len(type), d_out_re, d_out_im, out_dist, out_len(type), batch,
                               d_work, work_len, 2 * m);
    }

    // device pointers, asynchronous on `s`
    int nufft_dev(int type, int direction, const T *d_in_re, const T *d_in_im, size_t in_dist, T *d_out_re, T *d_out_im,
                  size_t out_dist, size_t batch, T *d_work, size_t work_len, hipStream_t s) const {
        int rc = check_dev(type, direction, d_in_re, d_in_im, in_dist, d_out_re, d_out_im, out_dist, batch, d_work, work_len);
        if (rc || batch == 0) return rc;
        if (batch == 1) {
            in_dist = in_len(type);
            out_dist = out_len(type);
        }
        const Planner<T> *pl = engine(s);
        PHAST_ON_DEVICE(device);
        typename Planner<T>::Lease L;
        rc = pl->lease(L, s);
        return rc ? rc : run(pl, L, type, direction, d_in_re, d_in_im, in_dist, d_out_re, d_out_im, out_dist, batch, d_work, work_len);
    }

    // host slices: staged through the staging buffer of a workspace checked out of the inner planner's pool (input planes,
    // output planes, then the grid), on that workspace's own stream; blocking.  in_im may be null: real data
    int nufft_host(int type, int direction, const T *in_re, const T *in_im, size_t num_in, T *out_re, T *out_im,
                   size_t num_out) const {
        if (!in_re || !out_re || !out_im) return PHAST_ERR_INVALID_ARG;
        if (direction != PHAST_FORWARD && direction != PHAST_REVERSE) return PHAST_ERR_INVALID_ARG;
        const size_t ni = in_len(type), no = out_len(type);
        if (num_in != ni || num_out != no) return PHAST_ERR_PLANNER_SIZE;
        const Planner<T> *pl = inner->route_small(1);
        PHAST_ON_DEVICE(device);
        typename Planner<T>::Lease L;
        int rc = pl->check_out(L, nullptr, 1);
        if (rc) return rc;
        const size_t x_len = (ni + 3) & ~(size_t)3, o_len = (no + 3) & ~(size_t)3;  // the grid stays 16-byte aligned
        void *stage = nullptr;
        rc = pl->stage(L, (2 * x_len + 2 * o_len + 2 * m) * sizeof(T), &stage);
        if (rc) return rc;
        T *d_re = reinterpret_cast<T *>(stage), *d_im = d_re + x_len, *d_or = d_im + x_len, *d_oi = d_or + o_len, *d_w = d_oi + o_len;
        PHAST_HIP(hipMemcpyAsync(d_re, in_re, ni * sizeof(T), hipMemcpyHostToDevice, L.stream));
        if (in_im) PHAST_HIP(hipMemcpyAsync(d_im, in_im, ni * sizeof(T), hipMemcpyHostToDevice, L.stream));
        rc = run(pl, L, type, direction, d_re, in_im ? d_im : nullptr, ni, d_or, d_oi, no, 1, d_w, 2 * m);
        if (rc) return rc;
        PHAST_HIP(hipMemcpyAsync(out_re, d_or, no * sizeof(T), hipMemcpyDeviceToHost, L.stream));
        PHAST_HIP(hipMemcpyAsync(out_im, d_oi, no * sizeof(T), hipMemcpyDeviceToHost, L.stream));
        PHAST_HIP(hipStreamSynchronize(L.stream));
        return PHAST_OK;
    }

    // measurement hook: ms[0..2] = average milliseconds of the three stages (spread or pre, the n_g-point transform,
    // deconvolve or interpolate) over `reps` Forward calls of one chunk (work_len / 2 n_g >= batch) at the natural distances;
    // ms[3] and ms[4] are 0 (the timer of the any-length planners has five slots); blocks
    int time_stages(int type, const T *d_in_re, const T *d_in_im, T *d_out_re, T *d_out_im, size_t batch, T *d_work,
                    size_t work_len, int reps, float *ms, hipStream_t s) const {
        if (!ms || reps < 1 || batch == 0 || (type != 1 && type != 2)) return PHAST_ERR_INVALID_ARG;
        const size_t ni = in_len(type), no = out_len(type);
        int rc = check_dev(type, PHAST_FORWARD, d_in_re, d_in_im, ni, d_out_re, d_out_im, no, batch, d_work, work_len);
        if (rc) return rc;
        if (work_len < 2 * m * batch) return PHAST_ERR_INVALID_ARG;
        const Planner<T> *pl = engine(s);
        PHAST_ON_DEVICE(device);
        return time_stages_of(pl, reps, ms, s, [&](const auto &L, hipEvent_t *ev) {
            return run(pl, L, type, PHAST_FORWARD, d_in_re, d_in_im, ni, d_out_re, d_out_im, no, batch, d_work, work_len, ev);
        });
    }
};

template <typename P> static int nufft_planner_new(size_t n_modes, const double *x, size_t m_points, double eps, bool f32, P **out) {
    return nufft_planner_make(out, [&] { return nufft_bad_args(n_modes, m_points, x, eps, f32); }, n_modes, x, m_points, eps);
}

// the same from M doubles in device memory, ordered after the earlier work of `s`
template <typename P>
static int nufft_planner_new_dev(size_t n_modes, const double *d_x, size_t m_points, double eps, bool f32, hipStream_t s, P **out) {
    return nufft_planner_make_dev(out, [&] { return nufft_bad_sizes(n_modes, m_points, d_x, eps, f32); }, s, n_modes, d_x, m_points, eps);
}

}  // namespace phast
