// planner_nufft_nd.hpp -- NufftNdPlanner<T, D>: non-uniform FFTs of types 1 and 2 in D = 2 or 3 dimensions (nufft_nd.hpp) of
// M points and N1 x .. x ND modes on an owned NdPlanner<T> of dims (g1, .., gD).  Immutable after init but for set_points_dev: the Nd planner, the point set sorted by grid cell (positions, permutation, cell starts) and the N1 + .. + ND
// reciprocals 1 / phi^(k) on the device.  What a call mutates is the caller's workspace (_dev calls) or a device buffer of the
// call's own (host-slice calls), so graph capture and concurrent streams and threads need nothing beyond what the Nd planner
// already does.  The checks, the binning, the kernels' arguments and their launcher are generic in D too.
//
// Workspace (elements of T) of a chunk of c transforms: c re grids, c im grids, then what the Nd planner asks for c arrays of
// (g1, .., gD) (its transposed copies, 2 c G: every axis is a power of two, so there is no Bluestein part): per() = 4 G per
// transform, G = g1 .. gD, read from the Nd planner and not assumed.
#pragma once

#include "nufft_nd.hpp"
#include "planner_nd.hpp"
#include "planner_nufft_common.hpp"

namespace phast {

template <typename T, size_t D> struct NufftNdPlanner {
    static_assert(D == 2 || D == 3, "the kernels exist for two and three dimensions");
    size_t n[D] = {}, g[D] = {};  // the modes N_i and the fine grid g_i
    size_t cells = 0, points = 0;  // G = g1 .. gD, M
    unsigned log_g[D] = {};
    int w = 0, device = -1;
    double eps = 0;
    NdPlanner<T> nd;
    double *d_coord[D] = {};  // the sorted positions per axis
    uint32_t *d_perm = nullptr, *d_cell = nullptr;
    T *d_inv[D] = {};

    ~NufftNdPlanner() {
        DeviceGuard on(device);
        for (size_t i = 0; i < D; ++i) {
            if (d_coord[i]) hipFree(d_coord[i]);
            if (d_inv[i]) hipFree(d_inv[i]);
        }
        for (void *p : {(void *)d_perm, (void *)d_cell})
            if (p) hipFree(p);
    }

    template <typename E> int room(E **dst, size_t count) {
        PHAST_HIP(hipMalloc(reinterpret_cast<void **>(dst), count * sizeof(E)));
        return PHAST_OK;
    }

    // what does not depend on the points: the sizes, the Nd planner, 1 / phi^ on the device, and room for the point tables
    int init_grid(const size_t (&n_)[D], size_t m_points, double eps_) {
        points = m_points;
        eps = eps_;
        w = nufft_width(eps);
        cells = 1;
        for (size_t i = 0; i < D; ++i) {
            n[i] = n_[i];
            g[i] = (size_t)nufft_grid(n[i], w);
            log_g[i] = ilog2(g[i]);
            cells *= g[i];
        }
        int rc = nd.init(g, D);
        if (rc) return rc;
        device = nd.device;
        std::vector<T> inv[D];
        for (size_t i = 0; i < D; ++i) inv[i] = nufft_inv_table<T>(w, n[i], g[i]);
        PHAST_ON_DEVICE(device);
        for (size_t i = 0; i < D; ++i)
            if ((rc = room(&d_coord[i], points))) return rc;
        if ((rc = room(&d_perm, points)) || (rc = room(&d_cell, cells + 1))) return rc;
        for (size_t i = 0; i < D; ++i) {
            if ((rc = room(&d_inv[i], n[i]))) return rc;
            PHAST_HIP(hipMemcpy(d_inv[i], inv[i].data(), n[i] * sizeof(T), hipMemcpyHostToDevice));
        }
        return PHAST_OK;
    }

    // `x`: per axis M host doubles in turns; the arguments were checked by nufft_nd_bad_args
    int init(const size_t (&n_)[D], const double *const (&x)[D], size_t m_points, double eps_) {
        int rc = init_grid(n_, m_points, eps_);
        if (rc) return rc;
        std::vector<double> xs[D];
        double *xp[D];
        for (size_t i = 0; i < D; ++i) {
            xs[i].resize(points);
            xp[i] = xs[i].data();
        }
        std::vector<uint32_t> perm(points), cell(cells + 1);
        nufft_nd_bin<D>(x, points, log_g, xp, perm.data(), cell.data());
        PHAST_ON_DEVICE(device);
        for (size_t i = 0; i < D; ++i) PHAST_HIP(hipMemcpy(d_coord[i], xp[i], points * sizeof(double), hipMemcpyHostToDevice));
        PHAST_HIP(hipMemcpy(d_perm, perm.data(), points * sizeof(uint32_t), hipMemcpyHostToDevice));
        PHAST_HIP(hipMemcpy(d_cell, cell.data(), (cells + 1) * sizeof(uint32_t), hipMemcpyHostToDevice));
        return PHAST_OK;
    }

    // the point tables from `d_x`: per axis M doubles in device memory (nufft_sort.hpp; its third axis is absent in 2-D)
    int sort_points(const double *const (&d_x)[D], hipStream_t s, float *ms) {
        return nufft_sort_build(d_x[0], d_x[1], D > 2 ? d_x[D - 1] : nullptr, points, log_g[0], log_g[1], D > 2 ? log_g[D - 1] : 0,
                                d_perm, d_cell, d_coord[0], d_coord[1], D > 2 ? d_coord[D - 1] : nullptr, s, ms);
    }

    // as init, with the points in device memory, ordered after the earlier work of `s`; blocks.  The arguments but the points'
    // values were checked by nufft_nd_bad_sizes; PHAST_ERR_INVALID_ARG for a coordinate that is not finite
    int init_dev(const size_t (&n_)[D], const double *const (&d_x)[D], size_t m_points, double eps_, hipStream_t s) {
        int rc = init_grid(n_, m_points, eps_);
        if (rc) return rc;
        PHAST_ON_DEVICE(device);
        return sort_points(d_x, s, nullptr);
    }

    // new points, the same M of them, from device memory: the rules of NufftPlanner::set_points_dev (planner_nufft.hpp) -- the
    // tables are rewritten in place, a rejected point set leaves the planner as it was, the call blocks, and it orders itself
    // after the earlier work of `s` ONLY: the caller must have finished the work on other streams that uses the planner
    int set_points_dev(const double *const (&d_x)[D], size_t m_points, hipStream_t s, float *ms = nullptr) {
        for (const double *p : d_x)
            if (!p) return PHAST_ERR_INVALID_ARG;
        if (m_points != points) return PHAST_ERR_PLANNER_SIZE;
        PHAST_ON_DEVICE(device);
        if (nufft_sort_stream_busy(s)) return PHAST_ERR_INVALID_ARG;
        return sort_points(d_x, s, ms);
    }

    // elements of T per transform: the two grid planes and the Nd planner's own share (4 G)
    size_t per() const { return 2 * cells + nd.workspace_len(1); }
    size_t workspace_len(size_t batch) const { return per() * batch; }
    size_t grid_len() const { return cells; }
    size_t modes() const {
        size_t all = 1;
        for (size_t ni : n) all *= ni;
        return all;
    }
    size_t table_bytes() const {
        size_t inv = 0;
        for (size_t ni : n) inv += ni;
        return points * (D * sizeof(double) + sizeof(uint32_t)) + (cells + 1) * sizeof(uint32_t) + inv * sizeof(T);
    }
    size_t device_bytes() const { return table_bytes() + nd.device_bytes(); }
    std::string describe() const {
        char f[48];
        std::snprintf(f, sizeof f, " eps=%.3g w=%d", eps, w);
        auto by = [](const size_t (&v)[D]) {
            std::string s = std::to_string(v[0]);
            for (size_t i = 1; i < D; ++i) s += "x" + std::to_string(v[i]);
            return s;
        };
        return "nufft" + std::to_string(D) + "d N=" + by(n) + " M=" + std::to_string(points) + f + " grid=" + by(g) + ": " + nd.describe();
    }
    size_t in_len(int type) const { return type == 1 ? points : modes(); }
    size_t out_len(int type) const { return type == 1 ? modes() : points; }

    // `c` transforms of type 1 or 2: input planes (re, im or null) at b * in_dist -> output planes at b * out_dist, through
    // the workspace wk (c per() elements: c re grids, c im grids, the Nd planner's).  ev: optional 4 events around the three stages
    int run_chunk(int type, int direction, const T *x_re, const T *x_im, size_t in_dist, T *o_re, T *o_im, size_t out_dist,
                  size_t c, T *wk, hipStream_t s, hipEvent_t *ev = nullptr) const {
        constexpr unsigned V = 16 / sizeof(T);
        T *w_re = wk, *w_im = wk + c * cells, *w_nd = wk + 2 * c * cells;
        auto al = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; };
        // 16-byte accesses: aligned planes and workspace, and the transforms' planes a multiple of the group apart (one
        // transform has no distance to meet)
        auto vec = [&](const T *re, const T *im, size_t dist) { return al(re) && al(im) && al(wk) && (c == 1 || dist % V == 0); };
        NufftNdArgs<D> a{};
        for (size_t i = 0; i < D; ++i) {
            a.xs[i] = d_coord[i];
            a.inv[i] = d_inv[i];
            a.n[i] = n[i];
            a.log_g[i] = log_g[i];
        }
        a.perm = d_perm;
        a.cell_start = d_cell;
        a.in_dist = in_dist;
        a.out_dist = out_dist;
        a.m = points;
        a.w = w;
        if (ev) PHAST_HIP(hipEventRecord(ev[0], s));
        a.in_re = x_re;
        a.in_im = x_im;
        a.out_re = w_re;
        a.out_im = w_im;
        if (type == 1) {
            a.groups = c * cells;
            PHAST_HIP((launch_nufft_nd<T, D>(0, false, a, s)));
        } else {
            a.groups = c * (cells / V);
            PHAST_HIP((launch_nufft_nd<T, D>(2, vec(x_re, x_im, in_dist), a, s)));
        }
        if (ev) PHAST_HIP(hipEventRecord(ev[1], s));
        // always the Forward transform (Reverse of the Nd planner scales by 1 / G).  Reverse by the swap trick: the FFT of
        // (im, re) is (im, re) of the transform with the + sign
        T *e_re = direction == PHAST_REVERSE ? w_im : w_re, *e_im = direction == PHAST_REVERSE ? w_re : w_im;
        int rc = nd.fft_dev_nd(e_re, e_im, cells, c, cells, PHAST_FORWARD, w_nd, nd.workspace_len(c), s);
        if (rc) return rc;
        if (ev) PHAST_HIP(hipEventRecord(ev[2], s));
        a.in_re = w_re;
        a.in_im = w_im;
        a.out_re = o_re;
        a.out_im = o_im;
        if (type == 1) {
            a.gpt = (unsigned)(modes() / n[D - 1] * ((n[D - 1] + V - 1) / V));  // sweeps along the last axis
            a.groups = c * a.gpt;
            PHAST_HIP((launch_nufft_nd<T, D>(3, vec(o_re, o_im, out_dist), a, s)));
        } else {
            a.groups = c * points;
            PHAST_HIP((launch_nufft_nd<T, D>(1, false, a, s)));
        }
        if (ev) PHAST_HIP(hipEventRecord(ev[3], s));
        return PHAST_OK;
    }

    // the batch in chunks of floor(work_len / per()) transforms; the Nd planner's plans do not depend on the chunk, so neither
    // do the bits
    int run(int type, int direction, const T *x_re, const T *x_im, size_t in_dist, T *o_re, T *o_im, size_t out_dist,
            size_t batch, T *work, size_t work_len, hipStream_t s, hipEvent_t *ev = nullptr) const {
        size_t chunk = work_len / per();
        const size_t cap = ((size_t)1 << 38) / cells;  // a launch's groups stay below 2^38
        if (chunk > cap) chunk = cap;
        for (size_t b0 = 0; b0 < batch; b0 += chunk) {
            const size_t c = batch - b0 < chunk ? batch - b0 : chunk;
            int rc = run_chunk(type, direction, x_re + b0 * in_dist, x_im ? x_im + b0 * in_dist : nullptr, in_dist,
                               o_re + b0 * out_dist, o_im + b0 * out_dist, out_dist, c, work, s, ev);
            if (rc) return rc;
        }
        return PHAST_OK;
    }

    int check_dev(int type, int direction, const T *d_in_re, const T *d_in_im, size_t in_dist, const T *d_out_re,
                  const T *d_out_im, size_t out_dist, size_t batch, const T *d_work, size_t work_len) const {
        return nufft_check_dev(direction, d_in_re, d_in_im, in_dist, in_len(type), d_out_re, d_out_im, out_dist, out_len(type), batch,
                               d_work, work_len, per());
    }

    // device pointers, asynchronous on `s`: no allocation, no synchronisation
    int nufft_dev(int type, int direction, const T *d_in_re, const T *d_in_im, size_t in_dist, T *d_out_re, T *d_out_im,
                  size_t out_dist, size_t batch, T *d_work, size_t work_len, hipStream_t s) const {
        int rc = check_dev(type, direction, d_in_re, d_in_im, in_dist, d_out_re, d_out_im, out_dist, batch, d_work, work_len);
        if (rc || batch == 0) return rc;
        if (batch == 1) {
            in_dist = in_len(type);
            out_dist = out_len(type);
        }
        PHAST_ON_DEVICE(device);
        return run(type, direction, d_in_re, d_in_im, in_dist, d_out_re, d_out_im, out_dist, batch, d_work, work_len, s);
    }

    // host slices: through a device buffer of the call's own (input planes, output planes, then the workspace), on the null
    // stream; blocking.  in_im may be null: real data
    int nufft_host(int type, int direction, const T *in_re, const T *in_im, size_t num_in, T *out_re, T *out_im,
                   size_t num_out) const {
        if (!in_re || !out_re || !out_im) return PHAST_ERR_INVALID_ARG;
        if (direction != PHAST_FORWARD && direction != PHAST_REVERSE) return PHAST_ERR_INVALID_ARG;
        const size_t ni = in_len(type), no = out_len(type);
        if (num_in != ni || num_out != no) return PHAST_ERR_PLANNER_SIZE;
        PHAST_ON_DEVICE(device);
        const size_t x_len = (ni + 3) & ~(size_t)3, o_len = (no + 3) & ~(size_t)3;  // every part 16-byte aligned
        DevBuf buf;
        int rc = buf.alloc((2 * x_len + 2 * o_len + per()) * sizeof(T));
        if (rc) return rc;
        T *d_re = reinterpret_cast<T *>(buf.p), *d_im = d_re + x_len, *d_or = d_im + x_len, *d_oi = d_or + o_len, *d_w = d_oi + o_len;
        PHAST_HIP(hipMemcpy(d_re, in_re, ni * sizeof(T), hipMemcpyHostToDevice));
        if (in_im) PHAST_HIP(hipMemcpy(d_im, in_im, ni * sizeof(T), hipMemcpyHostToDevice));
        rc = run(type, direction, d_re, in_im ? d_im : nullptr, ni, d_or, d_oi, no, 1, d_w, per(), nullptr);
        if (rc) return rc;
        PHAST_HIP(hipMemcpy(out_re, d_or, no * sizeof(T), hipMemcpyDeviceToHost));
        PHAST_HIP(hipMemcpy(out_im, d_oi, no * sizeof(T), hipMemcpyDeviceToHost));
        return PHAST_OK;
    }

    // measurement hook: ms[0..2] = average milliseconds of the three stages (spread or pre, the D-dimensional transform of the
    // grid, deconvolve or interpolate) over `reps` Forward calls of one chunk (work_len >= workspace_len(batch)) at the natural
    // distances; ms[3] and ms[4] are 0 (the timer of the any-length planners has five slots); blocks
    int time_stages(int type, const T *d_in_re, const T *d_in_im, T *d_out_re, T *d_out_im, size_t batch, T *d_work,
                    size_t work_len, int reps, float *ms, hipStream_t s) const {
        if (!ms || reps < 1 || batch == 0 || (type != 1 && type != 2)) return PHAST_ERR_INVALID_ARG;
        const size_t ni = in_len(type), no = out_len(type);
        int rc = check_dev(type, PHAST_FORWARD, d_in_re, d_in_im, ni, d_out_re, d_out_im, no, batch, d_work, work_len);
        if (rc) return rc;
        if (work_len < workspace_len(batch) || batch > ((size_t)1 << 38) / cells) return PHAST_ERR_INVALID_ARG;
        PHAST_ON_DEVICE(device);
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
            rc = run(type, PHAST_FORWARD, d_in_re, d_in_im, ni, d_out_re, d_out_im, no, batch, d_work, work_len, s, ev.e);
            if (rc) return rc;
            PHAST_HIP(hipStreamSynchronize(s));
            for (int i = 0; i < 3; ++i) {
                float t = 0;
                PHAST_HIP(hipEventElapsedTime(&t, ev.e[i], ev.e[i + 1]));
                acc[i] += t;
            }
        }
        for (int i = 0; i < 5; ++i) ms[i] = i < 3 ? (float)(acc[i] / reps) : 0.0f;
        return PHAST_OK;
    }
};

// P over NufftNdPlanner<T, D> from host points (n: the mode counts, x: a pointer per coordinate); D comes from the two lists
template <typename P, size_t D>
static int nufft_nd_planner_new(const size_t (&n)[D], const double *const (&x)[D], size_t m_points, double eps, bool f32, P **out) {
    return nufft_planner_make(out, [&] { return nufft_nd_bad_args<D>(n, x, m_points, eps, f32); }, n, x, m_points, eps);
}
template <typename P, size_t D>
static int nufft_nd_planner_new_dev(const size_t (&n)[D], const double *const (&d_x)[D], size_t m_points, double eps, bool f32,
                                    hipStream_t s, P **out) {
    return nufft_planner_make_dev(out, [&] { return nufft_nd_bad_sizes<D>(n, d_x, m_points, eps, f32); }, s, n, d_x, m_points, eps);
}

}  // namespace phast
