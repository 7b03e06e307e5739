// planner_nufft2d.hpp -- Nufft2dPlanner<T>: non-uniform FFTs of types 1 and 2 in two dimensions (nufft2d.hpp) of M points and
// N1 x N2 modes on an owned NdPlanner<T> of dims (g1, g2).  Immutable after init but for set_points_dev: the Nd planner, the point set sorted by grid
// cell (positions, permutation, cell starts) and the N1 + N2 reciprocals 1 / phi^(k) on the device.  What a call mutates is the
// caller's workspace (_dev calls) or a device buffer of the call's own (host-slice calls), so graph capture and concurrent
// streams and threads need nothing beyond what the Nd planner already does.
//
// Workspace (elements of T) of a chunk of c transforms: c re grids, c im grids, then the Nd planner's 2 c G (its transposed
// copies; both axes are powers of two, so there is no Bluestein part): 4 G per transform, G = g1 g2.
#pragma once

#include "nufft2d.hpp"
#include "planner_nd.hpp"
#include "planner_nufft_sort.hpp"

namespace phast {

template <typename T> struct Nufft2dPlanner {
    size_t n1 = 0, n2 = 0, points = 0;  // N1, N2, M
    size_t g1 = 0, g2 = 0, cells = 0;   // the fine grid and G = g1 g2
    unsigned log_g1 = 0, log_g2 = 0;
    int w = 0, device = -1;
    double eps = 0;
    NdPlanner<T> nd;
    double *d_xs = nullptr, *d_ys = nullptr;
    uint32_t *d_perm = nullptr, *d_cell = nullptr;
    T *d_inv1 = nullptr, *d_inv2 = nullptr;

    ~Nufft2dPlanner() {
        DeviceGuard on(device);
        for (void *p : {(void *)d_xs, (void *)d_ys, (void *)d_perm, (void *)d_cell, (void *)d_inv1, (void *)d_inv2})
            if (p) hipFree(p);
    }

    // 1 / phi^(k) of an axis of n modes on g grid points in double, rounded to T; phi^ is even in k
    std::vector<T> inv_table(size_t n, size_t g) const {
        std::vector<T> inv(n);
        const NufftQuad hat(w, g);
        for (size_t k = 0; k <= n / 2; ++k) {
            const T r = (T)(1.0 / hat((long long)k));
            if (k < (n + 1) / 2) inv[k] = r;
            if (k > 0) inv[n - k] = r;
        }
        return inv;
    }

    // what does not depend on the points: the sizes, the Nd planner, 1 / phi^ on the device, and room for the point tables
    int init_grid(size_t n1_, size_t n2_, size_t m_points, double eps_) {
        n1 = n1_;
        n2 = n2_;
        points = m_points;
        eps = eps_;
        w = nufft_width(eps);
        g1 = (size_t)nufft_grid(n1, w);
        g2 = (size_t)nufft_grid(n2, w);
        cells = g1 * g2;
        log_g1 = ilog2(g1);
        log_g2 = ilog2(g2);
        const size_t dims[2] = {g1, g2};
        int rc = nd.init(dims, 2);
        if (rc) return rc;
        device = nd.device;
        const std::vector<T> inv1 = inv_table(n1, g1), inv2 = inv_table(n2, g2);
        PHAST_ON_DEVICE(device);
        PHAST_HIP(hipMalloc(reinterpret_cast<void **>(&d_xs), points * sizeof(double)));
        PHAST_HIP(hipMalloc(reinterpret_cast<void **>(&d_ys), points * sizeof(double)));
        PHAST_HIP(hipMalloc(reinterpret_cast<void **>(&d_perm), points * sizeof(uint32_t)));
        PHAST_HIP(hipMalloc(reinterpret_cast<void **>(&d_cell), (cells + 1) * sizeof(uint32_t)));
        PHAST_HIP(hipMalloc(reinterpret_cast<void **>(&d_inv1), n1 * sizeof(T)));
        PHAST_HIP(hipMalloc(reinterpret_cast<void **>(&d_inv2), n2 * sizeof(T)));
        PHAST_HIP(hipMemcpy(d_inv1, inv1.data(), n1 * sizeof(T), hipMemcpyHostToDevice));
        PHAST_HIP(hipMemcpy(d_inv2, inv2.data(), n2 * sizeof(T), hipMemcpyHostToDevice));
        return PHAST_OK;
    }

    // `x`, `y`: M host doubles in turns; the arguments were checked by nufft2d_bad_args
    int init(size_t n1_, size_t n2_, const double *x, const double *y, size_t m_points, double eps_) {
        int rc = init_grid(n1_, n2_, m_points, eps_);
        if (rc) return rc;
        std::vector<double> xs(points), ys(points);
        std::vector<uint32_t> perm(points), cell(cells + 1);
        nufft2d_bin(x, y, points, log_g1, log_g2, xs.data(), ys.data(), perm.data(), cell.data());
        PHAST_ON_DEVICE(device);
        PHAST_HIP(hipMemcpy(d_xs, xs.data(), points * sizeof(double), hipMemcpyHostToDevice));
        PHAST_HIP(hipMemcpy(d_ys, ys.data(), points * sizeof(double), hipMemcpyHostToDevice));
        PHAST_HIP(hipMemcpy(d_perm, perm.data(), points * sizeof(uint32_t), hipMemcpyHostToDevice));
        PHAST_HIP(hipMemcpy(d_cell, cell.data(), (cells + 1) * sizeof(uint32_t), hipMemcpyHostToDevice));
        return PHAST_OK;
    }

    // as init, with `d_x`, `d_y`: M doubles each in device memory (nufft_sort.hpp), ordered after the earlier work of `s`; blocks.
    // The arguments but the points' values were checked by nufft2d_bad_sizes; PHAST_ERR_INVALID_ARG for a coordinate that is not
    // finite
    int init_dev(size_t n1_, size_t n2_, const double *d_x, const double *d_y, size_t m_points, double eps_, hipStream_t s) {
        int rc = init_grid(n1_, n2_, m_points, eps_);
        if (rc) return rc;
        PHAST_ON_DEVICE(device);
        return nufft_sort_build(d_x, d_y, nullptr, points, log_g1, log_g2, 0, d_perm, d_cell, d_xs, d_ys, nullptr, s);
    }

    // new points, the same M of them, from device memory: the rules of NufftPlanner::set_points_dev (planner_nufft.hpp) -- the
    // tables are rewritten in place, a rejected point set leaves the planner as it was, the call blocks, and it orders itself
    // after the earlier work of `s` ONLY: the caller must have finished the work on other streams that uses the planner
    int set_points_dev(const double *d_x, const double *d_y, size_t m_points, hipStream_t s, float *ms = nullptr) {
        if (!d_x || !d_y) return PHAST_ERR_INVALID_ARG;
        if (m_points != points) return PHAST_ERR_PLANNER_SIZE;
        PHAST_ON_DEVICE(device);
        if (nufft_sort_stream_busy(s)) return PHAST_ERR_INVALID_ARG;
        return nufft_sort_build(d_x, d_y, nullptr, points, log_g1, log_g2, 0, d_perm, d_cell, d_xs, d_ys, nullptr, s, ms);
    }

    size_t workspace_len(size_t batch) const { return 4 * cells * batch; }
    size_t table_bytes() const {
        return points * (2 * sizeof(double) + sizeof(uint32_t)) + (cells + 1) * sizeof(uint32_t) + (n1 + n2) * sizeof(T);
    }
    size_t device_bytes() const { return table_bytes() + nd.device_bytes(); }
    std::string describe() const {
        char f[48];
        std::snprintf(f, sizeof f, " eps=%.3g w=%d", eps, w);
        return "nufft2d N=" + std::to_string(n1) + "x" + std::to_string(n2) + " M=" + std::to_string(points) + f +
               " grid=" + std::to_string(g1) + "x" + std::to_string(g2) + ": " + nd.describe();
    }
    size_t modes() const { return n1 * n2; }
    size_t in_len(int type) const { return type == 1 ? points : modes(); }
    size_t out_len(int type) const { return type == 1 ? modes() : points; }

    // `c` transforms of type 1 or 2: input planes (re, im or null) at b * in_dist -> output planes at b * out_dist, through
    // the workspace wk (4 c G elements: c re grids, c im grids, the Nd planner's 2 c G).  ev: optional 4 events around the
    // three stages
    int run_chunk(int type, int direction, const T *x_re, const T *x_im, size_t in_dist, T *o_re, T *o_im, size_t out_dist,
                  size_t c, T *wk, hipStream_t s, hipEvent_t *ev = nullptr) const {
        constexpr unsigned V = 16 / sizeof(T);
        T *w_re = wk, *w_im = wk + c * cells, *w_nd = wk + 2 * c * cells;
        auto al = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; };
        // 16-byte accesses: aligned planes and workspace, and the transforms' planes a multiple of the group apart (one
        // transform has no distance to meet)
        auto vec = [&](const T *re, const T *im, size_t dist) { return al(re) && al(im) && al(wk) && (c == 1 || dist % V == 0); };
        Nufft2dArgs a{};
        a.xs = d_xs;
        a.ys = d_ys;
        a.perm = d_perm;
        a.cell_start = d_cell;
        a.inv1 = d_inv1;
        a.inv2 = d_inv2;
        a.in_dist = in_dist;
        a.out_dist = out_dist;
        a.n1 = n1;
        a.n2 = n2;
        a.m = points;
        a.log_g1 = log_g1;
        a.log_g2 = log_g2;
        a.w = w;
        if (ev) PHAST_HIP(hipEventRecord(ev[0], s));
        a.in_re = x_re;
        a.in_im = x_im;
        a.out_re = w_re;
        a.out_im = w_im;
        if (type == 1) {
            a.groups = c * cells;
            PHAST_HIP(launch_nufft2d<T>(0, false, a, s));
        } else {
            a.groups = c * (cells / V);
            PHAST_HIP(launch_nufft2d<T>(2, vec(x_re, x_im, in_dist), a, s));
        }
        if (ev) PHAST_HIP(hipEventRecord(ev[1], s));
        // always the Forward transform (Reverse of the Nd planner scales by 1 / G).  Reverse by the swap trick: the FFT of
        // (im, re) is (im, re) of the transform with the + sign
        T *e_re = direction == PHAST_REVERSE ? w_im : w_re, *e_im = direction == PHAST_REVERSE ? w_re : w_im;
        int rc = nd.fft_dev_nd(e_re, e_im, cells, c, cells, PHAST_FORWARD, w_nd, 2 * c * cells, s);
        if (rc) return rc;
        if (ev) PHAST_HIP(hipEventRecord(ev[2], s));
        a.in_re = w_re;
        a.in_im = w_im;
        a.out_re = o_re;
        a.out_im = o_im;
        if (type == 1) {
            a.gpt = (unsigned)(n1 * ((n2 + V - 1) / V));
            a.groups = c * a.gpt;
            PHAST_HIP(launch_nufft2d<T>(3, vec(o_re, o_im, out_dist), a, s));
        } else {
            a.groups = c * points;
            PHAST_HIP(launch_nufft2d<T>(1, false, a, s));
        }
        if (ev) PHAST_HIP(hipEventRecord(ev[3], s));
        return PHAST_OK;
    }

    // the batch in chunks of floor(work_len / 4G) transforms; the Nd planner's plans do not depend on the chunk, so neither
    // do the bits
    int run(int type, int direction, const T *x_re, const T *x_im, size_t in_dist, T *o_re, T *o_im, size_t out_dist,
            size_t batch, T *work, size_t work_len, hipStream_t s, hipEvent_t *ev = nullptr) const {
        size_t chunk = work_len / (4 * cells);
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

    // [p, p + len) and [q, q + qlen) share an element
    static bool overlap(const T *p, size_t len, const T *q, size_t qlen) {
        const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
        return p && q && a < b + qlen * sizeof(T) && b < a + len * sizeof(T);
    }

    // the rules and return codes of NufftPlanner::check_dev
    int check_dev(int type, int direction, const T *d_in_re, const T *d_in_im, size_t in_dist, const T *d_out_re,
                  const T *d_out_im, size_t out_dist, size_t batch, const T *d_work, size_t work_len) const {
        if (!d_in_re || !d_out_re || !d_out_im) return PHAST_ERR_INVALID_ARG;  // d_in_im may be null: real data
        if (direction != PHAST_FORWARD && direction != PHAST_REVERSE) return PHAST_ERR_INVALID_ARG;
        const size_t ni = in_len(type), no = out_len(type);
        if (batch > 1 && (in_dist < ni || out_dist < no)) return PHAST_ERR_INVALID_ARG;
        if (batch && (!d_work || work_len < 4 * cells)) return PHAST_ERR_INVALID_ARG;
        if (batch) {  // the output is written while later chunks still read the input and the workspace
            const size_t in_span = (batch - 1) * (batch > 1 ? in_dist : 0) + ni, out_span = (batch - 1) * (batch > 1 ? out_dist : 0) + no;
            for (const T *o : {d_out_re, d_out_im})
                if (overlap(o, out_span, d_in_re, in_span) || overlap(o, out_span, d_in_im, in_span) ||
                    overlap(o, out_span, d_work, work_len))
                    return PHAST_ERR_INVALID_ARG;
            if (overlap(d_out_re, out_span, d_out_im, out_span)) return PHAST_ERR_INVALID_ARG;
            if (overlap(d_work, work_len, d_in_re, in_span) || overlap(d_work, work_len, d_in_im, in_span)) return PHAST_ERR_INVALID_ARG;
        }
        return PHAST_OK;
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
        int rc = buf.alloc((2 * x_len + 2 * o_len + 4 * cells) * sizeof(T));
        if (rc) return rc;
        T *d_re = reinterpret_cast<T *>(buf.p), *d_im = d_re + x_len, *d_or = d_im + x_len, *d_oi = d_or + o_len, *d_w = d_oi + o_len;
        PHAST_HIP(hipMemcpy(d_re, in_re, ni * sizeof(T), hipMemcpyHostToDevice));
        if (in_im) PHAST_HIP(hipMemcpy(d_im, in_im, ni * sizeof(T), hipMemcpyHostToDevice));
        rc = run(type, direction, d_re, in_im ? d_im : nullptr, ni, d_or, d_oi, no, 1, d_w, 4 * cells, nullptr);
        if (rc) return rc;
        PHAST_HIP(hipMemcpy(out_re, d_or, no * sizeof(T), hipMemcpyDeviceToHost));
        PHAST_HIP(hipMemcpy(out_im, d_oi, no * sizeof(T), hipMemcpyDeviceToHost));
        return PHAST_OK;
    }

    // measurement hook: ms[0..2] = average milliseconds of the three stages (spread or pre, the 2-D transform of the grid,
    // deconvolve or interpolate) over `reps` Forward calls of one chunk (work_len >= workspace_len(batch)) at the natural
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

template <typename P>
static int nufft2d_planner_new(size_t n1, size_t n2, const double *x, const double *y, size_t m_points, double eps, bool f32, P **out) {
    if (!out) return PHAST_ERR_INVALID_ARG;
    *out = nullptr;
    if (nufft2d_bad_args(n1, n2, m_points, x, y, eps, f32)) return PHAST_ERR_INVALID_ARG;  // before the device is touched
    auto *p = new (std::nothrow) P();
    if (!p) return PHAST_ERR_ALLOC;
    int rc = p->init(n1, n2, x, y, m_points, eps);
    if (rc) {
        delete p;
        return rc;
    }
    *out = p;
    return PHAST_OK;
}

// the same from M doubles per coordinate in device memory, ordered after the earlier work of `s`
template <typename P>
static int nufft2d_planner_new_dev(size_t n1, size_t n2, const double *d_x, const double *d_y, size_t m_points, double eps, bool f32,
                                   hipStream_t s, P **out) {
    if (!out) return PHAST_ERR_INVALID_ARG;
    *out = nullptr;
    if (nufft2d_bad_sizes(n1, n2, m_points, d_x, d_y, eps, f32)) return PHAST_ERR_INVALID_ARG;  // before the device is touched
    if (nufft_sort_stream_busy(s)) return PHAST_ERR_INVALID_ARG;
    auto *p = new (std::nothrow) P();
    if (!p) return PHAST_ERR_ALLOC;
    int rc = p->init_dev(n1, n2, d_x, d_y, m_points, eps, s);
    if (rc) {
        delete p;
        return rc;
    }
    *out = p;
    return PHAST_OK;
}

}  // namespace phast
