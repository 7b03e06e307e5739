// planner_nufft_t3.hpp -- NufftT3Planner<T>: the non-uniform FFT of type 3 (nufft_t3.hpp) of M sources and K targets.  It
// owns an inner NufftPlanner<T> -- the type-2 path of n_f modes at the K rescaled targets -- and runs the outer spread (fused
// with the inner "pre") in front of the inner planner's transform and interpolation, and the post sweep behind them.
// Immutable after init: the inner planner, the sources sorted by outer grid cell (positions, permutation, cell starts), the M
// prephase factors in sorted order and the K post factors on the device.  What a call mutates is the caller's workspace (_dev
// calls) or a workspace of the inner engine's pool (host-slice calls).
#pragma once

#include "nufft_t3.hpp"
#include "planner_nufft.hpp"

namespace phast {

template <typename T> struct NufftT3Planner {
    NufftPlanner<T> inner;  // N = n_f modes, the K points t_k; its grid is n_g = 2 n_f
    NufftT3Grid grid;
    size_t sources = 0, targets = 0;  // M, K
    double eps = 0;
    double *d_xs = nullptr;
    uint32_t *d_perm = nullptr, *d_cell = nullptr;
    T *d_pre = nullptr, *d_dre = nullptr, *d_dim = nullptr;

    ~NufftT3Planner() {
        DeviceGuard on(inner.device);
        for (void *p : {(void *)d_xs, (void *)d_perm, (void *)d_cell, (void *)d_pre, (void *)d_dre, (void *)d_dim})
            if (p) hipFree(p);
    }

    // `x`: M host doubles, `s`: K host doubles; the arguments were checked by nufft_t3_bad_args
    int init(const double *x, size_t m_sources, const double *s, size_t k_targets, double eps_) {
        sources = m_sources;
        targets = k_targets;
        eps = eps_;
        grid = nufft_t3_grid(x, sources, s, targets, eps);
        std::vector<double> t(targets);
        nufft_t3_targets(grid, s, targets, t.data());
        int rc = inner.init((size_t)grid.nf, t.data(), targets, eps);
        if (rc) return rc;
        if (inner.m != 2 * (size_t)grid.nf || inner.w != grid.w) return PHAST_ERR_INVALID_ARG;  // n_f >= max(2 w, 8): never
        std::vector<double> u(sources), xs(sources);
        std::vector<uint32_t> perm(sources), cell((size_t)grid.nf + 1);
        nufft_t3_positions(grid, x, sources, u.data());
        nufft_bin(u.data(), sources, grid.log_f, xs.data(), perm.data(), cell.data());
        std::vector<T> pre(2 * sources), dre(targets), dim(targets);
        nufft_t3_pre_table<T>(grid, x, perm.data(), sources, pre.data());
        nufft_t3_post_table<T>(grid, s, t.data(), targets, dre.data(), dim.data());
        PHAST_ON_DEVICE(inner.device);
        PHAST_HIP(hipMalloc(reinterpret_cast<void **>(&d_xs), sources * sizeof(double)));
        PHAST_HIP(hipMalloc(reinterpret_cast<void **>(&d_perm), sources * sizeof(uint32_t)));
        PHAST_HIP(hipMalloc(reinterpret_cast<void **>(&d_cell), cell.size() * sizeof(uint32_t)));
        PHAST_HIP(hipMalloc(reinterpret_cast<void **>(&d_pre), pre.size() * sizeof(T)));
        PHAST_HIP(hipMalloc(reinterpret_cast<void **>(&d_dre), targets * sizeof(T)));
        PHAST_HIP(hipMalloc(reinterpret_cast<void **>(&d_dim), targets * sizeof(T)));
        PHAST_HIP(hipMemcpy(d_xs, xs.data(), sources * sizeof(double), hipMemcpyHostToDevice));
        PHAST_HIP(hipMemcpy(d_perm, perm.data(), sources * sizeof(uint32_t), hipMemcpyHostToDevice));
        PHAST_HIP(hipMemcpy(d_cell, cell.data(), cell.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        PHAST_HIP(hipMemcpy(d_pre, pre.data(), pre.size() * sizeof(T), hipMemcpyHostToDevice));
        PHAST_HIP(hipMemcpy(d_dre, dre.data(), targets * sizeof(T), hipMemcpyHostToDevice));
        PHAST_HIP(hipMemcpy(d_dim, dim.data(), targets * sizeof(T), hipMemcpyHostToDevice));
        return PHAST_OK;
    }

    // the post sweep runs in place on the caller's output planes: nothing beyond the inner grid
    size_t workspace_len(size_t batch) const { return inner.workspace_len(batch); }
    size_t table_bytes() const {
        return sources * (sizeof(double) + sizeof(uint32_t) + 2 * sizeof(T)) + ((size_t)grid.nf + 1) * sizeof(uint32_t) +
               2 * targets * sizeof(T);
    }
    size_t device_bytes() const { return table_bytes() + inner.device_bytes(); }
    std::string describe() const {
        char f[96];
        std::snprintf(f, sizeof f, " eps=%.3g w=%d n_f=%llu n_g=%llu SX=%.6g", eps, grid.w, grid.nf, 2 * grid.nf, grid.S * grid.X);
        return "nufft_t3 M=" + std::to_string(sources) + " K=" + std::to_string(targets) + f + ": " + inner.describe();
    }

    // `c` transforms: sources (re, im or null) at b * in_dist -> targets at b * out_dist, through the workspace wk (2 c n_g
    // elements).  ev: optional 6 events; ev[0..4] bound the four stages
    int run_chunk(const Planner<T> *pl, const typename Planner<T>::Lease &L, const typename Planner<T>::Choice &ch, int direction,
                  const T *x_re, const T *x_im, size_t in_dist, T *o_re, T *o_im, size_t out_dist, size_t c, T *wk,
                  hipEvent_t *ev = nullptr) const {
        hipStream_t s = L.stream;
        constexpr unsigned V = 16 / sizeof(T);
        NufftT3Args a{};
        a.in_re = x_re;
        a.in_im = x_im;
        a.out_re = wk;
        a.out_im = wk + c * inner.m;
        a.xs = d_xs;
        a.perm = d_perm;
        a.cell_start = d_cell;
        a.pre = d_pre;
        a.inv_hat = inner.d_inv;
        a.d_re = d_dre;
        a.d_im = d_dim;
        a.in_dist = in_dist;
        a.out_dist = out_dist;
        a.k = targets;
        a.log_f = grid.log_f;
        a.w = grid.w;
        a.reverse = direction == PHAST_REVERSE;
        if (ev) PHAST_HIP(hipEventRecord(ev[0], s));
        a.groups = c * inner.m;
        PHAST_HIP(launch_nufft_t3<T>(0, false, a, s));
        if (ev) PHAST_HIP(hipEventRecord(ev[1], s));
        int rc = inner.transform(pl, L, ch, direction, c, wk);
        if (rc) return rc;
        if (ev) PHAST_HIP(hipEventRecord(ev[2], s));
        rc = inner.interpolate(inner.chunk_args(0, out_dist), c, wk, o_re, o_im, s);
        if (rc) return rc;
        if (ev) PHAST_HIP(hipEventRecord(ev[3], s));
        a.in_re = a.in_im = nullptr;
        a.out_re = o_re;
        a.out_im = o_im;
        a.gpt = (unsigned)((targets + V - 1) / V);
        a.groups = c * a.gpt;
        PHAST_HIP(launch_nufft_t3<T>(1, inner.aligned(o_re) && inner.aligned(o_im) && out_dist % V == 0, a, s));
        if (ev)
            for (int i = 4; i < 6; ++i) PHAST_HIP(hipEventRecord(ev[i], s));
        return PHAST_OK;
    }

    // the batch in chunks
    int run(const Planner<T> *pl, const typename Planner<T>::Lease &L, int direction, const T *x_re, const T *x_im, size_t in_dist,
            T *o_re, T *o_im, size_t out_dist, size_t batch, T *work, size_t work_len, hipEvent_t *ev = nullptr) const {
        const typename Planner<T>::Choice ch = pl->choose(kC2C, 1, 1);
        return inner.for_each_chunk(batch, work_len, [&](size_t b0, size_t c) {
            return run_chunk(pl, L, ch, direction, x_re + b0 * in_dist, x_im ? x_im + b0 * in_dist : nullptr, in_dist,
                             o_re + b0 * out_dist, o_im + b0 * out_dist, out_dist, c, work, ev);
        });
    }

    int check_dev(int direction, const T *d_in_re, const T *d_in_im, size_t in_dist, const T *d_out_re, const T *d_out_im,
                  size_t out_dist, size_t batch, const T *d_work, size_t work_len) const {
        if (!d_in_re || !d_out_re || !d_out_im) return PHAST_ERR_INVALID_ARG;  // d_in_im may be null: real data
        if (direction != PHAST_FORWARD && direction != PHAST_REVERSE) return PHAST_ERR_INVALID_ARG;
        const size_t ni = sources, no = targets;
        if (batch > 1 && (in_dist < ni || out_dist < no)) return PHAST_ERR_INVALID_ARG;
        if (batch && (!d_work || work_len < workspace_len(1))) return PHAST_ERR_INVALID_ARG;
        if (batch) {  // the output is written while later chunks still read the input and the workspace
            const size_t in_span = (batch - 1) * (batch > 1 ? in_dist : 0) + ni, out_span = (batch - 1) * (batch > 1 ? out_dist : 0) + no;
            auto overlap = nufft_overlap<T>;
            for (const T *o : {d_out_re, d_out_im})
                if (overlap(o, out_span, d_in_re, in_span) || overlap(o, out_span, d_in_im, in_span) ||
                    overlap(o, out_span, d_work, work_len))
                    return PHAST_ERR_INVALID_ARG;
            if (overlap(d_out_re, out_span, d_out_im, out_span)) return PHAST_ERR_INVALID_ARG;
            if (overlap(d_work, work_len, d_in_re, in_span) || overlap(d_work, work_len, d_in_im, in_span)) return PHAST_ERR_INVALID_ARG;
        }
        return PHAST_OK;
    }

    // device pointers, asynchronous on `s`
    int nufft_dev(int direction, const T *d_in_re, const T *d_in_im, size_t in_dist, T *d_out_re, T *d_out_im, size_t out_dist,
                  size_t batch, T *d_work, size_t work_len, hipStream_t s) const {
        int rc = check_dev(direction, d_in_re, d_in_im, in_dist, d_out_re, d_out_im, out_dist, batch, d_work, work_len);
        if (rc || batch == 0) return rc;
        if (batch == 1) {
            in_dist = sources;
            out_dist = targets;
        }
        const Planner<T> *pl = inner.engine(s);
        PHAST_ON_DEVICE(inner.device);
        typename Planner<T>::Lease L;
        rc = pl->lease(L, s);
        return rc ? rc : run(pl, L, direction, d_in_re, d_in_im, in_dist, d_out_re, d_out_im, out_dist, batch, d_work, work_len);
    }

    // host slices: staged through the staging buffer of a workspace checked out of the inner engine's pool (input planes,
    // output planes, then the grid), on that workspace's own stream; blocking.  in_im may be null: real data
    int nufft_host(int direction, const T *in_re, const T *in_im, size_t num_in, T *out_re, T *out_im, size_t num_out) const {
        if (!in_re || !out_re || !out_im) return PHAST_ERR_INVALID_ARG;
        if (direction != PHAST_FORWARD && direction != PHAST_REVERSE) return PHAST_ERR_INVALID_ARG;
        const size_t ni = sources, no = targets, wl = workspace_len(1);
        if (num_in != ni || num_out != no) return PHAST_ERR_PLANNER_SIZE;
        const Planner<T> *pl = inner.inner->route_small(1);
        PHAST_ON_DEVICE(inner.device);
        typename Planner<T>::Lease L;
        int rc = pl->check_out(L, nullptr, 1);
        if (rc) return rc;
        const size_t x_len = (ni + 3) & ~(size_t)3, o_len = (no + 3) & ~(size_t)3;  // the grid stays 16-byte aligned
        void *stage = nullptr;
        rc = pl->stage(L, (2 * x_len + 2 * o_len + wl) * sizeof(T), &stage);
        if (rc) return rc;
        T *d_re = reinterpret_cast<T *>(stage), *d_im = d_re + x_len, *d_or = d_im + x_len, *d_oi = d_or + o_len, *d_w = d_oi + o_len;
        PHAST_HIP(hipMemcpyAsync(d_re, in_re, ni * sizeof(T), hipMemcpyHostToDevice, L.stream));
        if (in_im) PHAST_HIP(hipMemcpyAsync(d_im, in_im, ni * sizeof(T), hipMemcpyHostToDevice, L.stream));
        rc = run(pl, L, direction, d_re, in_im ? d_im : nullptr, ni, d_or, d_oi, no, 1, d_w, wl);
        if (rc) return rc;
        PHAST_HIP(hipMemcpyAsync(out_re, d_or, no * sizeof(T), hipMemcpyDeviceToHost, L.stream));
        PHAST_HIP(hipMemcpyAsync(out_im, d_oi, no * sizeof(T), hipMemcpyDeviceToHost, L.stream));
        PHAST_HIP(hipStreamSynchronize(L.stream));
        return PHAST_OK;
    }

    // measurement hook: ms[0..3] = average milliseconds of the four stages (spread, the n_g-point transform, interpolate, post)
    // over `reps` Forward calls of one chunk (work_len >= workspace_len(batch)) at the natural distances; ms[4] is 0; blocks
    int time_stages(const T *d_in_re, const T *d_in_im, T *d_out_re, T *d_out_im, size_t batch, T *d_work, size_t work_len,
                    int reps, float *ms, hipStream_t s) const {
        if (!ms || reps < 1 || batch == 0) return PHAST_ERR_INVALID_ARG;
        int rc = check_dev(PHAST_FORWARD, d_in_re, d_in_im, sources, d_out_re, d_out_im, targets, batch, d_work, work_len);
        if (rc) return rc;
        if (work_len < workspace_len(batch)) return PHAST_ERR_INVALID_ARG;
        const Planner<T> *pl = inner.engine(s);
        PHAST_ON_DEVICE(inner.device);
        return time_stages_of(pl, reps, ms, s, [&](const auto &L, hipEvent_t *ev) {
            return run(pl, L, PHAST_FORWARD, d_in_re, d_in_im, sources, d_out_re, d_out_im, targets, batch, d_work, work_len, ev);
        });
    }
};

template <typename P>
static int nufft_t3_planner_new(const double *x, size_t m_sources, const double *s, size_t k_targets, double eps, bool f32, P **out) {
    if (!out) return PHAST_ERR_INVALID_ARG;
    *out = nullptr;
    if (nufft_t3_bad_args(x, m_sources, s, k_targets, eps, f32)) return PHAST_ERR_INVALID_ARG;  // before the device is touched
    auto *p = new (std::nothrow) P();
    if (!p) return PHAST_ERR_ALLOC;
    int rc = p->init(x, m_sources, s, k_targets, eps);
    if (rc) {
        delete p;
        return rc;
    }
    *out = p;
    return PHAST_OK;
}

}  // namespace phast
