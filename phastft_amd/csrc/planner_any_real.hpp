// planner_any_real.hpp -- AnyRealPlanner<T>: real transforms (R2C / C2R) of any length N (any_real.hpp).
// It holds exactly one of: a PlannerR2c<T>(N) (a power of two >= 4: the existing real path, same bits, no workspace), an
// AnyPlanner<T> of H = N / 2 (even N) or of N (odd N) whose table, spectrum sweep and engine plan it runs between its own
// sweeps, or, for N = 1 and 2, a Planner<T>(1) whose workspace pool stages host-slice calls.  Immutable after init, no
// per-call state: what a call mutates is the caller's workspace (_dev) or a workspace of the inner pool (host slices).  The
// convolution core, the chunk loop and the stage timer are AnyPlanner's (planner_any.hpp); this file has the real pad and
// post sweeps around the core, the direct N = 1, 2 kernel and the argument checks.
#pragma once

#include "any_real.hpp"
#include "planner_any.hpp"
#include "planner_r2c.hpp"

namespace phast {

template <typename T> struct AnyRealPlanner {
    size_t n = 0, half = 0;  // N and floor(N / 2): the half spectrum has half + 1 points
    size_t m = 0;            // the inner convolution length (0: no Bluestein)
    int device = -1;
    std::unique_ptr<PlannerR2c<T>> r2c;  // N a power of two >= 4
    std::unique_ptr<AnyPlanner<T>> any;  // Bluestein of l = H (even N) or N (odd N)
    std::unique_ptr<Planner<T>> tiny;    // N = 1, 2

    bool pow2() const { return r2c != nullptr; }

    int init(size_t num_points) {
        if (num_points == 0 || num_points > kAnyMaxN) return PHAST_ERR_INVALID_ARG;
        n = num_points;
        half = n / 2;
        int rc = ensure_device(&device);
        if (rc) return rc;
        if (n >= 4 && is_pow2(n)) {
            PlannerR2c<T> *p = nullptr;
            rc = r2c_planner_new(n, &p);
            r2c.reset(p);
            return rc;
        }
        if (n <= 2) {
            tiny.reset(new (std::nothrow) Planner<T>());
            if (!tiny) return PHAST_ERR_ALLOC;
            return tiny->init(1);
        }
        any.reset(new (std::nothrow) AnyPlanner<T>());
        if (!any) return PHAST_ERR_ALLOC;
        rc = any->init(n & 1 ? n : half);  // never a power of two: H is one only when N is
        m = any->m;
        return rc;
    }

    size_t workspace_len(size_t batch) const { return any ? 2 * m * batch : 0; }
    size_t device_bytes() const {
        if (r2c) return r2c->dit.device_bytes();
        if (any) return any->device_bytes();
        return tiny ? tiny->device_bytes() : 0;
    }
    std::string describe() const {
        const std::string head = "real any N=" + std::to_string(n);
        if (r2c) return head + " (power of two): R2C over " + r2c->dit.describe();
        if (tiny) return head + " (direct)";
        return head + (n & 1 ? " (odd): " : " (even, packed into H=" + std::to_string(half) + "): ") + any->describe();
    }

    // `c` transforms through the workspace w (2 c M elements): R2C reads in_a (the real signal) and writes the planes
    // (out_a, out_b); C2R reads the planes (in_a, in_b) and writes the real signal out_a.  ev: optional 6 events around the
    // five stages (time_stages)
    int run_chunk(bool c2r, const Planner<T> *pl, const typename Planner<T>::Lease &L, const typename Planner<T>::Choice &ch,
                  const T *in_a, const T *in_b, T *out_a, T *out_b, size_t c, size_t in_dist, size_t out_dist, T *w,
                  hipEvent_t *ev = nullptr) const {
        hipStream_t s = L.stream;
        constexpr unsigned V = 16 / sizeof(T);
        const bool odd = n & 1;
        const size_t l = any->n;
        T *w_re = w, *w_im = w + c * m;
        auto al = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; };
        AnyRealArgs a{};
        a.n = n;
        a.l = l;
        a.log_m = any->log_m;
        a.in_dist = in_dist;
        a.out_dist = out_dist;
        a.in_re = in_a;
        a.in_im = in_b;
        a.out_re = w_re;
        a.out_im = w_im;
        a.groups = c * (m / V);
        const bool vec_in = al(in_a) && (!c2r || al(in_b)) && (c == 1 || in_dist % V == 0);  // one transform: dist unused
        if (ev) PHAST_HIP(hipEventRecord(ev[0], s));
        PHAST_HIP(launch_any_real<T>(c2r ? (odd ? kC2rOddPad : kC2rPre) : (odd ? kR2cOddPad : kR2cPack), vec_in, a, s));
        int rc = any->convolve(pl, L, ch, w, c, ev);
        if (rc) return rc;
        a.in_re = w_re;
        a.in_im = w_im;
        a.out_re = out_a;
        a.out_im = out_b;
        int kind;
        size_t pts;  // points of a transform the post sweep owns (groups of V from point 0)
        if (!c2r) {
            kind = odd ? kR2cOddPost : kR2cUntangle;
            pts = odd ? (l - 1) / 2 + 1 : l / 2 + 1;  // k <= (N-1)/2; the pairs (k, H-k), k <= H/2
        } else {
            kind = odd ? kC2rOddPost : kC2rInterleave;
            pts = l;
            a.scale = 1.0 / (double)l;  // 1/N (odd), 1/H (even: the H-point inverse of the power-of-two path)
        }
        a.gpt = (unsigned)((pts + V - 1) / V);
        a.groups = c * a.gpt;
        const bool vec_out = al(out_a) && (c2r || al(out_b)) && (c == 1 || out_dist % V == 0);
        PHAST_HIP(launch_any_real<T>(kind, vec_out, a, s));
        if (ev) PHAST_HIP(hipEventRecord(ev[5], s));
        return PHAST_OK;
    }

    // the batch in chunks (AnyPlanner::for_each_chunk)
    int run(bool c2r, const Planner<T> *pl, const typename Planner<T>::Lease &L, const T *in_a, const T *in_b, T *out_a,
            T *out_b, size_t batch, size_t in_dist, size_t out_dist, T *work, size_t work_len, hipEvent_t *ev = nullptr) const {
        const typename Planner<T>::Choice ch = pl->choose(kC2C, 1, 1);
        return any->for_each_chunk(batch, work_len, [&](size_t b0, size_t c) {
            return run_chunk(c2r, pl, L, ch, in_a + b0 * in_dist, in_b ? in_b + b0 * in_dist : nullptr, out_a + b0 * out_dist,
                             out_b ? out_b + b0 * out_dist : nullptr, c, in_dist, out_dist, work, ev);
        });
    }

    int run_tiny(bool c2r, const T *in_a, T *out_a, T *out_b, size_t batch, size_t in_dist, size_t out_dist, hipStream_t s) const {
        AnyRealArgs a{};
        a.n = n;
        a.in_re = in_a;
        a.out_re = out_a;
        a.out_im = out_b;
        a.in_dist = in_dist;
        a.out_dist = out_dist;
        a.groups = batch;
        PHAST_HIP(launch_any_real<T>(c2r ? kC2rTiny : kR2cTiny, false, a, s));
        return PHAST_OK;
    }

    // the checks of a _dev call: R2C in = the real signal (dist >= N), out = the planes (dist >= N/2 + 1); C2R the reverse
    int check_dev(bool c2r, const void *a, const void *b, const void *c, size_t num, size_t batch, size_t in_dist,
                  size_t out_dist, const T *d_work, size_t work_len) const {
        if (!a || !b || !c) return PHAST_ERR_INVALID_ARG;
        if (num != n) return PHAST_ERR_PLANNER_SIZE;
        const size_t real_dist = c2r ? out_dist : in_dist, cx_dist = c2r ? in_dist : out_dist;
        if (batch > 1 && (real_dist < n || cx_dist < half + 1)) return PHAST_ERR_INVALID_ARG;
        if (any && batch && (!d_work || work_len < 2 * m)) return PHAST_ERR_INVALID_ARG;
        return PHAST_OK;
    }

    // device pointers, asynchronous on `s`
    int dev(bool c2r, const T *in_a, const T *in_b, T *out_a, T *out_b, size_t num, size_t batch, size_t in_dist,
            size_t out_dist, T *d_work, size_t work_len, hipStream_t s) const {
        int rc = c2r ? check_dev(true, in_a, in_b, out_a, num, batch, in_dist, out_dist, d_work, work_len)
                     : check_dev(false, in_a, out_a, out_b, num, batch, in_dist, out_dist, d_work, work_len);
        if (rc) return rc;
        if (batch == 0) return PHAST_OK;
        if (batch == 1) {
            in_dist = c2r ? half + 1 : n;
            out_dist = c2r ? n : half + 1;
        }
        if (r2c) return c2r ? r2c->c2r(in_a, in_b, out_a, batch, in_dist, out_dist, s)
                            : r2c->r2c(in_a, out_a, out_b, batch, in_dist, out_dist, s);
        PHAST_ON_DEVICE(device);
        if (tiny) return run_tiny(c2r, in_a, out_a, out_b, batch, in_dist, out_dist, s);
        const Planner<T> *pl = any->engine(s);
        typename Planner<T>::Lease L;
        rc = pl->lease(L, s);
        return rc ? rc : run(c2r, pl, L, in_a, in_b, out_a, out_b, batch, in_dist, out_dist, d_work, work_len);
    }

    // host slices, staged through the staging buffer of a workspace of the inner pool (input, output, convolution
    // workspace), on that workspace's own stream; blocking.  R2C: (a = the signal; b, c = the planes); C2R: (a, b = the
    // planes; c = the signal)
    int host(bool c2r, const T *in_a, size_t a_len, const T *in_b, size_t b_len, T *out_a, size_t oa_len, T *out_b,
             size_t ob_len) const {
        const size_t h1 = half + 1;
        if (!c2r) {
            if (!in_a || !out_a || !out_b) return PHAST_ERR_INVALID_ARG;
            if (a_len != n) return PHAST_ERR_R2C_INPUT_LEN;
            if (oa_len != h1) return PHAST_ERR_R2C_OUT_RE_LEN;
            if (ob_len != h1) return PHAST_ERR_R2C_OUT_IM_LEN;
            if (r2c) return r2c_host<T>(in_a, a_len, out_a, oa_len, out_b, ob_len, r2c.get());
        } else {
            if (!in_a || !in_b || !out_a) return PHAST_ERR_INVALID_ARG;
            if (oa_len != n) return PHAST_ERR_C2R_OUTPUT_LEN;
            if (a_len != h1) return PHAST_ERR_C2R_IN_RE_LEN;
            if (b_len != h1) return PHAST_ERR_C2R_IN_IM_LEN;
            if (r2c) return c2r_host<T>(in_a, a_len, in_b, b_len, out_a, oa_len, r2c.get(), false, 0, 0);
        }
        const Planner<T> *pl = tiny ? tiny.get() : any->inner->route_small(1);
        PHAST_ON_DEVICE(device);
        typename Planner<T>::Lease L;
        int rc = pl->check_out(L, nullptr, 1);
        if (rc) return rc;
        auto up = [](size_t k) { return (k + 3) & ~(size_t)3; };  // every part 16-byte aligned
        const size_t nr = up(n), nc = up(h1);
        void *stage = nullptr;
        rc = pl->stage(L, (nr + 2 * nc + 2 * m) * sizeof(T), &stage);
        if (rc) return rc;
        T *d_real = reinterpret_cast<T *>(stage), *d_re = d_real + nr, *d_im = d_re + nc, *d_w = d_im + nc;
        if (!c2r) {
            PHAST_HIP(hipMemcpyAsync(d_real, in_a, n * sizeof(T), hipMemcpyHostToDevice, L.stream));
            rc = tiny ? run_tiny(false, d_real, d_re, d_im, 1, n, h1, L.stream)
                      : run(false, pl, L, d_real, nullptr, d_re, d_im, 1, n, h1, d_w, 2 * m);
            if (rc) return rc;
            PHAST_HIP(hipMemcpyAsync(out_a, d_re, h1 * sizeof(T), hipMemcpyDeviceToHost, L.stream));
            PHAST_HIP(hipMemcpyAsync(out_b, d_im, h1 * sizeof(T), hipMemcpyDeviceToHost, L.stream));
        } else {
            PHAST_HIP(hipMemcpyAsync(d_re, in_a, h1 * sizeof(T), hipMemcpyHostToDevice, L.stream));
            PHAST_HIP(hipMemcpyAsync(d_im, in_b, h1 * sizeof(T), hipMemcpyHostToDevice, L.stream));
            rc = tiny ? run_tiny(true, d_re, d_real, nullptr, 1, h1, n, L.stream)
                      : run(true, pl, L, d_re, d_im, d_real, nullptr, 1, h1, n, d_w, 2 * m);
            if (rc) return rc;
            PHAST_HIP(hipMemcpyAsync(out_a, d_real, n * sizeof(T), hipMemcpyDeviceToHost, L.stream));
        }
        PHAST_HIP(hipStreamSynchronize(L.stream));
        return PHAST_OK;
    }

    // measurement hook: average milliseconds of the five stages (pad, forward engine, spectrum, inverse engine, post) over
    // `reps` calls of one chunk at the natural distances (work_len >= 2 M batch); blocks
    int time_stages(bool c2r, const T *in_a, const T *in_b, T *out_a, T *out_b, size_t batch, T *d_work, size_t work_len,
                    int reps, float *ms, hipStream_t s) const {
        if (!ms || reps < 1 || batch == 0) return PHAST_ERR_INVALID_ARG;
        const size_t in_dist = c2r ? half + 1 : n, out_dist = c2r ? n : half + 1;
        int rc = c2r ? check_dev(true, in_a, in_b, out_a, n, batch, in_dist, out_dist, d_work, work_len)
                     : check_dev(false, in_a, out_a, out_b, n, batch, in_dist, out_dist, d_work, work_len);
        if (rc) return rc;
        if (!any || work_len < 2 * m * batch) return PHAST_ERR_INVALID_ARG;
        const Planner<T> *pl = any->engine(s);
        PHAST_ON_DEVICE(device);
        return time_stages_of(pl, reps, ms, s, [&](const auto &L, hipEvent_t *ev) {
            return run(c2r, pl, L, in_a, in_b, out_a, out_b, batch, in_dist, out_dist, d_work, work_len, ev);
        });
    }
};

}  // namespace phast
