// planner_nd.hpp -- NdPlanner<T> (complex) and RealNdPlanner<T> (R2C / C2R): transforms over every axis of a row-major
// array of rank 1 .. 8 (nd.hpp).  The schedule (nd_schedule) alternates row transforms of the last axis on
// the one-axis planners with batched planar transposes (nd.hip).
//
// Each distinct axis length has one AnyPlanner<T> (the real last axis one AnyRealPlanner<T>).  Each transform step has ONE
// engine plan, fixed at init: the plan of its rows for one array (rows of the step), on the engine planner route_small(rows)
// picks for them.  It runs for every batch and chunk size, so for two or more non-unit axes the bits of a transform do not
// depend on the batch, the chunking, the stream, graph replay or host-slice vs _dev.  One non-unit axis is the one-axis
// call itself (same bits, its own batch rules).  Immutable after init, no per-call state: what a call mutates is the
// caller's workspace (_dev) or a device buffer of its own (host slices).
//
// Workspace (elements of T): transposed copies of the chunk's arrays (complex and R2C one, C2R two: it ping-pongs between
// them, as it may not write its input planes and the real output cannot hold a complex intermediate), then the largest
// Bluestein workspace a step needs for the chunk.  workspace_len(batch) runs the batch in one chunk (the real planner's
// counts C2R's two copies, so one length serves both directions); workspace_len(1) serves any batch, in chunks.  The
// smallest legal length is the copies of one array plus 2 M of the largest Bluestein axis (min_work): the Bluestein rows
// then run in chunks of a few rows.  An R2C call takes one copy of the half spectrum per array less.
#pragma once

#include <memory>
#include <vector>

#include "nd.hpp"
#include "planner_any.hpp"
#include "planner_any_real.hpp"

namespace phast {

template <typename T> struct NdCore {
    using Lease = typename Planner<T>::Lease;
    using Choice = typename Planner<T>::Choice;
    size_t rank = 0, dims[kNdMaxRank] = {};
    size_t q = 0, sq[kNdMaxRank] = {};  // the squeezed shape
    unsigned long long total = 0;       // prod dims (real: the real points)
    NdStep steps[2 * kNdMaxRank + 1] = {};
    size_t ns = 0;
    int device = -1;
    std::vector<std::unique_ptr<AnyPlanner<T>>> axis_pl;  // one per distinct complex axis length
    // per step: the one-axis planner and the engine plan of a transform step (kNdTransform)
    struct StepPlan {
        const AnyPlanner<T> *any = nullptr;
        const Planner<T> *eng = nullptr;
        Choice ch;
    };
    StepPlan plan[2 * kNdMaxRank + 1];

    const AnyPlanner<T> *any_of(size_t n) const {
        for (const auto &p : axis_pl)
            if (p->n == n) return p.get();
        return nullptr;
    }
    int init_core(const size_t *d, size_t r, int kind) {
        int bad = 1;
        q = nd_squeeze(d, r, kind, sq, &total, &bad);
        if (bad) return PHAST_ERR_INVALID_ARG;
        rank = r;
        for (size_t i = 0; i < r; ++i) dims[i] = d[i];
        ns = nd_schedule(sq, q, kind, steps);
        int rc = ensure_device(&device);
        if (rc) return rc;
        for (size_t i = 0; i < ns; ++i) {
            const NdStep &st = steps[i];
            if (st.op != kNdTransform) continue;
            if (!any_of(st.n)) {
                std::unique_ptr<AnyPlanner<T>> p(new (std::nothrow) AnyPlanner<T>());
                if (!p) return PHAST_ERR_ALLOC;
                rc = p->init(st.n);
                if (rc) return rc;
                axis_pl.push_back(std::move(p));
            }
            StepPlan &sp = plan[i];
            sp.any = any_of(st.n);
            sp.eng = sp.any->inner->route_small(st.rows);
            sp.ch = sp.eng->choose(kC2C, st.rows, st.rows);
        }
        return PHAST_OK;
    }
    // Bluestein elements a complex step of `arrays` arrays needs for full speed (0: a power of two)
    size_t blue_len(size_t i, size_t arrays) const {
        const NdStep &st = steps[i];
        return (st.op == kNdTransform && !plan[i].any->pow2()) ? 2 * plan[i].any->m * st.rows * arrays : 0;
    }
    size_t blue_min(size_t i) const {
        const NdStep &st = steps[i];
        return (st.op == kNdTransform && !plan[i].any->pow2()) ? 2 * plan[i].any->m : 0;
    }
    std::string shape_text() const {
        std::string s = "[";
        for (size_t i = 0; i < rank; ++i) s += (i ? "x" : "") + std::to_string(dims[i]);
        s += "] squeezed [";
        for (size_t i = 0; i < q; ++i) s += (i ? "x" : "") + std::to_string(sq[i]);
        return s + "]";
    }
    std::string route_text(const AnyPlanner<T> *a) const {
        return a->pow2() ? "pow2" : "bluestein M=" + std::to_string(a->m);
    }
    std::string steps_text() const {
        static const char *buf[] = {"X", "W", "W2", "R"};
        std::string s;
        for (size_t i = 0; i < ns; ++i) {
            const NdStep &st = steps[i];
            s += i ? "; " : "";
            if (st.op == kNdTranspose)
                s += "transpose " + std::to_string(st.rows) + "x" + std::to_string(st.n);
            else
                s += std::string(st.op == kNdTransform ? "fft " : st.op == kNdR2cRows ? "r2c " : "c2r ") +
                     std::to_string(st.rows) + " rows of " + std::to_string(st.n) + " (axis " + std::to_string(st.axis) + ")";
            s += std::string(" ") + buf[st.src] + "->" + buf[st.dst];
        }
        return s;
    }

    // `rows` rows of the complex transform step st (plan sp), from (i_re, i_im) to (o_re, o_im), rows n apart, scaled by
    // `scale`; `w`, `work_len`: Bluestein workspace
    int transform_rows(const StepPlan &sp, const NdStep &st, const T *i_re, const T *i_im, T *o_re, T *o_im, size_t rows,
                       double scale, T *w, size_t work_len, hipStream_t s) const {
        const size_t n = st.n;
        const Planner<T> *pl = sp.eng;
        Choice ch = sp.ch;
        const Planner<T> *base = sp.any->inner.get();
        if (pl != base && Planner<T>::capturing(s) && !pl->capture_ready(s)) {  // as Planner::exec: a cold twin in a capture
            pl = base;
            ch = base->choose(kC2C, st.rows, st.rows);
        }
        Lease L;
        int rc = pl->lease(L, s);
        if (rc) return rc;
        if (sp.any->pow2())
            return pl->exec_in(L, i_re, i_im, n, 0, o_re, o_im, n, 0, rows, scale, nullptr, nullptr, nullptr, nullptr, &ch);
        return sp.any->for_each_chunk(rows, work_len, [&](size_t r0, size_t c) {
            return sp.any->run_chunk(pl, L, ch, i_re + r0 * n, i_im + r0 * n, o_re + r0 * n, o_im + r0 * n, c, n, w, scale);
        });
    }
};

template <typename T> struct NdPlanner : NdCore<T> {
    using C = NdCore<T>;
    using C::q; using C::sq; using C::total; using C::steps; using C::ns; using C::plan; using C::device;

    int init(const size_t *d, size_t r) { return C::init_core(d, r, kNdC2C); }
    const AnyPlanner<T> *single() const { return q <= 1 ? plan[0].any : nullptr; }

    size_t workspace_len(size_t batch) const {
        if (single()) return single()->workspace_len(batch);
        size_t b = 0;
        for (size_t i = 0; i < ns; ++i) b = std::max(b, C::blue_len(i, batch));
        return 2 * (size_t)total * batch + b;
    }
    size_t min_work() const {
        if (single()) return single()->pow2() ? 0 : 2 * single()->m;
        size_t b = 0;
        for (size_t i = 0; i < ns; ++i) b = std::max(b, C::blue_min(i));
        return 2 * (size_t)total + b;
    }
    size_t device_bytes() const {
        size_t b = 0;
        for (const auto &p : C::axis_pl) b += p->device_bytes();
        return b;
    }
    std::string describe() const {
        std::string s = "nd " + C::shape_text() + " axes:";
        for (size_t i = 0; i < q; ++i) s += " " + std::to_string(sq[i]) + " " + C::route_text(C::any_of(sq[i])) + ";";
        return s + " schedule: " + C::steps_text();
    }

    int check_dev(const T *d_re, const T *d_im, size_t num, size_t batch, size_t dist, int direction, const T *d_work,
                  size_t work_len) const {
        if (!d_re || !d_im) return PHAST_ERR_INVALID_ARG;
        if (direction != PHAST_FORWARD && direction != PHAST_REVERSE) return PHAST_ERR_INVALID_ARG;
        if (num != total) return PHAST_ERR_PLANNER_SIZE;
        if (batch > 1 && dist < total) return PHAST_ERR_INVALID_ARG;
        const size_t need = min_work();
        if (need && batch && (!d_work || work_len < need)) return PHAST_ERR_INVALID_ARG;
        return PHAST_OK;
    }

    // ev: optional ns + 1 events recorded before every step and after the last (time_steps: one chunk)
    int fft_dev_nd(T *d_re, T *d_im, size_t num, size_t batch, size_t dist, int direction, T *d_work, size_t work_len,
                   hipStream_t s, hipEvent_t *ev = nullptr) const {
        int rc = check_dev(d_re, d_im, num, batch, dist, direction, d_work, work_len);
        if (rc) return rc;
        if (single()) return single()->fft_dev_any(d_re, d_im, single()->n, batch, dist, direction, d_work, work_len, s);
        if (batch == 0) return PHAST_OK;
        if (batch == 1) dist = total;
        PHAST_ON_DEVICE(device);
        const size_t tot = total, bmin = min_work() - 2 * tot;
        size_t chunk = (work_len - bmin) / (2 * tot);
        if (chunk > batch) chunk = batch;
        const bool inv = direction == PHAST_REVERSE;
        for (size_t b0 = 0; b0 < batch; b0 += chunk) {
            const size_t c = batch - b0 < chunk ? batch - b0 : chunk;
            T *x[2] = {d_re + b0 * dist, d_im + b0 * dist};
            T *w[2] = {d_work, d_work + c * tot};
            if (inv) {  // the swap trick: the forward transform of (im, re), every step scaled by 1 / n of its axis
                std::swap(x[0], x[1]);
                std::swap(w[0], w[1]);
            }
            T *blue = d_work + 2 * c * tot;
            const size_t blue_len = work_len - 2 * c * tot;
            for (size_t i = 0; i < ns; ++i) {
                const NdStep &st = steps[i];
                if (ev) PHAST_HIP(hipEventRecord(ev[i], s));
                T **src = st.src == kNdX ? x : w, **dst = st.dst == kNdX ? x : w;
                const size_t sd = st.src == kNdX ? dist : tot, dd = st.dst == kNdX ? dist : tot;
                if (st.op == kNdTranspose) {
                    PHAST_HIP(launch_nd_transpose<T>(src[0], src[1], dst[0], dst[1], c, st.rows, st.n, sd, dd, s));
                    continue;
                }
                const double scale = inv ? 1.0 / (double)st.n : 1.0;
                if (sd == tot && dd == tot) {  // the arrays' rows follow each other: one call
                    rc = C::transform_rows(plan[i], st, src[0], src[1], dst[0], dst[1], st.rows * c, scale, blue, blue_len, s);
                    if (rc) return rc;
                    continue;
                }
                for (size_t b = 0; b < c; ++b) {
                    rc = C::transform_rows(plan[i], st, src[0] + b * sd, src[1] + b * sd, dst[0] + b * dd, dst[1] + b * dd, st.rows,
                                           scale, blue, blue_len, s);
                    if (rc) return rc;
                }
            }
            if (ev) PHAST_HIP(hipEventRecord(ev[ns], s));
        }
        return PHAST_OK;
    }

    // measurement hook: average milliseconds of every step of the schedule (step_ms[0 .. ns-1], *n_steps = ns) over `reps`
    // forward calls of the batch in one chunk (two or more axes left, work_len >= workspace_len(batch)); blocks
    int time_steps(T *d_re, T *d_im, size_t batch, size_t dist, T *d_work, size_t work_len, int reps, float *step_ms,
                   size_t *n_steps, hipStream_t s) const {
        if (!step_ms || !n_steps || reps < 1 || batch == 0 || single()) return PHAST_ERR_INVALID_ARG;
        if (work_len < workspace_len(batch)) return PHAST_ERR_INVALID_ARG;
        int rc = check_dev(d_re, d_im, total, batch, dist, PHAST_FORWARD, d_work, work_len);
        if (rc) return rc;
        PHAST_ON_DEVICE(device);
        struct Events {
            hipEvent_t e[2 * kNdMaxRank + 2] = {};
            ~Events() {
                for (hipEvent_t x : e)
                    if (x) hipEventDestroy(x);
            }
        } ev;
        for (size_t i = 0; i <= ns; ++i) PHAST_HIP(hipEventCreate(&ev.e[i]));
        double acc[2 * kNdMaxRank + 1] = {};
        for (int r = 0; r < reps; ++r) {
            rc = fft_dev_nd(d_re, d_im, total, batch, dist, PHAST_FORWARD, d_work, work_len, s, ev.e);
            if (rc) return rc;
            PHAST_HIP(hipStreamSynchronize(s));
            for (size_t i = 0; i < ns; ++i) {
                float t = 0;
                PHAST_HIP(hipEventElapsedTime(&t, ev.e[i], ev.e[i + 1]));
                acc[i] += t;
            }
        }
        for (size_t i = 0; i < ns; ++i) step_ms[i] = (float)(acc[i] / reps);
        *n_steps = ns;
        return PHAST_OK;
    }

    // host slices: through a device buffer of the call's own, on the null stream; blocking
    int fft_host_nd(T *re, size_t re_len, T *im, size_t im_len, int direction) const {
        if ((!re && re_len) || (!im && im_len)) return PHAST_ERR_INVALID_ARG;
        if (direction != PHAST_FORWARD && direction != PHAST_REVERSE) return PHAST_ERR_INVALID_ARG;
        if (re_len != im_len) return PHAST_ERR_LEN_MISMATCH;
        if (re_len != total) return PHAST_ERR_PLANNER_SIZE;
        PHAST_ON_DEVICE(device);
        const size_t x_len = (total + 3) & ~(size_t)3, wl = min_work();  // every part 16-byte aligned (f32: 4 elements)
        DevBuf buf;
        int rc = buf.alloc((2 * x_len + wl) * sizeof(T));
        if (rc) return rc;
        T *d_re = reinterpret_cast<T *>(buf.p), *d_im = d_re + x_len, *d_w = d_im + x_len;
        const size_t bytes = total * sizeof(T);
        PHAST_HIP(hipMemcpy(d_re, re, bytes, hipMemcpyHostToDevice));
        PHAST_HIP(hipMemcpy(d_im, im, bytes, hipMemcpyHostToDevice));
        rc = fft_dev_nd(d_re, d_im, total, 1, total, direction, wl ? d_w : nullptr, wl, nullptr);
        if (rc) return rc;
        PHAST_HIP(hipMemcpy(re, d_re, bytes, hipMemcpyDeviceToHost));
        PHAST_HIP(hipMemcpy(im, d_im, bytes, hipMemcpyDeviceToHost));
        return PHAST_OK;
    }
};

template <typename T> struct RealNdPlanner : NdCore<T> {
    using C = NdCore<T>;
    using Lease = typename Planner<T>::Lease;
    using Choice = typename Planner<T>::Choice;
    using C::q; using C::sq; using C::total; using C::steps; using C::ns; using C::plan; using C::device;
    size_t last = 0, half = 0;        // the real axis and its n / 2 + 1 points
    unsigned long long total_cx = 0;  // points of the half spectrum
    std::unique_ptr<AnyRealPlanner<T>> real;
    // the engine plan of the real rows step (fixed at init, as the complex steps')
    const Planner<T> *r_eng = nullptr;
    const PlannerR2c<T> *r_pow2[2] = {nullptr, nullptr};  // R2C / C2R route of a power-of-two real axis
    Choice r_ch[2];

    int init(const size_t *d, size_t r) {
        int rc = C::init_core(d, r, kNdR2C);  // R2C and C2R share the planners; the C2R schedule is derived per call
        if (rc) return rc;
        last = sq[q - 1];
        half = last / 2 + 1;
        total_cx = total / last * half;
        real.reset(new (std::nothrow) AnyRealPlanner<T>());
        if (!real) return PHAST_ERR_ALLOC;
        rc = real->init(last);
        if (rc) return rc;
        c2r_ns = nd_schedule(sq, q, kNdC2R, c2r_steps);
        for (size_t i = 0; i < c2r_ns; ++i) {  // the C2R transform steps run the planners the R2C steps made
            const NdStep &st = c2r_steps[i];
            if (st.op != kNdTransform) continue;
            if (!C::any_of(st.n)) return PHAST_ERR_INVALID_ARG;  // (the same axes in another order)
            typename C::StepPlan &sp = c2r_plan[i];
            sp.any = C::any_of(st.n);
            sp.eng = sp.any->inner->route_small(st.rows);
            sp.ch = sp.eng->choose(kC2C, st.rows, st.rows);
        }
        const size_t rows = (size_t)(total / last);
        if (real->r2c) {
            for (int k = 0; k < 2; ++k) {
                r_pow2[k] = real->r2c->route_small(k == 1, rows);
                r_ch[k] = r_pow2[k]->dit.choose(k ? kC2R : kR2C, rows, rows);
            }
        } else if (real->any) {
            r_eng = real->any->inner->route_small(rows);
            r_ch[0] = r_ch[1] = r_eng->choose(kC2C, rows, rows);
        }
        return PHAST_OK;
    }
    NdStep c2r_steps[2 * kNdMaxRank + 1] = {};
    size_t c2r_ns = 0;
    typename C::StepPlan c2r_plan[2 * kNdMaxRank + 1];

    bool single() const { return q <= 1; }
    size_t real_blue(size_t rows) const { return real->any ? 2 * real->m * rows : 0; }
    // planes of half-spectrum points per array in the transposed copies: R2C runs in one copy, C2R ping-pongs between two
    static size_t copies(bool c2r) { return c2r ? 4 : 2; }
    size_t blue_need(size_t batch) const {
        size_t b = real_blue((size_t)(total / last) * batch);
        for (size_t i = 0; i < ns; ++i) b = std::max(b, C::blue_len(i, batch));
        return b;
    }
    // the length for full speed in either direction (C2R's two copies); an R2C-only caller may bring 2 half batch fewer
    size_t workspace_len(size_t batch) const {
        if (single()) return real->workspace_len(batch);
        return copies(true) * (size_t)total_cx * batch + blue_need(batch);
    }
    size_t min_work(bool c2r) const {
        if (single()) return real->any ? 2 * real->m : 0;
        size_t b = real_blue(1);
        for (size_t i = 0; i < ns; ++i) b = std::max(b, C::blue_min(i));
        return copies(c2r) * (size_t)total_cx + b;
    }
    size_t device_bytes() const {
        size_t b = real->device_bytes();
        for (const auto &p : C::axis_pl) b += p->device_bytes();
        return b;
    }
    std::string describe() const {
        std::string s = "real nd " + C::shape_text() + " axes:";
        for (size_t i = 0; i + 1 < q; ++i) s += " " + std::to_string(sq[i]) + " " + C::route_text(C::any_of(sq[i])) + ";";
        s += " real " + real->describe() + "; R2C schedule: " + C::steps_text();
        return s;
    }

    // `rows` real rows: R2C real (in_a) -> planes (out_a, out_b); C2R planes (in_a, in_b) -> real (out_a)
    int real_rows(bool c2r, const T *in_a, const T *in_b, T *out_a, T *out_b, size_t rows, T *w, size_t work_len,
                  hipStream_t s) const {
        const size_t in_dist = c2r ? half : last, out_dist = c2r ? last : half;
        if (real->tiny) return real->run_tiny(c2r, in_a, out_a, out_b, rows, in_dist, out_dist, s);
        if (const PlannerR2c<T> *p = r_pow2[c2r]) {
            Lease L;
            int rc = p->dit.lease(L, s);
            if (rc) return rc;
            return c2r ? p->c2r_in(L, in_a, in_b, out_a, rows, in_dist, out_dist, nullptr, &r_ch[1])
                       : p->r2c_in(L, in_a, out_a, out_b, rows, in_dist, out_dist, nullptr, &r_ch[0]);
        }
        const Planner<T> *pl = r_eng;
        Choice ch = r_ch[0];
        const Planner<T> *base = real->any->inner.get();
        if (pl != base && Planner<T>::capturing(s) && !pl->capture_ready(s)) {
            pl = base;
            ch = base->choose(kC2C, (size_t)(total / last), (size_t)(total / last));
        }
        Lease L;
        int rc = pl->lease(L, s);
        if (rc) return rc;
        return real->any->for_each_chunk(rows, work_len, [&](size_t r0, size_t c) {
            return real->run_chunk(c2r, pl, L, ch, in_a + r0 * in_dist, in_b ? in_b + r0 * in_dist : nullptr,
                                   out_a + r0 * out_dist, out_b ? out_b + r0 * out_dist : nullptr, c, in_dist, out_dist, w);
        });
    }

    // the checks of a _dev call: R2C in = the real arrays (dist >= prod n), out = the planes (dist >= the half spectrum);
    // C2R the reverse
    int check_dev(bool c2r, const void *a, const void *b, const void *c, size_t num, size_t batch, size_t in_dist,
                  size_t out_dist, const T *d_work, size_t work_len) const {
        if (!a || !b || !c) return PHAST_ERR_INVALID_ARG;
        if (num != total) return PHAST_ERR_PLANNER_SIZE;
        const size_t real_dist = c2r ? out_dist : in_dist, cx_dist = c2r ? in_dist : out_dist;
        if (batch > 1 && (real_dist < total || cx_dist < total_cx)) return PHAST_ERR_INVALID_ARG;
        const size_t need = min_work(c2r);
        if (need && batch && (!d_work || work_len < need)) return PHAST_ERR_INVALID_ARG;
        return PHAST_OK;
    }

    // device pointers, asynchronous on `s`.  R2C: (in_a = the real arrays; out_a, out_b = the planes); C2R: (in_a, in_b =
    // the planes; out_a = the real arrays).  Neither writes its input.
    int dev(bool c2r, const T *in_a, const T *in_b, T *out_a, T *out_b, size_t num, size_t batch, size_t in_dist,
            size_t out_dist, T *d_work, size_t work_len, hipStream_t s) const {
        int rc = c2r ? check_dev(true, in_a, in_b, out_a, num, batch, in_dist, out_dist, d_work, work_len)
                     : check_dev(false, in_a, out_a, out_b, num, batch, in_dist, out_dist, d_work, work_len);
        if (rc) return rc;
        if (single()) return real->dev(c2r, in_a, in_b, out_a, out_b, last, batch, in_dist, out_dist, d_work, work_len, s);
        if (batch == 0) return PHAST_OK;
        if (batch == 1) {
            in_dist = c2r ? total_cx : total;
            out_dist = c2r ? total : total_cx;
        }
        PHAST_ON_DEVICE(device);
        const size_t tc = total_cx, cp = copies(c2r), bmin = min_work(c2r) - cp * tc;
        size_t chunk = (work_len - bmin) / (cp * tc);
        if (chunk > batch) chunk = batch;
        const NdStep *st_all = c2r ? c2r_steps : steps;
        const typename C::StepPlan *pl_all = c2r ? c2r_plan : plan;
        const size_t n_steps = c2r ? c2r_ns : ns;
        const size_t real_dist = c2r ? out_dist : in_dist, cx_dist = c2r ? in_dist : out_dist;
        for (size_t b0 = 0; b0 < batch; b0 += chunk) {
            const size_t c = batch - b0 < chunk ? batch - b0 : chunk;
            // X: the caller's planes; W, W2: the copies; R: the caller's real arrays.  C2R runs the swap trick on the
            // complex steps: (im, re) everywhere; its real rows read (re, im) again.
            T *bufs[3][2] = {{c2r ? const_cast<T *>(in_a) + b0 * cx_dist : out_a + b0 * cx_dist,
                              c2r ? const_cast<T *>(in_b) + b0 * cx_dist : out_b + b0 * cx_dist},
                             {d_work, d_work + c * tc},
                             {d_work + 2 * c * tc, d_work + 3 * c * tc}};
            T *real_arr = c2r ? out_a + b0 * real_dist : const_cast<T *>(in_a) + b0 * real_dist;
            T *blue = d_work + cp * c * tc;  // (R2C: W2 is never used)
            const size_t blue_len = work_len - cp * c * tc;
            for (size_t i = 0; i < n_steps; ++i) {
                const NdStep &st = st_all[i];
                const size_t sd = st.src == kNdX ? cx_dist : tc, dd = st.dst == kNdX ? cx_dist : tc;
                if (st.op == kNdR2cRows || st.op == kNdC2rRows) {
                    const bool back = st.op == kNdC2rRows;
                    T **cx = bufs[back ? st.src : st.dst];
                    const size_t cd = back ? sd : dd;
                    const size_t rows = st.rows;
                    if (cd == tc && real_dist == total) {
                        rc = back ? real_rows(true, cx[0], cx[1], real_arr, nullptr, rows * c, blue, blue_len, s)
                                  : real_rows(false, real_arr, nullptr, cx[0], cx[1], rows * c, blue, blue_len, s);
                        if (rc) return rc;
                        continue;
                    }
                    for (size_t b = 0; b < c; ++b) {
                        rc = back ? real_rows(true, cx[0] + b * cd, cx[1] + b * cd, real_arr + b * real_dist, nullptr, rows,
                                              blue, blue_len, s)
                                  : real_rows(false, real_arr + b * real_dist, nullptr, cx[0] + b * cd, cx[1] + b * cd, rows,
                                              blue, blue_len, s);
                        if (rc) return rc;
                    }
                    continue;
                }
                const int ri = c2r ? 1 : 0, ii = c2r ? 0 : 1;  // C2R: (im, re)
                T **src = bufs[st.src], **dst = bufs[st.dst];
                if (st.op == kNdTranspose) {
                    PHAST_HIP(launch_nd_transpose<T>(src[ri], src[ii], dst[ri], dst[ii], c, st.rows, st.n, sd, dd, s));
                    continue;
                }
                const double scale = c2r ? 1.0 / (double)st.n : 1.0;
                const typename C::StepPlan &sp = pl_all[i];
                if (sd == tc && dd == tc) {  // the arrays' rows follow each other: one call
                    rc = C::transform_rows(sp, st, src[ri], src[ii], dst[ri], dst[ii], st.rows * c, scale, blue, blue_len, s);
                    if (rc) return rc;
                    continue;
                }
                for (size_t b = 0; b < c; ++b) {
                    rc = C::transform_rows(sp, st, src[ri] + b * sd, src[ii] + b * sd, dst[ri] + b * dd, dst[ii] + b * dd,
                                        st.rows, scale, blue, blue_len, s);
                    if (rc) return rc;
                }
            }
        }
        return PHAST_OK;
    }
    // host slices through a device buffer of the call's own, on the null stream; blocking.  R2C: (a = the real array;
    // b, c = the planes); C2R: (a, b = the planes; c = the real array)
    int host(bool c2r, const T *in_a, size_t a_len, const T *in_b, size_t b_len, T *out_a, size_t oa_len, T *out_b,
             size_t ob_len) const {
        if (!c2r) {
            if (!in_a || !out_a || !out_b) return PHAST_ERR_INVALID_ARG;
            if (a_len != total) return PHAST_ERR_R2C_INPUT_LEN;
            if (oa_len != total_cx) return PHAST_ERR_R2C_OUT_RE_LEN;
            if (ob_len != total_cx) return PHAST_ERR_R2C_OUT_IM_LEN;
        } else {
            if (!in_a || !in_b || !out_a) return PHAST_ERR_INVALID_ARG;
            if (oa_len != total) return PHAST_ERR_C2R_OUTPUT_LEN;
            if (a_len != total_cx) return PHAST_ERR_C2R_IN_RE_LEN;
            if (b_len != total_cx) return PHAST_ERR_C2R_IN_IM_LEN;
        }
        PHAST_ON_DEVICE(device);
        auto up = [](size_t k) { return (k + 3) & ~(size_t)3; };  // every part 16-byte aligned
        const size_t nr = up(total), nc = up(total_cx), wl = min_work(c2r);
        DevBuf buf;
        int rc = buf.alloc((nr + 2 * nc + wl) * sizeof(T));
        if (rc) return rc;
        T *d_real = reinterpret_cast<T *>(buf.p), *d_re = d_real + nr, *d_im = d_re + nc, *d_w = d_im + nc;
        if (!c2r) {
            PHAST_HIP(hipMemcpy(d_real, in_a, total * sizeof(T), hipMemcpyHostToDevice));
            rc = dev(false, d_real, nullptr, d_re, d_im, total, 1, total, total_cx, wl ? d_w : nullptr, wl, nullptr);
            if (rc) return rc;
            PHAST_HIP(hipMemcpy(out_a, d_re, total_cx * sizeof(T), hipMemcpyDeviceToHost));
            PHAST_HIP(hipMemcpy(out_b, d_im, total_cx * sizeof(T), hipMemcpyDeviceToHost));
        } else {
            PHAST_HIP(hipMemcpy(d_re, in_a, total_cx * sizeof(T), hipMemcpyHostToDevice));
            PHAST_HIP(hipMemcpy(d_im, in_b, total_cx * sizeof(T), hipMemcpyHostToDevice));
            rc = dev(true, d_re, d_im, d_real, nullptr, total, 1, total_cx, total, wl ? d_w : nullptr, wl, nullptr);
            if (rc) return rc;
            PHAST_HIP(hipMemcpy(out_a, d_real, total * sizeof(T), hipMemcpyDeviceToHost));
        }
        return PHAST_OK;
    }
};

// dims checked before the device is touched
template <typename P> static int nd_planner_new(const size_t *dims, size_t rank, int kind, P **out) {
    if (!out) return PHAST_ERR_INVALID_ARG;
    *out = nullptr;
    size_t sq[kNdMaxRank];
    unsigned long long total = 0;
    int bad = 1;
    (void)nd_squeeze(dims, rank, kind, sq, &total, &bad);
    if (bad) return PHAST_ERR_INVALID_ARG;
    auto *p = new (std::nothrow) P();
    if (!p) return PHAST_ERR_ALLOC;
    int rc = p->init(dims, rank);
    if (rc) {
        delete p;
        return rc;
    }
    *out = p;
    return PHAST_OK;
}

}  // namespace phast
