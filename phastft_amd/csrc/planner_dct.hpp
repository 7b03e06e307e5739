// planner_dct.hpp -- DctPlanner<T>: DCT / DST of types II and III, any length N (dct.hpp).
// It holds one AnyRealPlanner<T>(N) and nothing else: immutable after init, no per-call state.  A call runs, per chunk of
// transforms, a pre sweep (dct.hip), the real planner's own R2C (type II) or C2R (type III) on the workspace and a post
// sweep.  The caller's workspace holds, per transform, v (the real signal, vd >= N elements), V (the half spectrum, re and
// im planes of cd >= N/2 + 1) and the real planner's workspace; vd and cd are multiples of 16 bytes, so v's distance is even
// (the power-of-two R2C / C2R needs that) and every workspace row starts 16-byte aligned.
#pragma once

#include "dct.hpp"
#include "planner_any_real.hpp"

namespace phast {

template <typename T> struct DctPlanner {
    static constexpr size_t L = 16 / sizeof(T);
    size_t n = 0, half = 0;  // N and h = floor(N / 2)
    size_t vd = 0, cd = 0;   // the workspace distances of v and of V's planes
    std::unique_ptr<AnyRealPlanner<T>> real;

    int init(size_t num_points) {
        if (num_points == 0 || num_points > kAnyMaxN) return PHAST_ERR_INVALID_ARG;
        n = num_points;
        half = n / 2;
        vd = (n + L - 1) / L * L;
        cd = (half + 1 + L - 1) / L * L;
        real.reset(new (std::nothrow) AnyRealPlanner<T>());
        if (!real) return PHAST_ERR_ALLOC;
        return real->init(n);
    }

    // elements of T per transform, and L - 1 more to align the caller's base to 16 bytes
    size_t per() const { return vd + 2 * cd + real->workspace_len(1); }
    size_t workspace_len(size_t batch) const { return (batch ? batch : 1) * per() + (L - 1); }
    size_t device_bytes() const { return real->device_bytes(); }
    std::string describe() const { return "dct/dst II/III N=" + std::to_string(n) + " around " + real->describe(); }

    static bool valid(int type, int norm) { return (type == 2 || type == 3) && norm >= kDctBackward && norm <= kDctForward; }

    // `c` transforms of a chunk through the aligned workspace w: pre sweep, inner(c2r, in_a, in_b, out_a, out_b, c, in_dist,
    // out_dist, work, work_len) -- the real planner's transform -- and post sweep.  ev: optional 4 events around the 3 stages
    template <typename F>
    int run_chunk(int type, bool dst, int norm, const T *in, T *out, size_t c, size_t in_dist, size_t out_dist, T *w,
                  hipStream_t s, F &&inner, hipEvent_t *ev = nullptr) const {
        auto al = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; };
        T *v = w, *c_re = v + c * vd, *c_im = c_re + c * cd, *iw = c_im + c * cd;
        const size_t iw_len = real->workspace_len(c);
        const bool vec_in = al(in) && (c == 1 || in_dist % L == 0), vec_out = al(out) && (c == 1 || out_dist % L == 0);
        DctArgs a{};
        a.n = n;
        a.scale = dct_scale(type, norm, n);
        a.scale0 = dct_scale0(type, norm, n);
        const unsigned gpt_perm = (unsigned)(((n + 1) / 2 + L - 1) / L), gpt_half = (unsigned)((half + 1 + L - 1) / L);
        if (ev) PHAST_HIP(hipEventRecord(ev[0], s));
        int rc;
        if (type == 2) {
            a.in = in;
            a.in_dist = in_dist;
            a.out = v;
            a.out_dist = vd;
            a.gpt = gpt_perm;
            a.groups = c * a.gpt;
            PHAST_HIP(launch_dct<T>(kDct2Pre, dst, vec_in, a, s));
            if (ev) PHAST_HIP(hipEventRecord(ev[1], s));
            rc = inner(false, v, nullptr, c_re, c_im, c, vd, cd, iw, iw_len);
            if (rc) return rc;
            if (ev) PHAST_HIP(hipEventRecord(ev[2], s));
            a.in = c_re;
            a.in_im = c_im;
            a.in_dist = cd;
            a.out = out;
            a.out_dist = out_dist;
            a.gpt = gpt_half;
            a.groups = c * a.gpt;
            PHAST_HIP(launch_dct<T>(kDct2Post, dst, vec_out, a, s));
        } else {
            a.in = in;
            a.in_dist = in_dist;
            a.out = c_re;
            a.out_im = c_im;
            a.out_dist = cd;
            a.gpt = gpt_half;
            a.groups = c * a.gpt;
            PHAST_HIP(launch_dct<T>(kDct3Pre, dst, vec_in, a, s));
            if (ev) PHAST_HIP(hipEventRecord(ev[1], s));
            rc = inner(true, c_re, c_im, v, nullptr, c, cd, vd, iw, iw_len);
            if (rc) return rc;
            if (ev) PHAST_HIP(hipEventRecord(ev[2], s));
            a.in = v;
            a.in_dist = vd;
            a.out = out;
            a.out_dist = out_dist;
            a.gpt = gpt_perm;
            a.groups = c * a.gpt;
            PHAST_HIP(launch_dct<T>(kDct3Post, dst, vec_out, a, s));
        }
        if (ev) PHAST_HIP(hipEventRecord(ev[3], s));
        return PHAST_OK;
    }

    // the checks of a _dev call, before the device is touched
    int check_dev(int type, int norm, const T *in, const T *out, size_t num, size_t batch, size_t in_dist, size_t out_dist,
                  const T *d_work, size_t work_len) const {
        if (!in || !out || !valid(type, norm)) return PHAST_ERR_INVALID_ARG;
        if (num != n) return PHAST_ERR_PLANNER_SIZE;
        if (batch > 1 && (in_dist < n || out_dist < n || (in == out && in_dist != out_dist))) return PHAST_ERR_INVALID_ARG;
        if (batch && (!d_work || (reinterpret_cast<uintptr_t>(d_work) % sizeof(T)) || work_len < workspace_len(1)))
            return PHAST_ERR_INVALID_ARG;
        return PHAST_OK;
    }

    // the caller's workspace from its first 16-byte boundary on; its length in whole transforms (a launch's groups < 2^38)
    size_t chunk_of(T *d_work, size_t work_len, T **w) const {
        const size_t skip = ((16 - (reinterpret_cast<uintptr_t>(d_work) & 15u)) & 15u) / sizeof(T);
        *w = d_work + skip;
        size_t chunk = (work_len - skip) / per();
        const size_t cap = ((size_t)1 << 39) / per();
        return chunk > cap ? cap : chunk;
    }

    // device pointers, asynchronous on `s`; ev (time_stages) needs a batch that fits one chunk
    int dev(int type, bool dst, const T *in, T *out, size_t num, size_t batch, size_t in_dist, size_t out_dist, int norm,
            T *d_work, size_t work_len, hipStream_t s, hipEvent_t *ev = nullptr) const {
        int rc = check_dev(type, norm, in, out, num, batch, in_dist, out_dist, d_work, work_len);
        if (rc) return rc;
        if (batch == 0) return PHAST_OK;
        if (batch == 1) in_dist = out_dist = n;
        PHAST_ON_DEVICE(real->device);
        T *w = nullptr;
        const size_t chunk = chunk_of(d_work, work_len, &w);
        auto inner = [&](bool c2r, const T *ia, const T *ib, T *oa, T *ob, size_t c, size_t id, size_t od, T *iw, size_t il) {
            return real->dev(c2r, ia, ib, oa, ob, n, c, id, od, iw, il, s);
        };
        for (size_t b0 = 0; b0 < batch; b0 += chunk) {
            const size_t c = batch - b0 < chunk ? batch - b0 : chunk;
            rc = run_chunk(type, dst, norm, in + b0 * in_dist, out + b0 * out_dist, c, in_dist, out_dist, w, s, inner, ev);
            if (rc) return rc;
        }
        return PHAST_OK;
    }

    // host slices: one transform staged through the staging buffer of a workspace of the real planner's pool, on that
    // workspace's own stream, with the real transform run on that same lease (as AnyRealPlanner::host); blocking
    int host(int type, bool dst, const T *in, size_t in_len, T *out, size_t out_len, int norm) const {
        if (!in || !out || !valid(type, norm)) return PHAST_ERR_INVALID_ARG;
        if (in_len != out_len) return PHAST_ERR_LEN_MISMATCH;
        if (in_len != n) return PHAST_ERR_PLANNER_SIZE;
        const PlannerR2c<T> *rp = real->r2c ? real->r2c.get() : nullptr;
        const bool c2r = type == 3;
        const Planner<T> *pl;
        if (rp) {
            rp = rp->route_small(c2r);
            pl = &rp->dit;
        } else {
            pl = real->tiny ? real->tiny.get() : real->any->inner->route_small(1);
        }
        PHAST_ON_DEVICE(real->device);
        typename Planner<T>::Lease L;
        int rc = pl->check_out(L, nullptr, 1);
        if (rc) return rc;
        const size_t nr = (n + 3) & ~(size_t)3;  // 16-byte aligned parts for either T
        void *stage = nullptr;
        rc = pl->stage(L, (2 * nr + per()) * sizeof(T), &stage);
        if (rc) return rc;
        T *d_in = reinterpret_cast<T *>(stage), *d_out = d_in + nr, *d_w = d_out + nr;
        auto inner = [&](bool c2, const T *ia, const T *ib, T *oa, T *ob, size_t, size_t, size_t, T *iw, size_t il) {
            if (rp) return c2 ? rp->c2r_in(L, ia, ib, oa, 1, half + 1, n) : rp->r2c_in(L, ia, oa, ob, 1, n, half + 1);
            if (real->tiny) return real->run_tiny(c2, ia, oa, ob, 1, c2 ? half + 1 : n, c2 ? n : half + 1, L.stream);
            return real->run(c2, pl, L, ia, ib, oa, ob, 1, c2 ? half + 1 : n, c2 ? n : half + 1, iw, il);
        };
        PHAST_HIP(hipMemcpyAsync(d_in, in, n * sizeof(T), hipMemcpyHostToDevice, L.stream));
        rc = run_chunk(type, dst, norm, d_in, d_out, 1, n, n, d_w, L.stream, inner);
        if (rc) return rc;
        PHAST_HIP(hipMemcpyAsync(out, d_out, n * sizeof(T), hipMemcpyDeviceToHost, L.stream));
        PHAST_HIP(hipStreamSynchronize(L.stream));
        return PHAST_OK;
    }

    // measurement hook: average milliseconds of the pre sweep, the real transform and the post sweep of `type` over `reps`
    // calls of `batch` transforms at distance N in one chunk (work_len >= workspace_len(batch)); blocks
    int time_stages(int type, bool dst, int norm, const T *in, T *out, size_t batch, T *d_work, size_t work_len, int reps,
                    float *ms, hipStream_t s) const {
        if (!ms || reps < 1 || batch == 0) return PHAST_ERR_INVALID_ARG;
        int rc = check_dev(type, norm, in, out, n, batch, n, n, d_work, work_len);
        if (rc) return rc;
        if (work_len < workspace_len(batch)) return PHAST_ERR_INVALID_ARG;
        PHAST_ON_DEVICE(real->device);
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
            rc = dev(type, dst, in, out, n, batch, n, n, norm, d_work, work_len, s, ev.e);
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

}  // namespace phast
