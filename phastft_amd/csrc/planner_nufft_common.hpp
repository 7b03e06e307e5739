// planner_nufft_common.hpp -- what the NUFFT planners of every rank share on the host (planner_nufft.hpp, planner_nufft_nd.hpp; the
// type-3 planner takes nufft_overlap): the table of 1 / phi^, the argument check of the _dev calls and the two factories.
#pragma once

#include "nufft.hpp"
#include "planner_nufft_sort.hpp"

namespace phast {

// 1 / phi^(k) of an axis of n modes on g grid points at width w in double, rounded to T; phi^ is even in k
template <typename T> static std::vector<T> nufft_inv_table(int w, size_t n, size_t g) {
    std::vector<T> inv(n);
    const NufftQuad hat(w, g);
    for (size_t k = 0; k <= n / 2; ++k) {
        const T r = (T)(1.0 / hat((long long)k));
        if (k < (n + 1) / 2) inv[k] = r;
        if (k > 0) inv[n - k] = r;
    }
    return inv;
}

// [p, p + len) and [q, q + qlen) share an element
template <typename T> static bool nufft_overlap(const T *p, size_t len, const T *q, size_t qlen) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return p && q && a < b + qlen * sizeof(T) && b < a + len * sizeof(T);
}

// the arguments of a _dev call of `batch` transforms of ni -> no elements through a workspace of at least min_work
template <typename T>
static int nufft_check_dev(int direction, const T *d_in_re, const T *d_in_im, size_t in_dist, size_t ni, const T *d_out_re,
                           const T *d_out_im, size_t out_dist, size_t no, size_t batch, const T *d_work, size_t work_len,
                           size_t min_work) {
    if (!d_in_re || !d_out_re || !d_out_im) return PHAST_ERR_INVALID_ARG;  // d_in_im may be null: real data
    if (direction != PHAST_FORWARD && direction != PHAST_REVERSE) return PHAST_ERR_INVALID_ARG;
    if (batch > 1 && (in_dist < ni || out_dist < no)) return PHAST_ERR_INVALID_ARG;
    if (batch && (!d_work || work_len < min_work)) return PHAST_ERR_INVALID_ARG;
    if (batch) {  // the output is written while later chunks still read the input and the workspace
        const size_t in_span = (batch - 1) * (batch > 1 ? in_dist : 0) + ni, out_span = (batch - 1) * (batch > 1 ? out_dist : 0) + no;
        for (const T *o : {d_out_re, d_out_im})
            if (nufft_overlap(o, out_span, d_in_re, in_span) || nufft_overlap(o, out_span, d_in_im, in_span) ||
                nufft_overlap(o, out_span, d_work, work_len))
                return PHAST_ERR_INVALID_ARG;
        if (nufft_overlap(d_out_re, out_span, d_out_im, out_span)) return PHAST_ERR_INVALID_ARG;
        if (nufft_overlap(d_work, work_len, d_in_re, in_span) || nufft_overlap(d_work, work_len, d_in_im, in_span))
            return PHAST_ERR_INVALID_ARG;
    }
    return PHAST_OK;
}

// A planner P from host points: `bad()` is the rank's argument check (nufft*_bad_args), which runs before the device is touched;
// a...: the arguments of P::init
template <typename P, typename Bad, typename... A> static int nufft_planner_make(P **out, Bad bad, const A &...a) {
    if (!out) return PHAST_ERR_INVALID_ARG;
    *out = nullptr;
    if (bad()) return PHAST_ERR_INVALID_ARG;
    auto *p = new (std::nothrow) P();
    if (!p) return PHAST_ERR_ALLOC;
    int rc = p->init(a...);
    if (rc) {
        delete p;
        return rc;
    }
    *out = p;
    return PHAST_OK;
}

// the same from M doubles per coordinate in device memory, ordered after the earlier work of `s` (bad: nufft*_bad_sizes); a...,
// s: the arguments of P::init_dev
template <typename P, typename Bad, typename... A> static int nufft_planner_make_dev(P **out, Bad bad, hipStream_t s, const A &...a) {
    if (!out) return PHAST_ERR_INVALID_ARG;
    *out = nullptr;
    if (bad()) return PHAST_ERR_INVALID_ARG;
    if (nufft_sort_stream_busy(s)) return PHAST_ERR_INVALID_ARG;
    auto *p = new (std::nothrow) P();
    if (!p) return PHAST_ERR_ALLOC;
    int rc = p->init_dev(a..., s);
    if (rc) {
        delete p;
        return rc;
    }
    *out = p;
    return PHAST_OK;
}

}  // namespace phast
