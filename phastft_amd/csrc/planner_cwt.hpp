// planner_cwt.hpp -- CwtPlanner<T>: the continuous wavelet transform and the analytic signal (cwt.hpp).
// It holds L, P, the family, its parameter and the norm, the device tables (S scales s_j and S gains g_j = c_j times the
// family's constant, built on the host in double), whether the input is real or complex (a planner property, as on the
// channelizer), one forward planner of P -- the real one for real input, the complex one for complex input -- and one complex
// planner of P for the rows: immutable after init, no per-call state.
//
// The rows of a call are the (signal, scale) pairs in signal-major order.  Per chunk of whole rows:
//     forward   the signals the chunk touches into the workspace planes X (real input: R2C of the caller's signal, or of its
//               zero-extended copy when P > L; complex input: a zero-filling copy into X and the transform in place there)
//     bank      Y[row, k] = X[signal, k] conj(c_j psi0^(s_j w_k)), k < P, into the rows
//     inverse   the batched inverse transform in place in the rows
//     crop      when P > L: the first L of each row into the caller's planes
// When P = L the rows are the caller's output planes and no crop runs: a power-of-two P then needs workspace for X only.  When
// P > L the rows live in the workspace.  A row never straddles two chunks and every element of it is a function of its own
// signal and scale, so chunking does not show in the bits.  workspace_len(batch) holds the whole call in one chunk,
// workspace_min() one signal's X and one row; any length in between runs the largest chunk of rows that fits.
// The engine's distance rules are inherited: a batched power-of-two R2C (P >= 4) reads an even signal distance, so real input
// with P = L a power of two, batch > 1 and an odd sig_dist is refused (P > L reads the planner's own rows).
#pragma once

#include <vector>

#include "cwt.hpp"
#include "planner_any_real.hpp"

namespace phast {

template <typename T> struct CwtPlanner {
    static constexpr size_t V = 16 / sizeof(T);
    size_t l = 0, p = 0, s = 0;
    int family = 0, norm = 0, real_input = 0;
    double param = 0;
    CwtGeom geom{};
    int device = -1;
    double *d_tab = nullptr;                  // s scales, then s gains
    std::unique_ptr<AnyRealPlanner<T>> real;  // forward, real input
    std::unique_ptr<AnyPlanner<T>> cplx;      // forward, complex input, P > 1
    std::unique_ptr<AnyPlanner<T>> inv;       // the rows, P > 1

    ~CwtPlanner() {
        if (!d_tab) return;
        DeviceGuard on(device);
        hipFree(d_tab);
    }

    // `scales`: S host values; the arguments were checked by cwt_bad_args and cwt_bad_scale
    int init(size_t signal_len, size_t pad_len, const double *scales, size_t num_scales, int family_, double param_, int norm_,
             int real_) {
        l = signal_len;
        p = pad_len;
        s = num_scales;
        family = family_;
        param = family == kCwtStep ? 0.0 : param_;
        norm = norm_;
        real_input = real_ ? 1 : 0;
        geom = cwt_geom(p, s, real_input, sizeof(T));
        std::vector<double> tab(2 * s);
        for (size_t j = 0; j < s; ++j) {
            tab[j] = scales[j];
            tab[s + j] = cwt_gain(family, param, norm, scales[j]);
        }
        int rc = ensure_device(&device);
        if (rc) return rc;
        if (real_input) {
            real.reset(new (std::nothrow) AnyRealPlanner<T>());
            if (!real) return PHAST_ERR_ALLOC;
            if ((rc = real->init(p))) return rc;
        } else if (p > 1) {  // the transform of one point is the point
            cplx.reset(new (std::nothrow) AnyPlanner<T>());
            if (!cplx) return PHAST_ERR_ALLOC;
            if ((rc = cplx->init(p))) return rc;
        }
        if (p > 1) {
            inv.reset(new (std::nothrow) AnyPlanner<T>());
            if (!inv) return PHAST_ERR_ALLOC;
            if ((rc = inv->init(p))) return rc;
        }
        PHAST_ON_DEVICE(device);
        PHAST_HIP(hipMalloc(reinterpret_cast<void **>(&d_tab), tab.size() * sizeof(double)));
        PHAST_HIP(hipMemcpy(d_tab, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice));
        return PHAST_OK;
    }

    bool padded() const { return p > l; }
    size_t pd() const { return real_input && padded() ? geom.rd : 0; }  // the zero-extended copy of a real signal
    size_t fwd_ws(size_t n) const { return real ? real->workspace_len(n) : cplx ? cplx->workspace_len(n) : 0; }
    size_t inv_ws(size_t n) const { return inv ? inv->workspace_len(n) : 0; }
    // elements of T per signal a chunk touches, and per row
    size_t sig_per() const { return 2 * geom.xd + pd() + fwd_ws(1); }
    size_t row_per() const { return (padded() ? 2 * geom.rd : 0) + inv_ws(1); }
    size_t need(size_t rows, size_t batch) const { return (size_t)cwt_need(rows, s, batch, sig_per(), row_per(), V); }
    size_t workspace_len(size_t batch) const { return need((batch ? batch : 1) * s, batch ? batch : 1); }
    size_t workspace_min() const { return need(1, 1); }
    size_t device_bytes() const {
        return 2 * s * sizeof(double) + (real ? real->device_bytes() : 0) + (cplx ? cplx->device_bytes() : 0) +
               (inv ? inv->device_bytes() : 0);
    }
    static const char *family_name(int f) { return f == kCwtMorlet ? "morlet" : f == kCwtPaul ? "paul" : f == kCwtDog ? "dog" : "step"; }
    std::string describe() const {
        std::string fam = family_name(family);
        if (family == kCwtMorlet) fam += "(w0=" + std::to_string(param) + ")";
        if (family == kCwtPaul || family == kCwtDog) fam += "(m=" + std::to_string((int)param) + ")";
        return std::string("cwt ") + fam + (family == kCwtStep ? "" : norm == kCwtL2 ? " l2" : " peak") + (real_input ? " real" : " complex") +
               " L=" + std::to_string(l) + " P=" + std::to_string(p) + " S=" + std::to_string(s) + ": bank tile=" +
               std::to_string(geom.tile) + " bins x " + std::to_string(geom.group) + " scales (no LDS), rows " +
               (padded() ? "in the workspace, cropped" : "in the output planes") + ", chunks of whole rows (" + std::to_string(s) +
               " per signal; one row at workspace_min=" + std::to_string(workspace_min()) + ", all at workspace_len) forward " +
               (real ? real->describe() : cplx ? cplx->describe() : std::string("one point")) + " inverse " +
               (inv ? inv->describe() : std::string("one point"));
    }

    // the checks of a _dev call, before the device is touched
    int check_dev(const T *x_re, const T *x_im, const T *o_re, const T *o_im, size_t signal_len, size_t batch, size_t sig_dist,
                  size_t out_dist, const T *d_work, size_t work_len) const {
        if (!x_re || !o_re || !o_im) return PHAST_ERR_INVALID_ARG;
        if (real_input ? x_im != nullptr : x_im == nullptr) return PHAST_ERR_INVALID_ARG;
        if (signal_len != l) return PHAST_ERR_PLANNER_SIZE;
        if (batch > 1 && (sig_dist < l || out_dist < s * l)) return PHAST_ERR_INVALID_ARG;
        if (batch > ((size_t)1 << 40) / (s * p)) return PHAST_ERR_INVALID_ARG;
        if (x_re == o_re || x_re == o_im || x_im == o_re || x_im == o_im || o_re == o_im || x_re == x_im)
            return PHAST_ERR_INVALID_ARG;  // the forward transform reads the signal while rows are written
        if (real_input && !padded() && batch > 1 && p >= 4 && is_pow2(p) && (sig_dist & 1))
            return PHAST_ERR_INVALID_ARG;  // the engine's batched power-of-two R2C reads (even, odd) pairs
        if (batch && (!d_work || (reinterpret_cast<uintptr_t>(d_work) % sizeof(T)) || work_len < workspace_min()))
            return PHAST_ERR_INVALID_ARG;
        return PHAST_OK;
    }

    // the caller's workspace from its first 16-byte boundary on
    static size_t align_work(T *d_work, size_t work_len, T **w) {
        const size_t skip = ((16 - (reinterpret_cast<uintptr_t>(d_work) & 15u)) & 15u) / sizeof(T);
        *w = d_work + skip;
        return work_len - skip;
    }

    // device pointers, asynchronous on `st`: signal b at x_re (x_im) + b sig_dist, row (b, j) at o_re (o_im) + b out_dist + j L.
    // ev (time_stages): 5 events around the forward transform (with its copy), the bank, the inverse and the crop of a call
    // that fits one chunk
    int dev(const T *x_re, const T *x_im, T *o_re, T *o_im, size_t signal_len, size_t batch, size_t sig_dist, size_t out_dist,
            T *d_work, size_t work_len, hipStream_t st, hipEvent_t *ev = nullptr) const {
        int rc = check_dev(x_re, x_im, o_re, o_im, signal_len, batch, sig_dist, out_dist, d_work, work_len);
        if (rc) return rc;
        if (batch == 0) return PHAST_OK;
        if (batch == 1) {
            sig_dist = l;
            out_dist = s * l;
        }
        PHAST_ON_DEVICE(device);
        T *w = nullptr;
        const size_t wl = align_work(d_work, work_len, &w) + (V - 1);  // need() counts the way to the boundary
        const size_t total = batch * s;
        const size_t chunk = (size_t)cwt_rows_per_chunk(wl, total, s, batch, sig_per(), row_per(), V);  // >= 1: work_len >= workspace_min()
        const size_t xd = geom.xd, rd = geom.rd;
        for (size_t row0 = 0; row0 < total; row0 += chunk) {
            const size_t r = total - row0 < chunk ? total - row0 : chunk;
            const size_t b0 = (size_t)cwt_first_signal(row0, s), ns = (size_t)cwt_signals(row0, r, s);
            T *xr = w, *xi = xr + ns * xd, *next = xi + ns * xd;
            if (ev) PHAST_HIP(hipEventRecord(ev[0], st));
            // forward
            if (real_input) {
                const T *in = x_re + b0 * sig_dist;
                size_t in_dist = sig_dist;
                if (padded()) {
                    T *rows = next;
                    next += ns * pd();
                    CwtCopyArgs ca{};
                    ca.in[0] = x_re;
                    ca.out[0] = rows;
                    ca.n_in = l;
                    ca.n_out = p;
                    ca.s = 1;
                    ca.row0 = b0;
                    ca.rows = ns;
                    ca.in_sig = sig_dist;
                    ca.out_sig = pd();
                    ca.out_off = b0 * pd();
                    ca.groups = ns * p;
                    PHAST_HIP(launch_cwt_copy<T>(ca, st));
                    in = rows;
                    in_dist = pd();
                }
                T *fw = next;
                next += fwd_ws(ns);
                if ((rc = real->dev(false, in, nullptr, xr, xi, p, ns, in_dist, xd, fw, fwd_ws(ns), st))) return rc;
            } else {
                CwtCopyArgs ca{};
                ca.in[0] = x_re;
                ca.in[1] = x_im;
                ca.out[0] = xr;
                ca.out[1] = xi;
                ca.n_in = l;
                ca.n_out = p;
                ca.s = 1;
                ca.row0 = b0;
                ca.rows = ns;
                ca.in_sig = sig_dist;
                ca.out_sig = xd;
                ca.out_off = b0 * xd;
                ca.groups = 2 * ns * p;
                PHAST_HIP(launch_cwt_copy<T>(ca, st));
                T *fw = next;
                next += fwd_ws(ns);
                if (cplx && (rc = cplx->fft_dev_any(xr, xi, p, ns, xd, PHAST_FORWARD, fw, fwd_ws(ns), st))) return rc;
            }
            if (ev) PHAST_HIP(hipEventRecord(ev[1], st));
            // bank
            T *rr = nullptr, *ri = nullptr;
            if (padded()) {
                rr = next;
                ri = rr + r * rd;
                next = ri + r * rd;
            }
            CwtArgs a{};
            a.x[0] = xr;
            a.x[1] = xi;
            a.out[0] = padded() ? rr : o_re;
            a.out[1] = padded() ? ri : o_im;
            a.scales = d_tab;
            a.gains = d_tab + s;
            a.xd = xd;
            a.out_sig = padded() ? s * rd : out_dist;
            a.out_row = padded() ? rd : l;
            a.out_off = padded() ? row0 * rd : 0;
            a.p = p;
            a.s = s;
            a.row0 = row0;
            a.rows = r;
            a.sig0 = b0;
            a.tiles = geom.tiles;
            a.ngrp = geom.ngrp;
            a.grp0 = cwt_first_group(row0, s, geom.ngrp);
            a.groups = geom.tiles * cwt_groups(row0, r, s, geom.ngrp) * 256;
            a.param = param;
            a.family = family;
            a.real_input = real_input;
            PHAST_HIP(launch_cwt_bank<T>(a, st));
            if (ev) PHAST_HIP(hipEventRecord(ev[2], st));
            // inverse, in place in the rows
            if (inv) {
                T *iw = next;
                if (padded()) {
                    if ((rc = inv->fft_dev_any(rr, ri, p, r, rd, PHAST_REVERSE, iw, inv_ws(r), st))) return rc;
                } else if (out_dist == s * l) {
                    if ((rc = inv->fft_dev_any(o_re + row0 * l, o_im + row0 * l, p, r, l, PHAST_REVERSE, iw, inv_ws(r), st))) return rc;
                } else {  // the rows of one signal are L apart, the signals are not S L apart: one call per signal
                    for (size_t b = b0; b < b0 + ns; ++b) {
                        const size_t j0 = b == b0 ? row0 - b * s : 0, j1 = (b + 1) * s < row0 + r ? s : row0 + r - b * s;
                        const size_t at = b * out_dist + j0 * l;
                        if ((rc = inv->fft_dev_any(o_re + at, o_im + at, p, j1 - j0, l, PHAST_REVERSE, iw, inv_ws(j1 - j0), st))) return rc;
                    }
                }
            }
            if (ev) PHAST_HIP(hipEventRecord(ev[3], st));
            // crop
            if (padded()) {
                CwtCopyArgs ca{};
                ca.in[0] = rr;
                ca.in[1] = ri;
                ca.out[0] = o_re;
                ca.out[1] = o_im;
                ca.n_in = ca.n_out = l;
                ca.s = s;
                ca.row0 = row0;
                ca.rows = r;
                ca.in_sig = s * rd;
                ca.in_row = rd;
                ca.in_off = row0 * rd;
                ca.out_sig = out_dist;
                ca.out_row = l;
                ca.groups = 2 * r * l;
                PHAST_HIP(launch_cwt_copy<T>(ca, st));
            }
            if (ev) PHAST_HIP(hipEventRecord(ev[4], st));
        }
        return PHAST_OK;
    }

    // host slices: one signal through device buffers of the call's own on the null stream; blocking
    int host(const T *x_re, const T *x_im, size_t x_len, T *o_re, T *o_im, size_t o_len) const {
        if (!x_re || !o_re || !o_im || (real_input ? x_im != nullptr : x_im == nullptr)) return PHAST_ERR_INVALID_ARG;
        if (x_len != l) return PHAST_ERR_PLANNER_SIZE;
        if (o_len != s * l) return PHAST_ERR_LEN_MISMATCH;
        PHAST_ON_DEVICE(device);
        auto up = [](size_t n) { return (n + 3) & ~(size_t)3; };  // every part 16-byte aligned
        const size_t nx = up(l), no = up(s * l), nw = workspace_len(1);
        DevBuf buf;
        int rc = buf.alloc((2 * nx + 2 * no + nw + 4) * sizeof(T));
        if (rc) return rc;
        T *d_xr = reinterpret_cast<T *>(buf.p), *d_xi = d_xr + nx, *d_or = d_xi + nx, *d_oi = d_or + no, *d_w = d_oi + no;
        PHAST_HIP(hipMemcpy(d_xr, x_re, l * sizeof(T), hipMemcpyHostToDevice));
        if (x_im) PHAST_HIP(hipMemcpy(d_xi, x_im, l * sizeof(T), hipMemcpyHostToDevice));
        rc = dev(d_xr, x_im ? d_xi : nullptr, d_or, d_oi, l, 1, l, s * l, d_w, nw, nullptr);
        if (rc) return rc;
        PHAST_HIP(hipMemcpy(o_re, d_or, s * l * sizeof(T), hipMemcpyDeviceToHost));
        PHAST_HIP(hipMemcpy(o_im, d_oi, s * l * sizeof(T), hipMemcpyDeviceToHost));
        return PHAST_OK;
    }

    // measurement hook: ms[0..3] = the forward transform (with its copy), the bank, the inverse and the crop, average
    // milliseconds over `reps` calls of `batch` signals at distances L and S L in one chunk (work_len >= workspace_len(batch)); blocks
    int time_stages(const T *x_re, const T *x_im, T *o_re, T *o_im, size_t batch, T *d_work, size_t work_len, int reps, float *ms,
                    hipStream_t st) const {
        if (!ms || reps < 1 || batch == 0) return PHAST_ERR_INVALID_ARG;
        int rc = check_dev(x_re, x_im, o_re, o_im, l, batch, l, s * l, d_work, work_len);
        if (rc) return rc;
        if (work_len < workspace_len(batch)) return PHAST_ERR_INVALID_ARG;
        PHAST_ON_DEVICE(device);
        struct Events {
            hipEvent_t e[5] = {};
            ~Events() {
                for (hipEvent_t x : e)
                    if (x) hipEventDestroy(x);
            }
        } ev;
        for (hipEvent_t &x : ev.e) PHAST_HIP(hipEventCreate(&x));
        double acc[4] = {0, 0, 0, 0};
        for (int i = 0; i < reps; ++i) {
            if ((rc = dev(x_re, x_im, o_re, o_im, l, batch, l, s * l, d_work, work_len, st, ev.e))) return rc;
            PHAST_HIP(hipStreamSynchronize(st));
            for (int k = 0; k < 4; ++k) {
                float v = 0;
                PHAST_HIP(hipEventElapsedTime(&v, ev.e[k], ev.e[k + 1]));
                acc[k] += v;
            }
        }
        for (int k = 0; k < 4; ++k) ms[k] = (float)(acc[k] / reps);
        return PHAST_OK;
    }
};

template <typename T, typename P>
static int cwt_planner_new(size_t signal_len, size_t pad_len, const double *scales, size_t num_scales, int family, double param,
                           int norm, int real_input, P **out) {
    if (!out) return PHAST_ERR_INVALID_ARG;
    *out = nullptr;
    if (pad_len == 0) pad_len = signal_len;
    if (!scales || cwt_bad_args(signal_len, pad_len, num_scales, family, param, norm))  // before the device is touched
        return PHAST_ERR_INVALID_ARG;
    for (size_t j = 0; j < num_scales; ++j)
        if (cwt_bad_scale(scales[j])) return PHAST_ERR_INVALID_ARG;
    auto *p = new (std::nothrow) P();
    if (!p) return PHAST_ERR_ALLOC;
    int rc = p->init(signal_len, pad_len, scales, num_scales, family, param, norm, real_input);
    if (rc) {
        delete p;
        return rc;
    }
    *out = p;
    return PHAST_OK;
}

}  // namespace phast
