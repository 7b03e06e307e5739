// planner_mdct.hpp -- MdctPlanner<T>: the modified discrete cosine transform and its inverse (mdct.hpp).
// It holds one AnyPlanner<T>(h), h = N / 2, and one device buffer with the window and the DCT-IV's two twiddle tables:
// immutable after init, no per-call state.  The forward call runs, per chunk of frames, the fold-and-pre-twiddle sweep
// (mdct.hip) into the z planes of the workspace, the complex planner's own _dev transform of those rows in place, and the
// post sweep straight into the caller's coefficients; the inverse runs, per chunk of whole signals, the pre sweep of the
// caller's coefficients, the same transform, the post sweep into the workspace rows v and the overlap-add sweep.  The
// caller's workspace holds, per frame, one row of each z plane (hd >= h elements), a row v (nd >= N; the forward call leaves
// it unused) and the complex planner's workspace; hd and nd are multiples of 16 bytes, so every row starts 16-byte aligned.
#pragma once

#include <vector>

#include "mdct.hpp"
#include "planner_any.hpp"

namespace phast {

template <typename T> struct MdctPlanner {
    static constexpr size_t V = 16 / sizeof(T);
    size_t len = 0, n = 0, h = 0;  // L, N and h = N / 2
    size_t frames = 0, hd = 0, nd = 0, wd = 0;
    int padded = 0;
    double tdac_defect = 0;  // mdct_tdac_defect of the window as it was given (the sine window: before it is rounded to T)
    T *d_tab = nullptr;      // w[wd], then cos and sin of the pre twiddles and of the post twiddles, hd each (zeros beyond h)
    std::unique_ptr<AnyPlanner<T>> any;

    ~MdctPlanner() {
        if (!d_tab) return;
        DeviceGuard on(any ? any->device : -1);
        hipFree(d_tab);
    }

    // `window`: 2N host values or NULL (the sine window); the arguments were checked by mdct_bad_args
    int init(size_t signal_len, size_t num, const T *window, int padded_) {
        len = signal_len;
        n = num;
        h = n / 2;
        padded = padded_;
        frames = (size_t)mdct_frames(len, n, padded);
        hd = (h + V - 1) / V * V;
        nd = (n + V - 1) / V * V;
        wd = (2 * n + V - 1) / V * V;
        std::vector<double> w64(2 * n);
        std::vector<T> tab(wd + 4 * hd, T(0));
        for (size_t j = 0; j < n; ++j) {
            if (window) {
                w64[j] = window[j];
                w64[j + n] = window[j + n];
            } else {  // sin(pi (j + 1/2) / (2N)), symmetric
                long double c, s;
                dct4_twiddle(2 * j + 1, 4 * n, &c, &s);
                w64[j] = w64[2 * n - 1 - j] = (double)s;
            }
        }
        for (size_t j = 0; j < 2 * n; ++j) tab[j] = (T)w64[j];
        tdac_defect = mdct_tdac_defect(w64.data(), n);
        for (size_t m = 0; m < h; ++m) {
            long double c, s;
            dct4_twiddle(dct4_pre_num(m), 4 * n, &c, &s);
            tab[wd + m] = (T)c;
            tab[wd + hd + m] = (T)s;
            dct4_twiddle(dct4_post_num(m), 4 * n, &c, &s);
            tab[wd + 2 * hd + m] = (T)c;
            tab[wd + 3 * hd + m] = (T)s;
        }
        any.reset(new (std::nothrow) AnyPlanner<T>());
        if (!any) return PHAST_ERR_ALLOC;
        int rc = any->init(h);
        if (rc) return rc;
        PHAST_ON_DEVICE(any->device);
        PHAST_HIP(hipMalloc(reinterpret_cast<void **>(&d_tab), tab.size() * sizeof(T)));
        PHAST_HIP(hipMemcpy(d_tab, tab.data(), tab.size() * sizeof(T), hipMemcpyHostToDevice));
        return PHAST_OK;
    }

    // elements of T per frame, and V - 1 more to align the caller's base to 16 bytes
    size_t per() const { return 2 * hd + nd + any->workspace_len(1); }
    size_t workspace_len(size_t batch) const { return (batch ? batch : 1) * frames * per() + (V - 1); }
    size_t workspace_min(bool inverse) const { return (inverse ? frames : 1) * per() + (V - 1); }
    size_t device_bytes() const { return any->device_bytes() + (wd + 4 * hd) * sizeof(T); }
    std::string describe() const {
        return "mdct L=" + std::to_string(len) + " N=" + std::to_string(n) + (padded ? " padded" : " unpadded") + " frames=" +
               std::to_string(frames) + " around " + any->describe();
    }

    // the checks of a _dev call, before the device is touched
    int check_dev(bool inverse, const T *sig, const T *coefs, size_t signal_len, size_t batch, size_t sig_dist, const T *d_work,
                  size_t work_len) const {
        if (!sig || !coefs) return PHAST_ERR_INVALID_ARG;
        if (signal_len != len) return PHAST_ERR_PLANNER_SIZE;
        if (batch > 1 && sig_dist < len) return PHAST_ERR_INVALID_ARG;
        if (batch && (!d_work || (reinterpret_cast<uintptr_t>(d_work) % sizeof(T)) || work_len < workspace_min(inverse)))
            return PHAST_ERR_INVALID_ARG;
        return PHAST_OK;
    }

    // the caller's workspace from its first 16-byte boundary on; its length in whole frames (a launch's groups < 2^38)
    size_t rows_of(T *d_work, size_t work_len, T **w) const {
        const size_t skip = ((16 - (reinterpret_cast<uintptr_t>(d_work) & 15u)) & 15u) / sizeof(T);
        *w = d_work + skip;
        size_t rows = (work_len - skip) / per();
        const size_t cap = ((size_t)1 << 39) / per();
        return rows > cap ? cap : rows;
    }

    MdctArgs args(bool post) const {
        MdctArgs a{};
        a.win = d_tab;
        a.tw_c = d_tab + wd + (post ? 2 * hd : 0);
        a.tw_s = d_tab + wd + (post ? 3 * hd : hd);
        a.len = len;
        a.n = n;
        a.frames = frames;
        a.padded = padded;
        a.scale = 1.0;
        a.gpt = (unsigned)(hd / V);
        return a;
    }

    // Z = FFT_h(z) of `c` rows in place (h = 1: the identity)
    int transform(T *z_re, T *z_im, size_t c, T *iw, hipStream_t s) const {
        if (h == 1) return PHAST_OK;
        return any->fft_dev_any(z_re, z_im, h, c, hd, PHAST_FORWARD, iw, any->workspace_len(c), s);
    }

    // forward, device pointers, asynchronous on `s`: chunks of whole frames of the flattened (signal, frame) index.
    // ev (time_stages): 4 events around the three stages of a call that fits one chunk
    int mdct_dev(const T *sig, T *coefs, size_t signal_len, size_t batch, size_t sig_dist, T *d_work, size_t work_len,
                 hipStream_t s, hipEvent_t *ev = nullptr) const {
        int rc = check_dev(false, sig, coefs, signal_len, batch, sig_dist, d_work, work_len);
        if (rc) return rc;
        if (batch == 0) return PHAST_OK;
        if (batch == 1) sig_dist = len;
        PHAST_ON_DEVICE(any->device);
        T *w = nullptr;
        const size_t rows = rows_of(d_work, work_len, &w), total = batch * frames;
        for (size_t q0 = 0; q0 < total; q0 += rows) {
            const size_t c = total - q0 < rows ? total - q0 : rows;
            T *z_re = w, *z_im = z_re + c * hd, *iw = z_im + c * hd + c * nd;
            MdctArgs a = args(false);
            a.in = sig;
            a.in_dist = sig_dist;
            a.out = z_re;
            a.out_im = z_im;
            a.out_dist = hd;
            a.q0 = q0;
            a.groups = c * a.gpt;
            if (ev) PHAST_HIP(hipEventRecord(ev[0], s));
            PHAST_HIP(launch_mdct<T>(kMdctPre, false, a, s));
            if (ev) PHAST_HIP(hipEventRecord(ev[1], s));
            rc = transform(z_re, z_im, c, iw, s);
            if (rc) return rc;
            if (ev) PHAST_HIP(hipEventRecord(ev[2], s));
            a = args(true);
            a.in = z_re;
            a.in_im = z_im;
            a.in_dist = hd;
            a.out = coefs + q0 * n;
            a.out_dist = n;
            a.groups = c * a.gpt;
            PHAST_HIP(launch_mdct<T>(kDct4Post, true, a, s));
            if (ev) PHAST_HIP(hipEventRecord(ev[3], s));
        }
        return PHAST_OK;
    }

    // inverse, device pointers, asynchronous on `s`: chunks of whole signals (an output sample needs both its frames).
    // ev: 4 events around the pre sweep, the transform, and the post and overlap-add sweeps
    int imdct_dev(const T *coefs, T *sig, size_t signal_len, size_t batch, size_t sig_dist, T *d_work, size_t work_len,
                  hipStream_t s, hipEvent_t *ev = nullptr) const {
        int rc = check_dev(true, sig, coefs, signal_len, batch, sig_dist, d_work, work_len);
        if (rc) return rc;
        if (batch == 0) return PHAST_OK;
        if (batch == 1) sig_dist = len;
        PHAST_ON_DEVICE(any->device);
        T *w = nullptr;
        const size_t chunk = rows_of(d_work, work_len, &w) / frames;  // >= 1: work_len >= workspace_min(true)
        for (size_t b0 = 0; b0 < batch; b0 += chunk) {
            const size_t cb = batch - b0 < chunk ? batch - b0 : chunk, c = cb * frames;
            T *z_re = w, *z_im = z_re + c * hd, *v = z_im + c * hd, *iw = v + c * nd;
            MdctArgs a = args(false);
            a.in = coefs + b0 * frames * n;
            a.in_dist = n;
            a.out = z_re;
            a.out_im = z_im;
            a.out_dist = hd;
            a.groups = c * a.gpt;
            if (ev) PHAST_HIP(hipEventRecord(ev[0], s));
            PHAST_HIP(launch_mdct<T>(kDct4Pre, false, a, s));
            if (ev) PHAST_HIP(hipEventRecord(ev[1], s));
            rc = transform(z_re, z_im, c, iw, s);
            if (rc) return rc;
            if (ev) PHAST_HIP(hipEventRecord(ev[2], s));
            a = args(true);
            a.in = z_re;
            a.in_im = z_im;
            a.in_dist = hd;
            a.out = v;
            a.out_dist = nd;
            a.scale = 2.0 / (double)n;
            a.groups = c * a.gpt;
            PHAST_HIP(launch_mdct<T>(kDct4Post, false, a, s));
            a = args(false);
            a.in = v;
            a.in_dist = nd;
            a.out = sig + b0 * sig_dist;
            a.out_dist = sig_dist;
            a.gpt = (unsigned)((len + V - 1) / V);
            a.groups = cb * a.gpt;
            PHAST_HIP(launch_mdct<T>(kMdctOla, false, a, s));
            if (ev) PHAST_HIP(hipEventRecord(ev[3], s));
        }
        return PHAST_OK;
    }

    // host slices: one signal through device buffers of the call's own (signal, coefficients, the workspace of all its
    // frames) on the null stream; blocking
    int host(bool inverse, const T *in, size_t in_len, T *out, size_t out_len) const {
        const size_t pts = frames * n;
        if (!in || !out) return PHAST_ERR_INVALID_ARG;
        if ((inverse ? out_len : in_len) != len) return PHAST_ERR_PLANNER_SIZE;
        if ((inverse ? in_len : out_len) != pts) return PHAST_ERR_LEN_MISMATCH;
        PHAST_ON_DEVICE(any->device);
        auto up = [](size_t k) { return (k + 3) & ~(size_t)3; };  // every part 16-byte aligned
        const size_t ns = up(len), nc = up(pts), nw = workspace_len(1);
        DevBuf buf;
        int rc = buf.alloc((ns + nc + nw) * sizeof(T));
        if (rc) return rc;
        T *d_sig = reinterpret_cast<T *>(buf.p), *d_co = d_sig + ns, *d_w = d_co + nc;
        if (!inverse) {
            PHAST_HIP(hipMemcpy(d_sig, in, len * sizeof(T), hipMemcpyHostToDevice));
            rc = mdct_dev(d_sig, d_co, len, 1, len, d_w, nw, nullptr);
            if (rc) return rc;
            PHAST_HIP(hipMemcpy(out, d_co, pts * sizeof(T), hipMemcpyDeviceToHost));
        } else {
            PHAST_HIP(hipMemcpy(d_co, in, pts * sizeof(T), hipMemcpyHostToDevice));
            rc = imdct_dev(d_co, d_sig, len, 1, len, d_w, nw, nullptr);
            if (rc) return rc;
            PHAST_HIP(hipMemcpy(out, d_sig, len * sizeof(T), hipMemcpyDeviceToHost));
        }
        return PHAST_OK;
    }

    // measurement hook: ms[0..2] = the pre sweep, the complex transform, and the post sweep (the inverse: post and overlap-add),
    // average milliseconds over `reps` calls of `batch` signals at distance L in one chunk (work_len >= workspace_len(batch));
    // blocks
    int time_stages(bool inverse, T *sig, T *coefs, size_t batch, T *d_work, size_t work_len, int reps, float *ms,
                    hipStream_t s) const {
        if (!ms || reps < 1 || batch == 0) return PHAST_ERR_INVALID_ARG;
        int rc = check_dev(inverse, sig, coefs, len, batch, len, d_work, work_len);
        if (rc) return rc;
        if (work_len < workspace_len(batch) || batch * frames * per() > ((size_t)1 << 39)) return PHAST_ERR_INVALID_ARG;
        PHAST_ON_DEVICE(any->device);
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
            rc = inverse ? imdct_dev(coefs, sig, len, batch, len, d_work, work_len, s, ev.e)
                         : mdct_dev(sig, coefs, len, batch, len, d_work, work_len, s, ev.e);
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

template <typename T, typename P> static int mdct_planner_new(size_t signal_len, size_t n, const T *window, int padded, P **out) {
    if (!out) return PHAST_ERR_INVALID_ARG;
    *out = nullptr;
    if (mdct_bad_args(signal_len, n, padded)) return PHAST_ERR_INVALID_ARG;  // before the device is touched
    auto *p = new (std::nothrow) P();
    if (!p) return PHAST_ERR_ALLOC;
    int rc = p->init(signal_len, n, window, padded);
    if (rc) {
        delete p;
        return rc;
    }
    *out = p;
    return PHAST_OK;
}

}  // namespace phast
