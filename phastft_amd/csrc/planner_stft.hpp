// planner_stft.hpp -- StftPlanner<T>: the short-time Fourier transform and its inverse (stft.hpp).
// It holds one AnyRealPlanner<T>(F), the device copy of the window and the minimum of the window envelope: immutable after
// init, no per-call state.  The forward call runs, per chunk of frames, the frame sweep (stft.hip) into workspace rows and
// the real planner's own R2C of those rows straight into the caller's planes; the inverse runs, per chunk of whole signals,
// the real planner's C2R of the caller's planes into workspace rows and the overlap-add sweep.  The caller's workspace holds,
// per frame, a row of fd >= F elements (F rounded up to 16 bytes: even, as the power-of-two R2C / C2R needs, and every row
// 16-byte aligned) and the real planner's workspace.
#pragma once

#include "planner_any_real.hpp"
#include "stft.hpp"

namespace phast {

template <typename T> struct StftPlanner {
    static constexpr size_t V = 16 / sizeof(T);
    static constexpr double kNolaMin = 1e-11;  // torch.istft's threshold on the window envelope
    size_t len = 0, f = 0, h = 0, p = 0;  // L, F, H and the padding on either side
    size_t frames = 0, bins = 0, fd = 0;
    int center = 0, pad = 0;
    double env_min = 0;  // min over the samples some frame holds of sum_f w^2
    T *d_win = nullptr;  // fd elements: w, then zeros
    std::unique_ptr<AnyRealPlanner<T>> real;

    ~StftPlanner() {
        if (!d_win) return;
        DeviceGuard on(real ? real->device : -1);
        hipFree(d_win);
    }

    // `window`: F host values or NULL (all ones); the arguments were checked by stft_bad_args
    int init(size_t signal_len, size_t n_fft, size_t hop, const T *window, int center_, int pad_mode) {
        len = signal_len;
        f = n_fft;
        h = hop;
        center = center_;
        pad = pad_mode;
        p = center ? f / 2 : 0;
        frames = (size_t)stft_frames(len, f, h, p);
        bins = f / 2 + 1;
        fd = (f + V - 1) / V * V;
        std::vector<double> w64(f);
        std::vector<T> w(fd, T(0));
        for (size_t j = 0; j < f; ++j) w64[j] = w[j] = window ? window[j] : T(1);
        env_min = stft_envelope_min(w64.data(), len, f, h, p, frames);
        real.reset(new (std::nothrow) AnyRealPlanner<T>());
        if (!real) return PHAST_ERR_ALLOC;
        int rc = real->init(f);
        if (rc) return rc;
        PHAST_ON_DEVICE(real->device);
        PHAST_HIP(hipMalloc(reinterpret_cast<void **>(&d_win), fd * sizeof(T)));
        PHAST_HIP(hipMemcpy(d_win, w.data(), fd * sizeof(T), hipMemcpyHostToDevice));
        return PHAST_OK;
    }

    // elements of T per frame, and V - 1 more to align the caller's base to 16 bytes
    size_t per() const { return fd + real->workspace_len(1); }
    size_t workspace_len(size_t batch) const { return (batch ? batch : 1) * frames * per() + (V - 1); }
    size_t workspace_min(bool inverse) const { return (inverse ? frames : 1) * per() + (V - 1); }
    size_t device_bytes() const { return real->device_bytes() + fd * sizeof(T); }
    std::string describe() const {
        return "stft L=" + std::to_string(len) + " F=" + std::to_string(f) + " H=" + std::to_string(h) +
               (center ? (pad == kStftReflect ? " center/reflect" : " center/zero") : " uncentred") + " frames=" +
               std::to_string(frames) + " around " + real->describe();
    }

    // the checks of a _dev call, before the device is touched
    int check_dev(bool inverse, const T *sig, const T *re, const T *im, size_t signal_len, size_t batch, size_t sig_dist,
                  const T *d_work, size_t work_len) const {
        if (!sig || !re || !im) return PHAST_ERR_INVALID_ARG;
        if (signal_len != len) return PHAST_ERR_PLANNER_SIZE;
        if (inverse && !(env_min > kNolaMin)) return PHAST_ERR_INVALID_ARG;  // the window does not overlap-add to nonzero
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

    StftArgs args() const {
        StftArgs a{};
        a.win = d_win;
        a.len = len;
        a.f = f;
        a.h = h;
        a.p = p;
        a.frames = frames;
        a.fd = fd;
        a.pad = pad;
        return a;
    }

    // forward, device pointers, asynchronous on `s`: chunks of whole frames of the flattened (signal, frame) index.
    // ev (time_stages): 3 events around the sweep and the transform of a call that fits one chunk
    int stft_dev(const T *sig, T *re, T *im, size_t signal_len, size_t batch, size_t sig_dist, T *d_work, size_t work_len,
                 hipStream_t s, hipEvent_t *ev = nullptr) const {
        int rc = check_dev(false, sig, re, im, signal_len, batch, sig_dist, d_work, work_len);
        if (rc) return rc;
        if (batch == 0) return PHAST_OK;
        if (batch == 1) sig_dist = len;
        PHAST_ON_DEVICE(real->device);
        T *w = nullptr;
        const size_t rows = rows_of(d_work, work_len, &w), total = batch * frames;
        for (size_t q0 = 0; q0 < total; q0 += rows) {
            const size_t c = total - q0 < rows ? total - q0 : rows;
            StftArgs a = args();
            a.in = sig;
            a.sig_dist = sig_dist;
            a.out = w;
            a.q0 = q0;
            a.gpt = (unsigned)(fd / V);
            a.groups = c * a.gpt;
            if (ev) PHAST_HIP(hipEventRecord(ev[0], s));
            PHAST_HIP(launch_stft<T>(kStftFrame, a, s));
            if (ev) PHAST_HIP(hipEventRecord(ev[1], s));
            rc = real->dev(false, w, nullptr, re + q0 * bins, im + q0 * bins, f, c, fd, bins, w + c * fd, real->workspace_len(c), s);
            if (rc) return rc;
            if (ev) PHAST_HIP(hipEventRecord(ev[2], s));
        }
        return PHAST_OK;
    }

    // inverse, device pointers, asynchronous on `s`: chunks of whole signals (an output sample needs all its frames).
    // ev: 3 events around the transform and the sweep
    int istft_dev(const T *re, const T *im, T *sig, size_t signal_len, size_t batch, size_t sig_dist, T *d_work, size_t work_len,
                  hipStream_t s, hipEvent_t *ev = nullptr) const {
        int rc = check_dev(true, sig, re, im, signal_len, batch, sig_dist, d_work, work_len);
        if (rc) return rc;
        if (batch == 0) return PHAST_OK;
        if (batch == 1) sig_dist = len;
        PHAST_ON_DEVICE(real->device);
        T *w = nullptr;
        const size_t chunk = rows_of(d_work, work_len, &w) / frames;  // >= 1: work_len >= workspace_min(true)
        for (size_t b0 = 0; b0 < batch; b0 += chunk) {
            const size_t c = batch - b0 < chunk ? batch - b0 : chunk, rows = c * frames;
            if (ev) PHAST_HIP(hipEventRecord(ev[0], s));
            rc = real->dev(true, re + b0 * frames * bins, im + b0 * frames * bins, w, nullptr, f, rows, bins, fd, w + rows * fd,
                           real->workspace_len(rows), s);
            if (rc) return rc;
            if (ev) PHAST_HIP(hipEventRecord(ev[1], s));
            StftArgs a = args();
            a.in = w;
            a.out = sig + b0 * sig_dist;
            a.sig_dist = sig_dist;
            a.gpt = (unsigned)((len + V - 1) / V);
            a.groups = c * a.gpt;
            PHAST_HIP(launch_stft<T>(kStftOla, a, s));
            if (ev) PHAST_HIP(hipEventRecord(ev[2], s));
        }
        return PHAST_OK;
    }

    // host slices: one signal through device buffers of the call's own (signal, both planes, the workspace of all its
    // frames) on the null stream; blocking
    int host(bool inverse, const T *in_a, size_t a_len, const T *in_b, size_t b_len, T *out_a, size_t oa_len, T *out_b,
             size_t ob_len) const {
        const size_t pts = frames * bins;
        if (!in_a || !out_a || !(inverse ? in_b != nullptr : out_b != nullptr)) return PHAST_ERR_INVALID_ARG;
        if ((inverse ? oa_len : a_len) != len) return PHAST_ERR_PLANNER_SIZE;
        if (inverse ? (a_len != pts || b_len != pts) : (oa_len != pts || ob_len != pts)) return PHAST_ERR_LEN_MISMATCH;
        if (inverse && !(env_min > kNolaMin)) return PHAST_ERR_INVALID_ARG;
        PHAST_ON_DEVICE(real->device);
        auto up = [](size_t k) { return (k + 3) & ~(size_t)3; };  // every part 16-byte aligned
        const size_t ns = up(len), nc = up(pts), nw = workspace_len(1);
        DevBuf buf;
        int rc = buf.alloc((ns + 2 * nc + nw) * sizeof(T));
        if (rc) return rc;
        T *d_sig = reinterpret_cast<T *>(buf.p), *d_re = d_sig + ns, *d_im = d_re + nc, *d_w = d_im + nc;
        if (!inverse) {
            PHAST_HIP(hipMemcpy(d_sig, in_a, len * sizeof(T), hipMemcpyHostToDevice));
            rc = stft_dev(d_sig, d_re, d_im, len, 1, len, d_w, nw, nullptr);
            if (rc) return rc;
            PHAST_HIP(hipMemcpy(out_a, d_re, pts * sizeof(T), hipMemcpyDeviceToHost));
            PHAST_HIP(hipMemcpy(out_b, d_im, pts * sizeof(T), hipMemcpyDeviceToHost));
        } else {
            PHAST_HIP(hipMemcpy(d_re, in_a, pts * sizeof(T), hipMemcpyHostToDevice));
            PHAST_HIP(hipMemcpy(d_im, in_b, pts * sizeof(T), hipMemcpyHostToDevice));
            rc = istft_dev(d_re, d_im, d_sig, len, 1, len, d_w, nw, nullptr);
            if (rc) return rc;
            PHAST_HIP(hipMemcpy(out_a, d_sig, len * sizeof(T), hipMemcpyDeviceToHost));
        }
        return PHAST_OK;
    }

    // measurement hook: ms[0] = the sweep, ms[1] = the real transform, average milliseconds over `reps` calls of `batch`
    // signals at distance L in one chunk (work_len >= workspace_len(batch)); blocks
    int time_stages(bool inverse, T *sig, T *re, T *im, size_t batch, T *d_work, size_t work_len, int reps, float *ms,
                    hipStream_t s) const {
        if (!ms || reps < 1 || batch == 0) return PHAST_ERR_INVALID_ARG;
        int rc = check_dev(inverse, sig, re, im, len, batch, len, d_work, work_len);
        if (rc) return rc;
        if (work_len < workspace_len(batch) || batch * frames * per() > ((size_t)1 << 39)) return PHAST_ERR_INVALID_ARG;
        PHAST_ON_DEVICE(real->device);
        struct Events {
            hipEvent_t e[3] = {};
            ~Events() {
                for (hipEvent_t x : e)
                    if (x) hipEventDestroy(x);
            }
        } ev;
        for (hipEvent_t &x : ev.e) PHAST_HIP(hipEventCreate(&x));
        double acc[2] = {0, 0};
        for (int r = 0; r < reps; ++r) {
            rc = inverse ? istft_dev(re, im, sig, len, batch, len, d_work, work_len, s, ev.e)
                         : stft_dev(sig, re, im, len, batch, len, d_work, work_len, s, ev.e);
            if (rc) return rc;
            PHAST_HIP(hipStreamSynchronize(s));
            for (int i = 0; i < 2; ++i) {
                float t = 0;
                PHAST_HIP(hipEventElapsedTime(&t, ev.e[i], ev.e[i + 1]));
                acc[inverse ? 1 - i : i] += t;
            }
        }
        for (int i = 0; i < 2; ++i) ms[i] = (float)(acc[i] / reps);
        return PHAST_OK;
    }
};

template <typename T, typename P>
static int stft_planner_new(size_t signal_len, size_t n_fft, size_t hop, const T *window, int center, int pad_mode, P **out) {
    if (!out) return PHAST_ERR_INVALID_ARG;
    *out = nullptr;
    if (stft_bad_args(signal_len, n_fft, hop, center, pad_mode)) return PHAST_ERR_INVALID_ARG;  // before the device is touched
    auto *p = new (std::nothrow) P();
    if (!p) return PHAST_ERR_ALLOC;
    int rc = p->init(signal_len, n_fft, hop, window, center, pad_mode);
    if (rc) {
        delete p;
        return rc;
    }
    *out = p;
    return PHAST_OK;
}

}  // namespace phast
