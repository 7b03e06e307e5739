// planner_psd.hpp -- PsdPlanner<T>: Welch spectral estimation (psd.hpp): welch, csd, spectrogram.
// It holds one AnyRealPlanner<T>(F), the device copy of the window (doubles) and the scale constants: immutable after init,
// no per-call state.  A call runs, per chunk of whole frames of the flattened (signal, frame) index, the mean and frame sweeps
// (psd.hip) into workspace rows, the real planner's own R2C of those rows into spectrum planes of the workspace, and either
// the accumulate sweep into partial rows of doubles and -- for every signal whose last frame the chunk holds -- the final
// sweep into the caller's output, or (average = 0) the point sweep of every row.  A cross call carries the c frames of x and
// the same c frames of y through the same launches (rows 0 .. c and c .. 2c).
//
// The caller's workspace, from its first 16-byte boundary on, for a chunk of c frames (X = 2 for a cross call, else 1):
//     rows     X c fd elements of T     fd = F rounded up to 16 bytes
//     re, im   X c bd each              bd = bins rounded up to 16 bytes
//     real     the real planner's workspace_len(X c)
//     means    X c doubles, rounded up to 16 bytes
//     partial  slots * planes * slabs * bd doubles; planes = 4 for a cross call (re, im, |X|^2, |Y|^2), else 1.  A signal's
//              partial rows live in slot b mod slots while a chunk touches it; a chunk of c frames touches at most
//              slots(c) = min(batch, 1 + (c + S - 2) / S) signals.
// workspace_len(batch, cross) holds all frames of the batch in one chunk; any length >= workspace_min(cross) (one frame, one
// slot) runs the largest chunk that fits.  The sums are carried in double in the partial rows from chunk to chunk, so the
// result's bits do not depend on the chunking.
#pragma once

#include <vector>

#include "planner_any_real.hpp"
#include "psd.hpp"

namespace phast {

template <typename T> struct PsdPlanner {
    static constexpr size_t V = 16 / sizeof(T), D = sizeof(double) / sizeof(T);
    size_t len = 0, p = 0, h = 0, f = 0;  // L, P, H, F
    size_t frames = 0, bins = 0, fd = 0, bd = 0, q = 0, slabs = 0;
    int detrend = 0, scaling = 0;
    double fs = 1.0, sigma = 0;
    double *d_win = nullptr;  // fd doubles: w, then zeros
    std::unique_ptr<AnyRealPlanner<T>> real;

    ~PsdPlanner() {
        if (!d_win) return;
        DeviceGuard on(real ? real->device : -1);
        hipFree(d_win);
    }

    // `w`: the P window values; the arguments were checked by psd_bad_args and sigma by psd_sigma
    int init(size_t signal_len, size_t nperseg, size_t hop, size_t nfft, const std::vector<double> &w, int detrend_, int scaling_,
             double fs_, double sigma_) {
        len = signal_len;
        p = nperseg;
        h = hop;
        f = nfft;
        detrend = detrend_;
        scaling = scaling_;
        fs = fs_;
        sigma = sigma_;
        frames = (size_t)psd_segments(len, p, h);
        bins = (size_t)psd_bins(f);
        fd = (f + V - 1) / V * V;
        bd = (bins + V - 1) / V * V;
        q = (size_t)psd_slab_len(frames, bins);
        slabs = (size_t)psd_slabs(frames, q);
        std::vector<double> win(fd, 0.0);
        for (size_t j = 0; j < p; ++j) win[j] = w[j];
        real.reset(new (std::nothrow) AnyRealPlanner<T>());
        if (!real) return PHAST_ERR_ALLOC;
        int rc = real->init(f);
        if (rc) return rc;
        PHAST_ON_DEVICE(real->device);
        PHAST_HIP(hipMalloc(reinterpret_cast<void **>(&d_win), fd * sizeof(double)));
        PHAST_HIP(hipMemcpy(d_win, win.data(), fd * sizeof(double), hipMemcpyHostToDevice));
        return PHAST_OK;
    }

    // elements of T per frame of one signal, without the means and the partial rows
    size_t per() const { return fd + 2 * bd + real->workspace_len(1); }
    size_t slots_of(size_t c, size_t batch) const {
        const size_t s = 1 + (c + frames - 2) / frames;
        return s < batch ? s : batch;
    }
    // elements of T of a chunk of c frames with `slots` signals' partial rows (and V - 1 more to align the caller's base)
    size_t need(size_t c, size_t slots, bool cross) const {
        const size_t x = cross ? 2 : 1;
        return x * c * per() + (x * c + 1) / 2 * 2 * D + slots * (cross ? 4 : 1) * slabs * bd * D + (V - 1);
    }
    size_t workspace_len(size_t batch, bool cross) const {
        batch = batch ? batch : 1;
        return need(batch * frames, batch, cross);
    }
    size_t workspace_min(bool cross) const { return need(1, 1, cross); }
    size_t device_bytes() const { return real->device_bytes() + fd * sizeof(double); }
    std::string describe() const {
        return "psd L=" + std::to_string(len) + " P=" + std::to_string(p) + " H=" + std::to_string(h) + " F=" + std::to_string(f) +
               (detrend ? " detrend=constant" : " detrend=none") + (scaling == kPsdDensity ? " density" : " spectrum") +
               " segments=" + std::to_string(frames) + " slab=" + std::to_string(q) + " x " + std::to_string(slabs) + " around " +
               real->describe();
    }

    // the checks of a _dev call, before the device is touched.  out[0..3]: auto P_xx, or cross re, im, P_xx, P_yy
    int check_dev(const T *x, const T *y, bool cross, T *const *out, size_t signal_len, size_t batch, size_t sig_dist, int average,
                  const T *d_work, size_t work_len) const {
        if (!x || (cross && !y) || !out[0] || (cross && !out[1])) return PHAST_ERR_INVALID_ARG;
        if (average != 0 && average != 1) return PHAST_ERR_INVALID_ARG;
        if (signal_len != len) return PHAST_ERR_PLANNER_SIZE;
        if (batch > 1 && sig_dist < len) return PHAST_ERR_INVALID_ARG;
        if (batch && (!d_work || (reinterpret_cast<uintptr_t>(d_work) % sizeof(T)) || work_len < workspace_min(cross)))
            return PHAST_ERR_INVALID_ARG;
        return PHAST_OK;
    }

    // the caller's workspace from its first 16-byte boundary on; the frames of a chunk: the most that fit (a launch's groups
    // < 2^38), at least one since work_len >= workspace_min
    size_t chunk_of(T *d_work, size_t work_len, size_t batch, bool cross, T **w) const {
        const size_t skip = ((16 - (reinterpret_cast<uintptr_t>(d_work) & 15u)) & 15u) / sizeof(T);
        *w = d_work + skip;
        const size_t avail = work_len - skip + (V - 1), total = batch * frames;
        size_t cap = ((size_t)1 << 39) / ((cross ? 2 : 1) * per());
        if (cap > total) cap = total;
        size_t lo = 1, hi = cap < 1 ? 1 : cap;  // need() grows with c
        while (lo < hi) {
            const size_t mid = lo + (hi - lo + 1) / 2;
            if (need(mid, slots_of(mid, batch), cross) <= avail) lo = mid;
            else hi = mid - 1;
        }
        return lo;
    }

    PsdArgs args(bool cross) const {
        PsdArgs a{};
        a.win = d_win;
        a.p = p;
        a.h = h;
        a.frames = frames;
        a.fd = fd;
        a.bd = bd;
        a.bins = bins;
        a.nfft = f;
        a.q = q;
        a.slabs = slabs;
        a.tpr = psd_mean_threads(p);
        a.planes = cross ? 4 : 1;
        return a;
    }

    // device pointers, asynchronous on `s`.  y NULL: the auto spectrum into out[0]; else the cross spectrum into out[0] (re) and
    // out[1] (im), P_xx into out[2] and P_yy into out[3] where those are not NULL.  ev (time_stages): 4 events around the mean
    // and frame sweeps, the transform, and the accumulate and final sweeps of a call that fits one chunk; slab_q (time_stages,
    // >= q): the frames per slab of this call instead of the planner's
    int run(const T *x, const T *y, T *const *out, size_t signal_len, size_t batch, size_t sig_dist, int average, T *d_work,
            size_t work_len, hipStream_t s, hipEvent_t *ev = nullptr, size_t slab_q = 0) const {
        const bool cross = y != nullptr;
        int rc = check_dev(x, y, cross, out, signal_len, batch, sig_dist, average, d_work, work_len);
        if (rc) return rc;
        if (batch == 0) return PHAST_OK;
        if (batch == 1) sig_dist = len;
        PHAST_ON_DEVICE(real->device);
        T *w = nullptr;
        const size_t chunk = chunk_of(d_work, work_len, batch, cross, &w), total = batch * frames, nx = cross ? 2 : 1;
        const size_t slots = slots_of(chunk, batch);
        for (size_t q0 = 0; q0 < total; q0 += chunk) {
            const size_t c = total - q0 < chunk ? total - q0 : chunk, nr = nx * c, cap = nx * chunk;
            // the parts lie where a whole chunk puts them: the partial rows outlive a chunk, the last one may be shorter
            T *rows = w, *re = rows + cap * fd, *im = re + cap * bd, *iw = im + cap * bd;
            double *mean = reinterpret_cast<double *>(iw + real->workspace_len(cap)), *acc = mean + (cap + 1) / 2 * 2;
            PsdArgs a = args(cross);
            if (slab_q) {
                a.q = slab_q;
                a.slabs = (size_t)psd_slabs(frames, slab_q);
            }
            a.x = x;
            a.y = y;
            a.sig_dist = sig_dist;
            a.rows = rows;
            a.re = re;
            a.im = im;
            a.acc = acc;
            a.slots = slots;
            a.q0 = q0;
            a.c = c;
            for (int i = 0; i < (cross ? 4 : 1); ++i) a.out[i] = out[i];
            if (ev) PHAST_HIP(hipEventRecord(ev[0], s));
            if (detrend == kPsdDetrendConstant) {
                a.mean = mean;
                a.groups = nr * a.tpr;
                PHAST_HIP(launch_psd<T>(kPsdMean, a, s));
            }
            a.gpt = (unsigned)(fd / V);
            a.groups = nr * a.gpt;
            PHAST_HIP(launch_psd<T>(kPsdFrame, a, s));
            if (ev) PHAST_HIP(hipEventRecord(ev[1], s));
            rc = real->dev(false, rows, nullptr, re, im, f, nr, fd, bd, iw, real->workspace_len(nr), s);
            if (rc) return rc;
            if (ev) PHAST_HIP(hipEventRecord(ev[2], s));
            if (!average) {
                a.scale = sigma;
                a.count = c * bins;
                a.groups = (a.count + V - 1) / V;
                PHAST_HIP(launch_psd<T>(kPsdPoint, a, s));
            } else {
                const size_t b_lo = q0 / frames, nb = (q0 + c - 1) / frames - b_lo + 1;
                a.b0 = b_lo;
                a.s0 = 0;
                a.ns = a.slabs;
                if (nb == 1) {  // one signal: only the slabs the chunk touches
                    const size_t f_lo = q0 - b_lo * frames;
                    a.s0 = f_lo / a.q;
                    a.ns = (f_lo + c - 1) / a.q - a.s0 + 1;
                }
                a.gpt = (unsigned)(bd / V);
                a.groups = nb * a.ns * a.gpt;
                PHAST_HIP(launch_psd<T>(kPsdAccum, a, s));
                const size_t done = (q0 + c) / frames - b_lo;  // the signals whose last frame the chunk holds
                if (done) {
                    a.scale = sigma / (double)frames;
                    a.count = done * bins;
                    a.groups = (a.count + V - 1) / V;
                    PHAST_HIP(launch_psd<T>(kPsdFinal, a, s));
                }
            }
            if (ev) PHAST_HIP(hipEventRecord(ev[3], s));
        }
        return PHAST_OK;
    }

    // host slices: one signal (cross: one pair) through device buffers of the call's own on the null stream; blocking.
    // out_len[i]: the elements of out[i], bins (average) or S * bins each
    int host(const T *x, size_t x_len, const T *y, size_t y_len, T *const *out, const size_t *out_len, int average) const {
        const bool cross = y != nullptr;
        const int no = cross ? 4 : 1;
        if (!x || !out[0] || (cross && !out[1])) return PHAST_ERR_INVALID_ARG;
        if (average != 0 && average != 1) return PHAST_ERR_INVALID_ARG;
        if (x_len != len || (cross && y_len != len)) return PHAST_ERR_PLANNER_SIZE;
        const size_t pts = average ? bins : frames * bins;
        for (int i = 0; i < no; ++i)
            if (out[i] && out_len[i] != pts) return PHAST_ERR_LEN_MISMATCH;
        PHAST_ON_DEVICE(real->device);
        auto up = [](size_t k) { return (k + 3) & ~(size_t)3; };  // every part 16-byte aligned
        const size_t ns = up(len), nc = up(pts), nw = workspace_len(1, cross);
        DevBuf buf;
        int rc = buf.alloc((2 * ns + 4 * nc + nw) * sizeof(T));
        if (rc) return rc;
        T *d_x = reinterpret_cast<T *>(buf.p), *d_y = d_x + ns, *d_o = d_y + ns, *d_w = d_o + 4 * nc;
        T *d_out[4] = {nullptr, nullptr, nullptr, nullptr};
        for (int i = 0; i < no; ++i)
            if (out[i]) d_out[i] = d_o + i * nc;
        PHAST_HIP(hipMemcpy(d_x, x, len * sizeof(T), hipMemcpyHostToDevice));
        if (cross) PHAST_HIP(hipMemcpy(d_y, y, len * sizeof(T), hipMemcpyHostToDevice));
        rc = run(d_x, cross ? d_y : nullptr, d_out, len, 1, len, average, d_w, nw, nullptr);
        if (rc) return rc;
        for (int i = 0; i < no; ++i)
            if (out[i]) PHAST_HIP(hipMemcpy(out[i], d_out[i], pts * sizeof(T), hipMemcpyDeviceToHost));
        return PHAST_OK;
    }

    // measurement hook: ms[0..2] = the mean and frame sweeps, the real transform, and the accumulate and final sweeps (average
    // = 0: the point sweep), average milliseconds over `reps` auto-spectrum calls of `batch` signals at distance L in one chunk
    // (work_len >= workspace_len(batch, false)); blocks.  slab: 0, or the frames per slab to sum with instead of the planner's q
    // (>= q, so that the partial rows fit: what the slab rule buys is the accumulate sweep's time against slab = S)
    int time_stages(T *sig, T *d_out, size_t batch, int average, size_t slab, T *d_work, size_t work_len, int reps, float *ms,
                    hipStream_t s) const {
        if (!ms || reps < 1 || batch == 0 || (slab && slab < q)) return PHAST_ERR_INVALID_ARG;
        T *out[4] = {d_out, nullptr, nullptr, nullptr};
        int rc = check_dev(sig, nullptr, false, out, len, batch, len, average, d_work, work_len);
        if (rc) return rc;
        if (work_len < workspace_len(batch, false) || batch * frames * per() > ((size_t)1 << 39)) return PHAST_ERR_INVALID_ARG;
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
            rc = run(sig, nullptr, out, len, batch, len, average, d_work, work_len, s, ev.e, slab);
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

template <typename T, typename P>
static int psd_planner_new(size_t signal_len, size_t nperseg, size_t hop, size_t nfft, const double *window, int detrend,
                           int scaling, double fs, P **out) {
    if (!out) return PHAST_ERR_INVALID_ARG;
    *out = nullptr;
    if (psd_bad_args(signal_len, nperseg, hop, nfft, detrend, scaling, fs, (unsigned)(16 / sizeof(T)))) return PHAST_ERR_INVALID_ARG;
    std::vector<double> w(nperseg);
    for (size_t j = 0; j < nperseg; ++j) w[j] = window ? window[j] : (double)psd_hann(j, nperseg);
    double sigma = 0;
    if (psd_sigma(w.data(), nperseg, scaling, fs, &sigma)) return PHAST_ERR_INVALID_ARG;  // before the device is touched
    auto *p = new (std::nothrow) P();
    if (!p) return PHAST_ERR_ALLOC;
    int rc = p->init(signal_len, nperseg, hop, nfft, w, detrend, scaling, fs, sigma);
    if (rc) {
        delete p;
        return rc;
    }
    *out = p;
    return PHAST_OK;
}

}  // namespace phast
