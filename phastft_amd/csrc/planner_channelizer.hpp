// planner_channelizer.hpp -- ChannelizerPlanner<T>: the polyphase filter-bank channelizer (channelizer.hpp).
// It holds the taps on the device (T rows of M, zeros behind K), the schedule of the fold and one any-length planner of M --
// the complex one for complex signals, the real one for real signals: immutable after init, no per-call state.
//
// Complex signals: the fold writes both planes straight into the caller's output (rows of M, dense), and the complex
// planner transforms those rows in place.  The caller's workspace is that planner's alone: none for a power of two.
// Real signals, as StftPlanner: per chunk of whole frames of the flattened (signal, frame) index, the fold writes workspace
// rows of fd >= M elements (M rounded up to 16 bytes) and the real planner's R2C turns them into the caller's planes, rows of
// M / 2 + 1.  workspace_len(batch) holds every frame in one chunk; any length >= workspace_min() (one frame) runs the
// largest chunk that fits, to the same bits.
// Frames at or beyond full_frames meet only taps that are 0 or samples beyond L: they come out of the same fold as zeros.
// Indices: a frame index is below 2^31 + 1 (first_frame <= full_frames <= 2^30, out_frames <= 2^30) and D <= 2^29, so the
// sample index m D of the kernel is below 2^61.
#pragma once

#include <vector>

#include "channelizer.hpp"
#include "planner_any_real.hpp"

namespace phast {

template <typename T> struct ChannelizerPlanner {
    static constexpr size_t V = 16 / sizeof(T);
    size_t len = 0, k = 0, m = 0, d = 0, first = 0, out_frames = 0, full_frames = 0, t = 0, bins = 0, fd = 0;
    size_t ftiles = 0, ctiles = 0;
    int complex_input = 0;
    ChanGeom geom{};
    int device = -1;
    T *d_taps = nullptr;                       // t rows of m
    std::unique_ptr<AnyPlanner<T>> cplx;       // complex signals, M > 1
    std::unique_ptr<AnyRealPlanner<T>> real;   // real signals

    ~ChannelizerPlanner() {
        if (!d_taps) return;
        DeviceGuard on(device);
        hipFree(d_taps);
    }

    // `taps`: K host values; the arguments were checked by chan_bad_args
    int init(size_t signal_len, const T *taps, size_t num_taps, size_t channels, size_t hop, size_t first_, size_t out_frames_,
             int complex_) {
        len = signal_len;
        k = num_taps;
        m = channels;
        d = hop;
        first = first_;
        complex_input = complex_ ? 1 : 0;
        full_frames = (size_t)chan_full_frames(len, k, d);
        out_frames = out_frames_ ? out_frames_ : full_frames - first;
        t = (size_t)chan_t(k, m);
        bins = complex_input ? m : m / 2 + 1;
        fd = (m + V - 1) / V * V;
        geom = chan_geom(k, m, d);
        ftiles = (out_frames + geom.frames - 1) / geom.frames;
        ctiles = (m + geom.cols - 1) / geom.cols;
        std::vector<T> rows(t * m, T(0));
        for (size_t i = 0; i < k; ++i) rows[i] = taps[i];
        int rc = ensure_device(&device);
        if (rc) return rc;
        if (complex_input) {
            if (m > 1) {  // the transform of one point is the point
                cplx.reset(new (std::nothrow) AnyPlanner<T>());
                if (!cplx) return PHAST_ERR_ALLOC;
                if ((rc = cplx->init(m))) return rc;
            }
        } else {
            real.reset(new (std::nothrow) AnyRealPlanner<T>());
            if (!real) return PHAST_ERR_ALLOC;
            if ((rc = real->init(m))) return rc;
        }
        PHAST_ON_DEVICE(device);
        PHAST_HIP(hipMalloc(reinterpret_cast<void **>(&d_taps), rows.size() * sizeof(T)));
        PHAST_HIP(hipMemcpy(d_taps, rows.data(), rows.size() * sizeof(T), hipMemcpyHostToDevice));
        return PHAST_OK;
    }

    // real signals: elements of T per frame
    size_t per() const { return fd + real->workspace_len(1); }
    // (and V - 1 more to align the caller's base to 16 bytes, where there is a workspace at all)
    size_t need(size_t rows) const {
        const size_t w = complex_input ? (cplx ? cplx->workspace_len(rows) : 0) : rows * per();
        return w ? w + (V - 1) : 0;
    }
    size_t workspace_len(size_t batch) const { return need((batch ? batch : 1) * out_frames); }
    size_t workspace_min() const { return need(1); }
    size_t device_bytes() const {
        return t * m * sizeof(T) + (cplx ? cplx->device_bytes() : 0) + (real ? real->device_bytes() : 0);
    }
    std::string describe() const {
        return std::string("channelizer ") + (complex_input ? "complex" : "real") + " L=" + std::to_string(len) + " K=" +
               std::to_string(k) + " M=" + std::to_string(m) + " D=" + std::to_string(d) + " first=" + std::to_string(first) +
               " frames=" + std::to_string(out_frames) + " of " + std::to_string(full_frames) + ": T=" + std::to_string(t) +
               " tile=" + std::to_string(geom.frames) + " x " + std::to_string(geom.cols) + " chunk=" + std::to_string(geom.jc) +
               " periods=" + std::to_string(geom.rows) + (d % m == 0 && sizeof(T) == 8 ? " (taps held)" : "") + " around " +
               (real ? real->describe() : cplx ? cplx->describe() : std::string("one point"));
    }

    // the checks of a _dev call, before the device is touched
    int check_dev(const T *s_re, const T *s_im, const T *o_re, const T *o_im, size_t signal_len, size_t batch, size_t sig_dist,
                  const T *d_work, size_t work_len) const {
        if (!s_re || !o_re || !o_im) return PHAST_ERR_INVALID_ARG;
        if (complex_input ? s_im == nullptr : s_im != nullptr) return PHAST_ERR_INVALID_ARG;
        if (signal_len != len) return PHAST_ERR_PLANNER_SIZE;
        if (batch > 1 && sig_dist < len) return PHAST_ERR_INVALID_ARG;
        if (batch > ((size_t)1 << 40) / (out_frames * m)) return PHAST_ERR_INVALID_ARG;
        if (s_re == o_re || s_re == o_im || s_im == o_re || s_im == o_im || o_re == o_im || s_re == s_im)
            return PHAST_ERR_INVALID_ARG;  // the fold reads a signal while it writes the output
        if (batch && workspace_min() &&
            (!d_work || (reinterpret_cast<uintptr_t>(d_work) % sizeof(T)) || work_len < workspace_min()))
            return PHAST_ERR_INVALID_ARG;
        return PHAST_OK;
    }

    // the fold of the rows [q0, q0 + count) of the flattened (signal, frame) index into rows `ld` apart
    int fold(const T *s_re, const T *s_im, T *o_re, T *o_im, size_t sig_dist, size_t ld, size_t q0, size_t count,
             hipStream_t st) const {
        ChanArgs a{};
        a.x[0] = s_re;
        a.x[1] = s_im;
        a.out[0] = o_re;
        a.out[1] = o_im;
        a.taps = d_taps;
        a.sig_dist = sig_dist;
        a.ld = ld;
        a.len = len;
        a.t = t;
        a.m = m;
        a.d = d;
        a.first = first;
        a.out_frames = out_frames;
        a.q0 = q0;
        a.count = count;
        const size_t q1 = q0 + count - 1;
        a.ft0 = q0 / out_frames * ftiles + q0 % out_frames / geom.frames;
        a.ftn = q1 / out_frames * ftiles + q1 % out_frames / geom.frames - a.ft0 + 1;
        a.ftiles = ftiles;
        a.ctiles = ctiles;
        a.groups = (s_im ? 2 : 1) * a.ftn * ctiles * 256;
        a.dqv = (unsigned)(geom.frames > 1 ? d / m : 0);  // one frame: its steps are not used (and d / m may pass 32 bits)
        a.dm = (unsigned)(d % m);
        a.sq = (unsigned)(geom.per > 1 ? geom.fpp * d / m : 0);
        a.sm = (unsigned)(geom.per > 1 ? geom.fpp * d % m : 0);
        a.geom = geom;
        PHAST_HIP(launch_chan_fold<T>(a, st));
        return PHAST_OK;
    }

    // the caller's workspace from its first 16-byte boundary on
    static size_t align_work(T *d_work, size_t work_len, T **w) {
        const size_t skip = ((16 - (reinterpret_cast<uintptr_t>(d_work) & 15u)) & 15u) / sizeof(T);
        *w = d_work + skip;
        return work_len - skip;
    }

    // device pointers, asynchronous on `st`: signal b at s_re (s_im) + b sig_dist; element (b out_frames + i) bins + k of the
    // output planes.  ev (time_stages): 3 events around the fold and the transform of a call that fits one chunk
    int dev(const T *s_re, const T *s_im, T *o_re, T *o_im, size_t signal_len, size_t batch, size_t sig_dist, T *d_work,
            size_t work_len, hipStream_t st, hipEvent_t *ev = nullptr) const {
        int rc = check_dev(s_re, s_im, o_re, o_im, signal_len, batch, sig_dist, d_work, work_len);
        if (rc) return rc;
        if (batch == 0) return PHAST_OK;
        if (batch == 1) sig_dist = len;
        PHAST_ON_DEVICE(device);
        const size_t total = batch * out_frames;
        T *w = nullptr;
        size_t wl = 0;
        if (workspace_min()) wl = align_work(d_work, work_len, &w);
        if (complex_input) {
            if (ev) PHAST_HIP(hipEventRecord(ev[0], st));
            if ((rc = fold(s_re, s_im, o_re, o_im, sig_dist, m, 0, total, st))) return rc;
            if (ev) PHAST_HIP(hipEventRecord(ev[1], st));
            if (cplx && (rc = cplx->fft_dev_any(o_re, o_im, m, total, m, PHAST_FORWARD, w, wl, st))) return rc;
            if (ev) PHAST_HIP(hipEventRecord(ev[2], st));
            return PHAST_OK;
        }
        size_t rows = wl / per();  // >= 1: work_len >= workspace_min()
        const size_t cap = ((size_t)1 << 39) / per();
        if (rows > cap) rows = cap;
        for (size_t q0 = 0; q0 < total; q0 += rows) {
            const size_t c = total - q0 < rows ? total - q0 : rows;
            if (ev) PHAST_HIP(hipEventRecord(ev[0], st));
            if ((rc = fold(s_re, nullptr, w, nullptr, sig_dist, fd, q0, c, st))) return rc;
            if (ev) PHAST_HIP(hipEventRecord(ev[1], st));
            rc = real->dev(false, w, nullptr, o_re + q0 * bins, o_im + q0 * bins, m, c, fd, bins, w + c * fd, real->workspace_len(c), st);
            if (rc) return rc;
            if (ev) PHAST_HIP(hipEventRecord(ev[2], st));
        }
        return PHAST_OK;
    }

    // host slices: one signal through device buffers of the call's own on the null stream; blocking
    int host(const T *s_re, const T *s_im, size_t sig_len, T *o_re, T *o_im, size_t o_len) const {
        if (!s_re || !o_re || !o_im || (complex_input ? s_im == nullptr : s_im != nullptr)) return PHAST_ERR_INVALID_ARG;
        if (sig_len != len) return PHAST_ERR_PLANNER_SIZE;
        const size_t pts = out_frames * bins;
        if (o_len != pts) return PHAST_ERR_LEN_MISMATCH;
        PHAST_ON_DEVICE(device);
        auto up = [](size_t n) { return (n + 3) & ~(size_t)3; };  // every part 16-byte aligned
        const size_t ns = up(len), nc = up(pts), nw = workspace_len(1);
        DevBuf buf;
        int rc = buf.alloc((2 * ns + 2 * nc + nw + 4) * sizeof(T));
        if (rc) return rc;
        T *d_sr = reinterpret_cast<T *>(buf.p), *d_si = d_sr + ns, *d_or = d_si + ns, *d_oi = d_or + nc, *d_w = d_oi + nc;
        PHAST_HIP(hipMemcpy(d_sr, s_re, len * sizeof(T), hipMemcpyHostToDevice));
        if (s_im) PHAST_HIP(hipMemcpy(d_si, s_im, len * sizeof(T), hipMemcpyHostToDevice));
        rc = dev(d_sr, s_im ? d_si : nullptr, d_or, d_oi, len, 1, len, d_w, nw, nullptr);
        if (rc) return rc;
        PHAST_HIP(hipMemcpy(o_re, d_or, pts * sizeof(T), hipMemcpyDeviceToHost));
        PHAST_HIP(hipMemcpy(o_im, d_oi, pts * sizeof(T), hipMemcpyDeviceToHost));
        return PHAST_OK;
    }

    // measurement hook: ms[0] = the fold, ms[1] = the transform, average milliseconds over `reps` calls of `batch` signals
    // at distance L in one chunk (work_len >= workspace_len(batch)); blocks
    int time_stages(const T *s_re, const T *s_im, T *o_re, T *o_im, size_t batch, T *d_work, size_t work_len, int reps,
                    float *ms, hipStream_t st) const {
        if (!ms || reps < 1 || batch == 0) return PHAST_ERR_INVALID_ARG;
        int rc = check_dev(s_re, s_im, o_re, o_im, len, batch, len, d_work, work_len);
        if (rc) return rc;
        if (work_len < workspace_len(batch) || (real && batch * out_frames * per() > ((size_t)1 << 39))) return PHAST_ERR_INVALID_ARG;
        PHAST_ON_DEVICE(device);
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
            if ((rc = dev(s_re, s_im, o_re, o_im, len, batch, len, d_work, work_len, st, ev.e))) return rc;
            PHAST_HIP(hipStreamSynchronize(st));
            for (int i = 0; i < 2; ++i) {
                float v = 0;
                PHAST_HIP(hipEventElapsedTime(&v, ev.e[i], ev.e[i + 1]));
                acc[i] += v;
            }
        }
        for (int i = 0; i < 2; ++i) ms[i] = (float)(acc[i] / reps);
        return PHAST_OK;
    }
};

template <typename T, typename P>
static int channelizer_planner_new(size_t signal_len, const T *taps, size_t num_taps, size_t channels, size_t hop,
                                   size_t first_frame, size_t out_frames, int complex_input, P **out) {
    if (!out) return PHAST_ERR_INVALID_ARG;
    *out = nullptr;
    if (!taps || chan_bad_args(signal_len, num_taps, channels, hop, first_frame, out_frames))  // before the device is touched
        return PHAST_ERR_INVALID_ARG;
    auto *p = new (std::nothrow) P();
    if (!p) return PHAST_ERR_ALLOC;
    int rc = p->init(signal_len, taps, num_taps, channels, hop, first_frame, out_frames, complex_input);
    if (rc) {
        delete p;
        return rc;
    }
    *out = p;
    return PHAST_OK;
}

}  // namespace phast
