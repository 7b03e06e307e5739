// planner_synthesizer.hpp -- SynthesizerPlanner<T>: the polyphase synthesis filter bank (synthesizer.hpp).
// It holds the taps on the device (K values, M g[j] rounded once to T), the schedule of the unfold and one any-length planner
// of M -- the complex one for complex output, the real one for real output: immutable after init, no per-call state.
//
// Real output, as StftPlanner's inverse: per chunk of whole signals, the real planner's C2R turns the caller's rows of
// M / 2 + 1 bins into workspace rows of fd >= M elements (M rounded up to 16 bytes) and the unfold gathers the caller's plane
// from them.  The engine's C2R of an even M >= 4 runs the power-of-two preprocess formula, which does not ignore the
// imaginary parts of bin 0 and bin M / 2 as irfft does: there a copy sweep first brings the imaginary plane into the
// workspace with those two columns set to 0 (the caller's planes are never written).  Complex output: a copy sweep brings
// both planes into such rows, the complex planner's inverse runs in place there and the unfold gathers two planes; for M = 1
// the unfold reads the caller's rows and there is no workspace.
// workspace_len(batch) holds every frame in one chunk; workspace_min() holds one signal's frames, because an output sample
// needs all its frames; any length in between runs the largest chunk of whole signals that fits, to the same bits.
// Indices: n = first + i < 2^59 + 2^30 and m D <= n, so the kernel's sample index stays below 2^61.
#pragma once

#include <vector>

#include "planner_any_real.hpp"
#include "synthesizer.hpp"

namespace phast {

template <typename T> struct SynthesizerPlanner {
    static constexpr size_t V = 16 / sizeof(T);
    size_t frames = 0, k = 0, m = 0, d = 0, first = 0, out_len = 0, full_len = 0, bins = 0, fd = 0, tiles = 0;
    int complex_output = 0;
    SynthGeom geom{};
    int device = -1;
    T *d_taps = nullptr;                      // k values, M g[j]
    std::unique_ptr<AnyPlanner<T>> cplx;      // complex output, M > 1
    std::unique_ptr<AnyRealPlanner<T>> real;  // real output

    ~SynthesizerPlanner() {
        if (!d_taps) return;
        DeviceGuard on(device);
        hipFree(d_taps);
    }

    // `taps`: K host values; the arguments were checked by synth_bad_args
    int init(size_t frames_, const T *taps, size_t num_taps, size_t channels, size_t hop, size_t first_, size_t out_len_,
             int complex_) {
        frames = frames_;
        k = num_taps;
        m = channels;
        d = hop;
        first = first_;
        complex_output = complex_ ? 1 : 0;
        full_len = (size_t)synth_full_len(frames, k, d);
        out_len = out_len_ ? out_len_ : full_len - first;
        bins = complex_output ? m : m / 2 + 1;
        fd = (m + V - 1) / V * V;
        geom = synth_geom(k, m, d);
        tiles = (out_len + geom.tile - 1) / geom.tile;
        std::vector<T> tab(k);
        for (size_t i = 0; i < k; ++i) tab[i] = (T)((double)taps[i] * (double)m);  // the transform's inverse carries 1 / M
        int rc = ensure_device(&device);
        if (rc) return rc;
        if (complex_output) {
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
        PHAST_HIP(hipMalloc(reinterpret_cast<void **>(&d_taps), tab.size() * sizeof(T)));
        PHAST_HIP(hipMemcpy(d_taps, tab.data(), tab.size() * sizeof(T), hipMemcpyHostToDevice));
        return PHAST_OK;
    }

    // real output of an even M >= 4: the imaginary plane goes through a copy with bin 0 and bin M / 2 zeroed
    bool zeroed() const { return !complex_output && m >= 4 && m % 2 == 0; }
    // elements of T per frame: real output a row and the C2R's workspace; complex output two rows and the inverse's
    size_t per() const {
        if (complex_output) return cplx ? 2 * fd + cplx->workspace_len(1) : 0;
        return fd + (zeroed() ? (bins + V - 1) / V * V : 0) + real->workspace_len(1);
    }
    // (and V - 1 more to align the caller's base to 16 bytes, where there is a workspace at all)
    size_t need(size_t rows) const { return per() ? rows * per() + (V - 1) : 0; }
    size_t workspace_len(size_t batch) const { return need((batch ? batch : 1) * frames); }
    size_t workspace_min() const { return need(frames); }
    size_t device_bytes() const {
        return k * sizeof(T) + (cplx ? cplx->device_bytes() : 0) + (real ? real->device_bytes() : 0);
    }
    std::string describe() const {
        return std::string("synthesizer ") + (complex_output ? "complex" : "real") + " F=" + std::to_string(frames) + " K=" +
               std::to_string(k) + " M=" + std::to_string(m) + " D=" + std::to_string(d) + " first=" + std::to_string(first) +
               " samples=" + std::to_string(out_len) + " of " + std::to_string(full_len) + ": terms<=" + std::to_string(geom.terms) +
               " tile=" + std::to_string(geom.tile) + " (" + std::to_string(geom.per) + " per thread, no LDS) behind " +
               (real ? real->describe() : cplx ? cplx->describe() : std::string("one point"));
    }

    // the checks of a _dev call, before the device is touched
    int check_dev(const T *y_re, const T *y_im, const T *o_re, const T *o_im, size_t num_frames, size_t batch, size_t out_dist,
                  const T *d_work, size_t work_len) const {
        if (!y_re || !y_im || !o_re) return PHAST_ERR_INVALID_ARG;
        if (complex_output ? o_im == nullptr : o_im != nullptr) return PHAST_ERR_INVALID_ARG;
        if (num_frames != frames) return PHAST_ERR_PLANNER_SIZE;
        if (batch > 1 && out_dist < out_len) return PHAST_ERR_INVALID_ARG;
        if (batch > ((size_t)1 << 40) / (frames * m) || batch > ((size_t)1 << 40) / out_len) return PHAST_ERR_INVALID_ARG;
        if (y_re == o_re || y_re == o_im || y_im == o_re || y_im == o_im || o_re == o_im || y_re == y_im)
            return PHAST_ERR_INVALID_ARG;  // the unfold (M = 1) and the transforms read the input while the output is written
        if (batch && workspace_min() &&
            (!d_work || (reinterpret_cast<uintptr_t>(d_work) % sizeof(T)) || work_len < workspace_min()))
            return PHAST_ERR_INVALID_ARG;
        return PHAST_OK;
    }

    // the unfold of `count` signals from rows `ld` apart
    int unfold(const T *v_re, const T *v_im, T *o_re, T *o_im, size_t ld, size_t out_dist, size_t count, hipStream_t st) const {
        SynthArgs a{};
        a.v[0] = v_re;
        a.v[1] = v_im;
        a.out[0] = o_re;
        a.out[1] = o_im;
        a.taps = d_taps;
        a.ld = ld;
        a.out_dist = out_dist;
        a.f = frames;
        a.k = k;
        a.m = m;
        a.d = d;
        a.first = first;
        a.out_len = out_len;
        a.count = count;
        a.tiles = tiles;
        a.groups = (o_im ? 2 : 1) * count * tiles * 256;
        a.geom = geom;
        PHAST_HIP(launch_synth_unfold<T>(a, st));
        return PHAST_OK;
    }

    // the caller's workspace from its first 16-byte boundary on
    static size_t align_work(T *d_work, size_t work_len, T **w) {
        const size_t skip = ((16 - (reinterpret_cast<uintptr_t>(d_work) & 15u)) & 15u) / sizeof(T);
        *w = d_work + skip;
        return work_len - skip;
    }

    // device pointers, asynchronous on `st`: element (b F + m) bins + k of the input planes; signal b at o_re (o_im) + b out_dist.
    // ev (time_stages): 3 events around the transform (with its copy) and the unfold of a call that fits one chunk
    int dev(const T *y_re, const T *y_im, T *o_re, T *o_im, size_t num_frames, size_t batch, size_t out_dist, T *d_work,
            size_t work_len, hipStream_t st, hipEvent_t *ev = nullptr) const {
        int rc = check_dev(y_re, y_im, o_re, o_im, num_frames, batch, out_dist, d_work, work_len);
        if (rc) return rc;
        if (batch == 0) return PHAST_OK;
        if (batch == 1) out_dist = out_len;
        PHAST_ON_DEVICE(device);
        if (!per()) {  // complex output of one channel: v = Y
            if (ev) PHAST_HIP(hipEventRecord(ev[0], st));
            if (ev) PHAST_HIP(hipEventRecord(ev[1], st));
            if ((rc = unfold(y_re, y_im, o_re, o_im, 1, out_dist, batch, st))) return rc;
            if (ev) PHAST_HIP(hipEventRecord(ev[2], st));
            return PHAST_OK;
        }
        T *w = nullptr;
        const size_t wl = align_work(d_work, work_len, &w);
        size_t chunk = wl / (frames * per());  // >= 1: work_len >= workspace_min()
        const size_t cap = ((size_t)1 << 39) / (frames * per());
        if (chunk > cap) chunk = cap ? cap : 1;
        for (size_t b0 = 0; b0 < batch; b0 += chunk) {
            const size_t c = batch - b0 < chunk ? batch - b0 : chunk, rows = c * frames;
            const T *in_re = y_re + b0 * frames * bins, *in_im = y_im + b0 * frames * bins;
            T *sig_re = o_re + b0 * out_dist, *sig_im = o_im ? o_im + b0 * out_dist : nullptr;
            if (ev) PHAST_HIP(hipEventRecord(ev[0], st));
            if (complex_output) {
                T *v_re = w, *v_im = w + rows * fd, *tw = v_im + rows * fd;
                SynthCopyArgs ca{};
                ca.in[0] = in_re;
                ca.in[1] = in_im;
                ca.out[0] = v_re;
                ca.out[1] = v_im;
                ca.n = m;
                ca.in_ld = m;
                ca.out_ld = fd;
                ca.rows = rows;
                ca.zero_a = ca.zero_b = m;
                ca.groups = 2 * rows * m;
                PHAST_HIP(launch_synth_copy<T>(ca, st));
                if ((rc = cplx->fft_dev_any(v_re, v_im, m, rows, fd, PHAST_REVERSE, tw, cplx->workspace_len(rows), st))) return rc;
                if (ev) PHAST_HIP(hipEventRecord(ev[1], st));
                if ((rc = unfold(v_re, v_im, sig_re, sig_im, fd, out_dist, c, st))) return rc;
            } else {
                T *tw = w + rows * fd;
                if (zeroed()) {
                    SynthCopyArgs ca{};
                    ca.in[0] = in_im;
                    ca.out[0] = tw;
                    ca.n = ca.in_ld = ca.out_ld = bins;
                    ca.rows = rows;
                    ca.zero_a = 0;
                    ca.zero_b = m / 2;
                    ca.groups = rows * bins;
                    PHAST_HIP(launch_synth_copy<T>(ca, st));
                    in_im = tw;
                    tw += (rows * bins + V - 1) / V * V;
                }
                rc = real->dev(true, in_re, in_im, w, nullptr, m, rows, bins, fd, tw, real->workspace_len(rows), st);
                if (rc) return rc;
                if (ev) PHAST_HIP(hipEventRecord(ev[1], st));
                if ((rc = unfold(w, nullptr, sig_re, nullptr, fd, out_dist, c, st))) return rc;
            }
            if (ev) PHAST_HIP(hipEventRecord(ev[2], st));
        }
        return PHAST_OK;
    }

    // host slices: one signal's frames through device buffers of the call's own on the null stream; blocking
    int host(const T *y_re, const T *y_im, size_t y_len, T *o_re, T *o_im, size_t o_len) const {
        if (!y_re || !y_im || !o_re || (complex_output ? o_im == nullptr : o_im != nullptr)) return PHAST_ERR_INVALID_ARG;
        const size_t pts = frames * bins;
        if (y_len != pts) return PHAST_ERR_PLANNER_SIZE;
        if (o_len != out_len) return PHAST_ERR_LEN_MISMATCH;
        PHAST_ON_DEVICE(device);
        auto up = [](size_t n) { return (n + 3) & ~(size_t)3; };  // every part 16-byte aligned
        const size_t ns = up(out_len), nc = up(pts), nw = workspace_len(1);
        DevBuf buf;
        int rc = buf.alloc((2 * ns + 2 * nc + nw + 4) * sizeof(T));
        if (rc) return rc;
        T *d_yr = reinterpret_cast<T *>(buf.p), *d_yi = d_yr + nc, *d_or = d_yi + nc, *d_oi = d_or + ns, *d_w = d_oi + ns;
        PHAST_HIP(hipMemcpy(d_yr, y_re, pts * sizeof(T), hipMemcpyHostToDevice));
        PHAST_HIP(hipMemcpy(d_yi, y_im, pts * sizeof(T), hipMemcpyHostToDevice));
        rc = dev(d_yr, d_yi, d_or, o_im ? d_oi : nullptr, frames, 1, out_len, d_w, nw, nullptr);
        if (rc) return rc;
        PHAST_HIP(hipMemcpy(o_re, d_or, out_len * sizeof(T), hipMemcpyDeviceToHost));
        if (o_im) PHAST_HIP(hipMemcpy(o_im, d_oi, out_len * sizeof(T), hipMemcpyDeviceToHost));
        return PHAST_OK;
    }

    // measurement hook: ms[0] = the transform (with the copy in front of it), ms[1] = the unfold, average milliseconds over
    // `reps` calls of `batch` signals at distance out_len in one chunk (work_len >= workspace_len(batch)); blocks
    int time_stages(const T *y_re, const T *y_im, T *o_re, T *o_im, size_t batch, T *d_work, size_t work_len, int reps,
                    float *ms, hipStream_t st) const {
        if (!ms || reps < 1 || batch == 0) return PHAST_ERR_INVALID_ARG;
        int rc = check_dev(y_re, y_im, o_re, o_im, frames, batch, out_len, d_work, work_len);
        if (rc) return rc;
        if (work_len < workspace_len(batch) || batch * frames * per() > ((size_t)1 << 39)) return PHAST_ERR_INVALID_ARG;
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
            if ((rc = dev(y_re, y_im, o_re, o_im, frames, batch, out_len, d_work, work_len, st, ev.e))) return rc;
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
static int synthesizer_planner_new(size_t frames, const T *taps, size_t num_taps, size_t channels, size_t hop, size_t first,
                                   size_t out_len, int complex_output, P **out) {
    if (!out) return PHAST_ERR_INVALID_ARG;
    *out = nullptr;
    if (!taps || synth_bad_args(frames, num_taps, channels, hop, first, out_len))  // before the device is touched
        return PHAST_ERR_INVALID_ARG;
    auto *p = new (std::nothrow) P();
    if (!p) return PHAST_ERR_ALLOC;
    int rc = p->init(frames, taps, num_taps, channels, hop, first, out_len, complex_output);
    if (rc) {
        delete p;
        return rc;
    }
    *out = p;
    return PHAST_OK;
}

}  // namespace phast
