// planner_conv.hpp -- ConvPlanner<T>: overlap-save FIR convolution and correlation of real signals (conv.hpp).
// It holds one AnyRealPlanner<T>(B), the device copy of the filter's spectrum H^ and the geometry: immutable after init, no
// per-call state.  A call runs, per chunk of segments, the segment sweep (conv.hip) into workspace rows, the real planner's
// own R2C of those rows into two workspace planes, the spectrum sweep on the planes, the real planner's C2R back into the
// rows and the save sweep into the caller's output.  The caller's workspace holds, per segment, a row of fd >= B elements
// (B rounded up to 16 bytes: even, as the power-of-two R2C / C2R needs, and every row 16-byte aligned), two plane rows of
// bd >= B / 2 + 1 elements (rounded up likewise) and the real planner's workspace.
#pragma once

#include <type_traits>

#include "conv.hpp"
#include "planner_any_real.hpp"

namespace phast {

template <typename T> struct ConvPlanner {
    static constexpr size_t V = 16 / sizeof(T);
    size_t len = 0, k = 0, b = 0, s = 0;  // L, K, B and the hop S = B - K + 1
    size_t t0 = 0, out_len = 0, segs = 0, bins = 0, fd = 0, bd = 0;
    int mode = 0, flip = 0;
    T *d_h = nullptr;  // H^: bd real parts, then bd imaginary parts; zeros beyond the bins
    std::unique_ptr<AnyRealPlanner<T>> real;

    ~ConvPlanner() {
        if (!d_h) return;
        DeviceGuard on(real ? real->device : -1);
        hipFree(d_h);
    }

    // `taps`: K host values; the arguments were checked by conv_bad_args
    int init(size_t signal_len, const T *taps, size_t num_taps, int mode_, int flip_, size_t block) {
        len = signal_len;
        k = num_taps;
        mode = mode_;
        flip = flip_;
        b = block ? block : (size_t)conv_auto_block(len, k);
        s = b - k + 1;
        t0 = (size_t)conv_t0(k, mode);
        out_len = (size_t)conv_out_len(len, k, mode);
        segs = (size_t)conv_segments(out_len, k, b);
        bins = b / 2 + 1;
        fd = (size_t)conv_row(b, V);
        bd = (size_t)conv_row(bins, V);
        real.reset(new (std::nothrow) AnyRealPlanner<T>());
        if (!real) return PHAST_ERR_ALLOC;
        int rc = real->init(b);
        if (rc) return rc;
        // H^ in f64 from the f64-widened taps, then rounded to T: an f32 planner's table carries no f32 transform error
        std::vector<double> g(b, 0.0), h_re(bins), h_im(bins);
        for (size_t j = 0; j < k; ++j) g[j] = (double)taps[flip ? k - 1 - j : j];
        if constexpr (std::is_same<T, double>::value) {
            rc = real->host(false, g.data(), b, nullptr, 0, h_re.data(), bins, h_im.data(), bins);
        } else {
            AnyRealPlanner<double> wide;
            rc = wide.init(b);
            if (!rc) rc = wide.host(false, g.data(), b, nullptr, 0, h_re.data(), bins, h_im.data(), bins);
        }
        if (rc) return rc;
        std::vector<T> h(2 * bd, T(0));
        for (size_t j = 0; j < bins; ++j) {
            h[j] = (T)h_re[j];
            h[bd + j] = (T)h_im[j];
        }
        PHAST_ON_DEVICE(real->device);
        PHAST_HIP(hipMalloc(reinterpret_cast<void **>(&d_h), 2 * bd * sizeof(T)));
        PHAST_HIP(hipMemcpy(d_h, h.data(), 2 * bd * sizeof(T), hipMemcpyHostToDevice));
        return PHAST_OK;
    }

    // elements of T per segment, and V - 1 more to align the caller's base to 16 bytes
    size_t per() const { return fd + 2 * bd + real->workspace_len(1); }
    size_t workspace_len(size_t batch) const { return (batch ? batch : 1) * segs * per() + (V - 1); }
    size_t workspace_min() const { return per() + (V - 1); }
    size_t device_bytes() const { return real->device_bytes() + 2 * bd * sizeof(T); }
    std::string describe() const {
        static const char *const kModes[] = {"full", "same", "valid"};
        return std::string(flip ? "correlate" : "convolve") + " L=" + std::to_string(len) + " K=" + std::to_string(k) + " " +
               kModes[mode] + " out=" + std::to_string(out_len) + " B=" + std::to_string(b) + " S=" + std::to_string(s) +
               " segments=" + std::to_string(segs) + " around " + real->describe();
    }

    // the checks of a _dev call, before the device is touched
    int check_dev(const T *sig, const T *out, size_t signal_len, size_t batch, size_t sig_dist, size_t out_dist, const T *d_work,
                  size_t work_len) const {
        if (!sig || !out) return PHAST_ERR_INVALID_ARG;
        if (signal_len != len) return PHAST_ERR_PLANNER_SIZE;
        if (batch > 1 && (sig_dist < len || out_dist < out_len)) return PHAST_ERR_INVALID_ARG;
        if (batch && (!d_work || (reinterpret_cast<uintptr_t>(d_work) % sizeof(T)) || work_len < workspace_min()))
            return PHAST_ERR_INVALID_ARG;
        return PHAST_OK;
    }

    // the caller's workspace from its first 16-byte boundary on; its length in whole segments (a launch's groups < 2^38)
    size_t rows_of(T *d_work, size_t work_len, T **w) const {
        const size_t skip = ((16 - (reinterpret_cast<uintptr_t>(d_work) & 15u)) & 15u) / sizeof(T);
        *w = d_work + skip;
        size_t rows = (work_len - skip) / per();
        const size_t cap = ((size_t)1 << 39) / per();
        return rows > cap ? cap : rows;
    }

    // device pointers, asynchronous on `st`: chunks of whole segments of the flattened (signal, segment) index.
    // ev (time_stages): 6 events around the five stages of a call that fits one chunk
    int dev(const T *sig, T *out, size_t signal_len, size_t batch, size_t sig_dist, size_t out_dist, T *d_work, size_t work_len,
            hipStream_t st, hipEvent_t *ev = nullptr) const {
        int rc = check_dev(sig, out, signal_len, batch, sig_dist, out_dist, d_work, work_len);
        if (rc) return rc;
        if (batch == 0) return PHAST_OK;
        if (batch == 1) {
            sig_dist = len;
            out_dist = out_len;
        }
        PHAST_ON_DEVICE(real->device);
        T *w = nullptr;
        const size_t rows = rows_of(d_work, work_len, &w), total = batch * segs;
        ConvArgs a{};
        a.h_re = d_h;
        a.h_im = d_h + bd;
        a.sig_dist = sig_dist;
        a.out_dist = out_dist;
        a.len = len;
        a.k = k;
        a.b = b;
        a.s = s;
        a.t0 = t0;
        a.out_len = out_len;
        a.segs = segs;
        a.fd = fd;
        a.bd = bd;
        const size_t out_groups = (out_len + V - 1) / V;  // groups of a signal's output
        for (size_t q0 = 0; q0 < total; q0 += rows) {
            const size_t c = total - q0 < rows ? total - q0 : rows;
            T *row = w, *re = w + c * fd, *im = re + c * bd, *rw = im + c * bd;
            a.q0 = q0;
            a.q1 = q0 + c;
            a.in = sig;
            a.out = row;
            a.gpt = (unsigned)(fd / V);
            a.groups = c * a.gpt;
            if (ev) PHAST_HIP(hipEventRecord(ev[0], st));
            PHAST_HIP(launch_conv<T>(kConvSegment, a, st));
            if (ev) PHAST_HIP(hipEventRecord(ev[1], st));
            rc = real->dev(false, row, nullptr, re, im, b, c, fd, bd, rw, real->workspace_len(c), st);
            if (rc) return rc;
            if (ev) PHAST_HIP(hipEventRecord(ev[2], st));
            a.re = re;
            a.im = im;
            a.gpt = (unsigned)(bd / V);
            a.groups = c * a.gpt;
            PHAST_HIP(launch_conv<T>(kConvSpectrum, a, st));
            if (ev) PHAST_HIP(hipEventRecord(ev[3], st));
            rc = real->dev(true, re, im, row, nullptr, b, c, bd, fd, rw, real->workspace_len(c), st);
            if (rc) return rc;
            if (ev) PHAST_HIP(hipEventRecord(ev[4], st));
            // the output groups that hold a sample of segments [q0, q0 + c): from the first sample of the first segment to
            // the last sample of the last one, in the flattened (signal, group) index
            const size_t b_lo = q0 / segs, s_lo = q0 % segs, b_hi = (q0 + c - 1) / segs, s_hi = (q0 + c - 1) % segs;
            const size_t i_end = ((s_hi + 1) * s < out_len ? (s_hi + 1) * s : out_len) - 1;
            a.in = row;
            a.out = out;
            a.gpt = (unsigned)out_groups;
            a.first = b_lo * out_groups + s_lo * s / V;
            a.groups = b_hi * out_groups + i_end / V - a.first + 1;
            PHAST_HIP(launch_conv<T>(kConvSave, a, st));
            if (ev) PHAST_HIP(hipEventRecord(ev[5], st));
        }
        return PHAST_OK;
    }

    // host slices: one signal through device buffers of the call's own (signal, output, the workspace of all its segments)
    // on the null stream; blocking
    int host(const T *sig, size_t sig_len, T *out, size_t o_len) const {
        if (!sig || !out) return PHAST_ERR_INVALID_ARG;
        if (sig_len != len) return PHAST_ERR_PLANNER_SIZE;
        if (o_len != out_len) return PHAST_ERR_LEN_MISMATCH;
        PHAST_ON_DEVICE(real->device);
        auto up = [](size_t n) { return (n + 3) & ~(size_t)3; };  // every part 16-byte aligned
        const size_t ns = up(len), no = up(out_len), nw = workspace_len(1);
        DevBuf buf;
        int rc = buf.alloc((ns + no + nw) * sizeof(T));
        if (rc) return rc;
        T *d_sig = reinterpret_cast<T *>(buf.p), *d_out = d_sig + ns, *d_w = d_out + no;
        PHAST_HIP(hipMemcpy(d_sig, sig, len * sizeof(T), hipMemcpyHostToDevice));
        rc = dev(d_sig, d_out, len, 1, len, out_len, d_w, nw, nullptr);
        if (rc) return rc;
        PHAST_HIP(hipMemcpy(out, d_out, out_len * sizeof(T), hipMemcpyDeviceToHost));
        return PHAST_OK;
    }

    // measurement hook: ms[0..5) = segment sweep, R2C, spectrum sweep, C2R, save sweep, average milliseconds over `reps` calls
    // of `batch` signals at distances L and out_len in one chunk (work_len >= workspace_len(batch)); blocks
    int time_stages(const T *sig, T *out, size_t batch, T *d_work, size_t work_len, int reps, float *ms, hipStream_t st) const {
        if (!ms || reps < 1 || batch == 0) return PHAST_ERR_INVALID_ARG;
        int rc = check_dev(sig, out, len, batch, len, out_len, d_work, work_len);
        if (rc) return rc;
        if (work_len < workspace_len(batch) || batch * segs * per() > ((size_t)1 << 39)) return PHAST_ERR_INVALID_ARG;
        PHAST_ON_DEVICE(real->device);
        struct Events {
            hipEvent_t e[6] = {};
            ~Events() {
                for (hipEvent_t x : e)
                    if (x) hipEventDestroy(x);
            }
        } ev;
        for (hipEvent_t &x : ev.e) PHAST_HIP(hipEventCreate(&x));
        double acc[5] = {0, 0, 0, 0, 0};
        for (int r = 0; r < reps; ++r) {
            rc = dev(sig, out, len, batch, len, out_len, d_work, work_len, st, ev.e);
            if (rc) return rc;
            PHAST_HIP(hipStreamSynchronize(st));
            for (int i = 0; i < 5; ++i) {
                float t = 0;
                PHAST_HIP(hipEventElapsedTime(&t, ev.e[i], ev.e[i + 1]));
                acc[i] += t;
            }
        }
        for (int i = 0; i < 5; ++i) ms[i] = (float)(acc[i] / reps);
        return PHAST_OK;
    }
};

template <typename T, typename P>
static int conv_planner_new(size_t signal_len, const T *taps, size_t num_taps, int mode, int flip, size_t block, P **out) {
    if (!out) return PHAST_ERR_INVALID_ARG;
    *out = nullptr;
    if (!taps || conv_bad_args(signal_len, num_taps, mode, flip, block, 16 / sizeof(T)))  // before the device is touched
        return PHAST_ERR_INVALID_ARG;
    auto *p = new (std::nothrow) P();
    if (!p) return PHAST_ERR_ALLOC;
    int rc = p->init(signal_len, taps, num_taps, mode, flip, block);
    if (rc) {
        delete p;
        return rc;
    }
    *out = p;
    return PHAST_OK;
}

}  // namespace phast
