// planner_resample.hpp -- the two planners of sample-rate conversion (resample.hpp).
//
// UpfirdnPlanner<T>: the polyphase FIR of scipy.signal.upfirdn.  It holds the taps on the device, phase-major (up rows of Kp
// at a stride of Kp | 1, zeros behind a row's last tap), and the schedule of the kernel: immutable after init, no per-call state.  A call is one
// launch from the caller's signals into the caller's outputs; it needs no workspace (workspace_len is 0, and the _dev call
// takes any d_work, null included).
//
// ResamplePlanner<T>: the Fourier method of scipy.signal.resample.  It holds one AnyRealPlanner<T>(L) and, unless num = L,
// one of num.  A call runs, per chunk of whole signals, the R2C of L from the caller's signals into two workspace planes,
// the spectrum sweep into two more planes and the C2R of num into the caller's output.  The caller's workspace, from its
// first 16-byte boundary on, for a chunk of c signals:
//     X         2 c xd     xd = L / 2 + 1 rounded up to 16 bytes
//     Y         2 c yd     yd = num / 2 + 1 rounded up to 16 bytes
//     real      the larger of the two real planners' workspace_len(c)
// workspace_len(batch) holds the batch in one chunk; any length >= workspace_min() (one signal) runs the largest chunk that
// fits.  A signal never straddles two chunks.
#pragma once

#include <vector>

#include "planner_any_real.hpp"
#include "resample.hpp"

namespace phast {

template <typename T> struct UpfirdnPlanner {
    size_t len = 0, k = 0, up = 1, down = 1, first = 0, out_len = 0, full_len = 0, kp = 0, ts = 0, tiles = 0;
    UpfirdnGeom geom{};
    int device = -1;
    T *d_taps = nullptr;  // up rows of kp, ts = kp | 1 apart

    ~UpfirdnPlanner() {
        if (!d_taps) return;
        DeviceGuard on(device);
        hipFree(d_taps);
    }

    // `taps`: K host values; the arguments were checked by upfirdn_bad_args
    int init(size_t signal_len, const T *taps, size_t num_taps, size_t up_, size_t down_, size_t first_, size_t out_len_) {
        len = signal_len;
        k = num_taps;
        up = up_;
        down = down_;
        first = first_;
        full_len = (size_t)upfirdn_full_len(len, k, up, down);
        out_len = out_len_ ? out_len_ : full_len - first;
        kp = (size_t)upfirdn_kp(k, up);
        geom = upfirdn_geom(k, up, down);
        tiles = (out_len + geom.tile - 1) / geom.tile;
        ts = (size_t)upfirdn_table_stride(kp);
        std::vector<T> rows(up * ts, T(0));
        for (size_t i = 0; i < k; ++i) rows[(i % up) * ts + i / up] = taps[i];
        int rc = ensure_device(&device);
        if (rc) return rc;
        PHAST_HIP(hipMalloc(reinterpret_cast<void **>(&d_taps), rows.size() * sizeof(T)));
        PHAST_HIP(hipMemcpy(d_taps, rows.data(), rows.size() * sizeof(T), hipMemcpyHostToDevice));
        return PHAST_OK;
    }

    size_t workspace_len(size_t) const { return 0; }
    size_t workspace_min() const { return 0; }
    size_t device_bytes() const { return up * ts * sizeof(T); }
    std::string describe() const {
        return "upfirdn L=" + std::to_string(len) + " K=" + std::to_string(k) + " up=" + std::to_string(up) + " down=" +
               std::to_string(down) + " first=" + std::to_string(first) + " out=" + std::to_string(out_len) + " of " +
               std::to_string(full_len) + ": Kp=" + std::to_string(kp) + " tile=" + std::to_string(geom.tile) + " chunk=" +
               std::to_string(geom.jc) + " x " + std::to_string(geom.rows) + (geom.by_phase ? " phase rows" : " output rows");
    }

    // the checks of a _dev call, before the device is touched
    int check_dev(const T *sig, const T *out, size_t signal_len, size_t batch, size_t sig_dist, size_t out_dist) const {
        if (!sig || !out) return PHAST_ERR_INVALID_ARG;
        if (signal_len != len) return PHAST_ERR_PLANNER_SIZE;
        if (batch > 1 && (sig_dist < len || out_dist < out_len)) return PHAST_ERR_INVALID_ARG;
        if (batch > ((size_t)1 << 40) / tiles) return PHAST_ERR_INVALID_ARG;
        return PHAST_OK;
    }

    // device pointers, asynchronous on `st`: signal b at sig + b sig_dist, its out_len outputs at out + b out_dist
    int dev(const T *sig, T *out, size_t signal_len, size_t batch, size_t sig_dist, size_t out_dist, hipStream_t st) const {
        int rc = check_dev(sig, out, signal_len, batch, sig_dist, out_dist);
        if (rc) return rc;
        if (batch == 0) return PHAST_OK;
        if (batch == 1) {
            sig_dist = len;
            out_dist = out_len;
        }
        PHAST_ON_DEVICE(device);
        UpfirdnArgs a{};
        a.x = sig;
        a.out = out;
        a.taps = d_taps;
        a.sig_dist = sig_dist;
        a.out_dist = out_dist;
        a.len = len;
        a.kp = kp;
        a.ts = ts;
        a.up = up;
        a.down = down;
        a.first = first;
        a.out_len = out_len;
        a.tiles = tiles;
        a.groups = batch * tiles * 256;
        a.dq = 256 * down / up;
        a.dp = 256 * down % up;
        a.geom = geom;
        PHAST_HIP(launch_upfirdn<T>(a, st));
        return PHAST_OK;
    }

    // host slices: one signal through device buffers of the call's own on the null stream; blocking
    int host(const T *sig, size_t sig_len, T *out, size_t o_len) const {
        if (!sig || !out) return PHAST_ERR_INVALID_ARG;
        if (sig_len != len) return PHAST_ERR_PLANNER_SIZE;
        if (o_len != out_len) return PHAST_ERR_LEN_MISMATCH;
        PHAST_ON_DEVICE(device);
        DevBuf buf;
        int rc = buf.alloc((len + out_len) * sizeof(T));
        if (rc) return rc;
        T *d_sig = reinterpret_cast<T *>(buf.p), *d_out = d_sig + len;
        PHAST_HIP(hipMemcpy(d_sig, sig, len * sizeof(T), hipMemcpyHostToDevice));
        rc = dev(d_sig, d_out, len, 1, len, out_len, nullptr);
        if (rc) return rc;
        PHAST_HIP(hipMemcpy(out, d_out, out_len * sizeof(T), hipMemcpyDeviceToHost));
        return PHAST_OK;
    }

    // measurement hook: ms[0] = average milliseconds of the kernel over `reps` calls of `batch` signals at distances L and
    // out_len; blocks
    int time_stages(const T *sig, T *out, size_t batch, int reps, float *ms, hipStream_t st) const {
        if (!ms || reps < 1 || batch == 0) return PHAST_ERR_INVALID_ARG;
        int rc = check_dev(sig, out, len, batch, len, out_len);
        if (rc) return rc;
        PHAST_ON_DEVICE(device);
        struct Events {
            hipEvent_t e[2] = {};
            ~Events() {
                for (hipEvent_t x : e)
                    if (x) hipEventDestroy(x);
            }
        } ev;
        for (hipEvent_t &x : ev.e) PHAST_HIP(hipEventCreate(&x));
        PHAST_HIP(hipEventRecord(ev.e[0], st));
        for (int r = 0; r < reps; ++r)
            if ((rc = dev(sig, out, len, batch, len, out_len, st))) return rc;
        PHAST_HIP(hipEventRecord(ev.e[1], st));
        PHAST_HIP(hipStreamSynchronize(st));
        float t = 0;
        PHAST_HIP(hipEventElapsedTime(&t, ev.e[0], ev.e[1]));
        ms[0] = t / (float)reps;
        return PHAST_OK;
    }
};

template <typename T, typename P>
static int upfirdn_planner_new(size_t signal_len, const T *taps, size_t num_taps, size_t up, size_t down, size_t first,
                               size_t out_len, P **out) {
    if (!out) return PHAST_ERR_INVALID_ARG;
    *out = nullptr;
    if (!taps || upfirdn_bad_args(signal_len, num_taps, up, down, first, out_len))  // before the device is touched
        return PHAST_ERR_INVALID_ARG;
    auto *p = new (std::nothrow) P();
    if (!p) return PHAST_ERR_ALLOC;
    int rc = p->init(signal_len, taps, num_taps, up, down, first, out_len);
    if (rc) {
        delete p;
        return rc;
    }
    *out = p;
    return PHAST_OK;
}

template <typename T> struct ResamplePlanner {
    static constexpr size_t V = 16 / sizeof(T);
    size_t len = 0, num = 0, xd = 0, yd = 0, bins = 0;
    double scale = 1, last = 1;
    std::unique_ptr<AnyRealPlanner<T>> fwd, own_inv;  // of L; of num unless num = L
    const AnyRealPlanner<T> *inv = nullptr;

    int init(size_t signal_len, size_t num_) {
        len = signal_len;
        num = num_;
        xd = (len / 2 + 1 + V - 1) / V * V;
        yd = (num / 2 + 1 + V - 1) / V * V;
        bins = (size_t)resample_bins(len, num);
        scale = (double)num / (double)len;
        last = scale * resample_nyquist(len, num);
        fwd.reset(new (std::nothrow) AnyRealPlanner<T>());
        if (!fwd) return PHAST_ERR_ALLOC;
        int rc = fwd->init(len);
        if (rc) return rc;
        inv = fwd.get();
        if (num != len) {
            own_inv.reset(new (std::nothrow) AnyRealPlanner<T>());
            if (!own_inv) return PHAST_ERR_ALLOC;
            if ((rc = own_inv->init(num))) return rc;
            inv = own_inv.get();
        }
        return PHAST_OK;
    }

    size_t real_len(size_t c) const {
        const size_t a = fwd->workspace_len(c), b = inv->workspace_len(c);
        return a > b ? a : b;
    }
    // elements of T of a chunk of c signals (and V - 1 more to align the caller's base)
    size_t need(size_t c) const { return 2 * c * (xd + yd) + real_len(c) + (V - 1); }
    size_t workspace_len(size_t batch) const { return need(batch ? batch : 1); }
    size_t workspace_min() const { return need(1); }
    size_t device_bytes() const { return fwd->device_bytes() + (own_inv ? own_inv->device_bytes() : 0); }
    std::string describe() const {
        return "resample L=" + std::to_string(len) + " num=" + std::to_string(num) + " bins=" + std::to_string(bins) + ": " +
               fwd->describe() + (own_inv ? " -> " + own_inv->describe() : std::string(" (both ways)"));
    }

    int check_dev(const T *sig, const T *out, size_t signal_len, size_t batch, size_t sig_dist, size_t out_dist, const T *d_work,
                  size_t work_len) const {
        if (!sig || !out) return PHAST_ERR_INVALID_ARG;
        if (signal_len != len) return PHAST_ERR_PLANNER_SIZE;
        if (batch > 1 && (sig_dist < len || out_dist < num)) return PHAST_ERR_INVALID_ARG;
        // the power-of-two real transforms move the real side as (even, odd) pairs: a batch needs an even distance there
        if (batch > 1 && ((fwd->pow2() && sig_dist % 2) || (inv->pow2() && out_dist % 2))) return PHAST_ERR_INVALID_ARG;
        if (batch && (!d_work || (reinterpret_cast<uintptr_t>(d_work) % sizeof(T)) || work_len < workspace_min()))
            return PHAST_ERR_INVALID_ARG;
        return PHAST_OK;
    }

    // the caller's workspace from its first 16-byte boundary on; the signals of a chunk: the most that fit, at least one
    size_t chunk_of(T *d_work, size_t work_len, size_t batch, T **w) const {
        const size_t skip = ((16 - (reinterpret_cast<uintptr_t>(d_work) & 15u)) & 15u) / sizeof(T);
        *w = d_work + skip;
        const size_t avail = work_len - skip + (V - 1);
        size_t lo = 1, hi = batch;  // need() grows with c
        while (lo < hi) {
            const size_t mid = lo + (hi - lo + 1) / 2;
            if (need(mid) <= avail) lo = mid;
            else hi = mid - 1;
        }
        return lo;
    }

    // device pointers, asynchronous on `st`.  ev (time_stages): 4 events around the three stages of a call of one chunk
    int dev(const T *sig, T *out, size_t signal_len, size_t batch, size_t sig_dist, size_t out_dist, T *d_work, size_t work_len,
            hipStream_t st, hipEvent_t *ev = nullptr) const {
        int rc = check_dev(sig, out, signal_len, batch, sig_dist, out_dist, d_work, work_len);
        if (rc) return rc;
        if (batch == 0) return PHAST_OK;
        if (batch == 1) {
            sig_dist = len;
            out_dist = num;
        }
        PHAST_ON_DEVICE(fwd->device);
        T *w = nullptr;
        const size_t chunk = chunk_of(d_work, work_len, batch, &w);
        for (size_t b0 = 0; b0 < batch; b0 += chunk) {
            const size_t c = batch - b0 < chunk ? batch - b0 : chunk;
            T *x_re = w, *x_im = x_re + c * xd, *y_re = x_im + c * xd, *y_im = y_re + c * yd, *rw = y_im + c * yd;
            const size_t rl = real_len(c);
            if (ev) PHAST_HIP(hipEventRecord(ev[0], st));
            rc = fwd->dev(false, sig + b0 * sig_dist, nullptr, x_re, x_im, len, c, sig_dist, xd, rw, rl, st);
            if (rc) return rc;
            if (ev) PHAST_HIP(hipEventRecord(ev[1], st));
            ResampleArgs a{};
            a.x_re = x_re;
            a.x_im = x_im;
            a.y_re = y_re;
            a.y_im = y_im;
            a.xd = xd;
            a.yd = yd;
            a.bins = bins;
            a.zero_im = num % 2 ? ~0ull : num / 2;
            a.scale = scale;
            a.last = last;
            a.gpt = (unsigned)(yd / V);
            a.groups = c * a.gpt;
            PHAST_HIP(launch_resample_spectrum<T>(a, st));
            if (ev) PHAST_HIP(hipEventRecord(ev[2], st));
            rc = inv->dev(true, y_re, y_im, out + b0 * out_dist, nullptr, num, c, yd, out_dist, rw, rl, st);
            if (rc) return rc;
            if (ev) PHAST_HIP(hipEventRecord(ev[3], st));
        }
        return PHAST_OK;
    }

    // host slices: one signal through device buffers of the call's own on the null stream; blocking
    int host(const T *sig, size_t sig_len, T *out, size_t o_len) const {
        if (!sig || !out) return PHAST_ERR_INVALID_ARG;
        if (sig_len != len) return PHAST_ERR_PLANNER_SIZE;
        if (o_len != num) return PHAST_ERR_LEN_MISMATCH;
        PHAST_ON_DEVICE(fwd->device);
        auto up4 = [](size_t n) { return (n + 3) & ~(size_t)3; };  // every part 16-byte aligned
        const size_t ns = up4(len), no = up4(num), nw = workspace_len(1);
        DevBuf buf;
        int rc = buf.alloc((ns + no + nw) * sizeof(T));
        if (rc) return rc;
        T *d_sig = reinterpret_cast<T *>(buf.p), *d_out = d_sig + ns, *d_w = d_out + no;
        PHAST_HIP(hipMemcpy(d_sig, sig, len * sizeof(T), hipMemcpyHostToDevice));
        rc = dev(d_sig, d_out, len, 1, len, num, d_w, nw, nullptr);
        if (rc) return rc;
        PHAST_HIP(hipMemcpy(out, d_out, num * sizeof(T), hipMemcpyDeviceToHost));
        return PHAST_OK;
    }

    // measurement hook: ms[0..3) = R2C, spectrum sweep, C2R, average milliseconds over `reps` calls of `batch` signals at
    // distances L and num in one chunk (work_len >= workspace_len(batch)); blocks
    int time_stages(const T *sig, T *out, size_t batch, T *d_work, size_t work_len, int reps, float *ms, hipStream_t st) const {
        if (!ms || reps < 1 || batch == 0) return PHAST_ERR_INVALID_ARG;
        int rc = check_dev(sig, out, len, batch, len, num, d_work, work_len);
        if (rc) return rc;
        if (work_len < workspace_len(batch)) return PHAST_ERR_INVALID_ARG;
        PHAST_ON_DEVICE(fwd->device);
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
            rc = dev(sig, out, len, batch, len, num, d_work, work_len, st, ev.e);
            if (rc) return rc;
            PHAST_HIP(hipStreamSynchronize(st));
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

template <typename T, typename P> static int resample_planner_new(size_t signal_len, size_t num, P **out) {
    if (!out) return PHAST_ERR_INVALID_ARG;
    *out = nullptr;
    if (resample_bad_args(signal_len, num)) return PHAST_ERR_INVALID_ARG;  // before the device is touched
    auto *p = new (std::nothrow) P();
    if (!p) return PHAST_ERR_ALLOC;
    int rc = p->init(signal_len, num);
    if (rc) {
        delete p;
        return rc;
    }
    *out = p;
    return PHAST_OK;
}

}  // namespace phast
