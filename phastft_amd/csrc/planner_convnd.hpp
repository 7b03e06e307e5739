// planner_convnd.hpp -- ConvNdPlanner<T>: overlap-save convolution and correlation of real arrays of rank 1 .. 3
// (convnd.hpp).  It holds one RealNdPlanner<T> of the tile shape, the device copy of the filter's spectrum H^
// and the geometry: immutable after init, no per-call state.  A call runs, per chunk of tiles, the tile sweep (convnd.hip)
// into workspace rows, the N-d planner's own R2C of those rows into two workspace planes, conv.hip's spectrum sweep on the
// planes, the N-d planner's C2R back into the rows and the save sweep into the caller's output.  The caller's workspace
// holds, per tile, a row of fd >= prod B elements (rounded up to 16 bytes: every tile 16-byte aligned, its distance even),
// two plane rows of bd >= the half spectrum's points (rounded up likewise) and the N-d planner's workspace.
#pragma once

#include <type_traits>

#include "convnd.hpp"
#include "planner_nd.hpp"

namespace phast {

template <typename T> struct ConvNdPlanner {
    static constexpr size_t V = 16 / sizeof(T);
    ConvNdGeom g{};
    size_t rank = 0;  // the caller's
    size_t sig_pts = 0, out_pts = 0, tiles = 0, pts = 0, cx = 0, fd = 0, bd = 0;
    int mode = 0, flip = 0;
    T *d_h = nullptr;  // H^: bd real parts, then bd imaginary parts; zeros beyond the half spectrum
    std::unique_ptr<RealNdPlanner<T>> nd;

    ~ConvNdPlanner() {
        if (!d_h) return;
        DeviceGuard on(nd ? nd->device : -1);
        hipFree(d_h);
    }

    // `taps`: prod K host values, row-major; the arguments were checked by convnd_bad_args, which made `geom`
    int init(const ConvNdGeom &geom, size_t rank_, const T *taps, int mode_, int flip_) {
        g = geom;
        rank = rank_;
        mode = mode_;
        flip = flip_;
        sig_pts = (size_t)g.sig_pts;
        out_pts = (size_t)g.out_pts;
        tiles = (size_t)g.tiles;
        pts = (size_t)g.tile_pts;
        size_t dims[kConvNdMaxRank];
        for (unsigned i = 0; i < g.rank; ++i) dims[i] = (size_t)g.b[kConvNdMaxRank - g.rank + i];
        nd.reset(new (std::nothrow) RealNdPlanner<T>());
        if (!nd) return PHAST_ERR_ALLOC;
        int rc = nd->init(dims, g.rank);
        if (rc) return rc;
        cx = (size_t)nd->total_cx;
        fd = (size_t)conv_row(pts, V);
        bd = (size_t)conv_row(cx, V);
        // H^ in f64 from the f64-widened taps, then rounded to T: an f32 planner's table carries no f32 transform error
        std::vector<double> gp(pts, 0.0), h_re(cx), h_im(cx);
        const size_t k0 = (size_t)g.k[0], k1 = (size_t)g.k[1], k2 = (size_t)g.k[2];
        for (size_t a = 0; a < k0; ++a)
            for (size_t b = 0; b < k1; ++b)
                for (size_t c = 0; c < k2; ++c) {
                    const size_t src = flip ? ((k0 - 1 - a) * k1 + (k1 - 1 - b)) * k2 + (k2 - 1 - c) : (a * k1 + b) * k2 + c;
                    gp[(a * (size_t)g.b[1] + b) * (size_t)g.b[2] + c] = (double)taps[src];
                }
        if constexpr (std::is_same<T, double>::value) {
            rc = nd->host(false, gp.data(), pts, nullptr, 0, h_re.data(), cx, h_im.data(), cx);
        } else {
            RealNdPlanner<double> wide;
            rc = wide.init(dims, g.rank);
            if (!rc) rc = wide.host(false, gp.data(), pts, nullptr, 0, h_re.data(), cx, h_im.data(), cx);
        }
        if (rc) return rc;
        std::vector<T> h(2 * bd, T(0));
        for (size_t j = 0; j < cx; ++j) {
            h[j] = (T)h_re[j];
            h[bd + j] = (T)h_im[j];
        }
        PHAST_ON_DEVICE(nd->device);
        PHAST_HIP(hipMalloc(reinterpret_cast<void **>(&d_h), 2 * bd * sizeof(T)));
        PHAST_HIP(hipMemcpy(d_h, h.data(), 2 * bd * sizeof(T), hipMemcpyHostToDevice));
        return PHAST_OK;
    }

    // the caller's axes: the output shape and the blocks (a dropped axis: 1)
    void out_dims(size_t *d) const { spread(g.out, d); }
    void block(size_t *d) const { spread(g.b, d); }
    void spread(const unsigned long long *v, size_t *d) const {
        for (size_t i = 0; i < rank; ++i) d[i] = 1;
        for (unsigned i = kConvNdMaxRank - g.rank; i < kConvNdMaxRank; ++i) d[g.axis_of[i]] = (size_t)v[i];
    }

    // elements of T per tile, and V - 1 more to align the caller's base to 16 bytes
    size_t nd_work() const { return nd->workspace_len(1); }
    size_t per() const { return fd + 2 * bd + nd_work(); }
    size_t workspace_len(size_t batch) const { return (batch ? batch : 1) * tiles * per() + (V - 1); }
    size_t workspace_min() const { return per() + (V - 1); }
    size_t device_bytes() const { return nd->device_bytes() + 2 * bd * sizeof(T); }
    std::string describe() const {
        static const char *const kModes[] = {"full", "same", "valid"};
        auto shape = [&](const unsigned long long *v) {
            std::string s = "[";
            for (unsigned i = kConvNdMaxRank - g.rank; i < kConvNdMaxRank; ++i)
                s += (i > kConvNdMaxRank - g.rank ? "x" : "") + std::to_string(v[i]);
            return s + "]";
        };
        return std::string(flip ? "correlate" : "convolve") + " nd L=" + shape(g.len) + " K=" + shape(g.k) + " " + kModes[mode] +
               " out=" + shape(g.out) + " B=" + shape(g.b) + " S=" + shape(g.s) + " tiles=" + shape(g.segs) + " around " +
               nd->describe();
    }

    // the checks of a _dev call, before the device is touched
    int check_dev(const T *sig, const T *out, size_t signal_len, size_t batch, size_t sig_dist, size_t out_dist, const T *d_work,
                  size_t work_len) const {
        if (!sig || !out) return PHAST_ERR_INVALID_ARG;
        if (signal_len != sig_pts) return PHAST_ERR_PLANNER_SIZE;
        if (batch > 1 && (sig_dist < sig_pts || out_dist < out_pts)) return PHAST_ERR_INVALID_ARG;
        if (batch && (!d_work || (reinterpret_cast<uintptr_t>(d_work) % sizeof(T)) || work_len < workspace_min()))
            return PHAST_ERR_INVALID_ARG;
        return PHAST_OK;
    }

    // the caller's workspace from its first 16-byte boundary on; its length in whole tiles (a launch's groups < 2^38)
    size_t rows_of(T *d_work, size_t work_len, T **w) const {
        const size_t skip = ((16 - (reinterpret_cast<uintptr_t>(d_work) & 15u)) & 15u) / sizeof(T);
        *w = d_work + skip;
        size_t rows = (work_len - skip) / per();
        const size_t cap = ((size_t)1 << 39) / per();
        return rows > cap ? cap : rows;
    }

    // device pointers, asynchronous on `st`: chunks of whole tiles of the flattened (array, tile) index.
    // ev (time_stages): 6 events around the five stages of a call that fits one chunk
    int dev(const T *sig, T *out, size_t signal_len, size_t batch, size_t sig_dist, size_t out_dist, T *d_work, size_t work_len,
            hipStream_t st, hipEvent_t *ev = nullptr) const {
        int rc = check_dev(sig, out, signal_len, batch, sig_dist, out_dist, d_work, work_len);
        if (rc) return rc;
        if (batch == 0) return PHAST_OK;
        if (batch == 1) {
            sig_dist = sig_pts;
            out_dist = out_pts;
        }
        PHAST_ON_DEVICE(nd->device);
        T *w = nullptr;
        const size_t rows = rows_of(d_work, work_len, &w), total = batch * tiles;
        ConvNdArgs a{};
        a.sig_dist = sig_dist;
        a.out_dist = out_dist;
        a.fd = fd;
        a.tiles = (unsigned)tiles;
        a.pts = (unsigned)pts;
        for (unsigned i = 0; i < kConvNdMaxRank; ++i) {
            a.len[i] = (unsigned)g.len[i];
            a.k1[i] = (unsigned)(g.k[i] - 1);
            a.b[i] = (unsigned)g.b[i];
            a.s[i] = (unsigned)g.s[i];
            a.t0[i] = (unsigned)g.t0[i];
            a.n_out[i] = (unsigned)g.out[i];
            a.segs[i] = (unsigned)g.segs[i];
        }
        ConvArgs sp{};  // conv.hip's spectrum sweep: a tile's half spectrum is one row of bd elements
        sp.h_re = d_h;
        sp.h_im = d_h + bd;
        sp.bd = bd;
        sp.gpt = (unsigned)(bd / V);
        const unsigned gpr = (unsigned)convnd_save_groups(g.s[2], V);
        for (size_t q0 = 0; q0 < total; q0 += rows) {
            const size_t c = total - q0 < rows ? total - q0 : rows;
            T *row = w, *re = w + c * fd, *im = re + c * bd, *rw = im + c * bd;
            const size_t rw_len = c * nd_work();
            a.q0 = q0;
            a.q1 = q0 + c;
            a.in = sig;
            a.out = row;
            a.gpt = (unsigned)(fd / V);
            a.groups = c * a.gpt;
            if (ev) PHAST_HIP(hipEventRecord(ev[0], st));
            PHAST_HIP(launch_convnd<T>(kConvNdTile, a, st));
            if (ev) PHAST_HIP(hipEventRecord(ev[1], st));
            rc = nd->dev(false, row, nullptr, re, im, pts, c, fd, bd, rw, rw_len, st);
            if (rc) return rc;
            if (ev) PHAST_HIP(hipEventRecord(ev[2], st));
            sp.re = re;
            sp.im = im;
            sp.groups = c * sp.gpt;
            PHAST_HIP(launch_conv<T>(kConvSpectrum, sp, st));
            if (ev) PHAST_HIP(hipEventRecord(ev[3], st));
            rc = nd->dev(true, re, im, row, nullptr, pts, c, bd, fd, rw, rw_len, st);
            if (rc) return rc;
            if (ev) PHAST_HIP(hipEventRecord(ev[4], st));
            a.in = row;
            a.out = out;
            a.gpr = gpr;
            a.gpt = (unsigned)(g.s[0] * g.s[1] * gpr);
            a.groups = c * a.gpt;
            PHAST_HIP(launch_convnd<T>(kConvNdSave, a, st));
            if (ev) PHAST_HIP(hipEventRecord(ev[5], st));
        }
        return PHAST_OK;
    }

    // host slices: one array through device buffers of the call's own (array, output, the workspace of all its tiles) on the
    // null stream; blocking
    int host(const T *sig, size_t sig_len, T *out, size_t o_len) const {
        if (!sig || !out) return PHAST_ERR_INVALID_ARG;
        if (sig_len != sig_pts) return PHAST_ERR_PLANNER_SIZE;
        if (o_len != out_pts) return PHAST_ERR_LEN_MISMATCH;
        PHAST_ON_DEVICE(nd->device);
        auto up = [](size_t n) { return (n + 3) & ~(size_t)3; };  // every part 16-byte aligned
        const size_t ns = up(sig_pts), no = up(out_pts), nw = workspace_len(1);
        DevBuf buf;
        int rc = buf.alloc((ns + no + nw) * sizeof(T));
        if (rc) return rc;
        T *d_sig = reinterpret_cast<T *>(buf.p), *d_out = d_sig + ns, *d_w = d_out + no;
        PHAST_HIP(hipMemcpy(d_sig, sig, sig_pts * sizeof(T), hipMemcpyHostToDevice));
        rc = dev(d_sig, d_out, sig_pts, 1, sig_pts, out_pts, d_w, nw, nullptr);
        if (rc) return rc;
        PHAST_HIP(hipMemcpy(out, d_out, out_pts * sizeof(T), hipMemcpyDeviceToHost));
        return PHAST_OK;
    }

    // measurement hook: ms[0..5) = tile sweep, R2C, spectrum sweep, C2R, save sweep, average milliseconds over `reps` calls of
    // `batch` arrays at distances prod L and prod out in one chunk (work_len >= workspace_len(batch)); blocks
    int time_stages(const T *sig, T *out, size_t batch, T *d_work, size_t work_len, int reps, float *ms, hipStream_t st) const {
        if (!ms || reps < 1 || batch == 0) return PHAST_ERR_INVALID_ARG;
        int rc = check_dev(sig, out, sig_pts, batch, sig_pts, out_pts, d_work, work_len);
        if (rc) return rc;
        if (work_len < workspace_len(batch) || batch * tiles * per() > ((size_t)1 << 39)) return PHAST_ERR_INVALID_ARG;
        PHAST_ON_DEVICE(nd->device);
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
            rc = dev(sig, out, sig_pts, batch, sig_pts, out_pts, d_work, work_len, st, ev.e);
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
static int convnd_planner_new(const size_t *signal_dims, const size_t *tap_dims, size_t rank, const T *taps, int mode, int flip,
                              const size_t *block, P **out) {
    if (!out) return PHAST_ERR_INVALID_ARG;
    *out = nullptr;
    ConvNdGeom g{};
    if (!taps || convnd_bad_args(signal_dims, tap_dims, rank, mode, flip, block, 16 / sizeof(T), &g))  // before the device is touched
        return PHAST_ERR_INVALID_ARG;
    auto *p = new (std::nothrow) P();
    if (!p) return PHAST_ERR_ALLOC;
    int rc = p->init(g, rank, taps, mode, flip);
    if (rc) {
        delete p;
        return rc;
    }
    *out = p;
    return PHAST_OK;
}

}  // namespace phast
