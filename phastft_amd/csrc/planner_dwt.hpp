// planner_dwt.hpp -- the planner of the discrete wavelet transform (dwt.hpp).
//
// DwtPlanner<T> holds the four filters on the device, interleaved in the order the kernels' loops meet them (2F values for
// the analysis, 2F for the synthesis), and the geometry of the cascade: immutable after init, no per-call state.  wavedec runs
// one analysis launch per level on halving lengths, waverec one synthesis launch per level from J down.  Level l < J writes
// cD_l into the caller's packed row and cA_l into a workspace row; level J writes both bands to the packed row.  The caller's
// workspace, for a chunk of c signals (element alignment is all it needs):
//     rows A    c row_a    the approximations of odd level below J   (row_a = n_1)
//     rows B    c row_b    those of even level below J               (row_b = n_2; none for J = 2)
// (a signal shorter than the filter grows from level to level: a row then holds the longest of its levels).  workspace_len(batch)
// holds the batch in one chunk; any length >= workspace_min() (one signal) runs the largest chunk of whole signals that fits, to
// the same bits.  For J = 1 both are 0 and d_work is not read.
#pragma once

#include <string>
#include <vector>

#include "dwt.hpp"
#include "host_util.hpp"

namespace phast {

template <typename T> struct DwtPlanner {
    size_t len = 0, f = 0, levels = 0;
    int mode = kDwtSymmetric;
    DwtGeom geom{};
    int device = -1;
    T *d_taps = nullptr;  // 4F: the analysis table, then the synthesis table

    ~DwtPlanner() {
        if (!d_taps) return;
        DeviceGuard on(device);
        hipFree(d_taps);
    }

    // the filters: F host values each; the arguments were checked by dwt_bad_args
    int init(size_t signal_len, const T *dec_lo, const T *dec_hi, const T *rec_lo, const T *rec_hi, size_t filter_len,
             size_t level, int mode_) {
        len = signal_len;
        f = filter_len;
        levels = level;
        mode = mode_;
        geom = dwt_geom(len, (unsigned)f, (unsigned)levels, mode);
        const size_t h = f / 2;
        std::vector<T> table(4 * f);
        for (size_t p = 0; p < h; ++p) {  // analysis: taps 2p and 2p + 1, ascending
            table[4 * p + 0] = dec_lo[2 * p];
            table[4 * p + 1] = dec_hi[2 * p];
            table[4 * p + 2] = dec_lo[2 * p + 1];
            table[4 * p + 3] = dec_hi[2 * p + 1];
        }
        for (size_t i = 0; i < h; ++i) {  // synthesis: taps 2d and 2d + 1, d = h - 1 - i descending
            const size_t d = h - 1 - i;
            table[2 * f + 4 * i + 0] = rec_lo[2 * d];
            table[2 * f + 4 * i + 1] = rec_hi[2 * d];
            table[2 * f + 4 * i + 2] = rec_lo[2 * d + 1];
            table[2 * f + 4 * i + 3] = rec_hi[2 * d + 1];
        }
        int rc = ensure_device(&device);
        if (rc) return rc;
        PHAST_HIP(hipMalloc(reinterpret_cast<void **>(&d_taps), table.size() * sizeof(T)));
        PHAST_HIP(hipMemcpy(d_taps, table.data(), table.size() * sizeof(T), hipMemcpyHostToDevice));
        return PHAST_OK;
    }

    size_t per() const { return (size_t)(geom.row_a + geom.row_b); }
    size_t workspace_len(size_t batch) const { return (batch ? batch : 1) * per(); }
    size_t workspace_min() const { return per(); }
    size_t coeff_len() const { return (size_t)geom.coeff_len; }
    size_t level_len(size_t l) const { return l <= levels ? (size_t)geom.n[l] : 0; }
    size_t level_offset(size_t l) const { return l <= levels ? (size_t)geom.off[l] : 0; }
    size_t device_bytes() const { return 4 * f * sizeof(T); }
    std::string describe() const {
        static const char *names[] = {"zero", "constant", "symmetric", "reflect", "periodic", "periodization"};
        std::string s = "dwt L=" + std::to_string(len) + " F=" + std::to_string(f) + " J=" + std::to_string(levels) + " mode=" +
                        names[mode] + " coeffs=" + std::to_string(geom.coeff_len) + " tile=" + std::to_string(geom.tile) + " levels";
        for (size_t l = 1; l <= levels; ++l) s += (l == 1 ? " " : ",") + std::to_string(geom.n[l]);
        return s + " work=" + std::to_string(per());
    }

    // the checks of a _dev call, before the device is touched
    int check_dev(const T *sig, const T *coeffs, size_t signal_len, size_t batch, size_t sig_dist, size_t coeff_dist,
                  const T *d_work, size_t work_len) const {
        if (!sig || !coeffs || sig == coeffs) return PHAST_ERR_INVALID_ARG;
        if (signal_len != len) return PHAST_ERR_PLANNER_SIZE;
        if (batch > 1 && (sig_dist < len || coeff_dist < coeff_len())) return PHAST_ERR_INVALID_ARG;
        if (batch > ((size_t)1 << 40) / ((len + geom.tile - 1) / geom.tile)) return PHAST_ERR_INVALID_ARG;
        if (batch && per() && (!d_work || (reinterpret_cast<uintptr_t>(d_work) % sizeof(T)) || work_len < per()))
            return PHAST_ERR_INVALID_ARG;
        return PHAST_OK;
    }

    // the rows of level l's approximation in a chunk of c signals, and the distance between them
    T *row(T *w, size_t c, size_t l, size_t *dist) const {
        *dist = (size_t)(l % 2 ? geom.row_a : geom.row_b);
        return l % 2 ? w : w + c * (size_t)geom.row_a;
    }

    // device pointers, asynchronous on `st`.  inverse = false: signal b at sig + b sig_dist -> its packed row at
    // coeffs + b coeff_dist; inverse = true: the other way.  The input is not written.
    int dev(bool inverse, T *sig, T *coeffs, size_t signal_len, size_t batch, size_t sig_dist, size_t coeff_dist, T *d_work,
            size_t work_len, hipStream_t st) const {
        int rc = check_dev(sig, coeffs, signal_len, batch, sig_dist, coeff_dist, d_work, work_len);
        if (rc) return rc;
        if (batch == 0) return PHAST_OK;
        if (batch == 1) {
            sig_dist = len;
            coeff_dist = coeff_len();
        }
        PHAST_ON_DEVICE(device);
        size_t chunk = batch;
        if (per() && work_len / per() < chunk) chunk = work_len / per();
        for (size_t b0 = 0; b0 < batch; b0 += chunk) {
            const size_t c = batch - b0 < chunk ? batch - b0 : chunk;
            T *x = sig + b0 * sig_dist, *packed = coeffs + b0 * coeff_dist;
            for (size_t step = 1; step <= levels; ++step) {
                const size_t l = inverse ? levels + 1 - step : step;  // n_{l-1} samples <-> n_l coefficients per band
                size_t fine_dist = sig_dist, coarse_dist = coeff_dist;
                T *fine = l == 1 ? x : row(d_work, c, l - 1, &fine_dist);
                T *coarse = l == levels ? packed : row(d_work, c, l, &coarse_dist);
                DwtArgs a{};
                a.taps = d_taps;
                a.f = (unsigned)f;
                a.mode = mode;
                if (!inverse) {
                    a.in_lo = fine;
                    a.in_lo_dist = fine_dist;
                    a.out_lo = coarse;
                    a.out_lo_dist = coarse_dist;
                    a.out_hi = packed + geom.off[l];
                    a.out_hi_dist = coeff_dist;
                    a.n_in = geom.n[l - 1];
                    a.n_out = a.items = geom.n[l];
                } else {
                    a.in_lo = coarse;
                    a.in_lo_dist = coarse_dist;
                    a.in_hi = packed + geom.off[l];
                    a.in_hi_dist = coeff_dist;
                    a.out_lo = fine;
                    a.out_lo_dist = fine_dist;
                    a.n_in = geom.n[l];
                    a.n_out = geom.n[l - 1];
                    dwt_synth_pairs(a.n_out, a.f, mode, &a.q_first, &a.items);
                }
                a.tiles = (a.items + geom.tile - 1) / geom.tile;
                a.groups = c * a.tiles * 256;
                PHAST_HIP(inverse ? launch_dwt_synthesis<T>(a, st) : launch_dwt_analysis<T>(a, st));
            }
        }
        return PHAST_OK;
    }

    // host slices: one signal through device buffers of the call's own on the null stream; blocking
    int host(bool inverse, const T *in, size_t in_len, T *out, size_t out_len) const {
        if (!in || !out) return PHAST_ERR_INVALID_ARG;
        const size_t nc = coeff_len();
        if ((inverse ? out_len : in_len) != len) return PHAST_ERR_PLANNER_SIZE;
        if ((inverse ? in_len : out_len) != nc) return PHAST_ERR_LEN_MISMATCH;
        PHAST_ON_DEVICE(device);
        DevBuf buf;
        int rc = buf.alloc((len + nc + per() + 1) * sizeof(T));
        if (rc) return rc;
        T *d_sig = reinterpret_cast<T *>(buf.p), *d_co = d_sig + len, *d_w = d_co + nc;
        PHAST_HIP(hipMemcpy(inverse ? d_co : d_sig, in, in_len * sizeof(T), hipMemcpyHostToDevice));
        rc = dev(inverse, d_sig, d_co, len, 1, len, nc, d_w, per(), nullptr);
        if (rc) return rc;
        PHAST_HIP(hipMemcpy(out, inverse ? d_sig : d_co, out_len * sizeof(T), hipMemcpyDeviceToHost));
        return PHAST_OK;
    }

    // measurement hook: ms[0] = wavedec of the signals into the packed rows, ms[1] = waverec of the packed rows back into the
    // signals (which it overwrites with their reconstruction), average milliseconds over `reps` calls of `batch` signals at
    // distances L and coeff_len in one chunk (work_len >= workspace_len(batch)); blocks
    int time_stages(T *sig, T *coeffs, size_t batch, T *d_work, size_t work_len, int reps, float *ms, hipStream_t st) const {
        if (!ms || reps < 1 || batch == 0) return PHAST_ERR_INVALID_ARG;
        int rc = check_dev(sig, coeffs, len, batch, len, coeff_len(), d_work, work_len);
        if (rc) return rc;
        if (work_len < workspace_len(batch)) return PHAST_ERR_INVALID_ARG;
        PHAST_ON_DEVICE(device);
        struct Events {
            hipEvent_t e[2] = {};
            ~Events() {
                for (hipEvent_t x : e)
                    if (x) hipEventDestroy(x);
            }
        } ev;
        for (hipEvent_t &x : ev.e) PHAST_HIP(hipEventCreate(&x));
        for (int dir = 0; dir < 2; ++dir) {
            PHAST_HIP(hipEventRecord(ev.e[0], st));
            for (int r = 0; r < reps; ++r)
                if ((rc = dev(dir != 0, sig, coeffs, len, batch, len, coeff_len(), d_work, work_len, st))) return rc;
            PHAST_HIP(hipEventRecord(ev.e[1], st));
            PHAST_HIP(hipStreamSynchronize(st));
            float t = 0;
            PHAST_HIP(hipEventElapsedTime(&t, ev.e[0], ev.e[1]));
            ms[dir] = t / (float)reps;
        }
        return PHAST_OK;
    }
};

template <typename T, typename P>
static int dwt_planner_new(size_t signal_len, const T *dec_lo, const T *dec_hi, const T *rec_lo, const T *rec_hi,
                           size_t filter_len, size_t level, int mode, P **out) {
    if (!out) return PHAST_ERR_INVALID_ARG;
    *out = nullptr;
    if (!dec_lo || !dec_hi || !rec_lo || !rec_hi || dwt_bad_args(signal_len, filter_len, level, mode))  // before the device is touched
        return PHAST_ERR_INVALID_ARG;
    auto *p = new (std::nothrow) P();
    if (!p) return PHAST_ERR_ALLOC;
    int rc = p->init(signal_len, dec_lo, dec_hi, rec_lo, rec_hi, filter_len, level, mode);
    if (rc) {
        delete p;
        return rc;
    }
    *out = p;
    return PHAST_OK;
}

}  // namespace phast
