// planner_nufft_sort.hpp -- the host side of nufft_sort.hpp for the three NUFFT planners: one blocking call that turns coordinates
// in device memory into a planner's point tables.  The temporary device memory (nufft_sort_temp_bytes(M): 16 M bytes and a
// little) is allocated inside the call and freed before it returns, so a planner's device_bytes() does not know of it.
#pragma once

#include "host_util.hpp"
#include "nufft_sort.hpp"

namespace phast {

// a stream that is capturing cannot carry the call: it allocates, copies a flag back and blocks
static inline bool nufft_sort_stream_busy(hipStream_t s) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &st) != hipSuccess) {
        (void)hipGetLastError();
        return true;
    }
    return st != hipStreamCaptureStatusNone;
}

// d_x, d_y, d_z (d_y null in 1-D, d_z null below 3-D): M device doubles -> perm, cell, xs, ys, zs, the planner's tables on the
// current device.  Ordered after the earlier work of `s`; returns when the tables are written.  The keys, the finiteness flag
// and the sort go to temporaries first: PHAST_ERR_INVALID_ARG for a coordinate that is not finite, and the tables are then as
// they were.  ms: optional 3 floats, the milliseconds of the keys, the pairs and the tables stage of this call.
static int nufft_sort_build(const double *d_x, const double *d_y, const double *d_z, size_t m, unsigned log_g1, unsigned log_g2,
                            unsigned log_g3, uint32_t *perm, uint32_t *cell, double *xs, double *ys, double *zs, hipStream_t s,
                            float *ms = nullptr) {
    DevBuf buf;
    int rc = buf.alloc(nufft_sort_temp_bytes(m));
    if (rc) return rc;
    NufftSortArgs a{};
    a.x = d_x;
    a.y = d_y;
    a.z = d_z;
    a.m = m;
    a.log_g1 = log_g1;
    a.log_g2 = log_g2;
    a.log_g3 = log_g3;
    unsigned char *at = reinterpret_cast<unsigned char *>(buf.p);
    auto take = [&](unsigned long long bytes) {
        uint32_t *p = reinterpret_cast<uint32_t *>(at);
        at += nufft_sort_part(bytes);
        return p;
    };
    a.key[0] = take(4 * m);
    a.key[1] = take(4 * m);
    a.idx[0] = take(4 * m);
    a.idx[1] = take(4 * m);
    a.hist = take(4 * nufft_sort_hist_len(m));
    a.flag = take(4);
    a.perm = perm;
    a.cell_start = cell;
    a.xs = xs;
    a.ys = ys;
    a.zs = zs;
    struct Events {
        hipEvent_t e[5] = {};
        ~Events() {
            for (hipEvent_t x : e)
                if (x) hipEventDestroy(x);
        }
    } ev;
    if (ms)
        for (hipEvent_t &x : ev.e) PHAST_HIP(hipEventCreate(&x));
    PHAST_HIP(hipMemsetAsync(a.flag, 0, 4, s));
    if (ms) PHAST_HIP(hipEventRecord(ev.e[0], s));
    PHAST_HIP(launch_nufft_sort_keys(a, s));
    if (ms) PHAST_HIP(hipEventRecord(ev.e[1], s));
    int side = 0;
    PHAST_HIP(launch_nufft_sort_pairs(a, &side, s));
    if (ms) PHAST_HIP(hipEventRecord(ev.e[2], s));
    uint32_t flag = 0;
    PHAST_HIP(hipMemcpyAsync(&flag, a.flag, 4, hipMemcpyDeviceToHost, s));
    PHAST_HIP(hipStreamSynchronize(s));
    if (flag) return PHAST_ERR_INVALID_ARG;
    if (ms) PHAST_HIP(hipEventRecord(ev.e[3], s));  // the flag's way back is not part of a stage
    PHAST_HIP(launch_nufft_sort_tables(a, side, s));
    if (ms) PHAST_HIP(hipEventRecord(ev.e[4], s));
    PHAST_HIP(hipStreamSynchronize(s));
    if (ms)
        for (int i = 0; i < 3; ++i) PHAST_HIP(hipEventElapsedTime(&ms[i], ev.e[i == 2 ? 3 : i], ev.e[i == 2 ? 4 : i + 1]));
    return PHAST_OK;
}

}  // namespace phast
