// channelizer.hip -- the fold of the polyphase channelizer (channelizer.hpp has the definition and the schedule).
//
//     fold      workgroup w owns one tile: `frames` consecutive frames by `cols` consecutive columns of one plane of one
//               signal.  Thread t owns column t mod cols of the frames t div cols + i fpp (neighbouring lanes: neighbouring
//               columns, so neighbouring samples in LDS, neighbouring taps in the table and neighbouring elements of an output
//               row) and keeps for each its accumulator, the first tap r0 of its column there and the period of its newest
//               sample, counted from the tile's oldest.  Per tap chunk: all threads bring the periods of the signal the
//               chunk meets into LDS (zeros outside [0, L) and in the columns a last tile does not have), a barrier, then
//               acc = fma(tap, sample, acc) over the chunk in ascending j, a barrier.  One store per element, by elements:
//               pointers and distances need element alignment only.
// Launches are split at 2^31 - 1 workgroups, as in the other sweeps.  No atomics, no scratch memory.
#include "channelizer.hpp"

namespace phast {

// one rounding per product and sum, in T
__device__ inline double chan_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }
__device__ inline float chan_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

// (v div m, v mod m) of v < 2^40, by a 32-bit division where v allows it
__device__ inline unsigned chan_divmod(unsigned long long v, unsigned m, unsigned *rem) {
    const unsigned long long q = v < 0xffffffffull ? (unsigned)v / m : v / m;
    *rem = (unsigned)(v - q * m);
    return (unsigned)q;
}

template <typename T>
__global__ void __launch_bounds__(256) chan_fold_kernel(ChanArgs a) {
    __shared__ T sig[kChanLds];
    constexpr unsigned R = kChanPerThread;
    const unsigned t = threadIdx.x;
    const unsigned long long wg = (a.g0 >> 8) + blockIdx.x;
    if (wg * 256 >= a.groups) return;  // whole workgroups: all threads agree
    const ChanGeom g = a.geom;
    const unsigned m = (unsigned)a.m, cols = g.cols;
    // (plane, frame tile, column tile) of this workgroup; (signal, tile of the signal) of the frame tile
    const unsigned long long per_plane = a.ftn * a.ctiles;
    const unsigned plane = wg >= per_plane;
    const unsigned long long w = wg - plane * per_plane;
    const unsigned long long ftw = w < 0xffffffffull && a.ctiles < 0xffffffffull ? (unsigned)w / (unsigned)a.ctiles : w / a.ctiles;
    const unsigned ct = (unsigned)(w - ftw * a.ctiles);
    const unsigned long long fta = a.ft0 + ftw;
    const unsigned long long b = fta < 0xffffffffull && a.ftiles < 0xffffffffull ? (unsigned)fta / (unsigned)a.ftiles : fta / a.ftiles;
    const unsigned long long i0 = (fta - b * a.ftiles) * g.frames;                          // the tile's first frame of the window
    const unsigned n = a.out_frames - i0 < g.frames ? (unsigned)(a.out_frames - i0) : g.frames;  // its frames
    const unsigned p0 = ct * kChanMaxCols;                                                  // its first column (one tile: 0)
    const unsigned nc = m - p0 < cols ? m - p0 : cols;                                      // its columns
    const unsigned long long md0 = (a.first + i0) * a.d;                                    // < 2^61
    const unsigned long long qd0 = md0 / m;
    const unsigned a0 = (unsigned)(md0 - qd0 * m);
    const T *x = (const T *)a.x[plane] + b * a.sig_dist, *table = (const T *)a.taps;

    // this thread's column c and frames f = fs + i fpp.  (f D) div M and mod M of the first by one division (a0 + f dm <
    // 2^40), of the others by steps.  The period of the newest sample of column p in frame f is (md0 + f D - p) floor-div M;
    // dq is that minus the same of the tile's last column in its first frame: 0 <= dq < span.  A frame or column the tile
    // does not have runs on tap row r0 = 0 and period 0 and is not stored.
    const unsigned fs = t / cols, c = t - fs * cols, p = p0 + c;
    const unsigned pmax = p0 + nc - 1;
    const bool col_live = fs < g.fpp && c < nc;
    unsigned lrow[R], r0[R];
    bool live[R];
    T acc[R];
    {
        unsigned af;
        unsigned qf = fs * a.dqv + chan_divmod(a0 + (unsigned long long)fs * a.dm, m, &af);
        const unsigned top = g.jc - 1, base = a0 < pmax ? 1u : 0u;
#pragma unroll
        for (unsigned i = 0; i < R; ++i) {
            const unsigned f = fs + i * g.fpp;
            const unsigned long long q = b * a.out_frames + i0 + f;
            live[i] = col_live && i < g.per && f < n && q >= a.q0 && q < a.q0 + a.count;
            const bool in = col_live && i < g.per && f < n;  // its index arithmetic is within the tile's bounds
            r0[i] = in ? (af >= p ? af - p : af + m - p) : 0;
            const unsigned dq = in ? qf + base - (af < p ? 1u : 0u) : 0;
            lrow[i] = (dq + top) * cols + (in ? c : 0);
            acc[i] = T(0);
            qf += a.sq;
            af += a.sm;
            if (af >= m) {
                af -= m;
                ++qf;
            }
        }
    }
    // the tile's oldest newest-sample period: (md0 - pmax) floor-div M, and the periods the tile's newest samples span
    const long long qb = (long long)qd0 - (a0 < pmax ? 1 : 0);
    unsigned span;
    {
        unsigned al;
        const unsigned ql = (n - 1) * a.dqv + chan_divmod(a0 + (unsigned long long)(n - 1) * a.dm, m, &al);
        span = ql - (al < p0 ? 1u : 0u) + (a0 < pmax ? 1u : 0u) + 1;  // <= g.span (chan_geom)
    }
    const unsigned rows = span + g.jc - 1;  // <= g.rows: rows x cols <= kChanLds
    // D mod M = 0: r0 is the same in every frame, and f64 holds tap j in a register across the frames of a thread.  f32 does
    // not: measured slower there.  tools/channelizer_rate.py builds the library with the choice
    // flipped to time the other branch on the same cases; either way the order of an element's sum is the same.
#ifdef PHAST_CHAN_OTHER_BRANCH
    const bool hold = a.dm == 0 && sizeof(T) != 8;
#else
    const bool hold = a.dm == 0 && sizeof(T) == 8;
#endif

    for (unsigned long long j0 = 0; j0 < a.t; j0 += g.jc) {
        const unsigned jn = a.t - j0 < g.jc ? (unsigned)(a.t - j0) : g.jc;  // the tap rows of this chunk
        // LDS row r holds period q_lo + r, q_lo = qb - (j0 + jc - 1): sig[r cols + c] = x[(q_lo + r) M + p0 + c]
        const long long q_lo = qb - (long long)(j0 + g.jc - 1);
        if (cols == kChanMaxCols) {
            for (unsigned e = t; e < rows * kChanMaxCols; e += 256) {
                const long long s = (q_lo + (long long)(e >> 8)) * (long long)m + (long long)(p0 + t);
                sig[e] = t < nc && s >= 0 && s < (long long)a.len ? x[s] : T(0);
            }
        } else {  // one column tile of M < 256 columns: the periods are one run of the signal
            const long long s0 = q_lo * (long long)m;
            for (unsigned e = t; e < rows * cols; e += 256) {
                const long long s = s0 + (long long)e;
                sig[e] = s >= 0 && s < (long long)a.len ? x[s] : T(0);
            }
        }
        __syncthreads();
        // tap row j0 + jj meets the period (newest - j0 - jj): LDS row dq + (jc - 1) - jj.  `per` independent chains, each in
        // ascending j
        const T *tp = table + j0 * a.m;
        if (hold) {
            for (unsigned jj = 0; jj < jn; ++jj) {
                const T h = tp[(unsigned long long)jj * m + r0[0]];
#pragma unroll
                for (unsigned i = 0; i < R; ++i) acc[i] = chan_fma(h, sig[lrow[i] - jj * cols], acc[i]);
            }
        } else {
            for (unsigned jj = 0; jj < jn; ++jj) {
#pragma unroll
                for (unsigned i = 0; i < R; ++i)
                    acc[i] = chan_fma(tp[(unsigned long long)jj * m + r0[i]], sig[lrow[i] - jj * cols], acc[i]);
            }
        }
        __syncthreads();
    }
    T *out = (T *)a.out[plane];
#pragma unroll
    for (unsigned i = 0; i < R; ++i) {
        if (live[i]) {
            const unsigned long long q = b * a.out_frames + i0 + fs + i * g.fpp;
            out[(q - a.q0) * a.ld + p] = acc[i];
        }
    }
}

template <typename T> hipError_t launch_chan_fold(const ChanArgs &a0, hipStream_t stream) {
    ChanArgs a = a0;
    return launch_in_slices(a.groups, [&](dim3 grid, unsigned long long g0) {
        a.g0 = g0;
        hipLaunchKernelGGL(chan_fold_kernel<T>, grid, dim3(256), 0, stream, a);
    });
}
template hipError_t launch_chan_fold<double>(const ChanArgs &, hipStream_t);
template hipError_t launch_chan_fold<float>(const ChanArgs &, hipStream_t);

}  // namespace phast
