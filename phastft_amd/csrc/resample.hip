// resample.hip -- the polyphase FIR kernel and the spectrum sweep of sample-rate conversion (resample.hpp has the definitions
// and the schedule).
//
//     upfirdn   workgroup w owns tile (w mod tiles) of signal (w div tiles): `tile` consecutive outputs.  Thread t owns the
//               outputs t, t + 256, ... of the tile (neighbouring lanes: neighbouring outputs, samples down / up apart in LDS)
//               and keeps for each its accumulator, its LDS tap row and the distance of its q from the tile's first.  Per tap
//               chunk: all threads bring the chunk of the tile's rows and the run of the signal into LDS (zeros beyond a
//               row's Kp taps and outside [0, L)), a barrier, then acc = fma(tap, sample, acc) over the chunk in ascending
//               j, a barrier.  One store per output, by elements: pointers and distances need element alignment only.
//     spectrum  a thread owns V consecutive bins of both planes of one signal's Y: workspace planes, 16-byte accesses.
// Launches are split at 2^31 - 1 workgroups, as in the other sweeps.  No atomics, no scratch memory.
#include "resample.hpp"

namespace phast {

// one rounding per product and sum, in T
__device__ inline double fma_t(double a, double b, double c) { return __builtin_fma(a, b, c); }
__device__ inline float fma_t(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

template <typename T>
__global__ void __launch_bounds__(256) upfirdn_kernel(UpfirdnArgs a) {
    __shared__ T taps[kResampleTapLds + kResampleTapPad];
    __shared__ T sig[kResampleSigLds];
    constexpr unsigned R = kResamplePerThread;
    const unsigned t = threadIdx.x;
    const unsigned long long wg = (a.g0 >> 8) + blockIdx.x;
    if (wg * 256 >= a.groups) return;  // whole workgroups: all threads agree
    unsigned long long b;
    const unsigned long long tl = wg < 0xffffffffull && a.tiles < 0xffffffffull ? (b = (unsigned)wg / (unsigned)a.tiles, wg - b * a.tiles)
                                                                                : (b = wg / a.tiles, wg - b * a.tiles);
    const UpfirdnGeom g = a.geom;
    const unsigned up = (unsigned)a.up, down = (unsigned)a.down;
    const unsigned long long i0 = tl * g.tile;                                     // the tile's first output of the signal
    const unsigned n = a.out_len - i0 < g.tile ? (unsigned)(a.out_len - i0) : g.tile;  // its outputs
    const unsigned long long m0 = a.first + i0, md0 = m0 * down;
    const unsigned long long q0 = md0 / up;                                        // q and p of the tile's first output
    const unsigned p0 = (unsigned)(md0 - q0 * up);
    const T *x = (const T *)a.x + b * a.sig_dist, *table = (const T *)a.taps;

    // this thread's outputs: i = t + 256 r.  p and q - q0 of the first by a 32-bit division (p0 + 255 down < 2^29), of the
    // others by steps of (256 down).  An output the tile does not have runs on row 0 and sample 0 and is not stored.
    unsigned dq[R], row[R], ph[R];
    T acc[R];
    {
        const unsigned v = p0 + t * down;
        unsigned q = v / up, p = v - q * up;
#pragma unroll
        for (unsigned r = 0; r < R; ++r) {
            const unsigned i = t + 256 * r;
            const bool live = i < n;
            dq[r] = live ? q : 0;
            ph[r] = live ? p : 0;
            row[r] = (g.by_phase ? ph[r] : (live ? i : 0)) * g.stride;
            acc[r] = T(0);
            q += (unsigned)a.dq;
            p += (unsigned)a.dp;
            if (p >= up) {
                p -= up;
                ++q;
            }
        }
    }
    const unsigned span = (p0 + (n - 1) * down) / up + g.jc;  // (q of the last output - q0) + jc <= kResampleSigLds (upfirdn_geom)

    for (unsigned long long j0 = 0; j0 < a.kp; j0 += g.jc) {
        const unsigned jn = a.kp - j0 < g.jc ? (unsigned)(a.kp - j0) : g.jc;  // the taps of this chunk
        // the rows' chunk: row r, taps j0 .. j0 + jn
        if (g.by_phase) {
            if (g.jc == a.kp) {  // one chunk: the table's rows are g.stride apart, as in LDS -- a straight copy
                for (unsigned e = t; e < g.rows * g.stride; e += 256) taps[e] = table[e];
            } else {
                for (unsigned e = t; e < g.rows * g.jc; e += 256) {
                    const unsigned r = e / g.jc, jj = e - r * g.jc;
                    if (jj < jn) taps[r * g.stride + jj] = table[(unsigned long long)r * a.ts + j0 + jj];
                }
            }
        } else if (t < n) {  // one output per thread (tile <= 256): its own row
            for (unsigned jj = 0; jj < jn; ++jj) taps[row[0] + jj] = table[(unsigned long long)ph[0] * a.ts + j0 + jj];
        }
        // the run of the signal: sig[u] = x[lo + u], lo = q0 - (j0 + jc - 1)
        const long long lo = (long long)q0 - (long long)(j0 + g.jc - 1);
        for (unsigned u = t; u < span; u += 256) {
            const long long s = lo + (long long)u;
            sig[u] = s >= 0 && s < (long long)a.len ? x[s] : T(0);
        }
        __syncthreads();
        // tap j0 + jj meets x[q - j0 - jj] = sig[dq + (jc - 1) - jj]: R independent chains, each in ascending j
        const unsigned top = g.jc - 1;
        for (unsigned jj = 0; jj < jn; ++jj) {
#pragma unroll
            for (unsigned r = 0; r < R; ++r) acc[r] = fma_t(taps[row[r] + jj], sig[dq[r] + top - jj], acc[r]);
        }
        __syncthreads();
    }
    T *out = (T *)a.out + b * a.out_dist + i0;
#pragma unroll
    for (unsigned r = 0; r < R; ++r) {
        const unsigned i = t + 256 * r;
        if (i < n) out[i] = acc[r];
    }
}

template <typename T> hipError_t launch_upfirdn(const UpfirdnArgs &a0, hipStream_t stream) {
    UpfirdnArgs a = a0;
    return launch_in_slices(a.groups, [&](dim3 grid, unsigned long long g0) {
        a.g0 = g0;
        hipLaunchKernelGGL(upfirdn_kernel<T>, grid, dim3(256), 0, stream, a);
    });
}
template hipError_t launch_upfirdn<double>(const UpfirdnArgs &, hipStream_t);
template hipError_t launch_upfirdn<float>(const UpfirdnArgs &, hipStream_t);

// ---- spectrum: Y[b][k] = scale X[b][k] for k < bins (the last of them times `last` instead), 0 above; Im Y[0] = 0 and
// Im Y[zero_im] = 0 ----
template <typename T>
__global__ void __launch_bounds__(256) resample_spectrum_kernel(ResampleArgs a) {
    using V = typename AnyVec<T>::type;
    constexpr int L = AnyVec<T>::N;
    const unsigned long long g = global_group(a);
    if (g >= a.groups) return;
    unsigned long long b;
    const unsigned long long k0 = split_group(g, a.gpt, &b) * L;
    const T *xr = (const T *)a.x_re + b * a.xd, *xi = (const T *)a.x_im + b * a.xd;
    V re, im;
#pragma unroll
    for (int j = 0; j < L; ++j) {
        const unsigned long long k = k0 + j;
        const bool in = k < a.bins;  // (the rows of X are read by elements: xd and yd differ)
        const double f = k + 1 == a.bins ? a.last : a.scale;
        re[j] = in ? (T)((double)xr[k] * f) : T(0);
        im[j] = in && k != 0 && k != a.zero_im ? (T)((double)xi[k] * f) : T(0);
    }
    *(V *)((T *)a.y_re + b * a.yd + k0) = re;
    *(V *)((T *)a.y_im + b * a.yd + k0) = im;
}

template <typename T> hipError_t launch_resample_spectrum(const ResampleArgs &a0, hipStream_t stream) {
    ResampleArgs a = a0;
    return launch_in_slices(a.groups, [&](dim3 grid, unsigned long long g0) {
        a.g0 = g0;
        hipLaunchKernelGGL(resample_spectrum_kernel<T>, grid, dim3(256), 0, stream, a);
    });
}
template hipError_t launch_resample_spectrum<double>(const ResampleArgs &, hipStream_t);
template hipError_t launch_resample_spectrum<float>(const ResampleArgs &, hipStream_t);

}  // namespace phast
