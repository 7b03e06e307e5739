// nd.hip -- the batched planar transpose of the multi-dimensional transforms (nd.hpp): both planes of
// [B][R][C] -> [B][C][R], out of place, one launch.  One workgroup of 256 threads moves one tile of each plane through LDS.
//
// Square tiles (R, C >= TS, TS = 256 bytes of T: 32 f64 / 64 f32): TS x TS, LDS rows of TS + 1 elements (an odd pitch).
// The tile is read along the source rows and written along the destination rows, 16 bytes per lane where the pointers
// and distances allow it (`vec`), one element per lane otherwise.  LDS is accessed one element per lane on both sides
// (ds_write_b64 / ds_read_b64 for f64, _b32 for f32); the lane maps below keep both sides free of bank conflicts:
//   write (from the source):  8 lanes x 16 B per row (vec) or 128 B of elements, rows next: with the odd pitch the
//                             16 lanes of a ds_write_b64 group / 32 of a ds_write_b32 group land on distinct banks
//   read (to the destination): 32 lanes down one LDS column (element) or 32 / V lanes x V rows (vec): bank
//                             2 (2 g P + j) mod 64 (f64) and (4 g P + j) mod 32 (f32) are distinct for P odd
// Narrow tiles (one side S < TS, e.g. 2^20 x 3): a square tile would leave all but S of its TS lanes idle on that side.
// The tile instead spans the whole narrow side, so that the narrow side's memory is one contiguous run per tile: it is
// read (narrow C) or written (narrow R) flat at full coalescing, 16 bytes per lane where the run is aligned, and the wide
// side keeps its 16-byte accesses.  The LDS image has a pitch of S | 1 along the narrow side and a skew of one element per
// V wide-side entries when the wide side is vectorised, so that the V-strided lanes of a 16-byte access stay
// conflict-free.
// Addresses are 64-bit: a plane holds up to 2^30 points (8 GiB in f64).
#include "nd.hpp"
#include "kernels.hpp"

namespace phast {

namespace {

struct NdTArgs {
    const void *src_re, *src_im;
    void *dst_re, *dst_im;
    unsigned long long src_dist, dst_dist;  // elements between matrices
    unsigned long long rows, cols;          // R, C of the source
    unsigned long long tiles_r, tiles_c;    // tiles per matrix along R and along C
    unsigned long long t0;                  // first tile of this launch (launches split at 2^31 - 1 workgroups)
    unsigned span;                          // narrow tiles: wide-side entries per tile
};

template <typename T> struct Vec16;
template <> struct Vec16<double> { typedef double type __attribute__((ext_vector_type(2))); static constexpr int N = 2; };
template <> struct Vec16<float> { typedef float type __attribute__((ext_vector_type(4))); static constexpr int N = 4; };

// (matrix, tile row, tile column) of this workgroup's tile
__device__ inline void tile_of(const NdTArgs &a, unsigned long long *b, unsigned long long *tr, unsigned long long *tc) {
    const unsigned long long t = a.t0 + blockIdx.x, per = a.tiles_r * a.tiles_c;
    *b = t / per;
    const unsigned long long rem = t - *b * per;
    *tr = rem / a.tiles_c;
    *tc = rem - *tr * a.tiles_c;
}

// ---- square tiles ----
template <typename T, bool VIN, bool VOUT> __global__ void __launch_bounds__(256) nd_transpose_square(NdTArgs a) {
    constexpr int TS = 256 / (int)sizeof(T), P = TS + 1, V = Vec16<T>::N;
    constexpr int VI = VIN ? V : 1, VO = VOUT ? V : 1;
    constexpr int LL = VIN ? 8 : 128 / (int)sizeof(T);  // lanes along a source row (128 B)
    constexpr int RL = VOUT ? 32 / V : 32;              // lanes along a destination row
    constexpr int LOADS = TS * TS / VI / 256, STORES = TS * TS / VO / 256;
    typedef typename Vec16<T>::type vt;
    __shared__ T lds[2][TS * P];
    unsigned long long b, tr, tc;
    tile_of(a, &b, &tr, &tc);
    const unsigned long long r0 = tr * TS, c0 = tc * TS;
    const unsigned nr = (unsigned)(a.rows - r0 < TS ? a.rows - r0 : TS), nc = (unsigned)(a.cols - c0 < TS ? a.cols - c0 : TS);
    const unsigned tid = threadIdx.x;
    for (int p = 0; p < 2; ++p) {
        const T *src = reinterpret_cast<const T *>(p ? a.src_im : a.src_re) + b * a.src_dist + r0 * a.cols + c0;
        T v[LOADS][VI];
#pragma unroll
        for (int k = 0; k < LOADS; ++k) {
            const unsigned s = k * 256 + tid, rest = s / LL;
            const unsigned i = rest % TS, c = ((rest / TS) * LL + s % LL) * VI;
            if (i < nr && c < nc) {
                if constexpr (VIN) {
                    const vt x = *reinterpret_cast<const vt *>(src + (unsigned long long)i * a.cols + c);
#pragma unroll
                    for (int e = 0; e < VI; ++e) v[k][e] = x[e];
                } else {
                    v[k][0] = src[(unsigned long long)i * a.cols + c];
                }
            }
        }
#pragma unroll
        for (int k = 0; k < LOADS; ++k) {
            const unsigned s = k * 256 + tid, rest = s / LL;
            const unsigned i = rest % TS, c = ((rest / TS) * LL + s % LL) * VI;
            if (i < nr && c < nc)
#pragma unroll
                for (int e = 0; e < VI; ++e) lds[p][i * P + c + e] = v[k][e];
        }
    }
    __syncthreads();
    for (int p = 0; p < 2; ++p) {
        T *dst = reinterpret_cast<T *>(p ? a.dst_im : a.dst_re) + b * a.dst_dist + c0 * a.rows + r0;
#pragma unroll
        for (int k = 0; k < STORES; ++k) {
            const unsigned s = k * 256 + tid, rest = s / RL;
            const unsigned j = rest % TS, r = ((rest / TS) * RL + s % RL) * VO;
            if (j < nc && r < nr) {
                if constexpr (VOUT) {
                    vt x;
#pragma unroll
                    for (int e = 0; e < VO; ++e) x[e] = lds[p][(r + e) * P + j];
                    *reinterpret_cast<vt *>(dst + (unsigned long long)j * a.rows + r) = x;
                } else {
                    dst[(unsigned long long)j * a.rows + r] = lds[p][r * P + j];
                }
            }
        }
    }
}

// ---- narrow tiles: the tile spans the whole narrow side S (S < TS); `span` wide-side entries per tile ----
// NC (narrow C): source rows r0 .. r0 + span, all C columns: one contiguous run read flat; the destination's C rows are
// written along their `span` points, 16 bytes per lane when `VW`.  LDS image [r][c] at r * PC + c + (VW ? r / V : 0).
// !NC (narrow R): source R rows, columns c0 .. c0 + span read along the rows (16 bytes per lane when `VW`); the
// destination's span rows of R points are one contiguous run written flat.  LDS image [c][r] at c * PR + r + (VW ? c / V : 0).
// `VF`: the flat run starts 16-byte aligned (aligned planes, matrix distance a multiple of V; a tile starts at a multiple
// of 8 wide-side entries), so it moves 16 bytes per lane, its last partial group element by element.
// Quotients by the runtime S and groups-per-row are taken as (x + 0.5) * (1 / d) in f32: exact for x < 2^21 (the rounding
// error of the product, < 2^-22 of it, stays below the 0.5 / d margin to the next integer); x < E <= 4096 here.
__device__ inline unsigned fdiv(unsigned x, float inv) { return (unsigned)(((float)x + 0.5f) * inv); }

template <typename T, bool NC, bool VW, bool VF> __global__ void __launch_bounds__(256) nd_transpose_narrow(NdTArgs a) {
    constexpr int TS = 256 / (int)sizeof(T), E = TS * TS, V = Vec16<T>::N, VV = VW ? V : 1, FV = VF ? V : 1;
    constexpr int FLAT = E / FV / 256, WIDE = E / VV / 256;
    typedef typename Vec16<T>::type vt;
    __shared__ T lds[2][E];
    unsigned long long b, tr, tc;
    tile_of(a, &b, &tr, &tc);
    const unsigned tid = threadIdx.x;
    const unsigned S = (unsigned)(NC ? a.cols : a.rows), pitch = S | 1u;
    const unsigned long long w0 = (NC ? tr : tc) * a.span, wn_all = NC ? a.rows : a.cols;
    const unsigned wn = (unsigned)(wn_all - w0 < a.span ? wn_all - w0 : a.span);  // wide-side entries of this tile
    const unsigned flat = wn * S, groups = wn / VV, gpr = (a.span / VV);        // (wn % VV == 0 when VW)
    const float inv_s = 1.0f / (float)S, inv_gpr = 1.0f / (float)gpr;
    auto at = [&](unsigned w, unsigned n) { return w * pitch + n + (VW ? w / V : 0u); };  // LDS of (wide w, narrow n)
    auto lds_of_flat = [&](unsigned f) {  // LDS index of flat element f of the run (wide f / S, narrow f % S)
        const unsigned w = fdiv(f, inv_s);
        return at(w, f - w * S);
    };
    for (int p = 0; p < 2; ++p) {
        if constexpr (NC) {  // flat read of rows w0 .. w0 + wn
            const T *src = reinterpret_cast<const T *>(p ? a.src_im : a.src_re) + b * a.src_dist + w0 * a.cols;
            T v[FLAT][FV];
#pragma unroll
            for (int k = 0; k < FLAT; ++k) {
                const unsigned f0 = (k * 256 + tid) * FV;
                if (f0 + FV <= flat) {
                    if constexpr (VF) {
                        const vt x = *reinterpret_cast<const vt *>(src + f0);
#pragma unroll
                        for (int e = 0; e < FV; ++e) v[k][e] = x[e];
                    } else {
                        v[k][0] = src[f0];
                    }
                } else if (VF && f0 < flat) {
#pragma unroll
                    for (int e = 0; e < FV; ++e)
                        if (f0 + e < flat) v[k][e] = src[f0 + e];
                }
            }
#pragma unroll
            for (int k = 0; k < FLAT; ++k) {
                const unsigned f0 = (k * 256 + tid) * FV;
#pragma unroll
                for (int e = 0; e < FV; ++e)
                    if (f0 + e < flat) lds[p][lds_of_flat(f0 + e)] = v[k][e];
            }
        } else {  // source rows n < R, columns w0 .. w0 + wn, along the rows
            const T *src = reinterpret_cast<const T *>(p ? a.src_im : a.src_re) + b * a.src_dist + w0;
            T v[WIDE][VV];
#pragma unroll
            for (int k = 0; k < WIDE; ++k) {
                const unsigned s = k * 256 + tid, n = fdiv(s, inv_gpr), g = s - n * gpr;
                if (n < S && g < groups) {
                    const T *q = src + (unsigned long long)n * a.cols + g * VV;
                    if constexpr (VW) {
                        const vt x = *reinterpret_cast<const vt *>(q);
#pragma unroll
                        for (int e = 0; e < VV; ++e) v[k][e] = x[e];
                    } else {
                        v[k][0] = *q;
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < WIDE; ++k) {
                const unsigned s = k * 256 + tid, n = fdiv(s, inv_gpr), g = s - n * gpr;
                if (n < S && g < groups)
#pragma unroll
                    for (int e = 0; e < VV; ++e) lds[p][at(g * VV + e, n)] = v[k][e];
            }
        }
    }
    __syncthreads();
    for (int p = 0; p < 2; ++p) {
        if constexpr (NC) {  // destination rows n < C, points w0 .. w0 + wn, along the rows
            T *dst = reinterpret_cast<T *>(p ? a.dst_im : a.dst_re) + b * a.dst_dist + w0;
#pragma unroll
            for (int k = 0; k < WIDE; ++k) {
                const unsigned s = k * 256 + tid, n = fdiv(s, inv_gpr), g = s - n * gpr;
                if (n < S && g < groups) {
                    T *q = dst + (unsigned long long)n * a.rows + g * VV;
                    if constexpr (VW) {
                        vt x;
#pragma unroll
                        for (int e = 0; e < VV; ++e) x[e] = lds[p][at(g * VV + e, n)];
                        *reinterpret_cast<vt *>(q) = x;
                    } else {
                        *q = lds[p][at(g, n)];
                    }
                }
            }
        } else {  // flat write of destination rows w0 .. w0 + wn
            T *dst = reinterpret_cast<T *>(p ? a.dst_im : a.dst_re) + b * a.dst_dist + w0 * a.rows;
#pragma unroll
            for (int k = 0; k < FLAT; ++k) {
                const unsigned f0 = (k * 256 + tid) * FV;
                if (f0 + FV <= flat) {
                    if constexpr (VF) {
                        vt x;
#pragma unroll
                        for (int e = 0; e < FV; ++e) x[e] = lds[p][lds_of_flat(f0 + e)];
                        *reinterpret_cast<vt *>(dst + f0) = x;
                    } else {
                        dst[f0] = lds[p][lds_of_flat(f0)];
                    }
                } else if (VF && f0 < flat) {
#pragma unroll
                    for (int e = 0; e < FV; ++e)
                        if (f0 + e < flat) dst[f0 + e] = lds[p][lds_of_flat(f0 + e)];
                }
            }
        }
    }
}

template <typename T, bool NC> void launch_narrow(bool vw, bool vf, dim3 grid, hipStream_t stream, const NdTArgs &a) {
    if (vw && vf) hipLaunchKernelGGL((nd_transpose_narrow<T, NC, true, true>), grid, dim3(256), 0, stream, a);
    else if (vw) hipLaunchKernelGGL((nd_transpose_narrow<T, NC, true, false>), grid, dim3(256), 0, stream, a);
    else if (vf) hipLaunchKernelGGL((nd_transpose_narrow<T, NC, false, true>), grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL((nd_transpose_narrow<T, NC, false, false>), grid, dim3(256), 0, stream, a);
}

}  // namespace

template <typename T>
hipError_t launch_nd_transpose(const T *src_re, const T *src_im, T *dst_re, T *dst_im, unsigned long long batch,
                               unsigned long long rows, unsigned long long cols, unsigned long long src_dist,
                               unsigned long long dst_dist, hipStream_t stream) {
    constexpr unsigned long long TS = 256 / sizeof(T), E = TS * TS, V = 16 / sizeof(T);
    if (batch == 0 || rows == 0 || cols == 0) return hipSuccess;
    auto al = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; };
    // 16-byte accesses along the source rows / the destination rows
    const bool vin = al(src_re) && al(src_im) && cols % V == 0 && (batch == 1 || src_dist % V == 0);
    const bool vout = al(dst_re) && al(dst_im) && rows % V == 0 && (batch == 1 || dst_dist % V == 0);
    NdTArgs a{src_re, src_im, dst_re, dst_im, src_dist, dst_dist, rows, cols, 0, 0, 0, 0};
    int shape;  // 0 square, 1 narrow C, 2 narrow R
    bool vw = false, vf = false;  // 16-byte accesses on the wide side / on the flat run of the narrow side
    if (cols < TS && cols <= rows) {
        shape = 1;
        vw = vout;
        vf = al(src_re) && al(src_im) && (batch == 1 || src_dist % V == 0);
    } else if (rows < TS) {
        shape = 2;
        vw = vin;
        vf = al(dst_re) && al(dst_im) && (batch == 1 || dst_dist % V == 0);
    } else {
        shape = 0;
    }
    if (shape) {
        // entries of the wide side per tile: the LDS image (pitch S | 1, skew 1 per V when vectorised) fits E elements;
        // a multiple of 8 (16-byte groups never straddle tiles)
        const unsigned long long S = shape == 1 ? cols : rows, pitch = S | 1;
        unsigned long long span = vw ? E * V / (V * pitch + 1) : E / pitch;
        span &= ~7ull;
        const unsigned long long wide = shape == 1 ? rows : cols;
        a.tiles_r = shape == 1 ? (wide + span - 1) / span : 1;
        a.tiles_c = shape == 1 ? 1 : (wide + span - 1) / span;
        a.span = (unsigned)span;
    } else {
        a.tiles_r = (rows + TS - 1) / TS;
        a.tiles_c = (cols + TS - 1) / TS;
    }
    const unsigned long long tiles = batch * a.tiles_r * a.tiles_c;
    constexpr unsigned long long kMaxBlocks = 0x7fffffffull;
    for (unsigned long long t0 = 0; t0 < tiles; t0 += kMaxBlocks) {
        const dim3 grid((unsigned)(tiles - t0 < kMaxBlocks ? tiles - t0 : kMaxBlocks)), block(256);
        a.t0 = t0;
        if (shape == 0) {
            if (vin && vout) hipLaunchKernelGGL((nd_transpose_square<T, true, true>), grid, block, 0, stream, a);
            else if (vin) hipLaunchKernelGGL((nd_transpose_square<T, true, false>), grid, block, 0, stream, a);
            else if (vout) hipLaunchKernelGGL((nd_transpose_square<T, false, true>), grid, block, 0, stream, a);
            else hipLaunchKernelGGL((nd_transpose_square<T, false, false>), grid, block, 0, stream, a);
        } else if (shape == 1) {
            launch_narrow<T, true>(vw, vf, grid, stream, a);
        } else {
            launch_narrow<T, false>(vw, vf, grid, stream, a);
        }
    }
    return hipGetLastError();
}

template hipError_t launch_nd_transpose<double>(const double *, const double *, double *, double *, unsigned long long,
                                                unsigned long long, unsigned long long, unsigned long long, unsigned long long,
                                                hipStream_t);
template hipError_t launch_nd_transpose<float>(const float *, const float *, float *, float *, unsigned long long,
                                               unsigned long long, unsigned long long, unsigned long long, unsigned long long,
                                               hipStream_t);

}  // namespace phast
