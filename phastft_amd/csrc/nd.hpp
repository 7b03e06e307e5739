// nd.hpp -- multi-dimensional transforms: the schedule of steps over the axes, and the launch interface of the
// batched planar transpose (nd.hip).
//
// A row-major array [n_0 .. n_{r-1}] is transformed axis by axis, always along the contiguous last axis, by rotation:
//
//     transform the rows of the last axis (length L, P = prod / L rows)
//     transpose [P][L] -> [L][P]: the old last axis moves to the front, the next axis becomes the last
//
// After r rotations the axes are back in their original order: r transposes for rank r (transposing every axis there and
// back would cost 2 (r - 1)).  The transforms are the existing one-axis paths (PlannerAny / PlannerR2cAny); steps read one
// buffer and write another (or the same, in place), so that the last step lands in the caller's planes with no extra copy.
// Axes of length 1 are dropped before scheduling (a real transform keeps its last axis: it is the real one).  A shape with
// a single axis left runs the one-axis path alone.
//
//     complex   X = the caller's planes (in place), W = a transposed copy in the workspace
//     R2C       the real input (read only) -> X = the caller's half-spectrum planes, through W
//     C2R       X = the caller's half-spectrum planes (read only) -> W, W2 (two copies, ping-pong) -> the real output
//
// The top of this header (the schedule) has no HIP dependency: tests/test_nd_cpu.py compiles it with g++ and runs the steps
// in numpy.
#pragma once

#include <cstddef>

namespace phast {

constexpr size_t kNdMaxRank = 8;
constexpr unsigned long long kNdMaxAxis = 1ull << 29, kNdMaxPoints = 1ull << 30;

enum NdKind { kNdC2C = 0, kNdR2C = 1, kNdC2R = 2 };
enum NdBuf { kNdX = 0, kNdW = 1, kNdW2 = 2, kNdReal = 3 };
enum NdOp { kNdTransform = 0, kNdTranspose = 1, kNdR2cRows = 2, kNdC2rRows = 3 };

// One step over one array (a batch repeats it per array).  kNdTransform: `rows` complex rows of length n (contiguous, n
// apart), forward or inverse as the call; kNdR2cRows / kNdC2rRows: `rows` real rows of length n <-> rows of n / 2 + 1
// points; kNdTranspose: [rows][n] -> [n][rows].  `axis`: the index of the transformed axis in the squeezed shape.
struct NdStep {
    int op;
    int src, dst;  // NdBuf
    size_t rows, n;
    int axis;
};

// The squeezed shape: complex drops every axis of length 1, real every leading one (the last axis stays).  Returns its rank
// (0: every axis is 1 -- complex only), or 0 with *bad = 1 for an illegal shape: rank 0 or > 8, an axis 0 or > 2^29, a
// product > 2^30.  *total = the product of the axes.
inline size_t nd_squeeze(const size_t *dims, size_t rank, int kind, size_t *out, unsigned long long *total, int *bad) {
    *bad = 1;
    *total = 0;
    if (!dims || rank == 0 || rank > kNdMaxRank) return 0;
    unsigned long long prod = 1;
    for (size_t i = 0; i < rank; ++i) {
        if (dims[i] == 0 || dims[i] > kNdMaxAxis) return 0;
        prod *= dims[i];
        if (prod > kNdMaxPoints) return 0;
    }
    *bad = 0;
    *total = prod;
    size_t q = 0;
    for (size_t i = 0; i < rank; ++i)
        if (dims[i] > 1 || (kind != kNdC2C && i + 1 == rank)) out[q++] = dims[i];
    return q;
}

// The steps of a transform of the squeezed shape d[0 .. q-1] (q >= 1; complex q may be 0: a 1-point transform): at most
// 2 kNdMaxRank + 1 of them into `steps`; returns their count.
inline size_t nd_schedule(const size_t *d, size_t q, int kind, NdStep *steps) {
    size_t ns = 0;
    unsigned long long prod = 1;
    for (size_t i = 0; i < q; ++i) prod *= d[i];
    if (q <= 1) {  // one axis: the one-axis path, in place (complex) or real <-> X
        const size_t n = q ? d[0] : 1;
        if (kind == kNdC2C) steps[ns++] = NdStep{kNdTransform, kNdX, kNdX, 1, n, 0};
        else if (kind == kNdR2C) steps[ns++] = NdStep{kNdR2cRows, kNdReal, kNdX, 1, n, 0};
        else steps[ns++] = NdStep{kNdC2rRows, kNdX, kNdReal, 1, n, 0};
        return ns;
    }
    size_t cur[kNdMaxRank];  // the shape as it lies in memory now; the position of each original axis rotates
    int ax[kNdMaxRank];
    for (size_t i = 0; i < q; ++i) {
        cur[i] = d[i];
        ax[i] = (int)i;
    }
    const size_t h = d[q - 1] / 2 + 1;
    if (kind != kNdC2C) {
        prod = prod / d[q - 1] * h;  // the complex array [d_0 .. d_{q-2}][h]
        cur[q - 1] = h;
    }
    auto rotate = [&](int src, int dst) {  // [P][L] -> [L][P]
        const size_t L = cur[q - 1], P = (size_t)(prod / L);
        const int a = ax[q - 1];
        steps[ns++] = NdStep{kNdTranspose, src, dst, P, L, a};
        for (size_t i = q - 1; i > 0; --i) {
            cur[i] = cur[i - 1];
            ax[i] = ax[i - 1];
        }
        cur[0] = L;
        ax[0] = a;
    };
    auto rows_of = [&]() { return (size_t)(prod / cur[q - 1]); };
    if (kind == kNdC2C) {
        // q transposes alternate the buffer: start out of place when q is odd, so that the last one writes X
        int at = kNdX;
        for (size_t k = 0; k < q; ++k) {
            const int to = (k == 0 && (q & 1)) ? kNdW : at;
            steps[ns++] = NdStep{kNdTransform, at, to, rows_of(), cur[q - 1], ax[q - 1]};
            at = to;
            const int next = at == kNdX ? kNdW : kNdX;
            rotate(at, next);
            at = next;
        }
    } else if (kind == kNdR2C) {
        int at = (q & 1) ? kNdW : kNdX;
        steps[ns++] = NdStep{kNdR2cRows, kNdReal, at, (size_t)(prod / h), d[q - 1], (int)(q - 1)};
        for (size_t k = 0; k < q; ++k) {
            const int next = at == kNdX ? kNdW : kNdX;
            rotate(at, next);
            at = next;
            if (k + 1 < q) steps[ns++] = NdStep{kNdTransform, at, at, rows_of(), cur[q - 1], ax[q - 1]};
        }
    } else {
        int at = kNdX;  // read only: the first transpose copies it out
        for (size_t k = 0; k < q; ++k) {
            const int next = at == kNdW ? kNdW2 : kNdW;
            rotate(at, next);
            at = next;
            if (k + 1 < q) steps[ns++] = NdStep{kNdTransform, at, at, rows_of(), cur[q - 1], ax[q - 1]};
        }
        steps[ns++] = NdStep{kNdC2rRows, at, kNdReal, (size_t)(prod / h), d[q - 1], (int)(q - 1)};
    }
    return ns;
}

}  // namespace phast

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace phast {

// Both planes of `batch` matrices [rows][cols] -> [cols][rows], out of place: matrix b at src + b * src_dist and
// dst + b * dst_dist (elements).  Any rows, cols >= 1; any alignment (16-byte accesses where the pointers and distances
// allow them); launches split at 2^31 - 1 workgroups.
template <typename T>
hipError_t launch_nd_transpose(const T *src_re, const T *src_im, T *dst_re, T *dst_im, unsigned long long batch,
                               unsigned long long rows, unsigned long long cols, unsigned long long src_dist,
                               unsigned long long dst_dist, hipStream_t stream);

}  // namespace phast
#endif
