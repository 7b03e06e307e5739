// sweep_shim.hpp -- runs the product's streaming sweep kernels on the host, one thread after the other (TEST INFRASTRUCTURE:
// the product package never includes it).
//
// Included after <hip/hip_runtime.h> in a host-only compile (hipcc --cuda-host-only -x hip) and BEFORE a product .hip file,
// which is then #included as it stands.  A kernel becomes a static host function, `threadIdx` and its kin thread-local
// structs, and hipLaunchKernelGGL a serial loop over grid x block that sets them and calls the kernel.  The sweeps this serves
// have one step per thread and no LDS, barriers or cross-lane operations, so the order of the threads does not matter.  The
// device math they call (sincospi) is computed in long double here: what this checks is addresses, bounds, alignment promises
// and the contract of each sweep, not the device's own rounding.  Nothing here calls into the HIP runtime, so a program built
// on it runs anywhere, under the host sanitizers, and never opens a GPU.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <cmath>

#undef __global__
#undef __device__
#undef __launch_bounds__
#define __global__ static
#define __device__
#define __launch_bounds__(...)

namespace sweep_shim {

struct Idx {
    unsigned x, y, z;
};
inline thread_local Idx thread_idx, block_idx, block_dim, grid_dim;
inline unsigned long long launches = 0, threads_run = 0;  // what a test program may print: proof that kernels ran here

template <typename K, typename... A> inline void launch(K kernel, dim3 grid, dim3 block, A... args) {
    ++launches;
    grid_dim = {grid.x, grid.y, grid.z};
    block_dim = {block.x, block.y, block.z};
    for (unsigned bz = 0; bz < grid.z; ++bz)
        for (unsigned by = 0; by < grid.y; ++by)
            for (unsigned bx = 0; bx < grid.x; ++bx)
                for (unsigned tz = 0; tz < block.z; ++tz)
                    for (unsigned ty = 0; ty < block.y; ++ty)
                        for (unsigned tx = 0; tx < block.x; ++tx) {
                            block_idx = {bx, by, bz};
                            thread_idx = {tx, ty, tz};
                            ++threads_run;
                            kernel(args...);
                        }
}

// sin(pi t), cos(pi t) with the argument reduced exactly (t is a double: t - 2 round(t / 2) and the quadrant are exact)
inline void sincospi_ld(long double t, long double *s, long double *c) {
    const long double pi = 3.141592653589793238462643383279502884L;
    t -= 2.0L * std::floor(t / 2.0L + 0.5L);  // [-1, 1)
    long double sign = 1.0L;
    if (t < 0) {
        t = -t;
        sign = -1.0L;
    }
    // t in [0, 1]: sin(pi t) = sin(pi (1 - t)), cos(pi t) = -cos(pi (1 - t))
    long double cs = 1.0L;
    if (t > 0.5L) {
        t = 1.0L - t;
        cs = -1.0L;
    }
    if (t == 0.5L) {
        *s = sign;
        *c = 0.0L;
    } else if (t == 0.0L) {
        *s = 0.0L;
        *c = cs;
    } else {
        *s = sign * sinl(pi * t);
        *c = cs * cosl(pi * t);
    }
}

}  // namespace sweep_shim

#define threadIdx (::sweep_shim::thread_idx)
#define blockIdx (::sweep_shim::block_idx)
#define blockDim (::sweep_shim::block_dim)
#define gridDim (::sweep_shim::grid_dim)

#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernel, grid, block, lds, stream, ...) ::sweep_shim::launch(kernel, dim3(grid), dim3(block), __VA_ARGS__)
#define hipExtLaunchKernelGGL(kernel, grid, block, lds, stream, e0, e1, flags, ...)                                      \
    ::sweep_shim::launch(kernel, dim3(grid), dim3(block), __VA_ARGS__)
#define hipGetLastError() (hipSuccess)  // the runtime's own answers 100 (no device) on a machine without one

// ---- device math of the sweeps, as host overloads (a kernel is a host function here) ----
inline void sincospi(double t, double *s, double *c) {
    long double ls, lc;
    ::sweep_shim::sincospi_ld((long double)t, &ls, &lc);
    *s = (double)ls;
    *c = (double)lc;
}
inline void sincospif(float t, float *s, float *c) {
    long double ls, lc;
    ::sweep_shim::sincospi_ld((long double)t, &ls, &lc);
    *s = (float)ls;
    *c = (float)lc;
}
