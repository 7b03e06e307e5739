// block_shim.hpp -- runs the product's kernels that move data through LDS between barriers on the host, one workgroup after
// the other and, inside a workgroup, every thread from one __syncthreads() to the next before any thread passes it (TEST
// INFRASTRUCTURE: the product package never includes it; a sibling of sweep_shim.hpp, which serves the kernels without LDS).
//
// Included after <hip/hip_runtime.h> in a host-only compile (hipcc --cuda-host-only -x hip) and BEFORE a product .hip file,
// which is then #included as it stands.  A kernel becomes a static host function and hipLaunchKernelGGL a loop over the grid.
// Every GPU thread of a workgroup is a fiber (a stack of its own, switches annotated for AddressSanitizer) on the ONE host thread:
// exactly one runs at a time, __syncthreads() hands control back to the scheduler, and the scheduler resumes the threads of the
// next phase only when every thread has arrived (or returned).  The ORDER in which the threads of a phase run is a launch
// parameter (block_shim::order: ascending or descending thread index), so the run is deterministic, and a missing barrier has
// teeth: a thread that reads LDS another thread has not yet written, or overwrites LDS another thread has not yet read, gets
// wrong bits in at least one of the two orders.
//
// LDS: `__shared__` is `static`, so a kernel's static LDS arrays are one object per kernel instantiation with
// AddressSanitizer's redzones round it (a global): an index past the array, silent on the device, is a report here.  Dynamic
// LDS (PHAST_DYNAMIC_LDS(name) in common.hpp, `extern __shared__ unsigned char name[]` on the device) is a heap block of exactly
// the bytes the launch asked for, new for every workgroup and filled with 0xA5.
//
// Lanes and waves (the FFT pass kernels: tests/cpp/pass_emu_test.cpp).  The fibers of a workgroup are grouped into waves of 64 by
// linear thread index, and there is a second kind of rendezvous: a fiber that reaches a wave-level operation yields, and the
// scheduler resumes it only once every lane of its wave that has not returned has reached the same operation.  On it stand
// v_permlane32_swap / v_permlane16_swap (the semantics of wave_fft.hpp: a.lanes[32..63] <-> b.lanes[0..31], a.rows{1,3} <->
// b.rows{0,2}), wave_barrier, readfirstlane -- which ABORTS when the live lanes do not all hold the same value: every use in the
// kernels claims uniformity -- and mbcnt as the lane number.  The order of the threads (ascending or descending) applies at
// both levels.  The scheduler aborts, naming kernel, workgroup and wave, when the lanes of one wave sit in different rendezvous
// or some have returned while others wait at a swap.
//
// Limits, stated so that nobody reads more into a green run than it says:
//   * of the cross-lane operations only the ones above exist (no DPP, ds_permute, readlane, ballot): a kernel that uses another
//     does not compile here; a swap with inactive lanes, whose result the hardware defines, is refused, not modelled;
//   * static LDS keeps the bytes of the previous workgroup (and launch), so a read before the write shows as WRONG DATA in the
//     result, not as an initialisation pattern;
//   * no timing, no memory model: two threads between the same two rendezvous never overlap, so a race between them that both
//     serial orders happen to survive is not seen; fences, s_sleep and s_memtime do nothing;
//   * the device's own arithmetic (rounding of 1.0f / d, sincos, contraction into FMAs) is the host's here.
// Nothing here calls into the HIP runtime: the program is linked without it, runs anywhere and never opens a GPU.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <sys/mman.h>
#include <ucontext.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <map>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#if defined(__has_feature)
#if __has_feature(address_sanitizer)
#include <sanitizer/asan_interface.h>
#include <sanitizer/common_interface_defs.h>
#define BLOCK_SHIM_ASAN 1
#endif
#endif

#undef __global__
#undef __device__
#undef __launch_bounds__
#undef __shared__
#define __global__ static
#define __device__
#define __launch_bounds__(...)
#define __shared__ static
// the one declaration the product cannot keep verbatim (an `extern` array cannot be a heap block): common.hpp defines this
// macro as today's `extern __shared__ __attribute__((aligned(16))) unsigned char name[]` unless it is defined already
#define PHAST_DYNAMIC_LDS(name) unsigned char *const name = ::block_shim::dyn_lds
// common.hpp's empty asm statements with AMDGPU register constraints (they only stop the compiler from keeping values live)
#define PHAST_LAUNDER_SGPR(x) ((void)(x))
#define PHAST_LAUNDER_VGPR(x) ((void)(x))
#define PHAST_HOST_WAVE_OPS 1  // wave_fft.hpp: take the wave index through readfirstlane here too (checked: see below)

namespace block_shim {

struct Idx {
    unsigned x, y, z;
};
enum Order { kAscending = 0, kDescending = 1 };
inline Idx thread_idx, block_idx, block_dim, grid_dim;
inline Order order = kAscending;           // of the threads of a workgroup between two barriers
inline unsigned char *dyn_lds = nullptr;   // this workgroup's dynamic LDS: exactly the launch's `lds` bytes
inline unsigned long long launches = 0, workgroups = 0, threads_run = 0, barriers = 0;  // proof that kernels ran here
inline std::map<std::string, unsigned long long> ran;  // launches per kernel instantiation, by name
inline std::map<std::string, unsigned long long> ran_in[2];  // ... and per thread order
inline std::string last_kernel;                        // the instantiation of the latest launch
inline unsigned force_grid = 0;  // != 0: every launch runs this many workgroups (a launcher that sizes its own grid, shrunken)
inline unsigned long long wave_ops = 0;  // wave-level rendezvous passed

// "(nd_transpose_narrow<T, NC, true, true>)" launched from "void launch_narrow(...) [T = double, NC = true]" is
// "nd_transpose_narrow<double, true, true, true>": the template parameters of the launching function, which the compiler
// spells out in __PRETTY_FUNCTION__, substituted into the macro argument's text.  A text that names no template (a function
// pointer variable) keeps the launching function's signature beside it.
inline std::string instantiation(const char *text, const char *where) {
    std::string t(text);
    while (!t.empty() && (t.front() == '(' || t.front() == ' ')) t.erase(0, 1);
    while (!t.empty() && (t.back() == ')' || t.back() == ' ')) t.pop_back();
    const std::string w(where);
    const size_t lb = w.rfind('['), rb = w.rfind(']');
    if (lb != std::string::npos && rb != std::string::npos && rb > lb) {
        const std::string list = w.substr(lb + 1, rb - lb - 1);
        size_t at = 0;
        while (at < list.size()) {
            size_t end = list.find(", ", at);
            if (end == std::string::npos) end = list.size();
            const std::string item = list.substr(at, end - at);
            const size_t eq = item.find(" = ");
            if (eq != std::string::npos) {
                const std::string name = item.substr(0, eq), value = item.substr(eq + 3);
                auto word = [](char c) { return (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z') || (c >= '0' && c <= '9') || c == '_'; };
                for (size_t p = t.find(name); p != std::string::npos; p = t.find(name, p)) {
                    const bool whole = (p == 0 || !word(t[p - 1])) && (p + name.size() == t.size() || !word(t[p + name.size()]));
                    if (whole) {
                        t.replace(p, name.size(), value);
                        p += value.size();
                    } else {
                        p += name.size();
                    }
                }
            }
            at = end + 2;
        }
    }
    const size_t ns = t.find("phast::");
    if (ns == 0) t.erase(0, 7);
    if (t.find('<') == std::string::npos) t += std::string(" in ") + where;
    return t;
}

// ---- fibers ----
// One stack per GPU thread of a workgroup, mapped once and reused by every workgroup, with a guard page below it: the kernels' frames
// are a few hundred bytes, and an overflow is a fault at once.
constexpr size_t kStackBytes = 32 * 1024, kGuardBytes = 4096;

// A context is a saved stack pointer: a switch pushes the callee-saved registers, exchanges the stack pointers and pops them again (the
// System V x86-64 calling convention; neither the kernels nor the shim change the floating-point control words).  ucontext does the same
// job anywhere, but every getcontext / swapcontext is a signal-mask system call, and AddressSanitizer's interceptors clear a stack's
// whole shadow at each: with millions of GPU threads per run that is most of the run's time.  -DBLOCK_SHIM_UCONTEXT selects it.
#if defined(__x86_64__) && !defined(BLOCK_SHIM_UCONTEXT)
struct Context {
    void *sp = nullptr;
};
__attribute__((naked, noinline)) inline void switch_stack(void ** /*save_sp: rdi*/, void * /*load_sp: rsi*/) {
    asm volatile("pushq %rbp\n pushq %rbx\n pushq %r12\n pushq %r13\n pushq %r14\n pushq %r15\n"
                 "movq %rsp, (%rdi)\n movq %rsi, %rsp\n"
                 "popq %r15\n popq %r14\n popq %r13\n popq %r12\n popq %rbx\n popq %rbp\n ret\n");
}
inline void context_init(Context &c, char *stack, void (*entry)()) {
#ifdef BLOCK_SHIM_ASAN
    __asan_unpoison_memory_region(stack, kStackBytes);  // the redzones of the frames the stack's previous thread never left
#endif
    void **top = reinterpret_cast<void **>(stack + kStackBytes);  // 16-byte aligned
    *--top = nullptr;                            // where `entry` would find its return address: it never returns
    *--top = reinterpret_cast<void *>(entry);    // the first switch's `ret` lands here, the stack as after a call
    for (int i = 0; i < 6; ++i) *--top = nullptr;  // rbp, rbx, r12 .. r15
    c.sp = top;
}
inline void context_switch(Context &from, Context &to) { switch_stack(&from.sp, to.sp); }
#else
struct Context {
    ucontext_t uc;
};
inline void context_init(Context &c, char *stack, void (*entry)()) {
    getcontext(&c.uc);
    c.uc.uc_stack.ss_sp = stack;
    c.uc.uc_stack.ss_size = kStackBytes;
    c.uc.uc_link = nullptr;
    makecontext(&c.uc, entry, 0);
}
inline void context_switch(Context &from, Context &to) { swapcontext(&from.uc, &to.uc); }
#endif

struct Fiber {
    Context ctx;
    char *stack = nullptr;
    void *fake = nullptr;  // AddressSanitizer's fake stack of this fiber while it is switched out
    Idx tid{};
    bool done = false, waiting = false;
    int wave_op = 0;          // != 0: waits at this wave-level operation (WaveOp)
    unsigned wa = 0, wb = 0;  // its operands on the way in, its results on the way out
};
enum WaveOp { kNoOp = 0, kWaveBarrier = 1, kFirstLane = 2, kSwap32 = 3, kSwap16 = 4 };
inline const char *wave_op_name(int op) {
    return op == kWaveBarrier ? "wave_barrier" : op == kFirstLane ? "readfirstlane" : op == kSwap32 ? "permlane32_swap" : op == kSwap16 ? "permlane16_swap" : "none";
}
inline std::vector<Fiber> fibers;  // stacks are mapped once and reused by every workgroup
inline Context sched_ctx;
inline void *sched_fake = nullptr;
inline const void *sched_bottom = nullptr;
inline size_t sched_size = 0;
inline Fiber *cur = nullptr;
struct Body {
    virtual void run() = 0;
    virtual ~Body() {}
};
inline Body *body = nullptr;

inline void start_switch(void **fake_save, const void *bottom, size_t size) {
#ifdef BLOCK_SHIM_ASAN
    __sanitizer_start_switch_fiber(fake_save, bottom, size);
#else
    (void)fake_save, (void)bottom, (void)size;
#endif
}
inline void finish_switch(void *fake, const void **bottom_old, size_t *size_old) {
#ifdef BLOCK_SHIM_ASAN
    __sanitizer_finish_switch_fiber(fake, bottom_old, size_old);
#else
    (void)fake, (void)bottom_old, (void)size_old;
#endif
}
// from a fiber back to the scheduler; `last`: the fiber returns for good and its fake stack is released
inline void to_scheduler(bool last) {
    Fiber *self = cur;
    start_switch(last ? nullptr : &self->fake, sched_bottom, sched_size);
    context_switch(self->ctx, sched_ctx);
    finish_switch(self->fake, nullptr, nullptr);
}
inline void fiber_main() {
    finish_switch(nullptr, &sched_bottom, &sched_size);
    body->run();
    cur->done = true;
    to_scheduler(true);
    std::abort();  // a finished fiber is never resumed
}
inline void barrier() {
    cur->waiting = true;
    to_scheduler(false);
}
struct Swapped {
    unsigned v[2];
    unsigned operator[](int i) const { return v[i]; }
};
inline Swapped wave_rendezvous(int op, unsigned a, unsigned b) {
    Fiber *self = cur;
    self->wave_op = op;
    self->wa = a;
    self->wb = b;
    to_scheduler(false);
    return Swapped{{self->wa, self->wb}};
}
inline int lane_id() { return (int)((cur - fibers.data()) & 63); }
[[noreturn]] inline void wave_abort(unsigned wave, const char *what) {
    std::fflush(stdout);
    std::fprintf(stderr, "block_shim: %s, workgroup (%u, %u, %u), wave %u: %s\n", last_kernel.c_str(), block_idx.x, block_idx.y, block_idx.z,
                 wave, what);
    std::fflush(stderr);
    std::abort();
}
// every live lane of wave `w` waits: at the workgroup barrier (false), or all at ONE wave-level operation, which is performed
// and the lanes released (true)
inline bool resolve_wave(unsigned w, unsigned nthreads) {
    const unsigned lo = w * 64, hi = std::min(lo + 64, nthreads);
    int op = -1;
    unsigned live = 0;
    for (unsigned t = lo; t < hi; ++t) {
        const Fiber &f = fibers[t];
        if (f.done) continue;
        ++live;
        const int here = f.waiting ? kNoOp : f.wave_op;
        if (op >= 0 && here != op) {
            char msg[160];
            std::snprintf(msg, sizeof msg, "divergence: lane %u waits at %s, an earlier lane at %s", t - lo, f.waiting ? "__syncthreads" : wave_op_name(here),
                          op == kNoOp ? "__syncthreads" : wave_op_name(op));
            wave_abort(w, msg);
        }
        op = here;
    }
    if (!live || op == kNoOp) return false;
    if (op == kSwap32 || op == kSwap16) {
        if (live != 64) wave_abort(w, "divergence: some lanes have returned (or the wave is partial) while others wait at a swap");
        Fiber *l = &fibers[lo];
        const unsigned half = op == kSwap32 ? 32 : 16;  // a.upper <-> b.lower of every pair of `half`-lane groups
        for (unsigned g = 0; g < 64; g += 2 * half)
            for (unsigned i = g; i < g + half; ++i) std::swap(l[i].wb, l[i + half].wa);
    } else if (op == kFirstLane) {
        unsigned first = 0;
        bool have = false;
        for (unsigned t = lo; t < hi; ++t) {
            Fiber &f = fibers[t];
            if (f.done) continue;
            if (!have) first = f.wa, have = true;
            if (f.wa != first) {
                char msg[160];
                std::snprintf(msg, sizeof msg, "readfirstlane of a value that is not wave-uniform: lane %u holds %u, the first live lane %u", t - lo, f.wa, first);
                wave_abort(w, msg);
            }
        }
    }
    for (unsigned t = lo; t < hi; ++t) fibers[t].wave_op = kNoOp;
    ++wave_ops;
    return true;
}

inline void run_workgroup(unsigned nthreads) {
    if (fibers.size() < nthreads) {
        const size_t had = fibers.size();
        fibers.resize(nthreads);
        for (size_t i = had; i < nthreads; ++i) {
            void *p = mmap(nullptr, kGuardBytes + kStackBytes, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
            if (p == MAP_FAILED || mprotect(p, kGuardBytes, PROT_NONE)) std::abort();
            fibers[i].stack = (char *)p + kGuardBytes;
        }
    }
    unsigned t = 0;
    for (unsigned tz = 0; tz < block_dim.z; ++tz)
        for (unsigned ty = 0; ty < block_dim.y; ++ty)
            for (unsigned tx = 0; tx < block_dim.x; ++tx, ++t) {
                Fiber &f = fibers[t];
                f.tid = {tx, ty, tz};
                f.done = f.waiting = false;
                f.wave_op = kNoOp;
                f.fake = nullptr;
                context_init(f.ctx, f.stack, fiber_main);
            }
    unsigned live = nthreads;
    while (live) {
        for (unsigned k = 0; k < nthreads; ++k) {
            Fiber &f = fibers[order == kAscending ? k : nthreads - 1 - k];
            if (f.done || f.waiting || f.wave_op) continue;
            cur = &f;
            thread_idx = f.tid;
            start_switch(&sched_fake, f.stack, kStackBytes);
            context_switch(sched_ctx, f.ctx);
            finish_switch(sched_fake, nullptr, nullptr);
            if (f.done) --live;
        }
        // every live thread now waits.  Waves whose lanes all wait at one wave-level operation go on; when there is none, the
        // whole workgroup stands at __syncthreads()
        bool released = false;
        for (unsigned w = 0; w * 64 < nthreads; ++w) released |= resolve_wave(w, nthreads);
        if (!released && live) {
            ++barriers;  // a barrier that every live thread of the workgroup has now passed
            for (unsigned t = 0; t < nthreads; ++t) fibers[t].waiting = false;
        }
    }
    cur = nullptr;
}

template <typename K, typename... A>
inline void launch(const char *text, const char *where, K kernel, dim3 grid, dim3 block, size_t lds, A... args) {
    ++launches;
    last_kernel = instantiation(text, where);
    if (last_kernel.find(" in ") != std::string::npos) {  // a function pointer variable: the second, third .. function it has held are #1, #2 ..
        static std::map<std::string, std::vector<const void *>> held;
        std::vector<const void *> &h = held[last_kernel];
        const void *fn = reinterpret_cast<const void *>(kernel);
        size_t at = std::find(h.begin(), h.end(), fn) - h.begin();
        if (at == h.size()) h.push_back(fn);
        if (at) last_kernel.insert(last_kernel.find(" in "), "#" + std::to_string(at));
    }
    ++ran[last_kernel];
    ++ran_in[order][last_kernel];
    if (force_grid) grid = dim3(force_grid);
    grid_dim = {grid.x, grid.y, grid.z};
    block_dim = {block.x, block.y, block.z};
    const unsigned nthreads = block.x * block.y * block.z;
    struct Call : Body {
        K kernel;
        std::tuple<A...> args;
        Call(K k, A... a) : kernel(k), args(a...) {}
        void run() override { std::apply(kernel, args); }
    } call(kernel, args...);
    body = &call;
    for (unsigned bz = 0; bz < grid.z; ++bz)
        for (unsigned by = 0; by < grid.y; ++by)
            for (unsigned bx = 0; bx < grid.x; ++bx) {
                block_idx = {bx, by, bz};
                void *mem = nullptr;
                if (lds) {
                    if (posix_memalign(&mem, 16, lds)) std::abort();
                    std::memset(mem, 0xA5, lds);
                }
                dyn_lds = (unsigned char *)mem;
                ++workgroups;
                threads_run += nthreads;
                run_workgroup(nthreads);
                dyn_lds = nullptr;
                std::free(mem);
            }
    body = nullptr;
}

inline void print_counters() {
    std::printf("  launches %llu  workgroups %llu  threads %llu  barriers %llu  wave operations %llu\n", launches, workgroups, threads_run, barriers,
                wave_ops);
}

}  // namespace block_shim

#define threadIdx (::block_shim::thread_idx)
#define blockIdx (::block_shim::block_idx)
#define blockDim (::block_shim::block_dim)
#define gridDim (::block_shim::grid_dim)

#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernel, grid, block, lds, stream, ...)                                                        \
    ::block_shim::launch(#kernel, __PRETTY_FUNCTION__, kernel, dim3(grid), dim3(block), (size_t)(lds), __VA_ARGS__)
#undef hipExtLaunchKernelGGL
#define hipExtLaunchKernelGGL(kernel, grid, block, lds, stream, e0, e1, flags, ...)                                      \
    ::block_shim::launch(#kernel, __PRETTY_FUNCTION__, kernel, dim3(grid), dim3(block), (size_t)(lds), __VA_ARGS__)
#define hipFuncGetAttributes(attr, func) ((void)(attr), (void)(func), hipErrorInvalidValue)  // (the launchers' occupancy query: not here)
#define hipGetLastError() (hipSuccess)  // the runtime's own answers 100 (no device) on a machine without one
// raise_lds_limit (common.hpp) succeeds without the runtime: device 0, and the attribute is taken as set
#define hipGetDevice(p) (*(p) = 0, hipSuccess)
#define hipFuncSetAttribute(func, attr, value) ((void)(func), (void)(value), hipSuccess)

// ---- device functions of these kernels, as host overloads (a kernel is a host function here) ----
inline unsigned __brev(unsigned x) {
    x = (x >> 16) | (x << 16);
    x = ((x & 0xff00ff00u) >> 8) | ((x & 0x00ff00ffu) << 8);
    x = ((x & 0xf0f0f0f0u) >> 4) | ((x & 0x0f0f0f0fu) << 4);
    x = ((x & 0xccccccccu) >> 2) | ((x & 0x33333333u) << 2);
    return ((x & 0xaaaaaaaau) >> 1) | ((x & 0x55555555u) << 1);
}
inline void __syncthreads() { ::block_shim::barrier(); }

// ---- wave-level operations (see the head of this file) ----
#define __builtin_amdgcn_permlane32_swap(a, b, fi, bc) ::block_shim::wave_rendezvous(::block_shim::kSwap32, (a), (b))
#define __builtin_amdgcn_permlane16_swap(a, b, fi, bc) ::block_shim::wave_rendezvous(::block_shim::kSwap16, (a), (b))
#define __builtin_amdgcn_wave_barrier() ((void)::block_shim::wave_rendezvous(::block_shim::kWaveBarrier, 0u, 0u))
#define __builtin_amdgcn_readfirstlane(x) ((int)::block_shim::wave_rendezvous(::block_shim::kFirstLane, (unsigned)(x), 0u)[0])
#define __builtin_amdgcn_mbcnt_lo(mask, x) ((x) + (unsigned)std::min(::block_shim::lane_id(), 32))      /* mask = ~0u in the kernels */
#define __builtin_amdgcn_mbcnt_hi(mask, x) ((x) + (unsigned)std::max(::block_shim::lane_id() - 32, 0))
#define __builtin_amdgcn_fence(...) ((void)0)
#define __builtin_amdgcn_s_sleep(x) ((void)0)
#define __builtin_amdgcn_s_memtime() (0ull)
inline int __double2loint(double x) {
    unsigned long long u;
    std::memcpy(&u, &x, 8);
    return (int)(unsigned)u;
}
inline int __double2hiint(double x) {
    unsigned long long u;
    std::memcpy(&u, &x, 8);
    return (int)(unsigned)(u >> 32);
}
inline double __hiloint2double(int hi, int lo) {
    const unsigned long long u = ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo;
    double x;
    std::memcpy(&x, &u, 8);
    return x;
}
inline unsigned __float_as_uint(float x) {
    unsigned u;
    std::memcpy(&u, &x, 4);
    return u;
}
inline float __uint_as_float(unsigned u) {
    float x;
    std::memcpy(&x, &u, 4);
    return x;
}
