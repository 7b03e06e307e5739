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
// Limits, stated so that nobody reads more into a green run than it says:
//   * no cross-lane operations (DPP, permute, readlane, ballot, shuffles): a kernel that uses them does not compile here;
//   * static LDS keeps the bytes of the previous workgroup (and launch), so a read before the write shows as WRONG DATA in the
//     result, not as an initialisation pattern;
//   * no timing, no memory model: two threads between the same two barriers never overlap, so a race between them that both
//     serial orders happen to survive is not seen;
//   * the device's own arithmetic (rounding of 1.0f / d, sincos) is the host's here.
// Nothing here calls into the HIP runtime: the program is linked without it, runs anywhere and never opens a GPU.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <sys/mman.h>
#include <ucontext.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
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
inline std::string last_kernel;                        // the instantiation of the latest launch

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
};
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
                f.fake = nullptr;
                context_init(f.ctx, f.stack, fiber_main);
            }
    unsigned live = nthreads;
    while (live) {
        bool waited = false;
        for (unsigned k = 0; k < nthreads; ++k) {
            Fiber &f = fibers[order == kAscending ? k : nthreads - 1 - k];
            if (f.done) continue;
            f.waiting = false;
            cur = &f;
            thread_idx = f.tid;
            start_switch(&sched_fake, f.stack, kStackBytes);
            context_switch(sched_ctx, f.ctx);
            finish_switch(sched_fake, nullptr, nullptr);
            if (f.done) --live;
            waited |= f.waiting;
        }
        if (waited) ++barriers;  // a barrier that every live thread of the workgroup has now passed
    }
    cur = nullptr;
}

template <typename K, typename... A>
inline void launch(const char *text, const char *where, K kernel, dim3 grid, dim3 block, size_t lds, A... args) {
    ++launches;
    last_kernel = instantiation(text, where);
    ++ran[last_kernel];
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
    std::printf("  launches %llu  workgroups %llu  threads %llu  barriers %llu\n", launches, workgroups, threads_run, barriers);
}

}  // namespace block_shim

#define threadIdx (::block_shim::thread_idx)
#define blockIdx (::block_shim::block_idx)
#define blockDim (::block_shim::block_dim)
#define gridDim (::block_shim::grid_dim)

#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernel, grid, block, lds, stream, ...)                                                        \
    ::block_shim::launch(#kernel, __PRETTY_FUNCTION__, kernel, dim3(grid), dim3(block), (size_t)(lds), __VA_ARGS__)
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
