// hip/hip_runtime.h — TEST CODE, found only through -I tests/cpp/simt: a host stand-in for the HIP runtime under which a
// kernel source compiles UNCHANGED with the host compiler and executes lane by lane (tests/cpp/multi_sim.cpp).
//
//   lanes      every lane of a workgroup is a fiber with a stack of its own, all in one host thread.  A lane runs until
//              its next collective (__shfl, __shfl_xor, __shfl_up, __shfl_down, __ballot, __syncthreads), posts its operand and
//              yields; when every lane of its wave has arrived the wave goes on.  Width 64.  __shfl_down alone honours a
//              narrower `width` (what csrc/functor_kernel.inc needs): its collective is then the aligned group of `width`
//              lanes, which may run apart from the other groups of the wave — some skip a round, some return earlier.
//   out of step  every collective records its kind and operand size, and the lanes of a wave are compared after each
//              exchange (the lanes of a group, under a narrower width): a mismatch, or a lane that has returned while
//              others wait in a collective, ends the program
//              with a message naming the wave and its collective count (exit status 3) — no deadlock.
//   blocks     run one after another, so `__shared__` (= static) is shared by exactly one workgroup at a time.
//              Waves of a workgroup meet only in __syncthreads.
//   memory     hipMalloc is an aligned host allocation filled with 0x5A: an int32 never written reads as 1 515 870 810
//              (a row far outside any Y of a test), a float as 1.5e16, a double as 1.7e127.
//   alignment  float4 / double2 are alignas(16): the host's alignment check fires on a 16-byte access to an address
//              that is not 16-byte aligned.
// Covered: what csrc/multi.hip, csrc/coo_csr.hip, csrc/functor_kernel.inc and csrc/common.hpp use.  No LDS-staging builtins, no sched_barrier; the
// atomics and copies of the units that have them are in tests/cpp/sim_runtime.hpp.
#pragma once

#include <sys/mman.h>

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <type_traits>

#if defined(__has_feature)
#if __has_feature(address_sanitizer)
#define SIMT_ASAN 1
#endif
#endif
#if defined(__SANITIZE_ADDRESS__) && !defined(SIMT_ASAN)
#define SIMT_ASAN 1
#endif
#ifdef SIMT_ASAN
#include <sanitizer/common_interface_defs.h>
#endif
#if !defined(__x86_64__) || defined(SIMT_USE_UCONTEXT)
#include <ucontext.h>
#define SIMT_UCONTEXT 1
#endif

#define __global__
#define __device__
#define __host__
#define __forceinline__ inline __attribute__((always_inline))
#define __launch_bounds__(...)
#define __shared__ static

struct dim3 {
    unsigned x, y, z;
    constexpr dim3(unsigned x_ = 1, unsigned y_ = 1, unsigned z_ = 1) : x(x_), y(y_), z(z_) {}
};
struct alignas(16) float4 { float x, y, z, w; };
struct alignas(16) double2 { double x, y; };

typedef struct ihipStream_t* hipStream_t;
enum hipError_t { hipSuccess = 0, hipErrorInvalidValue = 1, hipErrorOutOfMemory = 2 };
inline const char* hipGetErrorString(hipError_t e) {
    return e == hipSuccess ? "no error" : e == hipErrorOutOfMemory ? "out of memory" : "invalid argument";
}
inline hipError_t hipGetLastError() { return hipSuccess; }

inline hipError_t hipMalloc(void** p, size_t bytes) {
    if (!p) return hipErrorInvalidValue;
    *p = nullptr;
    if (bytes == 0) return hipSuccess;
    if (posix_memalign(p, 256, bytes) != 0) { *p = nullptr; return hipErrorOutOfMemory; }
    memset(*p, 0x5A, bytes);
    return hipSuccess;
}
template <typename T>
inline hipError_t hipMalloc(T** p, size_t bytes) { return hipMalloc(reinterpret_cast<void**>(p), bytes); }
inline hipError_t hipFree(void* p) { free(p); return hipSuccess; }

inline int min(int a, int b) { return b < a ? b : a; }
inline int max(int a, int b) { return a < b ? b : a; }
inline int __clzll(unsigned long long v) { return v ? __builtin_clzll(v) : 64; }
inline int __popcll(unsigned long long v) { return __builtin_popcountll(v); }
inline int __ffsll(long long v) { return __builtin_ffsll(v); }      // 1 + the index of the lowest set bit; 0 for 0

namespace simt {

constexpr int kWidth = 64;
constexpr int kMaxBlock = 1024;
constexpr size_t kStackBytes = 256 * 1024;

struct Index { unsigned x, y, z; };

enum Kind : uint8_t { kRunning = 0, kShfl, kShflXor, kShflUp, kBallot, kSync, kShflDown };
inline const char* kind_name(uint8_t k) {
    static const char* const names[] = {"(no collective)", "__shfl", "__shfl_xor", "__shfl_up", "__ballot", "__syncthreads", "__shfl_down"};
    return k < 7 ? names[k] : "?";
}

struct Lane {
#ifdef SIMT_UCONTEXT
    ucontext_t ctx;
#else
    void* sp = nullptr;
#endif
    unsigned char* stack = nullptr;     // kStackBytes above one guard page
    void* fake_stack = nullptr;
    uint8_t kind = kRunning, size = 0;  // the collective the lane waits in
    uint8_t width = kWidth;             // ... and the lanes that take part in it: the aligned group of `width` around the lane
    bool done = false;
    uint64_t ops = 0;                   // collectives finished
};

struct Machine {
    Lane lanes[kMaxBlock];
    int cur = -1;
    unsigned block_threads = 0;
    uint64_t xchg[2][kWidth];           // one wave runs at a time between barriers; double-buffered by collective parity
    const std::function<void()>* body = nullptr;
    uint64_t launches = 0, block = 0;
#ifdef SIMT_UCONTEXT
    ucontext_t sched;
#else
    void* sched_sp = nullptr;
#endif
    const void* sched_bottom = nullptr;
    size_t sched_size = 0;
};
inline Machine g;

}  // namespace simt

inline simt::Index threadIdx{0, 0, 0}, blockIdx{0, 0, 0};
inline dim3 blockDim, gridDim;

namespace simt {

[[noreturn]] inline void fail(int wave, const char* what) {
    const Lane& l0 = g.lanes[wave * kWidth];
    fprintf(stderr, "simt: launch %llu block %llu wave %d, collective %llu: %s\n", (unsigned long long)g.launches,
            (unsigned long long)g.block, wave, (unsigned long long)l0.ops, what);
    for (int i = 0; i < kWidth; ++i) {
        const Lane& l = g.lanes[wave * kWidth + i];
        fprintf(stderr, "  lane %2d: %s size %d after %llu collectives\n", i, l.done ? "returned" : kind_name(l.kind), int(l.size),
                (unsigned long long)l.ops);
    }
    fflush(stderr);
    _Exit(3);
}

#ifndef SIMT_UCONTEXT
// callee-saved registers on the old stack, stack pointers swapped, the new stack's popped
extern "C" void simt_switch(void** save_sp, void* next_sp);
asm(R"(
.text
.globl simt_switch
.type simt_switch,@function
simt_switch:
    pushq %rbp
    pushq %rbx
    pushq %r12
    pushq %r13
    pushq %r14
    pushq %r15
    movq %rsp, (%rdi)
    movq %rsi, %rsp
    popq %r15
    popq %r14
    popq %r13
    popq %r12
    popq %rbx
    popq %rbp
    ret
.size simt_switch,.-simt_switch
.section .note.GNU-stack,"",@progbits
.text
)");
#endif

inline void to_lane(Lane& l) {
#ifdef SIMT_ASAN
    void* fake = nullptr;
    __sanitizer_start_switch_fiber(&fake, l.stack, kStackBytes);
#endif
#ifdef SIMT_UCONTEXT
    swapcontext(&g.sched, &l.ctx);
#else
    simt_switch(&g.sched_sp, l.sp);
#endif
#ifdef SIMT_ASAN
    __sanitizer_finish_switch_fiber(fake, nullptr, nullptr);
#endif
}

inline void to_scheduler(Lane& l, bool leaving) {
#ifdef SIMT_ASAN
    __sanitizer_start_switch_fiber(leaving ? nullptr : &l.fake_stack, g.sched_bottom, g.sched_size);
#endif
#ifdef SIMT_UCONTEXT
    swapcontext(&l.ctx, &g.sched);
#else
    simt_switch(&l.sp, g.sched_sp);
#endif
#ifdef SIMT_ASAN
    __sanitizer_finish_switch_fiber(l.fake_stack, nullptr, nullptr);
#endif
    (void)leaving;
}

inline void lane_entry() {
#ifdef SIMT_ASAN
    __sanitizer_finish_switch_fiber(nullptr, &g.sched_bottom, &g.sched_size);
#endif
    Lane& l = g.lanes[g.cur];
    (*g.body)();
    l.done = true;
    to_scheduler(l, true);
    abort();    // a finished lane is never resumed
}

inline void prepare_lane(Lane& l) {
    if (!l.stack) {
        void* m = mmap(nullptr, kStackBytes + 4096, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (m == MAP_FAILED) { perror("simt: mmap"); _Exit(4); }
        mprotect(m, 4096, PROT_NONE);
        l.stack = static_cast<unsigned char*>(m) + 4096;
    }
    l.kind = kRunning; l.size = 0; l.width = kWidth; l.done = false; l.ops = 0; l.fake_stack = nullptr;
#ifdef SIMT_UCONTEXT
    getcontext(&l.ctx);
    l.ctx.uc_stack.ss_sp = l.stack;
    l.ctx.uc_stack.ss_size = kStackBytes;
    l.ctx.uc_link = nullptr;
    makecontext(&l.ctx, lane_entry, 0);
#else
    // six popped registers, then the `ret` into lane_entry with the stack as after a call (16n + 8)
    void** top = reinterpret_cast<void**>(l.stack + kStackBytes);
    *--top = nullptr;                                    // return address of lane_entry (it never returns)
    *--top = reinterpret_cast<void*>(&lane_entry);
    for (int i = 0; i < 6; ++i) *--top = nullptr;
    l.sp = top;
#endif
}

// the calling lane posts `bits`, waits for its wave and gets the wave's posted operands
inline const uint64_t* collective(uint8_t kind, uint8_t size, uint64_t bits, int width = kWidth) {
    Lane& l = g.lanes[g.cur];
    if (width < 1 || width > kWidth || (width & (width - 1))) { fprintf(stderr, "simt: collective of width %d\n", width); _Exit(4); }
    l.kind = kind;
    l.size = size;
    l.width = uint8_t(width);
    g.xchg[l.ops & 1][g.cur & (kWidth - 1)] = bits;
    to_scheduler(l, false);
    const uint64_t* got = g.xchg[l.ops & 1];
    l.kind = kRunning;
    ++l.ops;
    return got;
}

// runs wave w until it has returned (true) or stands in __syncthreads (false)
inline bool run_wave(int w) {
    Lane* L = g.lanes + w * kWidth;
    for (;;) {
        for (int i = 0; i < kWidth; ++i) {
            if (L[i].done) continue;
            g.cur = w * kWidth + i;
            threadIdx.x = unsigned(g.cur);
            to_lane(L[i]);
        }
        int done = 0, sync = 0;
        for (int i = 0; i < kWidth; ++i) { done += L[i].done; sync += !L[i].done && L[i].kind == kSync; }
        if (done == kWidth) return true;
        // every waiting lane's group (the whole wave, but for a narrower __shfl_down) waits with it, in the same collective
        for (int i = 0; i < kWidth;) {
            if (L[i].done) { ++i; continue; }
            const int width = L[i].width, first = i & ~(width - 1);
            for (int j = first; j < first + width; ++j) {
                if (L[j].done) fail(w, "lanes have returned while others of the wave wait in a collective");
                if (L[j].kind != L[i].kind || L[j].size != L[i].size || L[j].ops != L[i].ops || L[j].width != L[i].width)
                    fail(w, "the lanes of the wave are out of step (kind or operand size of the collective differs)");
            }
            i = first + width;
        }
        if (sync) return false;
    }
}

inline void launch(dim3 grid, dim3 block, const std::function<void()>& body) {
    if (block.x == 0 || block.x % kWidth || block.x > kMaxBlock || block.y != 1 || block.z != 1 || grid.y != 1 || grid.z != 1) {
        fprintf(stderr, "simt: launch shape (%u,%u,%u) x (%u,%u,%u) is not one this stand-in runs\n", grid.x, grid.y, grid.z,
                block.x, block.y, block.z);
        _Exit(4);
    }
    ++g.launches;
    g.body = &body;
    g.block_threads = block.x;
    blockDim = block;
    gridDim = grid;
    const int waves = int(block.x) / kWidth;
    for (unsigned b = 0; b < grid.x; ++b) {
        g.block = b;
        blockIdx.x = b;
        for (unsigned i = 0; i < block.x; ++i) prepare_lane(g.lanes[i]);
        bool finished[kMaxBlock / kWidth] = {};
        for (bool all = false; !all;) {
            all = true;
            for (int w = 0; w < waves; ++w) {
                if (!finished[w]) finished[w] = run_wave(w);
                all = all && finished[w];
            }
            // every wave that has not returned stands in __syncthreads: the barrier opens
        }
    }
    g.body = nullptr;
    g.cur = -1;
}

template <typename T>
inline uint64_t to_bits(T v) {
    static_assert(std::is_trivially_copyable<T>::value && sizeof(T) <= 8, "shuffle operand");
    uint64_t b = 0;
    memcpy(&b, &v, sizeof(T));
    return b;
}
template <typename T>
inline T from_bits(uint64_t b) {
    T v;
    memcpy(&v, &b, sizeof(T));
    return v;
}

}  // namespace simt

template <typename T>
inline T __shfl(T v, int src, int width = simt::kWidth) {
    (void)width;
    const uint64_t* w = simt::collective(simt::kShfl, sizeof(T), simt::to_bits(v));
    return simt::from_bits<T>(w[src & (simt::kWidth - 1)]);
}
template <typename T>
inline T __shfl_xor(T v, int mask, int width = simt::kWidth) {
    (void)width;
    const int lane = simt::g.cur & (simt::kWidth - 1);
    const uint64_t* w = simt::collective(simt::kShflXor, sizeof(T), simt::to_bits(v));
    return simt::from_bits<T>(w[(lane ^ mask) & (simt::kWidth - 1)]);
}
template <typename T>
inline T __shfl_up(T v, unsigned delta, int width = simt::kWidth) {
    (void)width;
    const int lane = simt::g.cur & (simt::kWidth - 1);
    const uint64_t* w = simt::collective(simt::kShflUp, sizeof(T), simt::to_bits(v));
    return simt::from_bits<T>(w[unsigned(lane) < delta ? lane : lane - int(delta)]);
}
template <typename T>
inline T __shfl_down(T v, unsigned delta, int width = simt::kWidth) {
    const int lane = simt::g.cur & (simt::kWidth - 1);
    const uint64_t* w = simt::collective(simt::kShflDown, sizeof(T), simt::to_bits(v), width);
    return simt::from_bits<T>(w[unsigned(lane & (width - 1)) + delta >= unsigned(width) ? lane : lane + int(delta)]);
}
inline unsigned long long __ballot(int pred) {
    const uint64_t* w = simt::collective(simt::kBallot, sizeof(int), pred ? 1 : 0);
    unsigned long long m = 0;
    for (int i = 0; i < simt::kWidth; ++i) m |= (unsigned long long)(w[i] & 1) << i;
    return m;
}
inline void __syncthreads() { simt::collective(simt::kSync, 0, 0); }

// hipLaunchKernelGGL((kernel<...>), grid, block, lds_bytes, stream, args...): the blocks one after another, now
template <typename... P, typename... A>
inline void hipLaunchKernelGGL(void (*kernel)(P...), dim3 grid, dim3 block, size_t, hipStream_t, A... args) {
    const std::function<void()> body = [=] { kernel(args...); };
    simt::launch(grid, block, body);
}
