// sim_runtime.hpp — TEST CODE shared by multi_perm_sim and coo_sim: what csrc/multi_perm.hip and csrc/coo_csr.hip use of the
// HIP runtime and the stand-in (tests/cpp/simt/hip/hip_runtime.h) leaves out, because csrc/multi.hip copies nothing between
// host and device and has no atomics.  Device memory is host memory here, a stream runs at once, and the lanes of a kernel
// are fibers of one thread: an atomic is its plain operation.  Included before the unit that needs it.
#pragma once

#include <hip/hip_runtime.h>

#include <cstring>

enum hipMemcpyKind { hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2, hipMemcpyDeviceToDevice = 3 };
inline hipError_t hipMemcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind) { memcpy(dst, src, bytes); return hipSuccess; }
inline hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind, hipStream_t) { memcpy(dst, src, bytes); return hipSuccess; }
inline hipError_t hipMemsetAsync(void* dst, int value, size_t bytes, hipStream_t) { memset(dst, value, bytes); return hipSuccess; }
inline hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
inline unsigned long long atomicMin(unsigned long long* p, unsigned long long v) {
    const unsigned long long old = *p;
    if (v < old) *p = v;
    return old;
}
inline unsigned long long atomicAdd(unsigned long long* p, unsigned long long v) {
    const unsigned long long old = *p;
    *p = old + v;
    return old;
}
