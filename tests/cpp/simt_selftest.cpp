// simt_selftest — TEST CODE.  What tests/cpp/simt/hip/hip_runtime.h promises, on kernels of a few lines: the host
// execution of csrc/multi.hip (multi_sim.cpp) means what it says only while these hold.
//   simt_selftest semantics   shuffles (__shfl_down under a width, its groups running apart), __ffsll, ballot, barrier, __shared__ and its reuse behind a second barrier, block order, the
//                             hipMalloc fill:                                                   exit status 0
//   simt_selftest returned    a lane returns while the others of its wave wait in a collective: exit status 3
//   simt_selftest kind        one lane calls another collective than the others:                exit status 3
//   simt_selftest size        one lane's operand has another size:                              exit status 3
//   simt_selftest down        one lane calls __shfl_down where the others call __shfl_up:       exit status 3
#include <hip/hip_runtime.h>

#include <cstring>

__global__ void semantics(int* ok, int* order) {
    __shared__ int total[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x / 64;
    bool good = true;
    for (unsigned d = 0; d < 64; d = d ? d * 2 : 1)         // __shfl_up: the lane's own value where lane < d
        good = good && __shfl_up(lane + 100, d) == (unsigned(lane) < d ? lane + 100 : lane + 100 - int(d));
    for (unsigned d = 0; d < 64; d = d ? d * 2 : 1)         // __shfl_down: lanes 64 - d .. 63 keep their own value
        good = good && __shfl_down(lane + 100, d) == (unsigned(lane) + d >= 64 ? lane + 100 : lane + 100 + int(d));
    good = good && __shfl_down(int64_t(lane) << 40, 3) == int64_t(lane < 61 ? lane + 3 : lane) << 40 && __popcll(~0ull) == 64 && __popcll(0) == 0;
    good = good && __shfl(lane, 64 + 3) == 3 && __shfl(lane, 63) == 63 && __shfl(lane, -1) == 63;   // src & 63
    good = good && __shfl_xor(lane, 8) == (lane ^ 8) && __shfl_xor(double(lane), 1) == double(lane ^ 1);
    good = good && __shfl(int64_t(lane) << 40, 5) == int64_t(5) << 40 && __shfl(float(lane) / 4, 9) == 2.25f;
    good = good && __ballot(lane & 1) == 0xAAAAAAAAAAAAAAAAull && __ballot(lane == 63) == 1ull << 63 && __ballot(0) == 0;
    good = good && __clzll(0) == 64 && __clzll(1) == 63;
    good = good && __ffsll(0) == 0 && __ffsll(1) == 1 && __ffsll(0x60) == 6 && __ffsll((long long)(1ull << 63)) == 64;
    for (unsigned d = 1; d < 8; d *= 2)                     // __shfl_down under a width: the last d lanes of each group keep theirs
        good = good && __shfl_down(lane + 100, d, 8) == ((lane & 7) + d >= 8 ? lane + 100 : lane + 100 + int(d));
    if (lane == 0) total[wave] = int(blockIdx.x) * 10 + wave;
    __syncthreads();                                        // the waves of a block meet here, and only here
    for (int w = 0; w < 4; ++w) good = good && total[w] == int(blockIdx.x) * 10 + w;
    ok[blockIdx.x * blockDim.x + threadIdx.x] = good;
    if (threadIdx.x == 0) order[blockIdx.x] = order[gridDim.x]++;      // blocks run one after another, in order
}

// block_exclusive_scan of csrc/coo_csr.hip in small: a __shared__ array that lane 63 of each of the four waves writes, all
// read behind a barrier, and the next call writes again behind a second one
__device__ inline int sum_before(int own) {
    __shared__ int wave_sum[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = own;
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
    }
    if (lane == 63) wave_sum[wave] = inc;
    __syncthreads();
    int before = inc - own;
    for (int w = 0; w < wave; ++w) before += wave_sum[w];
    __syncthreads();
    return before;
}

__global__ void lds_reuse(int* ok) {
    const int t = threadIdx.x, b = blockIdx.x;
    const int ones = sum_before(1), ramp = sum_before(t + b), again = sum_before(2);
    ok[b * blockDim.x + t] = ones == t && ramp == t * (t - 1) / 2 + b * t && again == 2 * t;
}

// groups of a narrower __shfl_down run apart (csrc/functor_kernel.inc, rows_body): the odd groups of 8 lanes return at
// once, group 0 goes a second round, and every group sums its own lanes only
__global__ void groups_apart(int* sum) {
    const int lane = threadIdx.x & 63, group = lane / 8;
    if (group & 1) return;
    for (int round = 0; round < (group == 0 ? 2 : 1); ++round) {
        int t = lane + round;
        for (int o = 4; o >= 1; o >>= 1) t += __shfl_down(t, o, 8);
        if ((lane & 7) == 0) sum[(threadIdx.x / 8) * 2 + round] = t;
    }
}

__global__ void out_of_step(int mode) {
    const int lane = threadIdx.x & 63;
    if (lane == 7) {
        if (mode == 0) return;
        if (mode == 1) { __ballot(1); return; }
        if (mode == 2) { __shfl(double(lane), 0); return; }
        if (mode == 3) { __shfl_down(lane, 1); return; }
    }
    if (mode == 3) __shfl_up(lane, 1);
    else __shfl(lane, 0);
}

int main(int argc, char** argv) {
    const char* what = argc > 1 ? argv[1] : "";
    if (!strcmp(what, "semantics")) {
        unsigned char* fill = nullptr;
        if (hipMalloc(&fill, 300) != hipSuccess) return 1;
        for (int i = 0; i < 300; ++i)
            if (fill[i] != 0x5A) { fprintf(stderr, "hipMalloc: byte %d is not 0x5A\n", i); return 1; }
        if (reinterpret_cast<uintptr_t>(fill) % 256) { fprintf(stderr, "hipMalloc: not 256-byte aligned\n"); return 1; }
        hipFree(fill);
        static int ok[3 * 256], order[3 + 1];
        hipLaunchKernelGGL(semantics, dim3(3), dim3(256), 0, nullptr, ok, order);
        for (int i = 0; i < 3 * 256; ++i)
            if (!ok[i]) { fprintf(stderr, "a collective's result is wrong in thread %d\n", i); return 1; }
        for (int b = 0; b < 3; ++b)
            if (order[b] != b) { fprintf(stderr, "block %d ran out of order\n", b); return 1; }
        memset(ok, 0, sizeof(ok));
        hipLaunchKernelGGL(lds_reuse, dim3(3), dim3(256), 0, nullptr, ok);
        for (int i = 0; i < 3 * 256; ++i)
            if (!ok[i]) { fprintf(stderr, "a sum over __shared__ reused behind a second barrier is wrong in thread %d\n", i); return 1; }
        static int sum[2 * 32];
        hipLaunchKernelGGL(groups_apart, dim3(1), dim3(256), 0, nullptr, sum);
        for (int g8 = 0; g8 < 32; ++g8)
            for (int round = 0; round < 2; ++round) {
                const bool ran = !(g8 & 1) && round < ((g8 & 7) == 0 ? 2 : 1);
                const int first = (g8 & 7) * 8, want = ran ? 8 * first + 28 + 8 * round : 0;
                if (sum[g8 * 2 + round] != want) { fprintf(stderr, "groups of 8 lanes running apart: group %d round %d sums to %d\n", g8, round, sum[g8 * 2 + round]); return 1; }
            }
        return alignof(float4) == 16 && alignof(double2) == 16 ? 0 : 1;
    }
    const int mode = !strcmp(what, "returned") ? 0 : !strcmp(what, "kind") ? 1 : !strcmp(what, "size") ? 2 : !strcmp(what, "down") ? 3 : -1;
    if (mode < 0) { fprintf(stderr, "usage: simt_selftest semantics | returned | kind | size | down\n"); return 2; }
    hipLaunchKernelGGL(out_of_step, dim3(1), dim3(128), 0, nullptr, mode);
    return 0;   // not reached: the stand-in ends the program with status 3
}
