// sim_io.hpp — TEST CODE shared by the host simulation programs (each defines SIM_NAME, its own name in its messages, and
// includes its unit of csrc/ first): the two functions that those call and the library defines in other
// units, an allocation placed against a 64-byte boundary, and the reading and writing of the batch and result files.
#pragma once

#include <cstdarg>
#include <cstdio>
#include <cstdlib>

namespace mi355 {
static char g_error[512];
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
}
}  // namespace mi355
extern "C" int mi355_spmv_stream_synchronize(void*) { return MI355_SPMV_OK; }

namespace {

struct Buf {    // an allocation whose base is `off` elements past a 64-byte boundary
    void* raw = nullptr;
    char* p = nullptr;
    void alloc(size_t elems, size_t elem_bytes, size_t off) {
        release();
        if (posix_memalign(&raw, 64, (elems + off) * elem_bytes + (elems + off == 0)) != 0) { perror(SIM_NAME ": allocation"); exit(4); }
        p = static_cast<char*>(raw) + off * elem_bytes;
    }
    void release() { free(raw); raw = nullptr; p = nullptr; }
    ~Buf() { release(); }
};

FILE* g_in;
FILE* g_out;

void get(void* dst, size_t bytes) {
    if (bytes && fread(dst, 1, bytes, g_in) != bytes) { fprintf(stderr, SIM_NAME ": batch file ends inside a record\n"); exit(4); }
}
int64_t word() { int64_t v; get(&v, 8); return v; }
void put(const void* src, size_t bytes) {
    if (bytes && fwrite(src, 1, bytes, g_out) != bytes) { perror(SIM_NAME ": write"); exit(4); }
}

}  // namespace
