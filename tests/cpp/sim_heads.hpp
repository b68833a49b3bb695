// sim_heads.hpp — TEST CODE shared by attention_heads_sim and attention_bwd_heads_sim, included after sim_io.hpp and
// sim_operand.hpp: an operand of several heads as ONE allocation exactly as long as a heads call may touch, so that a read
// or write one element outside is a sanitizer report, and the comparison of a heads execute with the single-head executes.
#pragma once

#include <cstdint>
#include <cstring>
#include <vector>

namespace {

// `heads` matrices of rows x width elements of eb bytes at leading dimension ld, head h beginning h * stride elements
// behind head 0 (stride 0: one matrix that every head shares).  Every element starts as pad_bits; read() then takes the
// heads' compact values from the batch file.  p stays null until make(): an operand that a run does not pass.
struct HeadsOperand : Buf {
    int64_t heads = 0, rows = 0, width = 0, ld = 0, stride = 0, pad_bits = 0, elems = 0;
    size_t eb = 0;
    int64_t stored() const { return stride == 0 ? 1 : heads; }      // matrices that exist
    void make(int64_t heads_, int64_t rows_, int64_t width_, int64_t ld_, int64_t stride_, size_t eb_, int64_t off, int64_t pad_bits_) {
        heads = heads_; rows = rows_; width = width_; ld = ld_; stride = stride_; eb = eb_; pad_bits = pad_bits_;
        elems = rows > 0 ? (stored() - 1) * stride + int64_t(span(rows, ld, width)) : 0;
        alloc(size_t(elems), eb, size_t(off));
        fill(p, size_t(elems), pad_bits, eb);
    }
    char* head(int64_t h) const { return p ? p + size_t(h * stride) * eb : nullptr; }
    void read() {
        std::vector<char> row(size_t(width) * eb);
        for (int64_t h = 0; h < stored(); ++h)
            for (int64_t r = 0; r < rows; ++r) {
                get(row.data(), row.size());
                memcpy(head(h) + size_t(r * ld) * eb, row.data(), row.size());
            }
    }
    // the elements outside every head's rows x width that no longer hold pad_bits
    int64_t lost() const {
        if (!p) return 0;
        std::vector<char> inside(size_t(elems), 0);
        for (int64_t h = 0; h < stored(); ++h)
            for (int64_t r = 0; r < rows; ++r) memset(inside.data() + h * stride + r * ld, 1, size_t(width));
        int64_t n = 0;
        for (int64_t i = 0; i < elems; ++i) n += !inside[size_t(i)] && memcmp(p + size_t(i) * eb, &pad_bits, eb) != 0;
        return n;
    }
    // every head's rows, compact, to the result file
    void write() const {
        for (int64_t h = 0; p && h < stored(); ++h)
            for (int64_t r = 0; r < rows; ++r) put(head(h) + size_t(r * ld) * eb, size_t(width) * eb);
    }
    // an output of the same layout, all canary
    void like(const HeadsOperand& o) { make(o.heads, o.rows, o.width, o.ld, o.stride, o.eb, (o.p - static_cast<char*>(o.raw)) / int64_t(o.eb), o.pad_bits); }
};

// The bytes of a scratch behind its first `used` bytes are set to a pattern before a heads execute, and must hold it after:
// an execute of fewer heads than reserved leaves the other heads' scratch alone.
void poison_rest(void* scratch, size_t bytes, size_t used) {
    if (scratch && bytes > used) memset(static_cast<char*>(scratch) + used, 0xA5, bytes - used);
}
int64_t rest_touched(const void* scratch, size_t bytes, size_t used) {
    int64_t n = 0;
    for (size_t i = used; scratch && i < bytes; ++i) n += static_cast<const unsigned char*>(scratch)[i] != 0xA5;
    return n;
}

}  // namespace
