// sim_operand.hpp — TEST CODE shared by multi_sim, attention_sim and attention_bwd_sim, included after sim_io.hpp: dense
// operands as bit patterns.  Element sizes come from the MI355_VAL_* type words and every fill value arrives as bits, so
// nothing here knows a floating-point format.
#pragma once

#include <cstring>
#include <vector>

namespace {

size_t type_bytes(int type) { return type == MI355_VAL_F64 ? 8 : type == MI355_VAL_F16 || type == MI355_VAL_BF16 ? 2 : 4; }

// n elements at dst, each the low sizeof(W) bytes of bits (a copy of constant size: no call per element)
template <typename W>
void fill_as(char* dst, size_t n, int64_t bits) {
    const W w = W(bits);
    for (size_t i = 0; i < n; ++i) memcpy(dst + i * sizeof(W), &w, sizeof(W));
}
void fill(char* dst, size_t n, int64_t bits, size_t eb) {
    eb == 8 ? fill_as<uint64_t>(dst, n, bits) : eb == 4 ? fill_as<uint32_t>(dst, n, bits) : fill_as<uint16_t>(dst, n, bits);
}

// the elements a call may touch of `rows` rows of `width` elements at leading dimension ld
size_t span(int64_t rows, int64_t ld, int64_t width) { return rows > 0 ? size_t((rows - 1) * ld + width) : 0; }

// rows x width elements of eb bytes at leading dimension ld: an allocation of its own, exactly span() long, whose base is
// `off` elements past a 64-byte boundary — a read or write one element outside is a sanitizer report.  p stays null until
// make(): an output that a run does not ask for.
struct Operand : Buf {
    int64_t rows = 0, width = 0, ld = 0, pad_bits = 0;
    size_t eb = 0;
    // every element pad_bits (the NaN of an input's padding columns, the canary of an output); then, with src, row r =
    // columns col0 .. col0 + width of row r of src, whose leading dimension is src_ld
    void make(int64_t rows_, int64_t width_, int64_t ld_, size_t eb_, int64_t off, int64_t pad_bits_, const char* src = nullptr,
              int64_t src_ld = 0, int64_t col0 = 0) {
        rows = rows_; width = width_; ld = ld_; eb = eb_; pad_bits = pad_bits_;
        alloc(span(rows, ld, width), eb, size_t(off));
        fill(p, span(rows, ld, width), pad_bits, eb);
        for (int64_t r = 0; src && r < rows; ++r) memcpy(p + size_t(r * ld) * eb, src + size_t(r * src_ld + col0) * eb, size_t(width) * eb);
    }
    // rows x width compact elements from the batch file
    void read(int64_t rows_, int64_t width_, int64_t ld_, size_t eb_, int64_t off, int64_t pad_bits_) {
        std::vector<char> full(size_t(rows_ * width_) * eb_);
        get(full.data(), full.size());
        make(rows_, width_, ld_, eb_, off, pad_bits_, full.data(), width_);
    }
    // the padding elements that no longer hold pad_bits
    int64_t lost() const {
        int64_t n = 0;
        for (int64_t r = 0; p && r + 1 < rows; ++r)
            for (int64_t j = width; j < ld; ++j) n += memcmp(p + size_t(r * ld + j) * eb, &pad_bits, eb) != 0;
        return n;
    }
    // the rows, compact, to the result file
    void write() const {
        for (int64_t r = 0; p && r < rows; ++r) put(p + size_t(r * ld) * eb, size_t(width) * eb);
    }
};

}  // namespace
