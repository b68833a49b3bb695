// row_softmax_sim — TEST CODE.  csrc/row_softmax.hip, unchanged, compiled with the HOST compiler over tests/cpp/simt (a
// stand-in <hip/hip_runtime.h> that runs every lane of a workgroup as a fiber) and driven through the real extern "C"
// entry points: mi355_spmv_row_softmax_create, then the object's set_scale / execute / backward / destroy, so the three
// launches of an execute and the object's scratch run as well.  Built with -fsanitize=address,undefined
// (tests/cpp/Makefile).
//
//   row_softmax_sim BATCH OUT      reads records from BATCH, writes one result per run record to OUT
//
// Records are int64 words followed by raw little-endian arrays (tests/row_softmax_cases.py writes them, write_batch):
//   1  matrix    off_type val_type n_rows n_cols nnz ap_off aj_off | Ap[n_rows + 1] Aj[nnz]
//   4  run       backward in_place a_off b_off out_off | scale (1 double) | A[nnz], and B[nnz] of a backward
//   0  end
// A run is execute(x = A, out) or backward(p = A, dp = B, dx = out).  in_place: 0 = out is an allocation of its own
// (filled with NaN), 1 = out is A (out == x; dx == p), 2 = out is B (dx == dp).  *_off = elements between a 64-byte
// boundary and the operand's base.  Every operand is an allocation of its own, exactly nnz elements long — so a read or
// write one element outside is a report.  A result is: status, count = nnz, then out as count values.
#include <cstring>
#include <limits>
#include <vector>

#include "../../spmv-samples_amd/csrc/row_softmax.hip"

#define SIM_NAME "row_softmax_sim"
#include "sim_io.hpp"

namespace {

struct State {
    int off_type = 0, val_type = 0;
    size_t vb = 0;
    int64_t n_rows = 0, n_cols = 0, nnz = 0;
    Buf Ap, Aj;
    mi355_spmv_row_softmax* plan = nullptr;
};

void run(State& s) {
    const int64_t backward = word(), in_place = word(), a_off = word(), b_off = word(), out_off = word();
    double scale;
    get(&scale, sizeof(scale));
    if (!s.plan || in_place < 0 || in_place > 2 || (in_place == 2 && !backward)) { fprintf(stderr, "row_softmax_sim: bad run record\n"); exit(4); }
    Buf ba, bb, bo;
    ba.alloc(size_t(s.nnz), s.vb, a_off);
    get(ba.p, size_t(s.nnz) * s.vb);
    if (backward) {
        bb.alloc(size_t(s.nnz), s.vb, b_off);
        get(bb.p, size_t(s.nnz) * s.vb);
    }
    char* out = in_place == 1 ? ba.p : in_place == 2 ? bb.p : nullptr;
    if (!out) {
        bo.alloc(size_t(s.nnz), s.vb, out_off);
        const float nan32 = std::numeric_limits<float>::quiet_NaN();
        const double nan64 = std::numeric_limits<double>::quiet_NaN();
        const void* nan = s.vb == 8 ? static_cast<const void*>(&nan64) : &nan32;
        for (size_t n = 0; n < size_t(s.nnz); ++n) memcpy(bo.p + n * s.vb, nan, s.vb);
        out = bo.p;
    }
    int64_t st = mi355_spmv_row_softmax_set_scale(s.plan, scale);
    if (st == MI355_SPMV_OK)
        st = backward ? mi355_spmv_row_softmax_backward(s.plan, ba.p, bb.p, out, nullptr) : mi355_spmv_row_softmax_execute(s.plan, ba.p, out, nullptr);
    if (st != MI355_SPMV_OK) fprintf(stderr, "row_softmax_sim: execute -> %d (%s)\n", int(st), mi355::g_error);
    put(&st, 8);
    put(&s.nnz, 8);
    put(out, size_t(s.nnz) * s.vb);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: row_softmax_sim BATCH OUT\n"); return 2; }
    g_in = fopen(argv[1], "rb");
    g_out = fopen(argv[2], "wb");
    if (!g_in || !g_out) { perror("row_softmax_sim: open"); return 2; }
    State s;
    for (;;) {
        const int64_t tag = word();
        if (tag == 0) break;
        if (tag == 1) {
            if (s.plan) { mi355_spmv_row_softmax_destroy(s.plan); s.plan = nullptr; }
            s.off_type = int(word()); s.val_type = int(word());
            s.n_rows = word(); s.n_cols = word(); s.nnz = word();
            const int64_t ap_off = word(), aj_off = word();
            const size_t ob = s.off_type == MI355_OFF_I64 ? 8 : 4;
            s.vb = s.val_type == MI355_VAL_F64 ? 8 : 4;
            s.Ap.alloc(size_t(s.n_rows) + 1, ob, ap_off);
            s.Aj.alloc(size_t(s.nnz), 4, aj_off);
            get(s.Ap.p, (size_t(s.n_rows) + 1) * ob);
            get(s.Aj.p, size_t(s.nnz) * 4);
            const int st = mi355_spmv_row_softmax_create(&s.plan, s.off_type, s.val_type, int32_t(s.n_rows), int32_t(s.n_cols), s.nnz, s.Ap.p,
                                                         reinterpret_cast<const int32_t*>(s.Aj.p));
            if (st != MI355_SPMV_OK) { fprintf(stderr, "row_softmax_sim: create -> %d (%s)\n", st, mi355::g_error); return 5; }
            mi355_spmv_row_softmax_info info;
            if (mi355_spmv_row_softmax_get_info(s.plan, &info) != MI355_SPMV_OK || info.n_slices != (s.n_rows + s.nnz + info.slice_len - 1) / info.slice_len) {
                fprintf(stderr, "row_softmax_sim: get_info\n");
                return 5;
            }
        } else if (tag == 4) {
            run(s);
        } else {
            fprintf(stderr, "row_softmax_sim: unknown record %lld\n", (long long)tag);
            return 4;
        }
    }
    if (s.plan && mi355_spmv_row_softmax_destroy(s.plan) != MI355_SPMV_OK) return 5;
    const int64_t end = -1;
    put(&end, 8);
    if (fclose(g_out) != 0) return 4;
    fclose(g_in);
    return 0;
}
