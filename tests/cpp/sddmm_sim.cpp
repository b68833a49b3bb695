// sddmm_sim — TEST CODE.  csrc/sddmm.hip with what it includes (sddmm_slice_walk.inc, sddmm_half_kernel.hpp), unchanged,
// compiled with the HOST compiler over tests/cpp/simt (a stand-in <hip/hip_runtime.h> that runs every lane of a workgroup
// as a fiber) and driven through the real extern "C" entry points: mi355_spmv_sddmm_create or _create_half, then the
// object's set_alpha_beta / execute / destroy, so the choice of C from k, u_vec / v_vec and the valued / pattern dispatch
// run as well.  One program for both tables (tests/sddmm_cases.py, tests/sddmm_half_cases.py): the matrix record's type
// word says which create it is.  Where the host compiler has no _Float16, half_convert.hpp holds binary16 as uint16_t and
// converts in software.  Built with -fsanitize=address,undefined (tests/cpp/Makefile).
//
//   sddmm_sim BATCH OUT      reads records from BATCH, writes one result per run record to OUT
//
// Records are int64 words followed by raw little-endian arrays (tests/sddmm_cases.py writes them, write_batch):
//   1  matrix    off_type type n_rows n_cols nnz ap_off aj_off ax_off | Ap[n_rows + 1] Aj[nnz] Ax[nnz] O0[nnz]
//   2  operands  kf | U[n_rows * kf] V[n_cols * kf]              (row-major, kf columns: a run takes columns c0 .. c0 + k)
//   4  run       k c0 ldu ldv u_off v_off out_off valued out0_nan nan_bits | alpha beta (2 doubles)
//   0  end
// type = the MI355_VAL_* of U and V.  F32 / F64: mi355_spmv_sddmm_create, and Ax, O0 and out have that type too.  F16 /
// BF16: mi355_spmv_sddmm_create_half (the object must then report F32 values and that type of U and V), U and V are
// 16-bit patterns, and Ax, O0 and out are fp32.  nan_bits = the bit pattern of a NaN of U's and V's type.
// *_off = elements between a 64-byte boundary and the operand's base (0 or 1).  Every operand is an allocation of its
// own, exactly as long as the call may touch: U is (n_rows - 1) * ldu + k elements, V likewise, out nnz — so a read or
// write one element outside is a report.  Padding columns of U and V hold nan_bits; out holds O0, or NaN with out0_nan.
// A result is: status, count = nnz, then out as count values.
#include <cstring>
#include <limits>
#include <vector>

#include "../../spmv-samples_amd/csrc/sddmm.hip"

#define SIM_NAME "sddmm_sim"
#include "sim_io.hpp"

namespace {

struct State {
    int off_type = 0, type = 0;
    size_t ub = 0, vb = 0;          // bytes of an element of U and V, and of Ax, O0 and out
    int64_t n_rows = 0, n_cols = 0, nnz = 0, kf = 0;
    Buf Ap, Aj, Ax;
    std::vector<char> O0, U, V;     // O0: nnz values; U, V: kf columns, dense
    mi355_spmv_sddmm* plan = nullptr;
};

// `rows` rows of k elements, columns c0 .. c0 + k of the dense src, at stride ld in dst; every other element is nan_bits
void place(char* dst, size_t elems, const std::vector<char>& src, const State& s, int64_t rows, int64_t k, int64_t c0, int64_t ld,
           int64_t nan_bits) {
    for (size_t i = 0; i < elems; ++i) memcpy(dst + i * s.ub, &nan_bits, s.ub);
    for (int64_t r = 0; r < rows; ++r) memcpy(dst + size_t(r * ld) * s.ub, src.data() + size_t(r * s.kf + c0) * s.ub, size_t(k) * s.ub);
}

void run(State& s) {
    const int64_t k = word(), c0 = word(), ldu = word(), ldv = word(), u_off = word(), v_off = word(), out_off = word(),
                  valued = word(), out0_nan = word(), nan_bits = word();
    double ab[2];
    get(ab, sizeof(ab));
    if (!s.plan || k < 1 || c0 < 0 || c0 + k > s.kf || ldu < k || ldv < k) { fprintf(stderr, "sddmm_sim: bad run record\n"); exit(4); }
    const size_t u_elems = s.n_rows ? size_t(s.n_rows - 1) * ldu + k : 0, v_elems = s.n_cols ? size_t(s.n_cols - 1) * ldv + k : 0;
    Buf bu, bv, bo;
    bu.alloc(u_elems, s.ub, u_off);
    bv.alloc(v_elems, s.ub, v_off);
    bo.alloc(size_t(s.nnz), s.vb, out_off);
    place(bu.p, u_elems, s.U, s, s.n_rows, k, c0, ldu, nan_bits);
    place(bv.p, v_elems, s.V, s, s.n_cols, k, c0, ldv, nan_bits);
    const float nan32 = std::numeric_limits<float>::quiet_NaN();
    const double nan64 = std::numeric_limits<double>::quiet_NaN();
    const void* nan = s.vb == 8 ? static_cast<const void*>(&nan64) : &nan32;
    for (size_t n = 0; n < size_t(s.nnz); ++n) memcpy(bo.p + n * s.vb, out0_nan ? nan : s.O0.data() + n * s.vb, s.vb);
    int64_t st = mi355_spmv_sddmm_set_alpha_beta(s.plan, ab[0], ab[1]);
    if (st == MI355_SPMV_OK) st = mi355_spmv_sddmm_execute(s.plan, valued ? s.Ax.p : nullptr, bu.p, ldu, bv.p, ldv, bo.p, int32_t(k), nullptr);
    if (st != MI355_SPMV_OK) fprintf(stderr, "sddmm_sim: execute -> %d (%s)\n", int(st), mi355::g_error);
    put(&st, 8);
    put(&s.nnz, 8);
    put(bo.p, size_t(s.nnz) * s.vb);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: sddmm_sim BATCH OUT\n"); return 2; }
    g_in = fopen(argv[1], "rb");
    g_out = fopen(argv[2], "wb");
    if (!g_in || !g_out) { perror("sddmm_sim: open"); return 2; }
    State s;
    for (;;) {
        const int64_t tag = word();
        if (tag == 0) break;
        if (tag == 1) {
            if (s.plan) { mi355_spmv_sddmm_destroy(s.plan); s.plan = nullptr; }
            s.off_type = int(word()); s.type = int(word());
            s.n_rows = word(); s.n_cols = word(); s.nnz = word();
            const int64_t ap_off = word(), aj_off = word(), ax_off = word();
            const bool half = s.type == MI355_VAL_F16 || s.type == MI355_VAL_BF16;
            const size_t ob = s.off_type == MI355_OFF_I64 ? 8 : 4;
            s.ub = half ? 2 : s.type == MI355_VAL_F64 ? 8 : 4;
            s.vb = s.type == MI355_VAL_F64 ? 8 : 4;
            s.Ap.alloc(size_t(s.n_rows) + 1, ob, ap_off);
            s.Aj.alloc(size_t(s.nnz), 4, aj_off);
            s.Ax.alloc(size_t(s.nnz), s.vb, ax_off);
            s.O0.resize(size_t(s.nnz) * s.vb);
            get(s.Ap.p, (size_t(s.n_rows) + 1) * ob);
            get(s.Aj.p, size_t(s.nnz) * 4);
            get(s.Ax.p, size_t(s.nnz) * s.vb);
            get(s.O0.data(), s.O0.size());
            s.kf = 0;
            const int32_t* Aj = reinterpret_cast<const int32_t*>(s.Aj.p);
            const int st = half ? mi355_spmv_sddmm_create_half(&s.plan, s.off_type, s.type, int32_t(s.n_rows), int32_t(s.n_cols), s.nnz, s.Ap.p, Aj)
                                : mi355_spmv_sddmm_create(&s.plan, s.off_type, s.type, int32_t(s.n_rows), int32_t(s.n_cols), s.nnz, s.Ap.p, Aj);
            if (st != MI355_SPMV_OK) { fprintf(stderr, "sddmm_sim: create%s -> %d (%s)\n", half ? "_half" : "", st, mi355::g_error); return 5; }
            int val_type = -1, vec_type = -1;
            if (half && (mi355_spmv_sddmm_get_types(s.plan, &val_type, &vec_type) != MI355_SPMV_OK || val_type != MI355_VAL_F32 ||
                         vec_type != s.type)) {
                fprintf(stderr, "sddmm_sim: get_types -> (%d, %d)\n", val_type, vec_type);
                return 5;
            }
        } else if (tag == 2) {
            s.kf = word();
            s.U.resize(size_t(s.n_rows * s.kf) * s.ub);
            s.V.resize(size_t(s.n_cols * s.kf) * s.ub);
            get(s.U.data(), s.U.size());
            get(s.V.data(), s.V.size());
        } else if (tag == 4) {
            run(s);
        } else {
            fprintf(stderr, "sddmm_sim: unknown record %lld\n", (long long)tag);
            return 4;
        }
    }
    if (s.plan && mi355_spmv_sddmm_destroy(s.plan) != MI355_SPMV_OK) return 5;
    const int64_t end = -1;
    put(&end, 8);
    if (fclose(g_out) != 0) return 4;
    fclose(g_in);
    return 0;
}
