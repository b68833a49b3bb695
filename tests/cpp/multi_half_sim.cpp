// multi_half_sim — TEST CODE.  csrc/multi.hip (with multi_kernels.hpp and multi_half_kernels.hpp, which it includes),
// unchanged, compiled with the HOST compiler over tests/cpp/simt and driven through the real extern "C" entry points:
// mi355_spmv_multi_create_half / set_alpha_beta / execute / destroy — binary16 and bfloat16 vectors, the matrix in the
// vectors' type and in fp32.  Built with -fsanitize=address,undefined by tests/test_multi_half_sim_cpu.py (the SIM_SAN
// flags of tests/cpp/Makefile).  Where the host compiler has no _Float16, multi_half_kernels.hpp holds binary16 as
// uint16_t and converts in software; the program only moves 16-bit patterns.
//
//   multi_half_sim BATCH OUT      reads records from BATCH, writes one result per run record to OUT
//
// Records are int64 words followed by raw little-endian arrays (tests/multi_half_cases.py writes them, write_batch):
//   1  matrix   off_type vec_type mat_type n_rows n_cols nnz ap_off aj_off ax_off | Ap[n_rows + 1] Aj[nnz] Ax[nnz]
//   2  vectors  kf | X[n_cols * kf] Y0[n_rows * kf]                   (16-bit patterns, row-major, kf columns)
//   3  plan     k_max                                                (destroys the plan before it)
//   4  run      k c0 ldx ldy x_off y_off y0_poison x_pad_bits y_poison_bits canary_bits | alpha beta (2 doubles)
//   0  end
// *_off = elements between a 64-byte boundary and the operand's base (0 or 1).  Every operand is an allocation of its
// own, exactly as long as the call may touch: X is (n_cols - 1) * ldx + k elements, Y likewise — so a read or write one
// element outside is a report.  Padding columns of X hold x_pad_bits (NaN), of Y the canary; with y0_poison the k
// columns of Y hold y_poison_bits (NaN).
// A result is: status, count = n_rows * ldy, then Y as count 16-bit patterns (the missing tail of the last row as canary).
#include <vector>

#include "../../spmv-samples_amd/csrc/multi.hip"

#define SIM_NAME "multi_half_sim"
#include "sim_io.hpp"

namespace {

struct State {
    int off_type = 0, vec_type = 0, mat_type = 0;
    int64_t n_rows = 0, n_cols = 0, nnz = 0, kf = 0;
    Buf Ap, Aj, Ax;
    std::vector<uint16_t> X, Y0;    // kf columns, dense
    mi355_spmv_multi* plan = nullptr;
};

void run(State& s) {
    const int64_t k = word(), c0 = word(), ldx = word(), ldy = word(), x_off = word(), y_off = word(), y0_poison = word();
    const uint16_t x_pad = uint16_t(word()), y_poison = uint16_t(word()), canary = uint16_t(word());
    double ab[2];
    get(ab, sizeof(ab));
    if (!s.plan || k < 1 || c0 < 0 || c0 + k > s.kf || ldx < k || ldy < k) {
        fprintf(stderr, "multi_half_sim: bad run record\n");
        exit(4);
    }
    const size_t x_elems = s.n_cols ? size_t(s.n_cols - 1) * ldx + k : 0, y_elems = s.n_rows ? size_t(s.n_rows - 1) * ldy + k : 0;
    Buf bx, by;
    bx.alloc(x_elems, 2, x_off);
    by.alloc(y_elems, 2, y_off);
    uint16_t* X = reinterpret_cast<uint16_t*>(bx.p);
    uint16_t* Y = reinterpret_cast<uint16_t*>(by.p);
    for (size_t i = 0; i < x_elems; ++i) X[i] = x_pad;
    for (size_t i = 0; i < y_elems; ++i) Y[i] = canary;
    for (int64_t c = 0; c < s.n_cols; ++c)
        for (int64_t j = 0; j < k; ++j) X[c * ldx + j] = s.X[c * s.kf + c0 + j];
    for (int64_t r = 0; r < s.n_rows; ++r)
        for (int64_t j = 0; j < k; ++j) Y[r * ldy + j] = y0_poison ? y_poison : s.Y0[r * s.kf + c0 + j];
    int64_t st = mi355_spmv_multi_set_alpha_beta(s.plan, ab[0], ab[1]);
    if (st == MI355_SPMV_OK) st = mi355_spmv_multi_execute(s.plan, s.Ax.p, X, ldx, Y, ldy, int32_t(k), nullptr);
    if (st != MI355_SPMV_OK) fprintf(stderr, "multi_half_sim: execute -> %d (%s)\n", int(st), mi355::g_error);
    const int64_t count = s.n_rows * ldy;
    put(&st, 8);
    put(&count, 8);
    put(Y, y_elems * 2);
    for (int64_t i = int64_t(y_elems); i < count; ++i) put(&canary, 2);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: multi_half_sim BATCH OUT\n"); return 2; }
    g_in = fopen(argv[1], "rb");
    g_out = fopen(argv[2], "wb");
    if (!g_in || !g_out) { perror("multi_half_sim: open"); return 2; }
    State s;
    for (;;) {
        const int64_t tag = word();
        if (tag == 0) break;
        if (tag == 1) {
            if (s.plan) { mi355_spmv_multi_destroy(s.plan); s.plan = nullptr; }
            s.off_type = int(word()); s.vec_type = int(word()); s.mat_type = int(word());
            s.n_rows = word(); s.n_cols = word(); s.nnz = word();
            const int64_t ap_off = word(), aj_off = word(), ax_off = word();
            const size_t ob = s.off_type == MI355_OFF_I64 ? 8 : 4, vb = s.mat_type == MI355_VAL_F32 ? 4 : 2;
            s.Ap.alloc(size_t(s.n_rows) + 1, ob, ap_off);
            s.Aj.alloc(size_t(s.nnz), 4, aj_off);
            s.Ax.alloc(size_t(s.nnz), vb, ax_off);
            get(s.Ap.p, (size_t(s.n_rows) + 1) * ob);
            get(s.Aj.p, size_t(s.nnz) * 4);
            get(s.Ax.p, size_t(s.nnz) * vb);
            s.kf = 0;
        } else if (tag == 2) {
            s.kf = word();
            s.X.resize(size_t(s.n_cols * s.kf));
            get(s.X.data(), s.X.size() * 2);
            s.Y0.resize(size_t(s.n_rows * s.kf));
            get(s.Y0.data(), s.Y0.size() * 2);
        } else if (tag == 3) {
            if (s.plan) { mi355_spmv_multi_destroy(s.plan); s.plan = nullptr; }
            const int64_t k_max = word();
            const int st = mi355_spmv_multi_create_half(&s.plan, s.off_type, s.mat_type, s.vec_type, int32_t(s.n_rows), int32_t(s.n_cols),
                                                        s.nnz, s.Ap.p, reinterpret_cast<const int32_t*>(s.Aj.p), int32_t(k_max));
            if (st != MI355_SPMV_OK) { fprintf(stderr, "multi_half_sim: create_half -> %d (%s)\n", st, mi355::g_error); return 5; }
        } else if (tag == 4) {
            run(s);
        } else {
            fprintf(stderr, "multi_half_sim: unknown record %lld\n", (long long)tag);
            return 4;
        }
    }
    if (s.plan && mi355_spmv_multi_destroy(s.plan) != MI355_SPMV_OK) return 5;
    const int64_t end = -1;
    put(&end, 8);
    if (fclose(g_out) != 0) return 4;
    fclose(g_in);
    return 0;
}
