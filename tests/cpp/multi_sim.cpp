// multi_sim — TEST CODE.  csrc/multi.hip with what it includes (multi_kernels.hpp, multi_slice_walk.inc, semiring.hpp,
// multi_half_kernels.hpp), unchanged, compiled with the HOST compiler over tests/cpp/simt (a stand-in <hip/hip_runtime.h>
// that runs every lane of a workgroup as a fiber) and driven through the real extern "C" entry points:
// mi355_spmv_multi_create, _create_typed or _create_half, then the object's set_semiring / set_alpha_beta / execute /
// destroy, so launch_multi's tiles, passes, x_vec / y_vec and the fix-up launch condition run as well.  One program for
// the three tables (tests/multi_cases.py, tests/multi_semiring_cases.py, tests/multi_half_cases.py): the plan record says
// which create it is.  The program only moves bit patterns: element sizes come from the type words and every fill value
// arrives as bits.  Where the host compiler has no _Float16, half_convert.hpp holds binary16 as uint16_t and converts in
// software.  Built with -fsanitize=address,undefined (tests/cpp/Makefile).
//
//   multi_sim BATCH OUT      reads records from BATCH, writes one result per run record to OUT
//
// Records are int64 words followed by raw little-endian arrays (tests/multi_cases.py writes them, write_batch):
//   1  matrix   off_type vec_type mat_type n_rows n_cols nnz ap_off aj_off ax_off | Ap[n_rows + 1] Aj[nnz] Ax[nnz]
//   2  vectors  kf nx | X[nx][n_cols * kf] Y0[n_rows * kf]     (row-major, kf columns: a run takes columns c0 .. c0 + k)
//   3  plan     k_max how pattern                              (destroys the plan before it)
//   4  run      k c0 ldx ldy x_off y_off y0_poison semiring x_kind x_pad_bits y_poison_bits canary_bits | alpha beta (2 doubles)
//   0  end
// vec_type = the MI355_VAL_* of X and Y, mat_type that of Ax as stored (of vec_type's width, or F32 under F16 / BF16).
// how: 0 = mi355_spmv_multi_create(vec_type); 1 = _create_typed(pattern ? MI355_VAL_PATTERN : mat_type, vec_type), and a
// pattern plan is executed with Ax = NULL; 2 = _create_half(mat_type, vec_type).  After 1 and 2 the object must report
// those two types (mi355_spmv_multi_get_types).  nx = 1, or 3 for the typed table: X as drawn, with +inf, with -inf, of
// which a run takes x_kind.  semiring = -1: no set_semiring call, only set_alpha_beta(alpha, beta) before the execute;
// otherwise set_alpha_beta(1, 0), set_semiring(semiring), set_alpha_beta(alpha, beta): a semiring other than (+, *) is
// refused while alpha / beta are set.
// *_off = elements between a 64-byte boundary and the operand's base (0 or 1).  Every operand is an allocation of its
// own, exactly as long as the call may touch: X is (n_cols - 1) * ldx + k elements, Y likewise — so a read or write one
// element outside is a report.  *_bits = the bit pattern of a value of vec_type: padding columns of X hold x_pad_bits,
// of Y canary_bits; with y0_poison the k columns of Y hold y_poison_bits.
// A result is: status, count = n_rows * ldy, then Y as count values (the missing tail of the last row as canary).
// type_bytes and fill are sim_operand.hpp's.
#include <cstring>
#include <vector>

#include "../../spmv-samples_amd/csrc/multi.hip"

#define SIM_NAME "multi_sim"
#include "sim_io.hpp"
#include "sim_operand.hpp"

namespace {

struct State {
    int off_type = 0, vec_type = 0, mat_type = 0;
    size_t eb = 0;                  // bytes of an element of X and Y
    int64_t n_rows = 0, n_cols = 0, nnz = 0, kf = 0;
    bool pattern = false;
    Buf Ap, Aj, Ax;
    std::vector<std::vector<char>> X;   // nx variants of kf columns, dense
    std::vector<char> Y0;               // kf columns, dense
    mi355_spmv_multi* plan = nullptr;
};

// `rows` rows of k elements at stride ld in dst, every other element pad_bits: columns c0 .. c0 + k of the dense src, or
// row_bits where there is no src
void place(char* dst, size_t elems, const char* src, const State& s, int64_t rows, int64_t k, int64_t c0, int64_t ld, int64_t pad_bits,
           int64_t row_bits) {
    fill(dst, elems, pad_bits, s.eb);
    for (int64_t r = 0; r < rows; ++r) {
        char* row = dst + size_t(r * ld) * s.eb;
        if (src) memcpy(row, src + size_t(r * s.kf + c0) * s.eb, size_t(k) * s.eb);
        else fill(row, size_t(k), row_bits, s.eb);
    }
}

void run(State& s) {
    const int64_t k = word(), c0 = word(), ldx = word(), ldy = word(), x_off = word(), y_off = word(), y0_poison = word(),
                  semiring = word(), x_kind = word(), x_pad = word(), y_poison = word(), canary = word();
    double ab[2];
    get(ab, sizeof(ab));
    if (!s.plan || k < 1 || c0 < 0 || c0 + k > s.kf || ldx < k || ldy < k || x_kind < 0 || size_t(x_kind) >= s.X.size()) {
        fprintf(stderr, "multi_sim: bad run record\n");
        exit(4);
    }
    const size_t x_elems = s.n_cols ? size_t(s.n_cols - 1) * ldx + k : 0, y_elems = s.n_rows ? size_t(s.n_rows - 1) * ldy + k : 0;
    Buf bx, by;
    bx.alloc(x_elems, s.eb, x_off);
    by.alloc(y_elems, s.eb, y_off);
    place(bx.p, x_elems, s.X[x_kind].data(), s, s.n_cols, k, c0, ldx, x_pad, 0);
    place(by.p, y_elems, y0_poison ? nullptr : s.Y0.data(), s, s.n_rows, k, c0, ldy, canary, y_poison);
    int64_t st = MI355_SPMV_OK;
    if (semiring >= 0) {
        st = mi355_spmv_multi_set_alpha_beta(s.plan, 1.0, 0.0);
        if (st == MI355_SPMV_OK) st = mi355_spmv_multi_set_semiring(s.plan, int(semiring));
    }
    if (st == MI355_SPMV_OK) st = mi355_spmv_multi_set_alpha_beta(s.plan, ab[0], ab[1]);
    if (st == MI355_SPMV_OK) st = mi355_spmv_multi_execute(s.plan, s.pattern ? nullptr : s.Ax.p, bx.p, ldx, by.p, ldy, int32_t(k), nullptr);
    if (st != MI355_SPMV_OK) fprintf(stderr, "multi_sim: execute -> %d (%s)\n", int(st), mi355::g_error);
    const int64_t count = s.n_rows * ldy;
    put(&st, 8);
    put(&count, 8);
    put(by.p, y_elems * s.eb);
    for (int64_t i = int64_t(y_elems); i < count; ++i) put(&canary, s.eb);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: multi_sim BATCH OUT\n"); return 2; }
    g_in = fopen(argv[1], "rb");
    g_out = fopen(argv[2], "wb");
    if (!g_in || !g_out) { perror("multi_sim: open"); return 2; }
    State s;
    for (;;) {
        const int64_t tag = word();
        if (tag == 0) break;
        if (tag == 1) {
            if (s.plan) { mi355_spmv_multi_destroy(s.plan); s.plan = nullptr; }
            s.off_type = int(word()); s.vec_type = int(word()); s.mat_type = int(word());
            s.n_rows = word(); s.n_cols = word(); s.nnz = word();
            const int64_t ap_off = word(), aj_off = word(), ax_off = word();
            const size_t ob = s.off_type == MI355_OFF_I64 ? 8 : 4, vb = type_bytes(s.mat_type);
            s.eb = type_bytes(s.vec_type);
            s.Ap.alloc(size_t(s.n_rows) + 1, ob, ap_off);
            s.Aj.alloc(size_t(s.nnz), 4, aj_off);
            s.Ax.alloc(size_t(s.nnz), vb, ax_off);
            get(s.Ap.p, (size_t(s.n_rows) + 1) * ob);
            get(s.Aj.p, size_t(s.nnz) * 4);
            get(s.Ax.p, size_t(s.nnz) * vb);
            s.kf = 0;
            s.X.clear();
        } else if (tag == 2) {
            s.kf = word();
            s.X.resize(size_t(word()));
            for (auto& X : s.X) {
                X.resize(size_t(s.n_cols * s.kf) * s.eb);
                get(X.data(), X.size());
            }
            s.Y0.resize(size_t(s.n_rows * s.kf) * s.eb);
            get(s.Y0.data(), s.Y0.size());
        } else if (tag == 3) {
            if (s.plan) { mi355_spmv_multi_destroy(s.plan); s.plan = nullptr; }
            const int64_t k_max = word(), how = word();
            s.pattern = word() != 0;
            const int mat_type = s.pattern ? int(MI355_VAL_PATTERN) : s.mat_type;
            const int32_t* Aj = reinterpret_cast<const int32_t*>(s.Aj.p);
            if (how < 0 || how > 2 || (s.pattern && how != 1)) { fprintf(stderr, "multi_sim: bad plan record\n"); return 4; }
            const int st = how == 0 ? mi355_spmv_multi_create(&s.plan, s.off_type, s.vec_type, int32_t(s.n_rows), int32_t(s.n_cols), s.nnz,
                                                              s.Ap.p, Aj, int32_t(k_max))
                                    : (how == 1 ? mi355_spmv_multi_create_typed : mi355_spmv_multi_create_half)(
                                          &s.plan, s.off_type, mat_type, s.vec_type, int32_t(s.n_rows), int32_t(s.n_cols), s.nnz, s.Ap.p, Aj,
                                          int32_t(k_max));
            if (st != MI355_SPMV_OK) { fprintf(stderr, "multi_sim: create (how = %d) -> %d (%s)\n", int(how), st, mi355::g_error); return 5; }
            int got_mat = -1, got_vec = -1;
            if (how != 0 && (mi355_spmv_multi_get_types(s.plan, &got_mat, &got_vec, nullptr) != MI355_SPMV_OK || got_mat != mat_type ||
                             got_vec != s.vec_type)) {
                fprintf(stderr, "multi_sim: get_types -> (%d, %d)\n", got_mat, got_vec);
                return 5;
            }
        } else if (tag == 4) {
            run(s);
        } else {
            fprintf(stderr, "multi_sim: unknown record %lld\n", (long long)tag);
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
