// multi_semiring_sim — TEST CODE.  csrc/multi.hip (with multi_kernels.hpp and semiring.hpp, which it includes),
// unchanged, compiled with the HOST compiler over tests/cpp/simt and driven through the real extern "C" entry points:
// mi355_spmv_multi_create_typed / set_semiring / set_alpha_beta / execute / destroy — every semiring, the three value
// types, valued and pattern matrices.  Built with -fsanitize=address,undefined by tests/test_multi_semiring_sim_cpu.py
// (the SIM_SAN flags of tests/cpp/Makefile).
//
//   multi_semiring_sim BATCH OUT      reads records from BATCH, writes one result per run record to OUT
//
// Records are int64 words followed by raw little-endian arrays (tests/multi_semiring_cases.py writes them, write_batch):
//   1  matrix   off_type vec_type n_rows n_cols nnz ap_off aj_off ax_off | Ap[n_rows + 1] Aj[nnz] Ax[nnz]
//   2  vectors  kf | X[3][n_cols * kf] (as drawn, with +inf, with -inf) Y0[n_rows * kf]   (row-major, kf columns)
//   3  plan     k_max pattern                                   (destroys the plan before it)
//   4  run      k c0 ldx ldy x_off y_off y0_poison semiring x_kind y_poison_i32 x_pad_i32 | alpha beta (2 doubles)
//   0  end
// *_off = elements between a 64-byte boundary and the operand's base (0 or 1).  Every operand is an allocation of its
// own, exactly as long as the call may touch: X is (n_cols - 1) * ldx + k elements, Y likewise — so a read or write one
// element outside is a report.  A pattern plan is executed with Ax = NULL.  Padding columns of X hold NaN (int32:
// x_pad_i32), of Y a canary; with y0_poison the k columns of Y hold NaN (int32: y_poison_i32).
// A result is: status, count = n_rows * ldy, then Y as count values (the missing tail of the last row as canary).
#include <cmath>
#include <limits>
#include <vector>

#include "../../spmv-samples_amd/csrc/multi.hip"

#define SIM_NAME "multi_semiring_sim"
#include "sim_io.hpp"

namespace {

constexpr double kCanary = -777.25;

struct State {
    int off_type = 0, vec_type = 0;
    int64_t n_rows = 0, n_cols = 0, nnz = 0, kf = 0;
    bool pattern = false;
    Buf Ap, Aj, Ax;
    std::vector<char> X[3], Y0;     // kf columns, dense
    mi355_spmv_multi* plan = nullptr;
};

size_t value_bytes(int vec_type) { return vec_type == MI355_VAL_F64 ? 8 : 4; }

template <typename V>
void run(State& s) {
    const int64_t k = word(), c0 = word(), ldx = word(), ldy = word(), x_off = word(), y_off = word(), y0_poison = word();
    const int64_t semiring = word(), x_kind = word(), y_poison_i32 = word(), x_pad_i32 = word();
    double ab[2];
    get(ab, sizeof(ab));
    if (!s.plan || k < 1 || c0 < 0 || c0 + k > s.kf || ldx < k || ldy < k || x_kind < 0 || x_kind > 2) {
        fprintf(stderr, "multi_semiring_sim: bad run record\n");
        exit(4);
    }
    constexpr bool is_int = std::numeric_limits<V>::is_integer;
    const V x_pad = is_int ? V(x_pad_i32) : std::numeric_limits<V>::quiet_NaN();
    const V y_poison = is_int ? V(y_poison_i32) : std::numeric_limits<V>::quiet_NaN();
    const size_t x_elems = s.n_cols ? size_t(s.n_cols - 1) * ldx + k : 0, y_elems = s.n_rows ? size_t(s.n_rows - 1) * ldy + k : 0;
    Buf bx, by;
    bx.alloc(x_elems, sizeof(V), x_off);
    by.alloc(y_elems, sizeof(V), y_off);
    V* X = reinterpret_cast<V*>(bx.p);
    V* Y = reinterpret_cast<V*>(by.p);
    const V* Xf = reinterpret_cast<const V*>(s.X[x_kind].data());
    const V* Yf = reinterpret_cast<const V*>(s.Y0.data());
    for (size_t i = 0; i < x_elems; ++i) X[i] = x_pad;
    for (size_t i = 0; i < y_elems; ++i) Y[i] = V(kCanary);
    for (int64_t c = 0; c < s.n_cols; ++c)
        for (int64_t j = 0; j < k; ++j) X[c * ldx + j] = Xf[c * s.kf + c0 + j];
    for (int64_t r = 0; r < s.n_rows; ++r)
        for (int64_t j = 0; j < k; ++j) Y[r * ldy + j] = y0_poison ? y_poison : Yf[r * s.kf + c0 + j];
    // alpha / beta back to 1 / 0 first: a semiring other than (+, *) is refused while they are set
    int64_t st = mi355_spmv_multi_set_alpha_beta(s.plan, 1.0, 0.0);
    if (st == MI355_SPMV_OK) st = mi355_spmv_multi_set_semiring(s.plan, int(semiring));
    if (st == MI355_SPMV_OK) st = mi355_spmv_multi_set_alpha_beta(s.plan, ab[0], ab[1]);
    if (st == MI355_SPMV_OK) st = mi355_spmv_multi_execute(s.plan, s.pattern ? nullptr : s.Ax.p, X, ldx, Y, ldy, int32_t(k), nullptr);
    if (st != MI355_SPMV_OK) fprintf(stderr, "multi_semiring_sim: execute -> %d (%s)\n", int(st), mi355::g_error);
    const int64_t count = s.n_rows * ldy;
    put(&st, 8);
    put(&count, 8);
    put(Y, y_elems * sizeof(V));
    const V canary = V(kCanary);
    for (int64_t i = int64_t(y_elems); i < count; ++i) put(&canary, sizeof(V));
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: multi_semiring_sim BATCH OUT\n"); return 2; }
    g_in = fopen(argv[1], "rb");
    g_out = fopen(argv[2], "wb");
    if (!g_in || !g_out) { perror("multi_semiring_sim: open"); return 2; }
    State s;
    for (;;) {
        const int64_t tag = word();
        if (tag == 0) break;
        if (tag == 1) {
            if (s.plan) { mi355_spmv_multi_destroy(s.plan); s.plan = nullptr; }
            s.off_type = int(word()); s.vec_type = int(word());
            s.n_rows = word(); s.n_cols = word(); s.nnz = word();
            const int64_t ap_off = word(), aj_off = word(), ax_off = word();
            const size_t ob = s.off_type == MI355_OFF_I64 ? 8 : 4, vb = value_bytes(s.vec_type);
            s.Ap.alloc(size_t(s.n_rows) + 1, ob, ap_off);
            s.Aj.alloc(size_t(s.nnz), 4, aj_off);
            s.Ax.alloc(size_t(s.nnz), vb, ax_off);
            get(s.Ap.p, (size_t(s.n_rows) + 1) * ob);
            get(s.Aj.p, size_t(s.nnz) * 4);
            get(s.Ax.p, size_t(s.nnz) * vb);
            s.kf = 0;
        } else if (tag == 2) {
            s.kf = word();
            const size_t vb = value_bytes(s.vec_type);
            for (auto& X : s.X) {
                X.resize(size_t(s.n_cols * s.kf) * vb);
                get(X.data(), X.size());
            }
            s.Y0.resize(size_t(s.n_rows * s.kf) * vb);
            get(s.Y0.data(), s.Y0.size());
        } else if (tag == 3) {
            if (s.plan) { mi355_spmv_multi_destroy(s.plan); s.plan = nullptr; }
            const int64_t k_max = word();
            s.pattern = word() != 0;
            const int st = mi355_spmv_multi_create_typed(&s.plan, s.off_type, s.pattern ? int(MI355_VAL_PATTERN) : s.vec_type, s.vec_type,
                                                         int32_t(s.n_rows), int32_t(s.n_cols), s.nnz, s.Ap.p,
                                                         reinterpret_cast<const int32_t*>(s.Aj.p), int32_t(k_max));
            if (st != MI355_SPMV_OK) { fprintf(stderr, "multi_semiring_sim: create_typed -> %d (%s)\n", st, mi355::g_error); return 5; }
        } else if (tag == 4) {
            if (s.vec_type == MI355_VAL_F64) run<double>(s);
            else if (s.vec_type == MI355_VAL_I32) run<int32_t>(s);
            else run<float>(s);
        } else {
            fprintf(stderr, "multi_semiring_sim: unknown record %lld\n", (long long)tag);
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
