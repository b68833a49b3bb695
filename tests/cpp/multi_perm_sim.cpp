// multi_perm_sim — TEST CODE.  csrc/multi.hip (with multi_kernels.hpp and multi_slice_walk.inc) and csrc/multi_perm.hip,
// unchanged, compiled with the HOST compiler over tests/cpp/simt and driven through the real entry points:
// mi355_spmv_multi_create_permuted / _execute / _destroy, and beside it, in the same program, mi355_spmv_multi_create on the
// same structure executed on Ax[perm] materialised.  Both results are written; tests/test_multi_perm_sim_cpu.py holds
// them to each other bit for bit.  Built with -fsanitize=address,undefined (tests/cpp/Makefile).
//
//   multi_perm_sim BATCH OUT
//
// Records are int64 words followed by raw little-endian arrays (tests/multi_perm_cases.py writes them, write_batch):
//   1  matrix   off_type val_type n_rows n_cols nnz | Ap[n_rows + 1] Aj[nnz]
//   2  perm     perm_type n_values | perm[nnz] (4 or 8 bytes each) Ax[n_values]
//   3  run      k k_max ldx ldy | alpha beta (2 doubles) X[n_cols * k] Y0[n_rows * k] (dense)
//               -> status, count = (n_rows - 1) * ldy + k (0 without rows), Y of the permuted object, Y of the plain one
//   4  bad      pos value     perm with perm[pos] = value must be refused
//               -> status of the create, 1 if an object was made
//   0  end
// Every operand is an allocation of its own, exactly as long as the call may touch: Ax of n_values, perm of nnz, X of
// (n_cols - 1) * ldx + k, Y likewise — a read or write one element outside is a report.  Padding of X is NaN, of Y the
// canary -777.25; beta == 0 poisons Y with NaN first.
#include <cmath>
#include <cstring>
#include <vector>

#include "../../spmv-samples_amd/csrc/multi.hip"

#include "sim_runtime.hpp"     // what csrc/multi_perm.hip uses of the HIP runtime and the stand-in leaves out
#include "../../spmv-samples_amd/csrc/multi_perm.hip"

#define SIM_NAME "multi_perm_sim"
#include "sim_io.hpp"

namespace {

struct State {
    int off_type = 0, val_type = 0, perm_type = 0;
    size_t eb = 0, pb = 0;
    int64_t n_rows = 0, n_cols = 0, nnz = 0, n_values = 0;
    Buf Ap, Aj, perm, Ax, Axp;      // Axp = Ax[perm], nnz values
};

template <typename T>
void fill(char* dst, size_t n, double v) {
    const T t = T(v);
    for (size_t i = 0; i < n; ++i) memcpy(dst + i * sizeof(T), &t, sizeof(T));
}
void fill(const State& s, char* dst, size_t n, double v) { s.eb == 8 ? fill<double>(dst, n, v) : fill<float>(dst, n, v); }

int64_t perm_at(const State& s, int64_t i) {
    if (s.pb == 8) { int64_t v; memcpy(&v, s.perm.p + i * 8, 8); return v; }
    uint32_t v; memcpy(&v, s.perm.p + i * 4, 4); return int64_t(v);
}

int create_permuted(const State& s, mi355_spmv_multi** m, const void* perm, int64_t k_max) {
    return mi355_spmv_multi_create_permuted(m, s.off_type, s.val_type, int32_t(s.n_rows), int32_t(s.n_cols), s.nnz, s.Ap.p,
                                            reinterpret_cast<const int32_t*>(s.Aj.p), s.perm_type, perm, s.n_values, int32_t(k_max), nullptr);
}

void run(State& s) {
    const int64_t k = word(), k_max = word(), ldx = word(), ldy = word();
    double ab[2];
    get(ab, sizeof(ab));
    if (k < 1 || k > k_max || ldx < k || ldy < k) { fprintf(stderr, "multi_perm_sim: bad run record\n"); exit(4); }
    std::vector<char> X(size_t(s.n_cols * k) * s.eb), Y0(size_t(s.n_rows * k) * s.eb);
    get(X.data(), X.size());
    get(Y0.data(), Y0.size());
    const size_t x_elems = s.n_cols ? size_t(s.n_cols - 1) * ldx + k : 0, y_elems = s.n_rows ? size_t(s.n_rows - 1) * ldy + k : 0;
    Buf bx, by[2];
    bx.alloc(x_elems, s.eb, 0);
    fill(s, bx.p, x_elems, NAN);
    for (int64_t c = 0; c < s.n_cols; ++c) memcpy(bx.p + size_t(c * ldx) * s.eb, X.data() + size_t(c * k) * s.eb, size_t(k) * s.eb);
    for (Buf& b : by) {
        b.alloc(y_elems, s.eb, 0);
        fill(s, b.p, y_elems, -777.25);
        for (int64_t r = 0; r < s.n_rows; ++r) {
            if (ab[1] == 0.0) fill(s, b.p + size_t(r * ldy) * s.eb, size_t(k), NAN);
            else memcpy(b.p + size_t(r * ldy) * s.eb, Y0.data() + size_t(r * k) * s.eb, size_t(k) * s.eb);
        }
    }
    mi355_spmv_multi *mp = nullptr, *mq = nullptr;
    int64_t st = create_permuted(s, &mp, s.perm.p, k_max);
    if (st == MI355_SPMV_OK)
        st = mi355_spmv_multi_create(&mq, s.off_type, s.val_type, int32_t(s.n_rows), int32_t(s.n_cols), s.nnz, s.Ap.p,
                                     reinterpret_cast<const int32_t*>(s.Aj.p), int32_t(k_max));
    mi355_spmv_multi_info info;
    int64_t n_values = -1, held = -1;
    int owns = -1;
    if (st == MI355_SPMV_OK) st = mi355_spmv_multi_get_info(mp, &info);
    if (st == MI355_SPMV_OK) st = mi355_spmv_multi_get_perm_info(mp, &n_values, &held, &owns);
    if (st == MI355_SPMV_OK && (strcmp(info.main_kernel, "multi_perm_slice_kernel") != 0 || n_values != s.n_values || held != 4 * s.nnz || owns != 0 ||
                                mi355_spmv_multi_set_semiring(mp, MI355_SEMIRING_MIN_PLUS) != MI355_SPMV_ENOTSUP)) {
        fprintf(stderr, "multi_perm_sim: the object reports %s, %lld values, %lld bytes, owns %d, or took a semiring\n", info.main_kernel,
                (long long)n_values, (long long)held, owns);
        exit(5);
    }
    if (st == MI355_SPMV_OK) st = mi355_spmv_multi_set_alpha_beta(mp, ab[0], ab[1]);
    if (st == MI355_SPMV_OK) st = mi355_spmv_multi_set_alpha_beta(mq, ab[0], ab[1]);
    if (st == MI355_SPMV_OK) st = mi355_spmv_multi_execute(mp, s.Ax.p, bx.p, ldx, by[0].p, ldy, int32_t(k), nullptr);
    if (st == MI355_SPMV_OK) st = mi355_spmv_multi_execute(mq, s.Axp.p, bx.p, ldx, by[1].p, ldy, int32_t(k), nullptr);
    if (st != MI355_SPMV_OK) fprintf(stderr, "multi_perm_sim: -> %d (%s)\n", int(st), mi355::g_error);
    if (mi355_spmv_multi_destroy(mp) != MI355_SPMV_OK || mi355_spmv_multi_destroy(mq) != MI355_SPMV_OK) exit(5);
    const int64_t count = int64_t(y_elems);
    put(&st, 8);
    put(&count, 8);
    put(by[0].p, y_elems * s.eb);
    put(by[1].p, y_elems * s.eb);
}

void bad(State& s) {
    const int64_t pos = word(), value = word();
    if (pos < 0 || pos >= s.nnz) { fprintf(stderr, "multi_perm_sim: bad `bad` record\n"); exit(4); }
    Buf p;
    p.alloc(size_t(s.nnz), s.pb, 0);
    memcpy(p.p, s.perm.p, size_t(s.nnz) * s.pb);
    if (s.pb == 8) memcpy(p.p + pos * 8, &value, 8);
    else { const uint32_t v = uint32_t(value); memcpy(p.p + pos * 4, &v, 4); }
    mi355_spmv_multi* m = reinterpret_cast<mi355_spmv_multi*>(&s);     // must be cleared
    const int64_t st = create_permuted(s, &m, p.p, 4);
    const int64_t made = m != nullptr;
    if (m) mi355_spmv_multi_destroy(m);
    put(&st, 8);
    put(&made, 8);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: multi_perm_sim BATCH OUT\n"); return 2; }
    g_in = fopen(argv[1], "rb");
    g_out = fopen(argv[2], "wb");
    if (!g_in || !g_out) { perror("multi_perm_sim: open"); return 2; }
    State s;
    for (;;) {
        const int64_t tag = word();
        if (tag == 0) break;
        if (tag == 1) {
            s.off_type = int(word()); s.val_type = int(word());
            s.n_rows = word(); s.n_cols = word(); s.nnz = word();
            const size_t ob = s.off_type == MI355_OFF_I64 ? 8 : 4;
            s.eb = s.val_type == MI355_VAL_F64 ? 8 : 4;
            s.Ap.alloc(size_t(s.n_rows) + 1, ob, 0);
            s.Aj.alloc(size_t(s.nnz), 4, 0);
            get(s.Ap.p, (size_t(s.n_rows) + 1) * ob);
            get(s.Aj.p, size_t(s.nnz) * 4);
        } else if (tag == 2) {
            s.perm_type = int(word()); s.n_values = word();
            s.pb = s.perm_type == MI355_OFF_I64 ? 8 : 4;
            s.perm.alloc(size_t(s.nnz), s.pb, 0);
            s.Ax.alloc(size_t(s.n_values), s.eb, 0);
            s.Axp.alloc(size_t(s.nnz), s.eb, 0);
            get(s.perm.p, size_t(s.nnz) * s.pb);
            get(s.Ax.p, size_t(s.n_values) * s.eb);
            for (int64_t i = 0; i < s.nnz; ++i) {
                const int64_t p = perm_at(s, i);
                if (p < 0 || p >= s.n_values) { fprintf(stderr, "multi_perm_sim: bad perm record\n"); return 4; }
                memcpy(s.Axp.p + i * s.eb, s.Ax.p + p * s.eb, s.eb);
            }
        } else if (tag == 3) {
            run(s);
        } else if (tag == 4) {
            bad(s);
        } else {
            fprintf(stderr, "multi_perm_sim: unknown record %lld\n", (long long)tag);
            return 4;
        }
    }
    const int64_t end = -1;
    put(&end, 8);
    if (fclose(g_out) != 0) return 4;
    fclose(g_in);
    return 0;
}
