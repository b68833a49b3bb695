// sddmm_half_sim — TEST CODE.  csrc/sddmm.hip with csrc/sddmm_half_kernel.hpp (which it includes), unchanged, compiled
// with the HOST compiler over tests/cpp/simt (a stand-in <hip/hip_runtime.h> that runs every lane of a workgroup as a
// fiber) and driven through the real extern "C" entry points: mi355_spmv_sddmm_create_half, then the object's
// set_alpha_beta / execute / destroy, so the choice of C from ceil(k / 8), u_vec / v_vec and the valued / pattern
// dispatch run as well.  Where the host compiler has no _Float16, half_convert.hpp holds binary16 as uint16_t and
// converts in software.  Built with -fsanitize=address,undefined (tests/cpp/sddmm_half_sim.mk).
//
//   sddmm_half_sim BATCH OUT      reads records from BATCH, writes one result per run record to OUT
//
// Records are int64 words followed by raw little-endian arrays (tests/sddmm_half_cases.py writes them, write_batch):
//   1  matrix    off_type vec_type n_rows n_cols nnz ap_off aj_off ax_off | Ap[n_rows + 1] Aj[nnz] Ax[nnz] O0[nnz]  (fp32)
//   2  operands  kf | U[n_rows * kf] V[n_cols * kf]      (16-bit patterns, row-major, kf columns: a run takes c0 .. c0 + k)
//   4  run       k c0 ldu ldv u_off v_off out_off valued out0_nan nan_bits | alpha beta (2 doubles)
//   0  end
// *_off = elements between a 64-byte boundary and the operand's base (0 or 1).  Every operand is an allocation of its
// own, exactly as long as the call may touch: U is (n_rows - 1) * ldu + k elements, V likewise, out nnz — so a read or
// write one element outside is a report.  Padding columns of U and V hold nan_bits; out holds O0, or NaN with out0_nan.
// A result is: status, count = nnz, then out as count fp32 values.
#include <cmath>
#include <limits>
#include <vector>

#include "../../spmv-samples_amd/csrc/sddmm.hip"

#define SIM_NAME "sddmm_half_sim"
#include "sim_io.hpp"

namespace {

struct State {
    int off_type = 0, vec_type = 0;
    int64_t n_rows = 0, n_cols = 0, nnz = 0, kf = 0;
    Buf Ap, Aj, Ax;
    std::vector<float> O0;
    std::vector<uint16_t> U, V;     // kf columns, dense
    mi355_spmv_sddmm* plan = nullptr;
};

void run(State& s) {
    const int64_t k = word(), c0 = word(), ldu = word(), ldv = word(), u_off = word(), v_off = word(), out_off = word(),
                  valued = word(), out0_nan = word(), nan_bits = word();
    double ab[2];
    get(ab, sizeof(ab));
    if (!s.plan || k < 1 || c0 < 0 || c0 + k > s.kf || ldu < k || ldv < k) { fprintf(stderr, "sddmm_half_sim: bad run record\n"); exit(4); }
    const size_t u_elems = s.n_rows ? size_t(s.n_rows - 1) * ldu + k : 0, v_elems = s.n_cols ? size_t(s.n_cols - 1) * ldv + k : 0;
    Buf bu, bv, bo;
    bu.alloc(u_elems, 2, u_off);
    bv.alloc(v_elems, 2, v_off);
    bo.alloc(size_t(s.nnz), sizeof(float), out_off);
    uint16_t* U = reinterpret_cast<uint16_t*>(bu.p);
    uint16_t* V = reinterpret_cast<uint16_t*>(bv.p);
    float* out = reinterpret_cast<float*>(bo.p);
    for (size_t i = 0; i < u_elems; ++i) U[i] = uint16_t(nan_bits);
    for (size_t i = 0; i < v_elems; ++i) V[i] = uint16_t(nan_bits);
    for (int64_t r = 0; r < s.n_rows; ++r)
        for (int64_t j = 0; j < k; ++j) U[r * ldu + j] = s.U[size_t(r * s.kf + c0 + j)];
    for (int64_t c = 0; c < s.n_cols; ++c)
        for (int64_t j = 0; j < k; ++j) V[c * ldv + j] = s.V[size_t(c * s.kf + c0 + j)];
    for (int64_t n = 0; n < s.nnz; ++n) out[n] = out0_nan ? std::numeric_limits<float>::quiet_NaN() : s.O0[size_t(n)];
    int64_t st = mi355_spmv_sddmm_set_alpha_beta(s.plan, ab[0], ab[1]);
    if (st == MI355_SPMV_OK) st = mi355_spmv_sddmm_execute(s.plan, valued ? s.Ax.p : nullptr, U, ldu, V, ldv, out, int32_t(k), nullptr);
    if (st != MI355_SPMV_OK) fprintf(stderr, "sddmm_half_sim: execute -> %d (%s)\n", int(st), mi355::g_error);
    put(&st, 8);
    put(&s.nnz, 8);
    put(out, size_t(s.nnz) * sizeof(float));
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: sddmm_half_sim BATCH OUT\n"); return 2; }
    g_in = fopen(argv[1], "rb");
    g_out = fopen(argv[2], "wb");
    if (!g_in || !g_out) { perror("sddmm_half_sim: open"); return 2; }
    State s;
    for (;;) {
        const int64_t tag = word();
        if (tag == 0) break;
        if (tag == 1) {
            if (s.plan) { mi355_spmv_sddmm_destroy(s.plan); s.plan = nullptr; }
            s.off_type = int(word()); s.vec_type = int(word());
            s.n_rows = word(); s.n_cols = word(); s.nnz = word();
            const int64_t ap_off = word(), aj_off = word(), ax_off = word();
            const size_t ob = s.off_type == MI355_OFF_I64 ? 8 : 4;
            s.Ap.alloc(size_t(s.n_rows) + 1, ob, ap_off);
            s.Aj.alloc(size_t(s.nnz), 4, aj_off);
            s.Ax.alloc(size_t(s.nnz), sizeof(float), ax_off);
            s.O0.resize(size_t(s.nnz));
            get(s.Ap.p, (size_t(s.n_rows) + 1) * ob);
            get(s.Aj.p, size_t(s.nnz) * 4);
            get(s.Ax.p, size_t(s.nnz) * sizeof(float));
            get(s.O0.data(), s.O0.size() * sizeof(float));
            s.kf = 0;
            const int st = mi355_spmv_sddmm_create_half(&s.plan, s.off_type, s.vec_type, int32_t(s.n_rows), int32_t(s.n_cols), s.nnz,
                                                        s.Ap.p, reinterpret_cast<const int32_t*>(s.Aj.p));
            if (st != MI355_SPMV_OK) { fprintf(stderr, "sddmm_half_sim: create_half -> %d (%s)\n", st, mi355::g_error); return 5; }
            int val_type = -1, vec_type = -1;
            if (mi355_spmv_sddmm_get_types(s.plan, &val_type, &vec_type) != MI355_SPMV_OK || val_type != MI355_VAL_F32 ||
                vec_type != s.vec_type) {
                fprintf(stderr, "sddmm_half_sim: get_types -> (%d, %d)\n", val_type, vec_type);
                return 5;
            }
        } else if (tag == 2) {
            s.kf = word();
            s.U.resize(size_t(s.n_rows * s.kf));
            s.V.resize(size_t(s.n_cols * s.kf));
            get(s.U.data(), s.U.size() * 2);
            get(s.V.data(), s.V.size() * 2);
        } else if (tag == 4) {
            run(s);
        } else {
            fprintf(stderr, "sddmm_half_sim: unknown record %lld\n", (long long)tag);
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
