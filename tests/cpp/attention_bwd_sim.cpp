// attention_bwd_sim — TEST CODE.  csrc/attention_bwd.hip with what it includes (attention_bwd_slice_walk.inc,
// attention_bwd_half_kernel.hpp), unchanged, compiled with the HOST compiler over tests/cpp/simt (a stand-in
// <hip/hip_runtime.h> that runs every lane of a workgroup as a fiber) and driven through the real extern "C" entry points:
// mi355_spmv_attention_bwd_create or _create_half (whose transpose is csrc/coo_csr.hip, compiled the same way, as coo_sim
// does), then the object's set_scale / execute / destroy, so the delta kernel, the three roles of the walk, the fix-ups
// (narrowing under 16-bit features) and the object's scratch run as well.  One program for the two tables
// (tests/attention_bwd_cases.py, tests/attention_bwd_half_cases.py): the matrix record says which create it is.  The program
// only moves bit patterns: element sizes come from the type word and every fill value arrives as bits.  Built with
// -fsanitize=address,undefined (tests/cpp/Makefile).
//
//   attention_bwd_sim BATCH OUT      reads records from BATCH, writes one result per run record to OUT
//
// Records are int64 words followed by raw little-endian arrays (tests/attention_bwd_cases.py writes them, write_batch):
//   1  matrix    off_type feat_type n_rows n_cols nnz d_max dv_max | Ap[n_rows + 1] Aj[nnz]
//   4  run       d dv pad[8] shift has_bias need_dq need_dk need_dv want_dbias nan_bits canary_bits side_canary_bits |
//                scale (1 double) | Q[n_rows * d] K[n_cols * d] V[n_cols * dv] O[n_rows * dv] dO[n_rows * dv] lse[n_rows],
//                bias[nnz] with has_bias
//   0  end
// feat_type = the MI355_VAL_* of the eight matrices: F32 / F64 go through _create, F16 / BF16 through _create_half.  An
// element of a matrix has that type's bytes; one of lse, bias and dbias (the side arrays) 8 under F64 and 4 otherwise.
// pad = leading dimension - width of Q, K, V, O, dO, dQ, dK, dV; shift = elements between a 64-byte boundary and every
// operand's base.  Every operand is an allocation of its own, exactly as long as the call may touch: (rows - 1) * ld + width
// elements, the padding columns of the inputs filled with nan_bits, all of dQ, dK and dV with canary_bits and dbias with
// side_canary_bits — so a read or write one element outside is a report, and a write into an output's padding is counted.
// A result is: status, the padding elements that lost their canary, then dQ, dK, dV compact and dbias — those the run asked
// for.
#include "sim_runtime.hpp"

#include "../../spmv-samples_amd/csrc/coo_csr.hip"

#include "../../spmv-samples_amd/csrc/attention_bwd.hip"

#define SIM_NAME "attention_bwd_sim"
#include "sim_io.hpp"
#include "sim_operand.hpp"

namespace {

struct State {
    int off_type = 0, feat_type = 0;
    size_t eb = 0, sb = 0;          // bytes of an element of the eight matrices; of lse, bias and dbias
    int64_t n_rows = 0, n_cols = 0, nnz = 0;
    Buf Ap, Aj;
    mi355_spmv_attention_bwd* plan = nullptr;
};

void run(State& s) {
    const int64_t d = word(), dv = word();
    int64_t pad[8];
    for (int64_t& p : pad) p = word();
    const int64_t shift = word(), has_bias = word(), need_dq = word(), need_dk = word(), need_dv = word(), want_dbias = word();
    const int64_t nan_bits = word(), canary_bits = word(), side_canary_bits = word();
    double scale;
    get(&scale, sizeof(scale));
    if (!s.plan) { fprintf(stderr, "attention_bwd_sim: bad run record\n"); exit(4); }
    Operand Q, K, V, O, dO, lse, bias, dQ, dK, dV, dbias;
    Q.read(s.n_rows, d, d + pad[0], s.eb, shift, nan_bits);
    K.read(s.n_cols, d, d + pad[1], s.eb, shift, nan_bits);
    V.read(s.n_cols, dv, dv + pad[2], s.eb, shift, nan_bits);
    O.read(s.n_rows, dv, dv + pad[3], s.eb, shift, nan_bits);
    dO.read(s.n_rows, dv, dv + pad[4], s.eb, shift, nan_bits);
    lse.read(s.n_rows, 1, 1, s.sb, shift, 0);
    if (has_bias) bias.read(s.nnz, 1, 1, s.sb, shift, 0);
    if (need_dq) dQ.make(s.n_rows, d, d + pad[5], s.eb, shift, canary_bits);
    if (need_dk) dK.make(s.n_cols, d, d + pad[6], s.eb, shift, canary_bits);
    if (need_dv) dV.make(s.n_cols, dv, dv + pad[7], s.eb, shift, canary_bits);
    if (want_dbias) dbias.make(s.nnz, 1, 1, s.sb, shift, side_canary_bits);
    int64_t st = mi355_spmv_attention_bwd_set_scale(s.plan, scale);
    if (st == MI355_SPMV_OK)
        st = mi355_spmv_attention_bwd_execute(s.plan, int32_t(d), int32_t(dv), Q.p, Q.ld, K.p, K.ld, V.p, V.ld, bias.p, O.p, O.ld, dO.p, dO.ld, lse.p, dQ.p,
                                              d + pad[5], dK.p, d + pad[6], dV.p, dv + pad[7], dbias.p, nullptr);
    if (st != MI355_SPMV_OK) fprintf(stderr, "attention_bwd_sim: execute -> %d (%s)\n", int(st), mi355::g_error);
    const int64_t bad = dQ.lost() + dK.lost() + dV.lost();
    put(&st, 8);
    put(&bad, 8);
    dQ.write(); dK.write(); dV.write(); dbias.write();
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: attention_bwd_sim BATCH OUT\n"); return 2; }
    g_in = fopen(argv[1], "rb");
    g_out = fopen(argv[2], "wb");
    if (!g_in || !g_out) { perror("attention_bwd_sim: open"); return 2; }
    State s;
    for (;;) {
        const int64_t tag = word();
        if (tag == 0) break;
        if (tag == 1) {
            if (s.plan) { mi355_spmv_attention_bwd_destroy(s.plan); s.plan = nullptr; }
            s.off_type = int(word()); s.feat_type = int(word());
            s.n_rows = word(); s.n_cols = word(); s.nnz = word();
            const int64_t d_max = word(), dv_max = word();
            const size_t ob = s.off_type == MI355_OFF_I64 ? 8 : 4;
            const bool half = s.feat_type == MI355_VAL_F16 || s.feat_type == MI355_VAL_BF16;
            s.eb = type_bytes(s.feat_type);
            s.sb = s.feat_type == MI355_VAL_F64 ? 8 : 4;
            s.Ap.alloc(size_t(s.n_rows) + 1, ob, 0);
            s.Aj.alloc(size_t(s.nnz), 4, 0);
            get(s.Ap.p, (size_t(s.n_rows) + 1) * ob);
            get(s.Aj.p, size_t(s.nnz) * 4);
            const int st = (half ? mi355_spmv_attention_bwd_create_half : mi355_spmv_attention_bwd_create)(
                &s.plan, s.off_type, s.feat_type, int32_t(s.n_rows), int32_t(s.n_cols), s.nnz, s.Ap.p, reinterpret_cast<const int32_t*>(s.Aj.p),
                int32_t(d_max), int32_t(dv_max), nullptr);
            if (st != MI355_SPMV_OK) { fprintf(stderr, "attention_bwd_sim: create (type %d) -> %d (%s)\n", s.feat_type, st, mi355::g_error); return 5; }
            mi355_spmv_attention_bwd_info info;
            int val_type = -1, vec_type = -1;
            if (mi355_spmv_attention_bwd_get_info(s.plan, &info) != MI355_SPMV_OK ||
                info.n_slices != (s.n_rows + s.nnz + info.slice_len - 1) / info.slice_len ||
                info.n_slices_t != (s.n_cols + s.nnz + info.slice_len - 1) / info.slice_len ||
                (half && (info.val_type != MI355_VAL_F32 || info.widest_tile != 64 ||
                          mi355_spmv_attention_bwd_get_types(s.plan, &val_type, &vec_type) != MI355_SPMV_OK || val_type != MI355_VAL_F32 ||
                          vec_type != s.feat_type))) {
                fprintf(stderr, "attention_bwd_sim: get_info\n");
                return 5;
            }
        } else if (tag == 4) {
            run(s);
        } else {
            fprintf(stderr, "attention_bwd_sim: unknown record %lld\n", (long long)tag);
            return 4;
        }
    }
    if (s.plan && mi355_spmv_attention_bwd_destroy(s.plan) != MI355_SPMV_OK) return 5;
    const int64_t end = -1;
    put(&end, 8);
    if (fclose(g_out) != 0) return 4;
    fclose(g_in);
    return 0;
}
