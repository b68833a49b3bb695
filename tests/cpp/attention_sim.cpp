// attention_sim — TEST CODE.  csrc/attention.hip with what it includes (attention_slice_walk.inc, attention_half_kernel.hpp),
// unchanged, compiled with the HOST compiler over tests/cpp/simt (a stand-in <hip/hip_runtime.h> that runs every lane of a
// workgroup as a fiber) and driven through the real extern "C" entry points: mi355_spmv_attention_create or _create_half,
// then the object's set_scale / execute / destroy, so the slice passes, the fix-up (with its one narrowing under 16-bit
// features) and the object's scratch run as well.  One program for the two tables (tests/attention_cases.py,
// tests/attention_half_cases.py): the matrix record says which create it is.  The program only moves bit patterns: element
// sizes come from the type word and every fill value arrives as bits.  Built with -fsanitize=address,undefined
// (tests/cpp/Makefile).
//
//   attention_sim BATCH OUT      reads records from BATCH, writes one result per run record to OUT
//
// Records are int64 words followed by raw little-endian arrays (tests/attention_cases.py writes them, write_batch):
//   1  matrix    off_type feat_type n_rows n_cols nnz ap_off aj_off d_max dv_max | Ap[n_rows + 1] Aj[nnz]
//   2  data      kf kv has_bias | Q[n_rows * kf] K[n_cols * kf] V[n_cols * kv], and bias[nnz] with has_bias
//   4  run       d dv c0 cv0 ldq ldk ldv ldo q_off k_off v_off bias_off o_off lse_off want_lse nan_bits canary_bits
//                side_nan_bits | scale (1 double)
//   0  end
// feat_type = the MI355_VAL_* of Q, K, V and O: F32 / F64 go through _create, F16 / BF16 through _create_half.  An element of
// Q, K, V and O has that type's bytes; one of bias and lse (the side arrays) 8 under F64 and 4 otherwise.  A run takes
// columns c0 .. c0 + d of Q and K and cv0 .. cv0 + dv of V.  *_off = elements between a 64-byte boundary and the operand's
// base.  Every operand is an allocation of its own, exactly as long as the call may touch: (rows - 1) * ld + width elements,
// the padding columns of Q, K and V filled with nan_bits, all of O with canary_bits and lse with side_nan_bits — so a read
// or write one element outside is a report, and a write into O's padding is counted.  A result is: status, the padding
// elements of O that lost their canary, count = n_rows * dv, then O compact (count elements) and lse (n_rows side elements;
// side_nan_bits where not asked).
#include "../../spmv-samples_amd/csrc/attention.hip"

#define SIM_NAME "attention_sim"
#include "sim_io.hpp"
#include "sim_operand.hpp"

namespace {

struct State {
    int off_type = 0, feat_type = 0;
    size_t eb = 0, sb = 0;          // bytes of an element of Q, K, V and O; of bias and lse
    int64_t n_rows = 0, n_cols = 0, nnz = 0;
    Buf Ap, Aj;
    int64_t kf = 0, kv = 0;
    bool has_bias = false;
    std::vector<char> Q, K, V, bias;
    mi355_spmv_attention* plan = nullptr;
};

void run(State& s) {
    const int64_t d = word(), dv = word(), c0 = word(), cv0 = word(), ldq = word(), ldk = word(), ldv = word(), ldo = word();
    const int64_t q_off = word(), k_off = word(), v_off = word(), b_off = word(), o_off = word(), lse_off = word();
    const int64_t want_lse = word(), nan_bits = word(), canary_bits = word(), side_nan_bits = word();
    double scale;
    get(&scale, sizeof(scale));
    if (!s.plan || s.kf == 0 || c0 + d > s.kf || cv0 + dv > s.kv) { fprintf(stderr, "attention_sim: bad run record\n"); exit(4); }
    Operand Q, K, V, bias, O, lse;
    Q.make(s.n_rows, d, ldq, s.eb, q_off, nan_bits, s.Q.data(), s.kf, c0);
    K.make(s.n_cols, d, ldk, s.eb, k_off, nan_bits, s.K.data(), s.kf, c0);
    V.make(s.n_cols, dv, ldv, s.eb, v_off, nan_bits, s.V.data(), s.kv, cv0);
    if (s.has_bias) bias.make(s.nnz, 1, 1, s.sb, b_off, 0, s.bias.data(), 1);
    O.make(s.n_rows, dv, ldo, s.eb, o_off, canary_bits);
    lse.make(s.n_rows, 1, 1, s.sb, lse_off, side_nan_bits);
    int64_t st = mi355_spmv_attention_set_scale(s.plan, scale);
    if (st == MI355_SPMV_OK)
        st = mi355_spmv_attention_execute(s.plan, int32_t(d), int32_t(dv), Q.p, ldq, K.p, ldk, V.p, ldv, bias.p, O.p, ldo, want_lse ? lse.p : nullptr,
                                          nullptr);
    if (st != MI355_SPMV_OK) fprintf(stderr, "attention_sim: execute -> %d (%s)\n", int(st), mi355::g_error);
    const int64_t bad = O.lost(), count = s.n_rows * dv;
    put(&st, 8);
    put(&bad, 8);
    put(&count, 8);
    O.write();
    lse.write();
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: attention_sim BATCH OUT\n"); return 2; }
    g_in = fopen(argv[1], "rb");
    g_out = fopen(argv[2], "wb");
    if (!g_in || !g_out) { perror("attention_sim: open"); return 2; }
    State s;
    for (;;) {
        const int64_t tag = word();
        if (tag == 0) break;
        if (tag == 1) {
            if (s.plan) { mi355_spmv_attention_destroy(s.plan); s.plan = nullptr; }
            s.off_type = int(word()); s.feat_type = int(word());
            s.n_rows = word(); s.n_cols = word(); s.nnz = word();
            const int64_t ap_off = word(), aj_off = word(), d_max = word(), dv_max = word();
            const size_t ob = s.off_type == MI355_OFF_I64 ? 8 : 4;
            const bool half = s.feat_type == MI355_VAL_F16 || s.feat_type == MI355_VAL_BF16;
            s.eb = type_bytes(s.feat_type);
            s.sb = s.feat_type == MI355_VAL_F64 ? 8 : 4;
            s.kf = 0;
            s.Ap.alloc(size_t(s.n_rows) + 1, ob, size_t(ap_off));
            s.Aj.alloc(size_t(s.nnz), 4, size_t(aj_off));
            get(s.Ap.p, (size_t(s.n_rows) + 1) * ob);
            get(s.Aj.p, size_t(s.nnz) * 4);
            const int32_t* Aj = reinterpret_cast<const int32_t*>(s.Aj.p);
            const int st = half ? mi355_spmv_attention_create_half(&s.plan, s.off_type, s.feat_type, int32_t(s.n_rows), int32_t(s.n_cols), s.nnz, s.Ap.p,
                                                                   Aj, int32_t(d_max), int32_t(dv_max))
                                : mi355_spmv_attention_create(int32_t(s.n_rows), int32_t(s.n_cols), s.nnz, s.Ap.p, Aj, s.off_type, s.feat_type,
                                                              int32_t(d_max), int32_t(dv_max), &s.plan);
            if (st != MI355_SPMV_OK) { fprintf(stderr, "attention_sim: create (type %d) -> %d (%s)\n", s.feat_type, st, mi355::g_error); return 5; }
            mi355_spmv_attention_info info;
            int val_type = -1, vec_type = -1;
            if (mi355_spmv_attention_get_info(s.plan, &info) != MI355_SPMV_OK || info.n_slices != (s.n_rows + s.nnz + info.slice_len - 1) / info.slice_len ||
                info.passes != (dv_max + info.widest_tile - 1) / info.widest_tile ||
                (half && (info.widest_tile != 64 || info.val_type != MI355_VAL_F32 ||
                          mi355_spmv_attention_get_types(s.plan, &val_type, &vec_type) != MI355_SPMV_OK || val_type != MI355_VAL_F32 ||
                          vec_type != s.feat_type))) {
                fprintf(stderr, "attention_sim: get_info\n");
                return 5;
            }
        } else if (tag == 2) {
            s.kf = word(); s.kv = word(); s.has_bias = word() != 0;
            s.Q.resize(size_t(s.n_rows * s.kf) * s.eb);
            s.K.resize(size_t(s.n_cols * s.kf) * s.eb);
            s.V.resize(size_t(s.n_cols * s.kv) * s.eb);
            s.bias.resize(s.has_bias ? size_t(s.nnz) * s.sb : 0);
            get(s.Q.data(), s.Q.size());
            get(s.K.data(), s.K.size());
            get(s.V.data(), s.V.size());
            get(s.bias.data(), s.bias.size());
        } else if (tag == 4) {
            run(s);
        } else {
            fprintf(stderr, "attention_sim: unknown record %lld\n", (long long)tag);
            return 4;
        }
    }
    if (s.plan && mi355_spmv_attention_destroy(s.plan) != MI355_SPMV_OK) return 5;
    const int64_t end = -1;
    put(&end, 8);
    if (fclose(g_out) != 0) return 4;
    fclose(g_in);
    return 0;
}
