// attention_bwd_heads_sim — TEST CODE.  csrc/attention_bwd.hip (beside csrc/coo_csr.hip, the transpose that a create runs),
// unchanged, compiled with the HOST compiler over tests/cpp/simt and driven through the real mi355_spmv_attention_bwd_create /
// _create_half, _reserve_heads, _execute_heads and _execute: the backward cases of tests/attention_heads_cases.py.  As
// attention_heads_sim: every operand of all heads is ONE allocation exactly as long as the heads call may touch; the heads
// execute and the per-head executes write two sets of outputs of the same layout, and the test file compares them bit for
// bit.  Built with -fsanitize=address,undefined (tests/cpp/heads.mk).
//
//   attention_bwd_heads_sim BATCH OUT
//
// Records (int64 words, then raw little-endian arrays):
//   1  matrix   off_type feat_type n_rows n_cols nnz d_max dv_max | Ap[n_rows + 1] Aj[nnz]
//   4  run      n_heads n_heads_max d dv bias_heads (0: none) need_dq need_dk need_dv want_dbias shift |
//               ld and stride of Q, K, V, O, dO, dQ, dK, dV | stride of bias, lse, dbias | nan_bits canary_bits side_canary_bits |
//               scale (1 double) | the stored heads of Q, K, V, O, dO compact, then of lse, then of bias
//   8  refusal  n_heads | strides q k v bias o d_o lse dq dk dv dbias | d dv | ld of Q, K, V, O, dO, dQ, dK, dV | need_dq need_dk need_dv
//               want_dbias: execute_heads of the current object on dummy pointers, which a refusal never reads; the result is
//               the status and 256 bytes of the error text
//   0  end
// A result: status of reserve_heads, of execute_heads, the worst status of the executes, n_heads_max as reported, the
// elements outside every head's rows x width of the outputs (both sets) that lost their canary, the bytes of the other
// heads' scratch that were touched, scratch_bytes and held_bytes as get_info reports them; then, of those the run asked for,
// dQ, dK, dV and dbias of the heads call, each followed by that of the single calls.
#include "sim_runtime.hpp"

#include "../../spmv-samples_amd/csrc/coo_csr.hip"

#include "../../spmv-samples_amd/csrc/attention_bwd.hip"

#define SIM_NAME "attention_bwd_heads_sim"
#include "sim_io.hpp"
#include "sim_operand.hpp"
#include "sim_heads.hpp"

namespace {

struct State {
    int off_type = 0, feat_type = 0;
    size_t eb = 0, sb = 0;
    int64_t n_rows = 0, n_cols = 0, nnz = 0;
    Buf Ap, Aj;
    mi355_spmv_attention_bwd* plan = nullptr;
};

void run(State& s) {
    const int64_t H = word(), H_max = word(), d = word(), dv = word(), bias_heads = word();
    const int64_t need_dq = word(), need_dk = word(), need_dv = word(), want_dbias = word(), shift = word();
    int64_t ld[8], st[8];
    for (int i = 0; i < 8; ++i) { ld[i] = word(); st[i] = word(); }
    const int64_t s_bias = word(), s_lse = word(), s_dbias = word(), nan_bits = word(), canary_bits = word(), side_canary_bits = word();
    double scale;
    get(&scale, sizeof(scale));
    if (!s.plan) { fprintf(stderr, SIM_NAME ": bad run record\n"); exit(4); }
    HeadsOperand Q, K, V, O, dO, lse, bias, dQ, dK, dV, dbias, dQ1, dK1, dV1, dbias1;
    Q.make(H, s.n_rows, d, ld[0], st[0], s.eb, shift, nan_bits); Q.read();
    K.make(H, s.n_cols, d, ld[1], st[1], s.eb, shift, nan_bits); K.read();
    V.make(H, s.n_cols, dv, ld[2], st[2], s.eb, shift, nan_bits); V.read();
    O.make(H, s.n_rows, dv, ld[3], st[3], s.eb, shift, nan_bits); O.read();
    dO.make(H, s.n_rows, dv, ld[4], st[4], s.eb, shift, nan_bits); dO.read();
    lse.make(H, 1, s.n_rows, s.n_rows, s_lse, s.sb, shift, nan_bits); lse.read();
    if (bias_heads) { bias.make(H, 1, s.nnz, s.nnz, s_bias, s.sb, shift, nan_bits); bias.read(); }
    if (need_dq) { dQ.make(H, s.n_rows, d, ld[5], st[5], s.eb, shift, canary_bits); dQ1.like(dQ); }
    if (need_dk) { dK.make(H, s.n_cols, d, ld[6], st[6], s.eb, shift, canary_bits); dK1.like(dK); }
    if (need_dv) { dV.make(H, s.n_cols, dv, ld[7], st[7], s.eb, shift, canary_bits); dV1.like(dV); }
    if (want_dbias) { dbias.make(H, 1, s.nnz, s.nnz, s_dbias, s.sb, shift, side_canary_bits); dbias1.like(dbias); }
    const mi355_spmv_attention_bwd_head_strides hs{st[0], st[1], st[2], s_bias, st[3], st[4], s_lse, st[5], st[6], st[7], s_dbias};
    mi355_spmv_attention_bwd_info before, info;
    if (mi355_spmv_attention_bwd_get_info(s.plan, &before) != MI355_SPMV_OK) exit(5);
    int64_t st_reserve = mi355_spmv_attention_bwd_reserve_heads(s.plan, int32_t(H_max));
    int32_t reported = -1;
    if (mi355_spmv_attention_bwd_get_heads_max(s.plan, &reported) != MI355_SPMV_OK || mi355_spmv_attention_bwd_get_info(s.plan, &info) != MI355_SPMV_OK) exit(5);
    if (info.held_bytes != before.held_bytes) { fprintf(stderr, SIM_NAME ": reserve_heads changed held_bytes\n"); exit(5); }
    const size_t used = size_t(H) * mi355::attn_head_scratch_stride(s.plan->head_bytes);
    poison_rest(s.plan->scratch, s.plan->scratch_bytes, used);
    int64_t st_heads = mi355_spmv_attention_bwd_set_scale(s.plan, scale);
    if (st_heads == MI355_SPMV_OK)
        st_heads = mi355_spmv_attention_bwd_execute_heads(s.plan, int32_t(H), H > 1 ? &hs : nullptr, int32_t(d), int32_t(dv), Q.p, ld[0], K.p, ld[1], V.p, ld[2],
                                                          bias.p, O.p, ld[3], dO.p, ld[4], lse.p, dQ.p, ld[5], dK.p, ld[6], dV.p, ld[7], dbias.p, nullptr);
    if (st_heads != MI355_SPMV_OK) fprintf(stderr, SIM_NAME ": execute_heads -> %d (%s)\n", int(st_heads), mi355::g_error);
    const int64_t touched = rest_touched(s.plan->scratch, s.plan->scratch_bytes, used);
    int64_t st_single = 0;
    for (int64_t h = 0; h < H; ++h) {
        const int64_t e = mi355_spmv_attention_bwd_execute(s.plan, int32_t(d), int32_t(dv), Q.head(h), ld[0], K.head(h), ld[1], V.head(h), ld[2], bias.head(h),
                                                           O.head(h), ld[3], dO.head(h), ld[4], lse.head(h), dQ1.head(h), ld[5], dK1.head(h), ld[6],
                                                           dV1.head(h), ld[7], dbias1.head(h), nullptr);
        if (e != MI355_SPMV_OK) { fprintf(stderr, SIM_NAME ": execute -> %d (%s)\n", int(e), mi355::g_error); st_single = e; }
    }
    int64_t bad = 0;
    for (const HeadsOperand* o : {&dQ, &dK, &dV, &dbias, &dQ1, &dK1, &dV1, &dbias1}) bad += o->lost();
    const int64_t rep = reported, sbytes = info.scratch_bytes, hbytes = info.held_bytes, st_r = st_reserve, st_h = st_heads, st_s = st_single, tch = touched, lost = bad;
    for (const int64_t* v : {&st_r, &st_h, &st_s, &rep, &lost, &tch, &sbytes, &hbytes}) put(v, 8);
    dQ.write(); dQ1.write(); dK.write(); dK1.write(); dV.write(); dV1.write(); dbias.write(); dbias1.write();
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: " SIM_NAME " BATCH OUT\n"); return 2; }
    g_in = fopen(argv[1], "rb");
    g_out = fopen(argv[2], "wb");
    if (!g_in || !g_out) { perror(SIM_NAME ": open"); return 2; }
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
            if (st != MI355_SPMV_OK) { fprintf(stderr, SIM_NAME ": create (type %d) -> %d (%s)\n", s.feat_type, st, mi355::g_error); return 5; }
        } else if (tag == 4) {
            run(s);
        } else if (tag == 8) {
            int64_t v[26];
            for (int64_t& x : v) x = word();
            const mi355_spmv_attention_bwd_head_strides hs{v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9], v[10], v[11]};
            void* const dummy = reinterpret_cast<void*>(256);
            const int64_t st = mi355_spmv_attention_bwd_execute_heads(s.plan, int32_t(v[0]), &hs, int32_t(v[12]), int32_t(v[13]), dummy, v[14], dummy, v[15],
                                                                      dummy, v[16], nullptr, dummy, v[17], dummy, v[18], dummy, v[22] ? dummy : nullptr, v[19],
                                                                      v[23] ? dummy : nullptr, v[20], v[24] ? dummy : nullptr, v[21],
                                                                      v[25] ? dummy : nullptr, nullptr);
            char text[256] = {0};
            snprintf(text, sizeof(text), "%.255s", mi355::g_error);
            put(&st, 8);
            put(text, sizeof(text));
        } else {
            fprintf(stderr, SIM_NAME ": unknown record %lld\n", (long long)tag);
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
