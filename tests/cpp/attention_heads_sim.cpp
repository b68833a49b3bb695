// attention_heads_sim — TEST CODE.  csrc/attention.hip, unchanged, compiled with the HOST compiler over tests/cpp/simt and
// driven through the real mi355_spmv_attention_create / _create_half, _reserve_heads, _execute_heads and _execute: the table
// of tests/attention_heads_cases.py (its forward cases).  A run makes every operand of all heads as ONE allocation exactly as
// long as the heads call may touch, runs execute_heads into outputs full of a canary, then runs execute once per head, on
// the operands offset by h strides, into a second set of outputs of the same layout.  The result holds both sets; the test
// file compares them bit for bit.  Built with -fsanitize=address,undefined (tests/cpp/heads.mk).
//
//   attention_heads_sim BATCH OUT
//
// Records are int64 words followed by raw little-endian arrays (tests/attention_heads_cases.py writes them):
//   1  matrix   off_type feat_type n_rows n_cols nnz d_max dv_max | Ap[n_rows + 1] Aj[nnz]
//   4  run      n_heads n_heads_max d dv want_lse bias_heads (0: none) shift | ld and stride of Q, K, V, O | stride of bias, lse |
//               nan_bits canary_bits side_canary_bits | scale (1 double) | the stored heads of Q, K, V compact, then of bias
//   8  refusal  n_heads | strides q k v bias o lse | d dv ldq ldk ldv ldo want_lse: execute_heads of the current object on dummy
//               pointers, which a refusal never reads; the result is the status and 256 bytes of the error text
//   9  grid     n_heads n_slices width: the status of the grid check alone (no object can be that large in a test)
//   0  end
// A result of a run: status of reserve_heads, of execute_heads, the worst status of the executes, n_heads_max as the object
// reports it, the elements outside every head's rows x width of O (both sets) that lost their canary, the bytes of the other
// heads' scratch that were touched, scratch_bytes as get_info reports it; then O of the heads call, O of the single calls,
// lse of the heads call and lse of the single calls (every head compact).  A result of a grid record: the status.
#include "../../spmv-samples_amd/csrc/attention.hip"

#define SIM_NAME "attention_heads_sim"
#include "sim_io.hpp"
#include "sim_operand.hpp"
#include "sim_heads.hpp"

namespace {

struct State {
    int off_type = 0, feat_type = 0;
    size_t eb = 0, sb = 0;
    int64_t n_rows = 0, n_cols = 0, nnz = 0;
    Buf Ap, Aj;
    mi355_spmv_attention* plan = nullptr;
};

void run(State& s) {
    const int64_t H = word(), H_max = word(), d = word(), dv = word(), want_lse = word(), bias_heads = word(), shift = word();
    int64_t ld[4], st[4];
    for (int i = 0; i < 4; ++i) { ld[i] = word(); st[i] = word(); }
    const int64_t s_bias = word(), s_lse = word(), nan_bits = word(), canary_bits = word(), side_canary_bits = word();
    double scale;
    get(&scale, sizeof(scale));
    if (!s.plan) { fprintf(stderr, SIM_NAME ": bad run record\n"); exit(4); }
    HeadsOperand Q, K, V, bias, O, lse, O1, lse1;
    Q.make(H, s.n_rows, d, ld[0], st[0], s.eb, shift, nan_bits); Q.read();
    K.make(H, s.n_cols, d, ld[1], st[1], s.eb, shift, nan_bits); K.read();
    V.make(H, s.n_cols, dv, ld[2], st[2], s.eb, shift, nan_bits); V.read();
    if (bias_heads) { bias.make(H, 1, s.nnz, s.nnz, s_bias, s.sb, shift, nan_bits); bias.read(); }
    O.make(H, s.n_rows, dv, ld[3], st[3], s.eb, shift, canary_bits);
    O1.like(O);
    if (want_lse) { lse.make(H, 1, s.n_rows, s.n_rows, s_lse, s.sb, shift, side_canary_bits); lse1.like(lse); }
    const mi355_spmv_attention_head_strides hs{st[0], st[1], st[2], s_bias, st[3], s_lse};
    int64_t st_reserve = mi355_spmv_attention_reserve_heads(s.plan, int32_t(H_max));
    int32_t reported = -1;
    mi355_spmv_attention_info info;
    if (mi355_spmv_attention_get_heads_max(s.plan, &reported) != MI355_SPMV_OK || mi355_spmv_attention_get_info(s.plan, &info) != MI355_SPMV_OK) exit(5);
    const size_t used = size_t(H) * mi355::attn_head_scratch_stride(s.plan->head_bytes);
    poison_rest(s.plan->scratch, s.plan->scratch_bytes, used);
    int64_t st_heads = mi355_spmv_attention_set_scale(s.plan, scale);
    if (st_heads == MI355_SPMV_OK)
        st_heads = mi355_spmv_attention_execute_heads(s.plan, int32_t(H), H > 1 ? &hs : nullptr, int32_t(d), int32_t(dv), Q.p, ld[0], K.p, ld[1], V.p, ld[2],
                                                      bias.p, O.p, ld[3], lse.p, nullptr);
    if (st_heads != MI355_SPMV_OK) fprintf(stderr, SIM_NAME ": execute_heads -> %d (%s)\n", int(st_heads), mi355::g_error);
    const int64_t touched = rest_touched(s.plan->scratch, s.plan->scratch_bytes, used);
    int64_t st_single = 0;
    for (int64_t h = 0; h < H; ++h) {
        const int64_t e = mi355_spmv_attention_execute(s.plan, int32_t(d), int32_t(dv), Q.head(h), ld[0], K.head(h), ld[1], V.head(h), ld[2], bias.head(h),
                                                       O1.head(h), ld[3], lse1.head(h), nullptr);
        if (e != MI355_SPMV_OK) { fprintf(stderr, SIM_NAME ": execute -> %d (%s)\n", int(e), mi355::g_error); st_single = e; }
    }
    const int64_t bad = O.lost() + O1.lost() + lse.lost() + lse1.lost(), rep = reported, sbytes = info.scratch_bytes;
    const int64_t st_r = st_reserve, st_h = st_heads, st_s = st_single, tch = touched;
    for (const int64_t* v : {&st_r, &st_h, &st_s, &rep, &bad, &tch, &sbytes}) put(v, 8);
    O.write(); O1.write(); lse.write(); lse1.write();
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
            if (s.plan) { mi355_spmv_attention_destroy(s.plan); s.plan = nullptr; }
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
            const int32_t* Aj = reinterpret_cast<const int32_t*>(s.Aj.p);
            const int st = half ? mi355_spmv_attention_create_half(&s.plan, s.off_type, s.feat_type, int32_t(s.n_rows), int32_t(s.n_cols), s.nnz, s.Ap.p,
                                                                   Aj, int32_t(d_max), int32_t(dv_max))
                                : mi355_spmv_attention_create(int32_t(s.n_rows), int32_t(s.n_cols), s.nnz, s.Ap.p, Aj, s.off_type, s.feat_type,
                                                              int32_t(d_max), int32_t(dv_max), &s.plan);
            if (st != MI355_SPMV_OK) { fprintf(stderr, SIM_NAME ": create (type %d) -> %d (%s)\n", s.feat_type, st, mi355::g_error); return 5; }
        } else if (tag == 4) {
            run(s);
        } else if (tag == 8) {
            int64_t v[14];
            for (int64_t& x : v) x = word();
            const mi355_spmv_attention_head_strides hs{v[1], v[2], v[3], v[4], v[5], v[6]};
            void* const dummy = reinterpret_cast<void*>(256);
            const int64_t st = mi355_spmv_attention_execute_heads(s.plan, int32_t(v[0]), &hs, int32_t(v[7]), int32_t(v[8]), dummy, v[9], dummy, v[10], dummy,
                                                                  v[11], nullptr, dummy, v[12], v[13] ? dummy : nullptr, nullptr);
            char text[256] = {0};
            snprintf(text, sizeof(text), "%.255s", mi355::g_error);
            put(&st, 8);
            put(text, sizeof(text));
        } else if (tag == 9) {
            const int64_t H = word(), n_slices = word(), width = word();
            const int64_t st = mi355::attn_check_heads_grid(SIM_NAME, int32_t(H), n_slices, width);
            put(&st, 8);
        } else {
            fprintf(stderr, SIM_NAME ": unknown record %lld\n", (long long)tag);
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
