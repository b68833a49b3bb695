// attention_bwd_half_sim — TEST CODE.  csrc/attention_bwd.hip (with attention_bwd_half_kernel.hpp and
// attention_bwd_slice_walk.inc), unchanged, compiled with the HOST compiler over tests/cpp/simt (a stand-in
// <hip/hip_runtime.h> that runs every lane of a workgroup as a fiber) and driven through the real extern "C" entry points:
// mi355_spmv_attention_bwd_create_half (whose transpose is csrc/coo_csr.hip, compiled the same way), then the object's
// set_scale / execute / destroy, so the 16-bit delta kernel, the three roles of the walk, the narrowing fix-ups and the
// object's scratch run as well.  Built with -fsanitize=address,undefined (tests/cpp/attention_bwd_half_sim.mk).
//
//   attention_bwd_half_sim BATCH OUT      reads records from BATCH, writes one result per run record to OUT
//
// Records are int64 words followed by raw little-endian arrays (tests/attention_bwd_half_cases.py writes them, write_batch):
//   1  matrix    off_type vec_type n_rows n_cols nnz d_max dv_max | Ap[n_rows + 1] Aj[nnz]
//   4  run       d dv pad[8] shift has_bias need_dq need_dk need_dv want_dbias nan_bits canary_bits | scale (1 double) |
//                Q[n_rows * d] K[n_cols * d] V[n_cols * dv] O[n_rows * dv] dO[n_rows * dv] as 16-bit patterns, lse[n_rows]
//                as float, bias[nnz] as float with has_bias
//   0  end
// pad = leading dimension - width of Q, K, V, O, dO, dQ, dK, dV; shift = elements between a 64-byte boundary and every
// operand's base.  Every operand is an allocation of its own, exactly as long as the call may touch: (rows - 1) * ld + width
// elements, the padding columns of the inputs filled with the type's NaN bits and all of an output with a canary — so a read
// or write one element outside is a report, and a write into an output's padding is counted.  A result is: status, the
// padding elements that lost their canary, then dQ, dK, dV compact (16-bit patterns) and dbias (float) — those the run
// asked for.
#include <cstring>
#include <limits>
#include <vector>

#include "sim_runtime.hpp"

#include "../../spmv-samples_amd/csrc/coo_csr.hip"

#include "../../spmv-samples_amd/csrc/attention_bwd.hip"

#define SIM_NAME "attention_bwd_half_sim"
#include "sim_io.hpp"

namespace {

constexpr double kCanary = -776.0;      // the fp32 canary of dbias; the 16-bit one comes with the run record

struct State {
    int off_type = 0, vec_type = 0;
    int64_t n_rows = 0, n_cols = 0, nnz = 0;
    Buf Ap, Aj;
    mi355_spmv_attention_bwd* plan = nullptr;
};

void fill(char* p, size_t elems, size_t vb, double v64, int64_t bits, bool use_bits) {
    const float v32 = float(v64);
    for (size_t i = 0; i < elems; ++i) {
        if (use_bits) memcpy(p + i * vb, &bits, vb);
        else memcpy(p + i * vb, vb == 8 ? static_cast<const void*>(&v64) : &v32, vb);
    }
}

size_t span(int64_t rows, int64_t ld, int64_t width) { return rows > 0 ? size_t((rows - 1) * ld + width) : 0; }

// rows x width compact values from the batch, as an operand of leading dimension ld with NaN padding
void read_operand(Buf& b, int64_t rows, int64_t width, int64_t ld, size_t vb, int64_t off, int64_t nan_bits) {
    std::vector<char> full(size_t(rows * width) * vb);
    get(full.data(), full.size());
    b.alloc(span(rows, ld, width), vb, size_t(off));
    fill(b.p, span(rows, ld, width), vb, 0.0, nan_bits, true);
    for (int64_t r = 0; r < rows; ++r) memcpy(b.p + size_t(r * ld) * vb, full.data() + size_t(r * width) * vb, size_t(width) * vb);
}

struct Output {
    Buf b;
    int64_t rows = 0, width = 0, ld = 0;
    bool asked = false;
    size_t vb = 0;
    int64_t canary_bits = 0;        // of a 16-bit output; a 4-byte one (dbias) takes kCanary
    void make(bool want, int64_t rows_, int64_t width_, int64_t ld_, size_t vb_, int64_t off, int64_t bits) {
        asked = want; rows = rows_; width = width_; ld = ld_; vb = vb_; canary_bits = bits;
        if (!want) return;
        b.alloc(span(rows, ld, width), vb, size_t(off));
        fill(b.p, span(rows, ld, width), vb, kCanary, canary_bits, vb == 2);
    }
    int64_t bad() const {
        if (!asked) return 0;
        int64_t n = 0;
        std::vector<char> canary(vb);
        fill(canary.data(), 1, vb, kCanary, canary_bits, vb == 2);
        for (int64_t r = 0; r + 1 < rows; ++r)
            for (int64_t j = width; j < ld; ++j) n += memcmp(b.p + size_t(r * ld + j) * vb, canary.data(), vb) != 0;
        return n;
    }
    void write() const {
        if (!asked) return;
        for (int64_t r = 0; r < rows; ++r) put(b.p + size_t(r * ld) * vb, size_t(width) * vb);
    }
};

void run(State& s) {
    constexpr size_t vb = 2, fb = 4;        // bytes of a matrix element; of lse, bias and dbias
    const int64_t d = word(), dv = word();
    int64_t pad[8];
    for (int64_t& p : pad) p = word();
    const int64_t shift = word(), has_bias = word(), need_dq = word(), need_dk = word(), need_dv = word(), want_dbias = word(), nan_bits = word(), canary_bits = word();
    double scale;
    get(&scale, sizeof(scale));
    if (!s.plan) { fprintf(stderr, "attention_bwd_half_sim: bad run record\n"); exit(4); }
    const int64_t ldq = d + pad[0], ldk = d + pad[1], ldv = dv + pad[2], ldo = dv + pad[3], lddo = dv + pad[4];
    Buf bq, bk, bv, bo, bg, bl, bb;
    read_operand(bq, s.n_rows, d, ldq, vb, shift, nan_bits);
    read_operand(bk, s.n_cols, d, ldk, vb, shift, nan_bits);
    read_operand(bv, s.n_cols, dv, ldv, vb, shift, nan_bits);
    read_operand(bo, s.n_rows, dv, ldo, vb, shift, nan_bits);
    read_operand(bg, s.n_rows, dv, lddo, vb, shift, nan_bits);
    read_operand(bl, s.n_rows, 1, 1, fb, shift, 0x7FC00000);
    if (has_bias) read_operand(bb, s.nnz, 1, 1, fb, shift, 0x7FC00000);
    Output oq, ok, ov, ob;
    oq.make(need_dq != 0, s.n_rows, d, d + pad[5], vb, shift, canary_bits);
    ok.make(need_dk != 0, s.n_cols, d, d + pad[6], vb, shift, canary_bits);
    ov.make(need_dv != 0, s.n_cols, dv, dv + pad[7], vb, shift, canary_bits);
    ob.make(want_dbias != 0, s.nnz, 1, 1, fb, shift, 0);
    int64_t st = mi355_spmv_attention_bwd_set_scale(s.plan, scale);
    if (st == MI355_SPMV_OK)
        st = mi355_spmv_attention_bwd_execute(s.plan, int32_t(d), int32_t(dv), bq.p, ldq, bk.p, ldk, bv.p, ldv, has_bias ? bb.p : nullptr, bo.p, ldo, bg.p,
                                              lddo, bl.p, oq.asked ? oq.b.p : nullptr, oq.ld, ok.asked ? ok.b.p : nullptr, ok.ld,
                                              ov.asked ? ov.b.p : nullptr, ov.ld, ob.asked ? ob.b.p : nullptr, nullptr);
    if (st != MI355_SPMV_OK) fprintf(stderr, "attention_bwd_half_sim: execute -> %d (%s)\n", int(st), mi355::g_error);
    const int64_t bad = oq.bad() + ok.bad() + ov.bad();
    put(&st, 8);
    put(&bad, 8);
    oq.write(); ok.write(); ov.write(); ob.write();
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: attention_bwd_half_sim BATCH OUT\n"); return 2; }
    g_in = fopen(argv[1], "rb");
    g_out = fopen(argv[2], "wb");
    if (!g_in || !g_out) { perror("attention_bwd_half_sim: open"); return 2; }
    State s;
    for (;;) {
        const int64_t tag = word();
        if (tag == 0) break;
        if (tag == 1) {
            if (s.plan) { mi355_spmv_attention_bwd_destroy(s.plan); s.plan = nullptr; }
            s.off_type = int(word()); s.vec_type = int(word());
            s.n_rows = word(); s.n_cols = word(); s.nnz = word();
            const int64_t d_max = word(), dv_max = word();
            const size_t ob = s.off_type == MI355_OFF_I64 ? 8 : 4;
            s.Ap.alloc(size_t(s.n_rows) + 1, ob, 0);
            s.Aj.alloc(size_t(s.nnz), 4, 0);
            get(s.Ap.p, (size_t(s.n_rows) + 1) * ob);
            get(s.Aj.p, size_t(s.nnz) * 4);
            const int st = mi355_spmv_attention_bwd_create_half(&s.plan, s.off_type, s.vec_type, int32_t(s.n_rows), int32_t(s.n_cols), s.nnz, s.Ap.p,
                                                                reinterpret_cast<const int32_t*>(s.Aj.p), int32_t(d_max), int32_t(dv_max), nullptr);
            if (st != MI355_SPMV_OK) { fprintf(stderr, "attention_bwd_half_sim: create -> %d (%s)\n", st, mi355::g_error); return 5; }
            mi355_spmv_attention_bwd_info info;
            int val_type = -1, vec_type = -1;
            if (mi355_spmv_attention_bwd_get_info(s.plan, &info) != MI355_SPMV_OK || info.val_type != MI355_VAL_F32 || info.widest_tile != 64 ||
                mi355_spmv_attention_bwd_get_types(s.plan, &val_type, &vec_type) != MI355_SPMV_OK || val_type != MI355_VAL_F32 || vec_type != s.vec_type ||
                info.n_slices != (s.n_rows + s.nnz + info.slice_len - 1) / info.slice_len ||
                info.n_slices_t != (s.n_cols + s.nnz + info.slice_len - 1) / info.slice_len) {
                fprintf(stderr, "attention_bwd_half_sim: get_info\n");
                return 5;
            }
        } else if (tag == 4) {
            run(s);
        } else {
            fprintf(stderr, "attention_bwd_half_sim: unknown record %lld\n", (long long)tag);
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
