// coo_sim — TEST CODE.  csrc/coo_csr.hip, unchanged, compiled with the HOST compiler over tests/cpp/simt (a stand-in
// <hip/hip_runtime.h> that runs every lane of a workgroup as a fiber) and driven through the real extern "C" entry points:
// mi355_spmv_coo_to_csr, mi355_spmv_coo_to_csr_symmetric (after mi355_spmv_coo_symmetric_nnz) and mi355_spmv_csr_transpose,
// each with its size query first.  Because the unit is included as text, the kernels of mi355::coo are also launched alone,
// at sizes the entry points reach only with 2^28 entries.  Built with -fsanitize=address,undefined (tests/cpp/Makefile).
//
//   coo_sim BATCH OUT      reads records from BATCH, writes one result per record to OUT
//
// Records are int64 words followed by raw little-endian arrays (tests/coo_cases.py writes them, write_batch):
//   1  coo        off_type val_type want_perm n_rows n_cols nnz prefill compact | rows[nnz] cols[nnz] vals[nnz]
//   2  sym        off_type val_type want_perm n_rows n_cols nnz_stored nnz_expanded prefill compact | rows cols vals (stored)
//   3  transpose  off_type n_rows n_cols nnz prefill compact | Ap[n_rows + 1] Aj[nnz]
//   5  scan_sums  n | v[n] (uint32)                 scan_sums alone, in place
//   6  scan_chain n | counts[n] (uint32)            scan_reduce -> scan_sums -> scan_apply, as a pass runs them
//   7  offdiag    nnz | rows[nnz] cols[nnz]         offdiag_count on n_etiles + 1 workgroups -> scan_sums
//   0  end
// val_type -1: no values (vals and Ax are null).  want_perm 0: perm is null.  prefill: the byte the workspace holds
// before the call.  A result of 1-3 is: status, the length of the library's message, the message, then Ap (Apt), Aj (Ajt),
// Ax and perm as the call left them (those that exist); compact: Ap as a count and that many (index, value) pairs, one for
// index 0 and one wherever Ap[i] != Ap[i - 1] (lossless; 2^24 offsets are 64 MB).  A result of 5-7: 0, a count, that many
// uint32.
//
// Every operand and the workspace is an allocation of its own, exactly as long as the call may touch — the workspace exactly
// *workspace_bytes — so a read or write one element outside is a sanitizer report.  Outputs are filled with the byte 0xC3
// first (coo_cases.CANARY): a refused call must leave them so.
//
// The limit of this execution: the stand-in runs the lanes of a wave one after another between collectives, and the waves
// of a workgroup one after another between barriers.  An ordering that only lock-step execution provides is therefore not
// exercised here: in wave_digits every lane reads cnt[wave][d] before the last of its peers writes it, which on the host
// holds because the lower lanes run first.  The device run of the same table (tests/test_gpu_coo_edges.py) covers that.
#include <cstring>
#include <vector>

#include "sim_runtime.hpp"

#include "../../spmv-samples_amd/csrc/coo_csr.hip"

#define SIM_NAME "coo_sim"
#include "sim_io.hpp"

namespace {

constexpr int kCanary = 0xC3;

struct Out {       // an output of `elems` elements, or absent
    Buf b;
    size_t bytes = 0;
    void make(bool present, size_t elems, size_t elem_bytes) {
        if (!present) return;
        bytes = elems * elem_bytes;
        b.alloc(elems, elem_bytes, 0);
        memset(b.p, kCanary, bytes);
    }
    void write() const { put(b.p, bytes); }
};

void read_into(Buf& b, size_t elems, size_t elem_bytes) {
    b.alloc(elems, elem_bytes, 0);
    get(b.p, elems * elem_bytes);
}

void put_status(int64_t st) {
    const int64_t n = int64_t(strlen(mi355::g_error));
    put(&st, 8);
    put(&n, 8);
    put(mi355::g_error, size_t(n));
}

template <typename off_t>
void put_steps(const char* p, size_t n) {
    std::vector<int64_t> steps;
    off_t before = 0;
    for (size_t i = 0; i < n; ++i) {
        off_t v;
        memcpy(&v, p + i * sizeof(off_t), sizeof(off_t));
        if (i == 0 || v != before) { steps.push_back(int64_t(i)); steps.push_back(int64_t(v)); }
        before = v;
    }
    const int64_t m = int64_t(steps.size() / 2);
    put(&m, 8);
    put(steps.data(), steps.size() * 8);
}

void put_offsets(const Out& Ap, size_t n, size_t ob, bool compact) {
    if (!compact) Ap.write();
    else if (ob == 8) put_steps<int64_t>(Ap.b.p, n);
    else put_steps<int32_t>(Ap.b.p, n);
}

void workspace(Buf& ws, size_t bytes, int64_t prefill) {
    ws.alloc(bytes, 1, 0);
    memset(ws.p, int(prefill), bytes);
}

void coo(bool symmetric) {
    const int off_type = int(word()), val_type = int(word());
    const bool want_perm = word() != 0;
    const int64_t n_rows = word(), n_cols = word(), nnz = word(), expanded = symmetric ? word() : nnz, prefill = word();
    const bool compact = word() != 0;
    const size_t ob = off_type == MI355_OFF_I64 ? 8 : 4, vb = val_type < 0 ? 0 : val_type == MI355_VAL_F64 ? 8 : 4;
    const int vt = val_type < 0 ? MI355_VAL_F32 : val_type;
    Buf rows, cols, vals, ws;
    read_into(rows, size_t(nnz), 4);
    read_into(cols, size_t(nnz), 4);
    if (vb) read_into(vals, size_t(nnz), vb);
    Out Ap, Aj, Ax, perm;
    Ap.make(true, size_t(n_rows) + 1, ob);
    Aj.make(true, size_t(expanded), 4);
    Ax.make(vb != 0, size_t(expanded), vb);
    perm.make(want_perm, size_t(expanded), 8);
    const int32_t* r = reinterpret_cast<const int32_t*>(rows.p);
    const int32_t* c = reinterpret_cast<const int32_t*>(cols.p);
    size_t bytes = 0;
    int64_t st;
    if (symmetric) {
        int64_t counted = -1;       // the count is the caller's; the library's own must say what the reference says of valid entries
        if (mi355_spmv_coo_symmetric_nnz(nnz, r, c, nullptr, &counted) != MI355_SPMV_OK) { fprintf(stderr, "coo_sim: symmetric_nnz failed\n"); exit(5); }
        int64_t off_diagonal = 0;
        for (int64_t i = 0; i < nnz; ++i) off_diagonal += r[i] != c[i];
        if (counted != nnz + off_diagonal) { fprintf(stderr, "coo_sim: symmetric_nnz gives %lld, not %lld\n", (long long)counted, (long long)(nnz + off_diagonal)); exit(5); }
        st = mi355_spmv_coo_to_csr_symmetric(off_type, vt, int32_t(n_rows), int32_t(n_cols), nnz, expanded, nullptr, nullptr, nullptr, nullptr,
                                             nullptr, nullptr, nullptr, nullptr, &bytes, nullptr);
        if (st == MI355_SPMV_OK) {
            workspace(ws, bytes, prefill);
            st = mi355_spmv_coo_to_csr_symmetric(off_type, vt, int32_t(n_rows), int32_t(n_cols), nnz, expanded, r, c, vb ? vals.p : nullptr,
                                                 Ap.b.p, reinterpret_cast<int32_t*>(Aj.b.p), Ax.b.p, reinterpret_cast<int64_t*>(perm.b.p), ws.p,
                                                 &bytes, nullptr);
        }
    } else {
        st = mi355_spmv_coo_to_csr(off_type, vt, int32_t(n_rows), int32_t(n_cols), nnz, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                   nullptr, nullptr, &bytes, nullptr);
        if (st == MI355_SPMV_OK) {
            workspace(ws, bytes, prefill);
            st = mi355_spmv_coo_to_csr(off_type, vt, int32_t(n_rows), int32_t(n_cols), nnz, r, c, vb ? vals.p : nullptr, Ap.b.p,
                                       reinterpret_cast<int32_t*>(Aj.b.p), Ax.b.p, reinterpret_cast<int64_t*>(perm.b.p), ws.p, &bytes, nullptr);
        }
    }
    put_status(st);
    put_offsets(Ap, size_t(n_rows) + 1, ob, compact);
    Aj.write();
    Ax.write();
    perm.write();
}

void transpose() {
    const int off_type = int(word());
    const int64_t n_rows = word(), n_cols = word(), nnz = word(), prefill = word();
    const bool compact = word() != 0;
    const size_t ob = off_type == MI355_OFF_I64 ? 8 : 4;
    Buf Ap, Aj, ws;
    read_into(Ap, size_t(n_rows) + 1, ob);
    read_into(Aj, size_t(nnz), 4);
    Out Apt, Ajt, perm;
    Apt.make(true, size_t(n_cols) + 1, ob);
    Ajt.make(true, size_t(nnz), 4);
    perm.make(true, size_t(nnz), 4);
    size_t bytes = 0;
    int64_t st = mi355_spmv_csr_transpose(off_type, int32_t(n_rows), int32_t(n_cols), nnz, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                          &bytes, nullptr);
    if (st == MI355_SPMV_OK) {
        workspace(ws, bytes, prefill);
        st = mi355_spmv_csr_transpose(off_type, int32_t(n_rows), int32_t(n_cols), nnz, Ap.p, reinterpret_cast<const int32_t*>(Aj.p), Apt.b.p,
                                      reinterpret_cast<int32_t*>(Ajt.b.p), reinterpret_cast<uint32_t*>(perm.b.p), ws.p, &bytes, nullptr);
    }
    put_status(st);
    put_offsets(Apt, size_t(n_cols) + 1, ob, compact);
    Ajt.write();
    perm.write();
}

void put_counts(const Buf& b, int64_t n) {
    const int64_t st = 0;
    put(&st, 8);
    put(&n, 8);
    put(b.p, size_t(n) * 4);
}

// the kernels alone: each array exactly as long as its kernel may touch, the validation word clear
void kernels(int64_t tag) {
    using namespace mi355;
    using namespace mi355::coo;
    const int64_t n = word();
    Buf word0;
    word0.alloc(1, 8, 0);
    memcpy(word0.p, &kNoBad, 8);
    const unsigned long long* bad = reinterpret_cast<const unsigned long long*>(word0.p);
    if (tag == 5) {
        Buf v;
        read_into(v, size_t(n), 4);
        hipLaunchKernelGGL(scan_sums, dim3(1), dim3(kBlock), 0, nullptr, reinterpret_cast<uint32_t*>(v.p), uint64_t(n), bad);
        put_counts(v, n);
    } else if (tag == 6) {
        Buf counts, bsum;
        read_into(counts, size_t(n), 4);
        const uint64_t blocks = (uint64_t(n) + kScanChunk - 1) / kScanChunk;
        bsum.alloc(size_t(blocks), 4, 0);
        memset(bsum.p, kCanary, size_t(blocks) * 4);
        uint32_t* cp = reinterpret_cast<uint32_t*>(counts.p);
        uint32_t* bp = reinterpret_cast<uint32_t*>(bsum.p);
        hipLaunchKernelGGL(scan_reduce, dim3(unsigned(blocks)), dim3(kBlock), 0, nullptr, cp, uint64_t(n), bp, bad);
        hipLaunchKernelGGL(scan_sums, dim3(1), dim3(kBlock), 0, nullptr, bp, blocks, bad);
        hipLaunchKernelGGL(scan_apply, dim3(unsigned(blocks)), dim3(kBlock), 0, nullptr, cp, uint64_t(n), bp, bad);
        put_counts(counts, n);
    } else {
        Buf rows, cols, esum;
        read_into(rows, size_t(n), 4);
        read_into(cols, size_t(n), 4);
        const uint64_t n_etiles = (uint64_t(n) + kTile - 1) / kTile;
        esum.alloc(size_t(n_etiles) + 1, 4, 0);
        memset(esum.p, kCanary, (size_t(n_etiles) + 1) * 4);
        uint32_t* ep = reinterpret_cast<uint32_t*>(esum.p);
        hipLaunchKernelGGL(offdiag_count, dim3(unsigned(n_etiles + 1)), dim3(kBlock), 0, nullptr, reinterpret_cast<const int32_t*>(rows.p),
                           reinterpret_cast<const int32_t*>(cols.p), uint64_t(n), ep);
        hipLaunchKernelGGL(scan_sums, dim3(1), dim3(kBlock), 0, nullptr, ep, n_etiles + 1, bad);
        put_counts(esum, int64_t(n_etiles) + 1);
    }
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: coo_sim BATCH OUT\n"); return 2; }
    g_in = fopen(argv[1], "rb");
    g_out = fopen(argv[2], "wb");
    if (!g_in || !g_out) { perror("coo_sim: open"); return 2; }
    for (;;) {
        const int64_t tag = word();
        if (tag == 0) break;
        if (tag == 1 || tag == 2) coo(tag == 2);
        else if (tag == 3) transpose();
        else if (tag >= 5 && tag <= 7) kernels(tag);
        else { fprintf(stderr, "coo_sim: unknown record %lld\n", (long long)tag); return 4; }
    }
    const int64_t end = -1;
    put(&end, 8);
    if (fclose(g_out) != 0) return 4;
    fclose(g_in);
    return 0;
}
