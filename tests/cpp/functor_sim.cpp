// functor_sim — TEST CODE.  The kernel text of csrc/functor_kernel.inc, unchanged (the make rule takes off its two
// raw-string delimiter lines: functor_kernel.gen.inc), compiled with the HOST compiler over tests/cpp/simt (a stand-in
// <hip/hip_runtime.h> that runs every lane of a workgroup as a fiber) behind the prologue that
// mi355_spmv_functor_compile (csrc/functor_rtc.hip) writes in front of it: the two macros, the functor's source
// (tests/cpp/functor_texts.inc) and the five typedefs.  One program per type set: FS_FUNCTOR, FS_OFF, FS_MAT, FS_X and
// FS_Y are given on the command line of the compiler (tests/cpp/Makefile; tests/functor_cases.py, TYPE_SETS).  The launch
// shape is the product's functor_shape (csrc/functor_shape.hpp); a case may override the two grids, nothing else.  Built
// with -fsanitize=address,undefined.
//
//   functor_sim_<set> BATCH OUT      reads records from BATCH, writes one result per record to OUT
//
// Records are int64 words followed by raw little-endian arrays (tests/test_functor_sim_cpu.py writes them):
//   1  run     off_bytes mat_bytes x_bytes y_bytes n_rows n_cols nnz aj_off ax_off x_off rows_grid long_grid guard
//              | Ap[n_rows + 1] Aj[nnz] Ax[nnz] x[n_cols] y[n_rows + 2 guard]
//   2  shape   n_rows nnz
//   0  end
// *_bytes must be this program's sizeof; *_off = elements between a 64-byte boundary and the operand's base; rows_grid /
// long_grid = 0: the shape's own.  Every operand is an allocation of its own, exactly as long as the call may touch, so a
// read one element outside is a report; y comes with `guard` elements on either side, which the result carries back.
// A result is: T, long_len, rows_grid, long_launch, long_grid (as launched), then for a run the n_rows + 2 guard elements
// of y.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "../../include/mi355_spmv.h"
#include "../../spmv-samples_amd/csrc/functor_shape.hpp"

// ---- what mi355_spmv_functor_compile puts in front of the kernels ------------------------------------------------------
#ifndef INFINITY
#define INFINITY __builtin_huge_valf()
#endif
#ifndef NAN
#define NAN __builtin_nanf("")
#endif
#line 1 "functor_source"
#include "functor_texts.inc"

#line 1 "mi355_functor_kernels"
typedef FS_FUNCTOR mi355_functor_t;
typedef FS_OFF mi355_off_t;
typedef FS_MAT mi355_mat_t;
typedef FS_X mi355_x_t;
typedef FS_Y mi355_y_t;
#include "functor_kernel.gen.inc"
// ------------------------------------------------------------------------------------------------------------------------

#define SIM_NAME "functor_sim"
#include "sim_io.hpp"

namespace {

typedef void (*rows_kernel_t)(int, const mi355_off_t*, const int*, const mi355_mat_t*, const mi355_x_t*, mi355_y_t*, long long);
const rows_kernel_t kRows[mi355::kFunctorLaneChoices] = {mi355_functor_rows_2,  mi355_functor_rows_4,  mi355_functor_rows_8,
                                                        mi355_functor_rows_16, mi355_functor_rows_32, mi355_functor_rows_64};

void put_shape(const mi355::FunctorShape& s) {
    const int64_t w[5] = {s.T, s.long_len, s.rows_grid, s.long_launch, s.long_grid};
    put(w, sizeof(w));
}

void run() {
    const int64_t ob = word(), mb = word(), xb = word(), yb = word();
    if (ob != sizeof(mi355_off_t) || mb != sizeof(mi355_mat_t) || xb != sizeof(mi355_x_t) || yb != sizeof(mi355_y_t)) {
        fprintf(stderr, "functor_sim: the batch is of another type set (%d %d %d %d bytes)\n", int(ob), int(mb), int(xb), int(yb));
        exit(4);
    }
    const int64_t n_rows = word(), n_cols = word(), nnz = word(), aj_off = word(), ax_off = word(), x_off = word();
    const int64_t rows_grid = word(), long_grid = word(), guard = word();
    if (n_rows < 1 || n_cols < 0 || nnz < 0 || guard < 0 || rows_grid < 0 || long_grid < 0) { fprintf(stderr, "functor_sim: bad run record\n"); exit(4); }
    Buf Ap, Aj, Ax, x, y;
    Ap.alloc(size_t(n_rows) + 1, size_t(ob), 0);
    Aj.alloc(size_t(nnz), 4, size_t(aj_off));
    Ax.alloc(size_t(nnz), size_t(mb), size_t(ax_off));
    x.alloc(size_t(n_cols), size_t(xb), size_t(x_off));
    y.alloc(size_t(n_rows + 2 * guard), size_t(yb), 0);
    get(Ap.p, (size_t(n_rows) + 1) * size_t(ob));
    get(Aj.p, size_t(nnz) * 4);
    get(Ax.p, size_t(nnz) * size_t(mb));
    get(x.p, size_t(n_cols) * size_t(xb));
    get(y.p, size_t(n_rows + 2 * guard) * size_t(yb));
    mi355::FunctorShape s = mi355::functor_shape(int32_t(n_rows), nnz);
    if (rows_grid) s.rows_grid = unsigned(rows_grid);
    if (long_grid && s.long_launch) s.long_grid = unsigned(long_grid);
    // the two launches of mi355_spmv_functor_spmv
    hipLaunchKernelGGL(kRows[s.choice], dim3(s.rows_grid), dim3(mi355::kFunctorBlock), 0, nullptr, int(n_rows),
                       reinterpret_cast<const mi355_off_t*>(Ap.p), reinterpret_cast<const int*>(Aj.p),
                       reinterpret_cast<const mi355_mat_t*>(Ax.p), reinterpret_cast<const mi355_x_t*>(x.p),
                       reinterpret_cast<mi355_y_t*>(y.p) + guard, s.long_len);
    if (s.long_launch)
        hipLaunchKernelGGL(mi355_functor_long_rows, dim3(s.long_grid), dim3(mi355::kFunctorBlock), 0, nullptr, int(n_rows),
                           reinterpret_cast<const mi355_off_t*>(Ap.p), reinterpret_cast<const int*>(Aj.p),
                           reinterpret_cast<const mi355_mat_t*>(Ax.p), reinterpret_cast<const mi355_x_t*>(x.p),
                           reinterpret_cast<mi355_y_t*>(y.p) + guard, s.long_len);
    put_shape(s);
    put(y.p, size_t(n_rows + 2 * guard) * size_t(yb));
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: functor_sim BATCH OUT\n"); return 2; }
    static_assert(mi355::kFunctorBlock == mi355_functor::kBlock && mi355::kFunctorWave == mi355_functor::kWave, "functor_shape.hpp and functor_kernel.inc");
    g_in = fopen(argv[1], "rb");
    g_out = fopen(argv[2], "wb");
    if (!g_in || !g_out) { perror("functor_sim: open"); return 2; }
    for (;;) {
        const int64_t tag = word();
        if (tag == 0) break;
        if (tag == 1) {
            run();
        } else if (tag == 2) {
            const int64_t n_rows = word(), nnz = word();
            put_shape(mi355::functor_shape(int32_t(n_rows), nnz));
        } else {
            fprintf(stderr, "functor_sim: unknown record %lld\n", (long long)tag);
            return 4;
        }
    }
    const int64_t end = -1;
    put(&end, 8);
    if (fclose(g_out) != 0) return 4;
    fclose(g_in);
    return 0;
}
